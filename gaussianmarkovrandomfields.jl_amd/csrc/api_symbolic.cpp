// api_symbolic.cpp -- the C ABI of include/gmrfx.h: what a handle's symbolic analysis looks like (sizes, supernodes, sweep tasks).
#include "api_common.h"

extern "C" int32_t gmrfx_symbolic_sizes(const gmrfx_handle *h, int64_t *sizes) {
    if (!h || !sizes) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    sizes[0] = S.nsuper; sizes[1] = S.sum_rows; sizes[2] = S.panelptr[S.nsuper]; sizes[3] = S.nlevels;
    sizes[4] = S.cb_arena; sizes[5] = (int64_t)S.qsrc.size(); sizes[6] = 0; sizes[7] = 0;
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_symbolic_get(const gmrfx_handle *h, int64_t *super_first, int64_t *super_parent,
                                      int64_t *row_ptr, int64_t *rows, int64_t *rel, int64_t *panel_ptr,
                                      int64_t *panel_ld, int64_t *level, int64_t *q_src, int64_t *q_dst) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    const i32 ns = S.nsuper;
    if (super_first) for (i32 s = 0; s <= ns; s++) super_first[s] = S.sfirst[s];
    if (super_parent) for (i32 s = 0; s < ns; s++) super_parent[s] = S.sparent[s];
    if (row_ptr) for (i32 s = 0; s <= ns; s++) row_ptr[s] = S.rowptr[s];
    if (rows) for (i64 k = 0; k < S.sum_rows; k++) rows[k] = S.rows[k];
    if (rel) for (i64 k = 0; k < S.sum_rows; k++) rel[k] = S.rel[k];
    if (panel_ptr) for (i32 s = 0; s <= ns; s++) panel_ptr[s] = S.panelptr[s];
    if (panel_ld) for (i32 s = 0; s < ns; s++) panel_ld[s] = S.ld[s];
    if (level) for (i32 s = 0; s < ns; s++) level[s] = S.level[s];
    if (q_src) for (size_t k = 0; k < S.qsrc.size(); k++) q_src[k] = S.qsrc[k];
    if (q_dst) {
        for (size_t k = 0; k < S.qdst.size(); k++) q_dst[k] = S.qdst[k];
        // a sharded handle stores the panels of its own fronts only: the entries of Q that go into another rank's panel
        // have no destination here (-1)
        if (S.shard_plan)
            for (i32 s = 0; s < ns; s++) {
                if (!S.stored_here(s))      // (every member of its group stores the panel of a distributed front ...)
                    for (i64 k = S.qptr[s]; k < S.qptr[s + 1]; k++) q_dst[k] = -1;
                else if (S.compact_here(s)) {   // (... or, block-cyclic storage, its own 256-column blocks one behind the other)
                    const i64 ld = S.ld[s];
                    const i32 g = S.group_size(s), me = S.group_pos(s, S.shard_rank);
                    for (i64 k = S.qptr[s]; k < S.qptr[s + 1]; k++) {
                        const i64 rel = S.qdst[k] - S.panelptr[s], col = rel / ld, row = rel % ld, b = col >> 8;
                        q_dst[k] = b % g != me ? -1 : S.panelptr[s] + (col - 256 * (b - b / g)) * ld + row;
                    }
                }
            }
    }
    return GMRFX_OK;
}

// Sweep tasks (symbolic.h: swt_*): bottom subtrees whose triangular sweeps run on an LDS-resident local vector.
// ntasks / rows_cap always; first / last (ntasks each) and lrow (sum_rows) when non-null.
extern "C" int32_t gmrfx_symbolic_sweep_tasks(const gmrfx_handle *h, int64_t *ntasks, int64_t *rows_cap, int64_t *first,
                                              int64_t *last, int64_t *lrow) {
    if (!h || !ntasks) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    *ntasks = (int64_t)S.swt_first.size();
    if (rows_cap) *rows_cap = S.swt_rows;
    if (first) for (size_t k = 0; k < S.swt_first.size(); k++) first[k] = S.swt_first[k];
    if (last) for (size_t k = 0; k < S.swt_last.size(); k++) last[k] = S.swt_last[k];
    if (lrow) for (size_t k = 0; k < S.lrow.size(); k++) lrow[k] = S.lrow[k];
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_symbolic_sweep_chunks(const gmrfx_handle *h, int64_t *nchunks, int64_t *nrows, int64_t *task_ptr,
                                               int64_t *slot, int64_t *fwd, int64_t *bwd, int64_t *rows) {
    if (!h || !nchunks) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    nchunks[0] = (int64_t)S.swc_fwd.size();
    nchunks[1] = (int64_t)S.swc_bwd.size();
    if (nrows) *nrows = (int64_t)S.swc_rows.size();
    if (task_ptr) for (size_t k = 0; k < S.swc_ptr.size(); k++) { task_ptr[2 * k] = S.swc_ptr[k]; task_ptr[2 * k + 1] = S.swc_bptr[k]; }
    if (slot) for (size_t k = 0; k < S.swc_slot.size(); k++) slot[k] = S.swc_slot[k];
    auto put = [](const std::vector<Symbolic::SwChunk> &v, int64_t *out) {
        for (size_t k = 0; k < v.size(); k++) {
            const Symbolic::SwChunk &c = v[k];
            int64_t *o = out + 8 * k;
            o[0] = c.pa; o[1] = c.ld; o[2] = c.o; o[3] = c.cc; o[4] = c.nt; o[5] = c.lr; o[6] = c.nbar; o[7] = c.id;
        }
    };
    if (fwd) put(S.swc_fwd, fwd);
    if (bwd) put(S.swc_bwd, bwd);
    if (rows) for (size_t k = 0; k < S.swc_rows.size(); k++) rows[k] = S.swc_rows[k];
    return GMRFX_OK;
}
