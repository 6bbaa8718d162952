// api_shard.cpp -- the C ABI of include/gmrfx.h: the sharded protocol (metadata of what moves between ranks, and the phase calls).
#include "api_common.h"

extern "C" int32_t gmrfx_refactorize_phase(gmrfx_handle *h, const double *d_nzval, int32_t phase) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (phase == 0 && !d_nzval) throw std::invalid_argument("d_nzval is null");
        if (phase < 0 || phase > h->S.nlevels - h->S.shard_level) throw std::invalid_argument("phase must be 0 (own subtrees) or 1 + k (top level k)");
        h->D->refactorize_phase(d_nzval, phase);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_shard_info(const gmrfx_handle *h, int64_t *n_edges, int64_t *n_top_fronts, int64_t *shard_level) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    int64_t ntop = 0;
    for (i32 s = 0; s < S.nsuper; s++) ntop += S.is_top[s];
    if (n_edges) *n_edges = (int64_t)S.shard_edges.size();
    if (n_top_fronts) *n_top_fronts = ntop;
    if (shard_level) *shard_level = S.shard_level;
    return GMRFX_OK;
}
// cross-rank tree edges child -> parent, ordered by the level of the parent: what moves between two phases
extern "C" int32_t gmrfx_shard_edges(const gmrfx_handle *h, int64_t *child, int64_t *src, int64_t *dst, int64_t *level,
                                     int64_t *cb_offset, int64_t *cb_count, int64_t *w_row0, int64_t *w_nrows, int64_t *zb_offset,
                                     int64_t *child_level) {
    if (!h || !child || !src || !dst || !level || !cb_offset || !cb_count || !w_row0 || !w_nrows) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    const std::vector<i64> &wptr = S.wptr;      // cross-edge children come first, identically on every rank
    for (size_t k = 0; k < S.shard_edges.size(); k++) {
        const i32 d = S.shard_edges[k], p = S.sparent[d];
        const int64_t m = S.nrows(d) - S.ncols(d);
        child[k] = d; src[k] = S.owner[d]; dst[k] = S.owner[p]; level[k] = S.level[p];
        // offsets in THIS rank's arena (round 6: per-rank layouts); -1 when this rank is neither end of the edge
        const bool end = S.owner[d] == S.shard_rank || S.owner[p] == S.shard_rank;
        cb_offset[k] = end ? S.cbptr[d] : -1; cb_count[k] = m * m;
        w_row0[k] = wptr[d]; w_nrows[k] = m;
        if (zb_offset) zb_offset[k] = end ? S.zbptr[d] : -1;
        if (child_level) child_level[k] = S.level[d];
    }
    return GMRFX_OK;
}
// Distributed top fronts (symbolic.h: Symbolic::dist_fronts). counts[0] = number of distributed fronts, [1] = entries of all
// groups, [2] = contribution-block transfers of the factorisation, [3] = world. Per front (nullable arrays of counts[0]):
// supernode, columns, rows, offset of its panel in gmrfx_device_ptr(h, 1), leading dimension of the panel, tree level; gptr
// (counts[0] + 1) / grank (counts[1]): the ranks of its group. Panel block b (256 columns) is factored by grank[gptr[k] + b mod g].
extern "C" int32_t gmrfx_shard_dist_fronts(const gmrfx_handle *h, int64_t *counts, int64_t *front, int64_t *cols, int64_t *rows,
                                           int64_t *panel_offset, int64_t *panel_ld, int64_t *level, int64_t *gptr, int64_t *grank) {
    if (!h || !counts) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    const size_t nf = S.dist_fronts.size();
    counts[0] = (int64_t)nf; counts[1] = (int64_t)S.dist_grank.size(); counts[2] = (int64_t)S.xf_child.size(); counts[3] = S.shard_world;
    for (size_t k = 0; k < nf; k++) {
        const i32 s = S.dist_fronts[k];
        if (front) front[k] = s;
        if (cols) cols[k] = S.ncols(s);
        if (rows) rows[k] = S.nrows(s);
        if (panel_offset) panel_offset[k] = S.panelptr[s];
        if (panel_ld) panel_ld[k] = S.ld[s];
        if (level) level[k] = S.level[s];
    }
    if (gptr) for (size_t k = 0; k < S.dist_gptr.size(); k++) gptr[k] = S.dist_gptr[k];
    if (grank) for (size_t k = 0; k < S.dist_grank.size(); k++) grank[k] = S.dist_grank[k];
    return GMRFX_OK;
}
// Every contribution-block transfer of the sharded factorisation (symbolic.h: xf_*), ordered by the level of the parent:
// Where THIS rank keeps panel block `block` (256 columns) of the distributed front `front`, as an offset into gmrfx_device_ptr(h, 1)
// and a count of doubles (whole columns): the buffer it passes to the broadcast of that block inside the front's group. The owner of
// the front (and every member of a front that has a contribution block) stores the whole panel: offset = panel + 256 block ld. A
// member with block-cyclic storage (Symbolic::compact_here) keeps its OWN blocks one behind the other and receives the others into
// a window of two blocks (block & 1). offset = -1, count = 0 on ranks outside the group.
extern "C" int32_t gmrfx_dist_front_block(const gmrfx_handle *h, int32_t front, int32_t block, int64_t *offset, int64_t *count) {
    if (!h || !offset || !count) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    if (front < 0 || front >= S.nsuper || !S.is_dist(front) || block < 0 || block >= S.panel_blocks(front)) return GMRFX_ERR_INVALID_ARG;
    const i32 g = S.group_size(front), me = S.group_pos(front, S.shard_rank);
    *offset = -1; *count = 0;
    if (me < 0) return GMRFX_OK;
    const i64 ld = S.ld[front];
    *count = (i64)std::min<i64>(256, S.ncols(front) - 256 * (i64)block) * ld;
    if (!S.compact_here(front)) *offset = S.panelptr[front] + 256 * (i64)block * ld;
    else if (block % g == me) *offset = S.panelptr[front] + (i64)(block / g) * 256 * ld;
    else *offset = S.panelptr[front] + S.compact_window(front, block & 1);
    return GMRFX_OK;
}
// `count` doubles at `offset` of the arena (gmrfx_device_ptr(h, 0)) -- whole columns of `child`'s block -- go src -> dst before
// the fronts of `level` are assembled; col0 = the first of these columns. (Edges between fronts of one owner, neither
// distributed, have no entry.)
extern "C" int32_t gmrfx_shard_transfers(const gmrfx_handle *h, int64_t *child, int64_t *src, int64_t *dst, int64_t *level,
                                         int64_t *offset, int64_t *count, int64_t *col0) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    for (size_t k = 0; k < S.xf_child.size(); k++) {
        if (child) child[k] = S.xf_child[k];
        if (src) src[k] = S.xf_src[k];
        if (dst) dst[k] = S.xf_dst[k];
        if (level) level[k] = S.xf_level[k];
        if (offset) offset[k] = S.xf_off[k];
        if (count) count[k] = S.xf_cnt[k];
        if (col0) col0[k] = S.xf_col0[k];
    }
    return GMRFX_OK;
}
// Block phases of distributed front `front` (a supernode of gmrfx_shard_dist_fronts; a no-op on ranks outside its group).
// what = 0: assemble this rank's panel blocks (Q's entries + the children's columns received); 1: factor panel block `block`
// (its owner only); 2: apply panel block `block` (complete on every member after its broadcast) to this rank's later panel
// blocks; 3: this rank's column blocks of the contribution block (children's columns received - L21 L21'). Asynchronous on the
// handle's main stream when async phases are on.
extern "C" int32_t gmrfx_dist_front_phase(gmrfx_handle *h, const double *d_nzval, int32_t front, int32_t what, int32_t block) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        h->D->dist_front_phase(d_nzval, front, what, block);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_shard_owner(const gmrfx_handle *h, int64_t *owner, int64_t *is_top) {
    if (!h || !owner) return GMRFX_ERR_INVALID_ARG;
    for (i32 s = 0; s < h->S.nsuper; s++) { owner[s] = h->S.owner[s]; if (is_top) is_top[s] = h->S.is_top[s]; }
    return GMRFX_OK;
}
extern "C" int32_t gmrfx_solve_phase(gmrfx_handle *h, const double *d_B, int64_t ldb, int64_t nrhs, double *d_X, int64_t ldx, int32_t phase) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        if (phase == 0 && !d_B) throw std::invalid_argument("d_B is null");
        if (phase == 0 && ldb < h->S.n) throw std::invalid_argument("ldb < n");
        if (phase == 3 && (!d_X || ldx < h->S.n)) throw std::invalid_argument("d_X is null or ldx < n");
        h->D->solve_phase(d_B, ldb, nrhs, d_X, ldx, phase);
        return GMRFX_OK;
    });
}
// Row blocks of the right-hand-side buffer X (gmrfx_device_ptr(h, 2); row-major, leading dimension = nrhs) that the
// sharded solve moves: kind 2 = the own columns of every TOP front (owner broadcasts x after its backward step; level[]
// tells in which phase), kind 3 = the columns of every assigned subtree (gathered on rank 0 at the end).
extern "C" int32_t gmrfx_shard_rows(const gmrfx_handle *h, int32_t kind, int64_t *nblocks, int64_t *owner, int64_t *row0, int64_t *nrows,
                                    int64_t *level) {
    if (!h || !nblocks) return GMRFX_ERR_INVALID_ARG;
    const Symbolic &S = h->S;
    std::vector<int64_t> o, a, c, l;
    if (kind == 2) {
        for (i32 s = 0; s < S.nsuper; s++) if (S.is_top[s]) { o.push_back(S.owner[s]); a.push_back(S.sfirst[s]); c.push_back(S.ncols(s)); l.push_back(S.level[s]); }
    } else if (kind == 3) {
        for (size_t k = 0; k < S.shard_sub_root.size(); k++) {
            const i32 t = S.shard_sub_root[k];
            o.push_back(S.owner[t]); a.push_back(S.shard_sub_col0[k]); c.push_back(S.sfirst[t + 1] - S.shard_sub_col0[k]); l.push_back(S.level[t]);
        }
    } else return GMRFX_ERR_INVALID_ARG;
    *nblocks = (int64_t)o.size();
    if (owner && row0 && nrows)
        for (size_t k = 0; k < o.size(); k++) { owner[k] = o[k]; row0[k] = a[k]; nrows[k] = c[k]; if (level) level[k] = l[k]; }
    return GMRFX_OK;
}
// gmrfx_logdet under the protocol's name: a sharded handle sums over its own columns only
extern "C" int32_t gmrfx_logdet_partial(gmrfx_handle *h, double *out) { return gmrfx_logdet(h, out); }
// sharded selected inversion (include/gmrfx.h): what = 0 begin, 1 gather the trailing inverse blocks of other ranks'
// fronts at level hi (parents owned here), 2 this rank's fronts of levels hi-1 .. lo, 3 end
extern "C" int32_t gmrfx_selinv_phase(gmrfx_handle *h, int32_t what, int32_t hi, int32_t lo) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        h->D->selinv_phase(what, hi, lo);
        return GMRFX_OK;
    });
}
