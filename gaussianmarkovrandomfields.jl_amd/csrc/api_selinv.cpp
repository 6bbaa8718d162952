// api_selinv.cpp -- the C ABI of include/gmrfx.h: the selected inverse and the host-side planners of its patterns.
#include "api_common.h"
#include "selinv_offsets.h"

extern "C" int32_t gmrfx_selinv_compute(gmrfx_handle *h) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        h->D->selinv_compute();
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_selinv_diag(gmrfx_handle *h, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        if (!out) throw std::invalid_argument("out is null");
        h->D->selinv_compute();
        h->D->selinv_diag(out);
        return GMRFX_OK;
    });
}

// Pattern of the de-permuted selected inverse (both triangles, rows sorted) + panel offsets.
static void build_zpattern(gmrfx_handle *h) {
    if (h->zpat_built) return;
    const Symbolic &S = h->S;
    const i64 n = S.n;
    std::vector<i64> cnt(n + 1, 0);
    for (i32 s = 0; s < S.nsuper; s++) {
        const i32 c = S.ncols(s), r = S.nrows(s);
        const i32 *rows = S.rows.data() + S.rowptr[s];
        for (i32 j = 0; j < c; j++) {
            const i32 b = S.perm[S.sfirst[s] + j];
            cnt[b + 1] += r - j;                       // column b gets rows i >= j
            for (i32 i = j + 1; i < r; i++) cnt[S.perm[rows[i]] + 1]++;  // mirrored entry
        }
    }
    h->zcolptr.assign(n + 1, 0);
    for (i64 j = 0; j < n; j++) h->zcolptr[j + 1] = h->zcolptr[j] + cnt[j + 1];
    const i64 nz = h->zcolptr[n];
    std::vector<std::pair<i64, i64>> ent((size_t)nz);  // (row, offset), bucketed by column
    std::vector<i64> w(h->zcolptr.begin(), h->zcolptr.end() - 1);
    for (i32 s = 0; s < S.nsuper; s++) {
        const i32 c = S.ncols(s), r = S.nrows(s);
        const i32 *rows = S.rows.data() + S.rowptr[s];
        for (i32 j = 0; j < c; j++) {
            const i32 b = S.perm[S.sfirst[s] + j];
            for (i32 i = j; i < r; i++) {
                const i32 a = S.perm[rows[i]];
                // a sharded handle holds the panels of its own fronts only: every other entry reads the zeroed slack word
                const i64 off = (!S.shard_plan || S.owner[s] == S.shard_rank) ? S.panelptr[s] + (i64)j * S.ld[s] + i : S.panelptr[S.nsuper];
                ent[w[b]++] = {a, off};
                if (i != j) ent[w[a]++] = {b, off};
            }
        }
    }
    h->zrow.resize(nz);
    h->zoff.resize(nz);
    for (i64 j = 0; j < n; j++) {
        std::sort(ent.begin() + h->zcolptr[j], ent.begin() + h->zcolptr[j + 1]);
        for (i64 p = h->zcolptr[j]; p < h->zcolptr[j + 1]; p++) { h->zrow[p] = ent[p].first; h->zoff[p] = ent[p].second; }
    }
    h->zpat_built = true;
}

extern "C" int32_t gmrfx_selinv_nnz(gmrfx_handle *h, int64_t *nnz) {
    return guarded(h, [&]() -> int32_t {
        if (!nnz) throw std::invalid_argument("nnz is null");
        *nnz = 2 * h->S.nnz_l_stored - h->S.n;
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_selinv_csc(gmrfx_handle *h, int32_t base, int64_t *colptr, int64_t *rowval, double *nzval) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        if (!colptr || !rowval || !nzval) throw std::invalid_argument("null output");
        check_index_base(base);
        h->D->selinv_compute();
        build_zpattern(h);
        const i64 n = h->S.n, nz = h->zcolptr[n];
        for (i64 j = 0; j <= n; j++) colptr[j] = h->zcolptr[j] + base;
        for (i64 p = 0; p < nz; p++) rowval[p] = h->zrow[p] + base;
        h->D->gather_z((const long long *)h->zoff.data(), nz, nzval);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_selinv_extract(gmrfx_handle *h, int64_t ncol, const int64_t *colptr, const int64_t *rowval,
                                        int32_t base, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        const Symbolic &S = h->S;
        if (ncol != S.n) throw std::invalid_argument("pattern must have n columns");
        if (!colptr || !rowval || !out) throw std::invalid_argument("null argument");
        check_index_base(base);
        check_compressed_ptr(colptr, ncol, base, "colptr");
        h->D->selinv_compute();
        const i64 nz = colptr[ncol] - base;
        const std::vector<long long> off = z_offsets_csc(S, ncol, colptr, rowval, base);
        h->D->gather_z(off.data(), nz, out);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_selinv_dot(gmrfx_handle *h, int64_t ncol, const int64_t *colptr, const int64_t *rowval,
                                    const double *nzval, int32_t base, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        const Symbolic &S = h->S;
        if (ncol != S.n) throw std::invalid_argument("B must have n columns");
        if (!colptr || !rowval || !nzval || !out) throw std::invalid_argument("null argument");
        check_index_base(base);
        check_compressed_ptr(colptr, ncol, base, "colptr");
        h->D->selinv_compute();
        const i64 nz = colptr[ncol] - base;
        const std::vector<long long> off = z_offsets_csc(S, ncol, colptr, rowval, base);
        // fixed chunks of 4096 entries are summed on the device, the chunk sums on the host in order
        const i64 CH = 4096, nseg = (nz + CH - 1) / CH;
        std::vector<long long> seg((size_t)nseg + 1);
        for (i64 g = 0; g <= nseg; g++) seg[g] = std::min(g * CH, nz);
        std::vector<double> part((size_t)nseg);
        h->D->weighted_z_sums(seg.data(), nseg, off.data(), nzval + 0, part.data());
        double acc = 0.0;
        for (double v : part) acc += v;
        *out = acc;
        return GMRFX_OK;
    });
}

// pairs (p, q <= p) of the entries of every row of a sparse design matrix + the offsets of Sigma[j_p, j_q]
static void plan_row_pairs(const Symbolic &S, int64_t m, const int64_t *rowptr, const int64_t *colind, int32_t base,
                           std::vector<long long> &seg, std::vector<long long> &off, std::vector<int> &pi, std::vector<int> &qi) {
    check_compressed_ptr(rowptr, m, base, "rowptr");
    seg.assign((size_t)m + 1, 0);
    for (i64 i = 0; i < m; i++) {
        const i64 k = rowptr[i + 1] - rowptr[i];
        if (k < 0) throw std::invalid_argument("rowptr not monotone");
        seg[i + 1] = seg[i] + k * (k + 1) / 2;
    }
    const i64 nz = rowptr[m] - base;
    if (nz > 0x7fffffffLL) throw std::invalid_argument("design matrix too large");
    off.resize((size_t)seg[m]); pi.resize((size_t)seg[m]); qi.resize((size_t)seg[m]);
    parallel_ranges(m, [&](i64 lo, i64 hi) {
        for (i64 i = lo; i < hi; i++) {
            long long t = seg[i];
            for (i64 p = rowptr[i] - base; p < rowptr[i + 1] - base; p++) {
                const i64 jp = colind[p] - base;
                if (jp < 0 || jp >= S.n) throw std::invalid_argument("colind out of range");
                for (i64 q = rowptr[i] - base; q <= p; q++) {
                    const i64 jq = colind[q] - base;
                    if (jq < 0 || jq >= S.n) throw std::invalid_argument("colind out of range");
                    off[t] = z_offset(S, jp, jq);
                    pi[t] = (int)p; qi[t] = (int)q;
                    t++;
                }
            }
        }
    });
}

extern "C" int32_t gmrfx_selinv_row_diag(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind,
                                         const double *values, int32_t base, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        if (m < 0 || !rowptr || (m > 0 && !out)) throw std::invalid_argument("null argument");
        check_index_base(base);
        if (m == 0) return GMRFX_OK;
        if (rowptr[m] - base > 0 && (!colind || !values)) throw std::invalid_argument("null argument");
        h->D->selinv_compute();
        std::vector<long long> seg, off;
        std::vector<int> pi, qi;
        plan_row_pairs(h->S, m, rowptr, colind, base, seg, off, pi, qi);
        std::vector<double> w(off.size());
        for (size_t t = 0; t < w.size(); t++) w[t] = (pi[t] == qi[t] ? 1.0 : 2.0) * values[pi[t]] * values[qi[t]];
        h->D->weighted_z_sums(seg.data(), m, off.data(), w.data(), out);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_selinv_row_diag_plan(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind,
                                              int32_t base, int64_t *plan) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (m < 0 || !rowptr || !plan) throw std::invalid_argument("null argument");
        check_index_base(base);
        if (m > 0 && rowptr[m] - base > 0 && !colind) throw std::invalid_argument("null argument");
        std::vector<long long> seg, off;
        std::vector<int> pi, qi;
        plan_row_pairs(h->S, m, rowptr, colind, base, seg, off, pi, qi);
        *plan = h->D->rowdiag_plan_create(seg.data(), m, off.data(), pi.data(), qi.data(), m > 0 ? rowptr[m] - base : 0);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_selinv_row_diag_apply(gmrfx_handle *h, int64_t plan, const double *values, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        if (!values || !out) throw std::invalid_argument("null argument");
        h->D->selinv_compute();
        h->D->rowdiag_plan_apply(plan, values, out);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_selinv_row_diag_free(gmrfx_handle *h, int64_t plan) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        h->D->rowdiag_plan_free(plan);
        return GMRFX_OK;
    });
}
