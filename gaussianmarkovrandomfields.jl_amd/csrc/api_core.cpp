// api_core.cpp -- the C ABI of include/gmrfx.h: handle lifetime, errors, and the numeric calls of a plain handle (host and _dev twins
// side by side). The other subjects of the boundary: api_symbolic / api_shard / api_selinv / api_batch / api_constraints / api_kl_rbmc.cpp.
#include <cstdlib>

#include "api_common.h"

thread_local std::string g_create_err;

extern "C" const char *gmrfx_last_create_error(void) { return g_create_err.c_str(); }
extern "C" const char *gmrfx_last_error(const gmrfx_handle *h) { return h ? h->err.c_str() : "null handle"; }

// gmrfx_opts -> the analysis options (and the tuning / testing knobs of the environment)
void sym_options(const gmrfx_opts &o, SymOptions &so) {
    so.uplo = o.uplo;
    so.ordering = o.ordering;
    so.nd_leaf = o.nd_leaf;
    so.relax_cols = o.relax_cols;
    so.relax_zeros = o.relax_zeros;
    so.coord_dim = o.coords ? o.coord_dim : 0;
    so.coords = o.coords;
    if (so.coords && so.coord_dim != 2 && so.coord_dim != 3) throw std::invalid_argument("coord_dim must be 2 or 3");
    if (const char *e = std::getenv("GMRFX_SMALL_ROWS")) so.small_front_rows = std::atoi(e);   // tuning/testing knob
    if (const char *e = std::getenv("GMRFX_SUBTREE_MAX")) so.subtree_max = std::atoi(e);       // 0 disables subtree tasks
    if (const char *e = std::getenv("GMRFX_SWEEP_TASK_ROWS")) so.sweep_task_rows = std::atoi(e);   // 0 disables sweep tasks
    if (const char *e = std::getenv("GMRFX_MERGE_WIDE")) so.merge_wide = std::atoi(e);   // widest child with siblings that may still be merged into its parent
    if (const char *e = std::getenv("GMRFX_TOP_BY_DEPTH")) so.top_by_depth = std::atoi(e);   // top levels levelled by depth below the root (0: none)
    if (o.shard_world > 1 || (o.shard_world == 1 && o.shard_min_top > 0)) {
        so.shard_min_top = std::max(0, o.shard_min_top);
        if (o.shard_rank < 0 || o.shard_rank >= o.shard_world) throw std::invalid_argument("shard_rank out of range");
        so.shard_rank = o.shard_rank;
        so.shard_world = o.shard_world;
        if (const char *e = std::getenv("GMRFX_DIST_MIN")) so.dist_min_cols = std::atoi(e);   // columns from which a top front is factored by its whole group (0: never)
        so.subtree_max = 0;     // subtree tasks are not shard-aware
    }
}

extern "C" int32_t gmrfx_create(int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t index_base,
                                const int64_t *perm, const gmrfx_opts *opts, gmrfx_handle **out) {
    if (!out) { g_create_err = "out is null"; return GMRFX_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!colptr || !rowval) { g_create_err = "colptr/rowval is null"; return GMRFX_ERR_INVALID_ARG; }
    std::unique_ptr<gmrfx_handle> h(new gmrfx_handle());
    if (!read_opts(opts, h->opts)) return GMRFX_ERR_INVALID_ARG;
    if (int32_t e = create_guarded(true, [&]() -> int32_t {
            SymOptions so;
            sym_options(h->opts, so);
            analyze(n, colptr, rowval, index_base, perm, so, h->S);
            h->opts.coords = nullptr;  // caller-owned, not kept
            h->n_member = h->S.n; h->nnz_member = h->S.nnz_in;
            return GMRFX_OK;
        })) return e;
    if (int32_t e = attach_device(h.get(), false)) return e;
    *out = h.release();
    return GMRFX_OK;
}

extern "C" void gmrfx_destroy(gmrfx_handle *h) { delete h; }

extern "C" int32_t gmrfx_clone(const gmrfx_handle *h, gmrfx_handle **out) {
    if (!h || !out) return GMRFX_ERR_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<gmrfx_handle> c(new gmrfx_handle());
    try {
        c->S = h->S;
        c->opts = h->opts;
        c->nbatch = h->nbatch; c->n_member = h->n_member; c->nnz_member = h->nnz_member;
        if (h->D) {
            c->D.reset(new Device());
            c->D->clone_from(*h->D, c->S);
            if (h->D->batched()) c->D->set_batch((int)c->nbatch, c->n_member, c->nnz_member);
        }
        c->con = h->con;        // A and e travel; the clone recomputes what is derived from them
        if (c->D && c->con.m > 0) c->D->con_set(c->con);
        c->bcon = h->bcon;
        if (c->D && c->bcon.m > 0) c->D->bcon_set(c->bcon);
        c->obs = h->obs;        // the likelihood travels too (the prior's values do not: the clone calls gmrfx_set_prior itself)
        if (c->D && c->obs.nobs > 0) c->D->obs_set(c->obs);
        c->bobs = h->bobs;      // and so does the batch calls' (gmrfx_batch_obs_set)
        if (c->D && c->bobs.nobs > 0) {
            if (!c->D->batched()) c->D->set_batch(1, c->S.n, c->S.nnz_in);
            if (!c->rsym.built) rbmc_build_sym(c->S, c->rsym);
            c->D->bobs_set(c->rsym, c->bobs);
        }
    } catch (const std::exception &e) {
        g_create_err = e.what();
        return GMRFX_ERR_HIP;
    }
    *out = c.release();
    return GMRFX_OK;
}

static int32_t refactorize_impl(gmrfx_handle *h, const double *nz, int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (!nz) throw std::invalid_argument("nzval is null");
        h->D->refactorize(nz, dev);
        return pivot_status(h, info);
    });
}
extern "C" int32_t gmrfx_refactorize(gmrfx_handle *h, const double *nzval, int64_t *info) { return refactorize_impl(h, nzval, info, false); }
extern "C" int32_t gmrfx_refactorize_dev(gmrfx_handle *h, const double *d_nzval, int64_t *info) { return refactorize_impl(h, d_nzval, info, true); }

// workspace_solve with a stale factorisation (src/workspace/gmrf_workspace.jl:170-178, 207-215: ensure_numeric! -> refactorize!,
// then backend_solve) as one pipelined call: Device::refactorize_solve. X is only meaningful when *info == 0.
static int32_t refactorize_solve_impl(gmrfx_handle *h, const double *nz, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx,
                                      int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (!nz) throw std::invalid_argument("nzval is null");
        check_rhs(h, B, ldb, X, ldx, nrhs, "B/X");
        h->D->refactorize_solve(nz, dev, B, ldb, nrhs, X, ldx, dev);
        return pivot_status(h, info);
    });
}
extern "C" int32_t gmrfx_refactorize_solve(gmrfx_handle *h, const double *nzval, const double *B, int64_t ldb, int64_t nrhs, double *X,
                                           int64_t ldx, int64_t *info) { return refactorize_solve_impl(h, nzval, B, ldb, nrhs, X, ldx, info, false); }
extern "C" int32_t gmrfx_refactorize_solve_dev(gmrfx_handle *h, const double *d_nzval, const double *d_B, int64_t ldb, int64_t nrhs, double *d_X,
                                               int64_t ldx, int64_t *info) { return refactorize_solve_impl(h, d_nzval, d_B, ldb, nrhs, d_X, ldx, info, true); }

// ---- Newton loop on the device -----------------------------------------------------------
extern "C" int32_t gmrfx_set_prior(gmrfx_handle *h, const double *prior_nzval, const int64_t *map, int64_t cnt, int32_t index_base) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (!prior_nzval || (cnt > 0 && !map) || cnt < 0) throw std::invalid_argument("prior_nzval / map is null");
        std::vector<long long> m((size_t)cnt);
        for (int64_t k = 0; k < cnt; k++) m[k] = map[k] - index_base;
        h->D->set_prior(prior_nzval, m.data(), cnt);
        return GMRFX_OK;
    });
}
static int32_t refactorize_update_impl(gmrfx_handle *h, const double *hv, int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        h->D->refactorize_update(hv, dev);
        return pivot_status(h, info);
    });
}
// One logpdf evaluation of the hyper-parameter loop in one call (Device::refactorize_logpdf): device pointers.
extern "C" int32_t gmrfx_refactorize_logpdf_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t nvec,
                                                const double *d_mu, double *quad, double *logdet, int64_t *info) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (!d_nzval) throw std::invalid_argument("nzval is null");
        if (nvec > 0 && (!d_X || !quad)) throw std::invalid_argument("X / quad is null");
        h->D->refactorize_logpdf(d_nzval, d_X, ldx, nvec, d_mu, quad, logdet);
        return pivot_status(h, info);
    });
}
// One Newton iterate in one pipelined call (Device::refactorize_update_solve): Hessian values in, new mean's solve out.
static int32_t refactorize_update_solve_impl(gmrfx_handle *h, const double *hv, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx,
                                             int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        check_rhs(h, B, ldb, X, ldx, nrhs, "B/X");
        h->D->refactorize_update_solve(hv, dev, B, ldb, nrhs, X, ldx, dev);
        return pivot_status(h, info);
    });
}
extern "C" int32_t gmrfx_refactorize_update_solve(gmrfx_handle *h, const double *hvals, const double *B, int64_t ldb, int64_t nrhs, double *X,
                                                  int64_t ldx, int64_t *info) { return refactorize_update_solve_impl(h, hvals, B, ldb, nrhs, X, ldx, info, false); }
extern "C" int32_t gmrfx_refactorize_update_solve_dev(gmrfx_handle *h, const double *d_hvals, const double *d_B, int64_t ldb, int64_t nrhs,
                                                      double *d_X, int64_t ldx, int64_t *info) { return refactorize_update_solve_impl(h, d_hvals, d_B, ldb, nrhs, d_X, ldx, info, true); }
extern "C" int32_t gmrfx_refactorize_update(gmrfx_handle *h, const double *hvals, int64_t *info) { return refactorize_update_impl(h, hvals, info, false); }
extern "C" int32_t gmrfx_refactorize_update_dev(gmrfx_handle *h, const double *d_hvals, int64_t *info) { return refactorize_update_impl(h, d_hvals, info, true); }

static int32_t solve_impl(gmrfx_handle *h, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx, bool dev, int mode) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        check_rhs(h, B, ldb, X, ldx, nrhs, "B/X");
        if (nrhs == 0) return GMRFX_OK;
        h->D->solve(B, ldb, nrhs, X, ldx, dev, mode);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_solve(gmrfx_handle *h, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx) { return solve_impl(h, B, ldb, nrhs, X, ldx, false, 0); }
extern "C" int32_t gmrfx_solve_dev(gmrfx_handle *h, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx) { return solve_impl(h, B, ldb, nrhs, X, ldx, true, 0); }
extern "C" int32_t gmrfx_backward_solve(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t nrhs, double *X, int64_t ldx) { return solve_impl(h, Z, ldz, nrhs, X, ldx, false, 1); }
extern "C" int32_t gmrfx_backward_solve_dev(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t nrhs, double *X, int64_t ldx) { return solve_impl(h, Z, ldz, nrhs, X, ldx, true, 1); }

extern "C" int32_t gmrfx_logdet(gmrfx_handle *h, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        if (!out) throw std::invalid_argument("out is null");
        *out = h->D->logdet();
        return GMRFX_OK;
    });
}

static int32_t quadform_impl(gmrfx_handle *h, const double *nz, const double *X, int64_t ldx, int64_t nvec,
                             const double *mu, double *out, bool dev) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (nvec < 0 || (nvec > 0 && (!X || !out))) { h->err = "quadform: null X/out or negative nvec"; return GMRFX_ERR_INVALID_ARG; }
        if (nvec == 0) return GMRFX_OK;
        if (ldx < h->S.n) { h->err = "quadform: ldx < n"; return GMRFX_ERR_INVALID_ARG; }
        if (dev) { h->D->quadform(nz, X, ldx, nvec, mu, out); return GMRFX_OK; }
        const i64 n = h->S.n;
        DevBlock bx, bm, bn;
        stage_up(h, bx, X, ldx, n, nvec);
        if (mu) stage_up(h, bm, mu, n);
        if (nz) stage_up(h, bn, nz, h->S.nnz_in);
        h->D->quadform(bn, bx, n, nvec, bm, out);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_quadform(gmrfx_handle *h, const double *nzval, const double *X, int64_t ldx, int64_t nvec,
                                  const double *mu, double *out) {
    return quadform_impl(h, nzval, X, ldx, nvec, mu, out, false);
}
extern "C" int32_t gmrfx_quadform_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t nvec,
                                      const double *d_mu, double *out) {
    return quadform_impl(h, d_nzval, d_X, ldx, nvec, d_mu, out, true);
}

// ---- dense-operator leg of the separable (Kronecker) path, SURVEY 8 f3 (separable.jl:122-172) -------------
extern "C" int32_t gmrfx_dense_apply_dev(gmrfx_handle *h, int64_t n1, int64_t n2, const double *d_D, const double *d_T, double *d_R) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (n1 < 0 || n2 < 0 || n1 > 0x7fffffffLL) throw std::invalid_argument("dense_apply: bad dimensions");
        if (n1 > 0 && n2 > 0 && (!d_D || !d_T || !d_R)) throw std::invalid_argument("dense_apply: null pointer");
        if (d_T == d_R) throw std::invalid_argument("dense_apply: T and R must not alias");
        if (n1 > 0 && n2 > 0 && (n2 + 63) / 64 * ((n1 + 63) / 64) > 0x0fffffffLL) throw std::invalid_argument("dense_apply: too many tiles");
        h->D->dense_apply(d_D, d_T, d_R, n1, n2);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_transpose_dev(gmrfx_handle *h, int64_t rows, int64_t cols, const double *d_src, double *d_dst) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (rows < 0 || cols < 0) throw std::invalid_argument("transpose: bad dimensions");
        if (rows > 0 && cols > 0 && (!d_src || !d_dst || d_src == d_dst)) throw std::invalid_argument("transpose: null or aliased pointers");
        if (((rows + 63) >> 6) * ((cols + 63) >> 6) > 0x7fffffffLL) throw std::invalid_argument("transpose: too many tiles");
        h->D->transpose(d_src, d_dst, rows, cols);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_get_perm(const gmrfx_handle *h, int32_t base, int64_t *perm) {
    if (!h || !perm) return GMRFX_ERR_INVALID_ARG;
    for (i64 k = 0; k < h->S.n; k++) perm[k] = (i64)h->S.perm[k] + base;
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_get_stats(const gmrfx_handle *h, gmrfx_stats *out, int32_t struct_size) {
    if (!h || !out || struct_size <= 0) return GMRFX_ERR_INVALID_ARG;
    gmrfx_stats st;
    std::memset(&st, 0, sizeof(st));
    const Symbolic &S = h->S;
    st.n = S.n; st.nnz_q_tri = S.nnz_q_tri; st.nnz_l = S.nnz_l_true; st.nnz_l_stored = S.nnz_l_stored;
    st.nsuper = S.nsuper; st.nlevels = S.nlevels; st.max_cols = S.max_cols; st.max_rows = S.max_rows;
    st.sum_rows = S.sum_rows; st.n_small_fronts = S.n_small; st.n_big_fronts = S.n_big;
    st.factor_flops = S.flops;
    st.bytes_factor = 8.0 * (double)S.panelptr[S.nsuper];
    st.bytes_cb_arena = 8.0 * (double)S.cb_arena;
    st.ms_symbolic = S.ms_symbolic;
    st.fail_col = -1;
    if (h->D) {
        Device &D = *h->D;       // (the handle is const, its device state is not: syrk_ms / fail_col read their events lazily)
        st.bytes_device_total = D.bytes_total;
        st.ms_factor = D.ms_factor; st.ms_solve = D.ms_solve; st.ms_solve_fwd = D.ms_fwd; st.ms_solve_bwd = D.ms_bwd;
        st.ms_solve_perm = D.ms_perm; st.ms_backward_solve = D.ms_bsolve; st.ms_logdet = D.ms_logdet; st.ms_selinv = D.ms_selinv;
        st.last_nrhs = D.last_nrhs;
        st.ms_syrk = D.syrk_ms(); st.syrk_flops = D.syrk_flops; st.syrk_launches = D.syrk_launches;
        st.ms_quadform = D.ms_quadform;
        st.inv_cap = D.inv_cap();
        st.ms_inv_decide = D.ms_inv_decide;
        st.ms_rbmc = D.ms_rbmc;
        if (D.factorized) st.fail_col = D.fail_col();
    }
    std::memcpy(out, &st, std::min<size_t>((size_t)struct_size, sizeof(st)));
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_get_factor_values(gmrfx_handle *h, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, true)) return e;
        if (!out) throw std::invalid_argument("out is null");
        h->D->copy_factor(out);
        return GMRFX_OK;
    });
}

// Profiling aid (handles created with GMRFX_LEVEL_MARK=1): HIP-event time of every tree level of the most recent
// factorisation (which = 0), forward (1) or backward (2) sweep. ms[0] = the sweep tasks, ms[1 + l] = level l.
extern "C" int32_t gmrfx_level_times(gmrfx_handle *h, int32_t which, double *ms, int64_t cap, int64_t *count) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        if (!ms || !count) throw std::invalid_argument("null output");
        *count = h->D->level_times(which, ms, (int)cap);
        return GMRFX_OK;
    });
}
// The slicing of host_upload (download = 0) / host_download (1) for an n x nrhs array: plan = {columns per slice, row pieces per
// column, rows per piece, doubles per ring slot, slices, doubles reserved}. No handle, no device: arithmetic only.
extern "C" int32_t gmrfx_host_io_plan(int64_t n, int64_t nrhs, int32_t download, int64_t *plan) {
    if (!plan || n < 0 || nrhs < 0) return GMRFX_ERR_INVALID_ARG;
    const HostIoPlan p = host_io_plan_dir(n, nrhs, download);
    plan[0] = p.cols_per; plan[1] = p.ppc; plan[2] = p.rows_per; plan[3] = p.slot_doubles; plan[4] = p.nsl; plan[5] = p.reserve;
    return GMRFX_OK;
}
extern "C" int32_t gmrfx_set_stream(gmrfx_handle *h, void *hip_stream, int32_t use_external, int32_t async_phases) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_device(h, false)) return e;
        h->D->set_external_stream((hipStream_t)hip_stream, use_external != 0, async_phases != 0);
        return GMRFX_OK;
    });
}
extern "C" void *gmrfx_device_ptr(gmrfx_handle *h, int32_t which) {
    if (!h || !h->D) return nullptr;
    try {
        if (which == 2 || which == 3) h->D->ensure_rhs(64);
    } catch (...) { return nullptr; }
    switch (which) {
        case 0: return h->D->cb_arena();
        case 1: return h->D->factor_panels();
        case 2: return h->D->rhs_x();
        case 3: return h->D->rhs_w();
        default: return nullptr;
    }
}
