// api_kl_rbmc.cpp -- the C ABI of include/gmrfx.h: the KL (Vecchia-type) sparse approximate Cholesky and the RBMC marginal variances.
#include "api_common.h"
#include "kernels.h"

extern "C" int32_t gmrfx_kl_cholesky(int64_t n, const double *theta, int64_t ldt, int32_t theta_on_device,
                                     const int64_t *L_colptr, int64_t ntasks, const int64_t *task_rowptr,
                                     const int64_t *task_rows, const int64_t *task_colptr, const int64_t *task_cols,
                                     int32_t base, double reg, int32_t device, double *nzval, int64_t *info) {
    if (info) *info = 0;
    return create_guarded(false, [&]() -> int32_t {
        if (n <= 0 || !theta || ldt < n || !L_colptr || !nzval) throw std::invalid_argument("kl_cholesky: null argument / ldt < n");
        if (ntasks < 0 || (ntasks > 0 && (!task_rowptr || !task_rows || !task_colptr || !task_cols)))
            throw std::invalid_argument("kl_cholesky: null task arrays");
        check_index_base(base);
        if (n > 0x7fffffffLL || ntasks > 0x7fffffffLL) throw std::invalid_argument("kl_cholesky: too large");
        std::vector<long long> colptr((size_t)n + 1);
        for (i64 j = 0; j <= n; j++) colptr[j] = L_colptr[j] - base;
        for (i64 j = 0; j < n; j++) if (colptr[j + 1] < colptr[j]) throw std::invalid_argument("L_colptr not monotone");
        const i64 nnzL = colptr[n];
        std::vector<KlTask> tasks((size_t)ntasks);
        const i64 nr = ntasks ? task_rowptr[ntasks] - base : 0, nc = ntasks ? task_colptr[ntasks] - base : 0;
        std::vector<int> rows((size_t)nr), cols((size_t)nc);
        for (i64 k = 0; k < nr; k++) {
            const i64 v = task_rows[k] - base;
            if (v < 0 || v >= n) throw std::invalid_argument("task_rows out of range");
            rows[k] = (int)v;
        }
        for (i64 k = 0; k < nc; k++) {
            const i64 v = task_cols[k] - base;
            if (v < 0 || v >= n) throw std::invalid_argument("task_cols out of range");
            cols[k] = (int)v;
        }
        for (i64 t = 0; t < ntasks; t++) {
            KlTask &tk = tasks[t];
            tk.rows_off = task_rowptr[t] - base; tk.cols_off = task_colptr[t] - base;
            const i64 a = task_rowptr[t + 1] - task_rowptr[t], b = task_colptr[t + 1] - task_colptr[t];
            if (a <= 0 || b < 0) throw std::invalid_argument("kl_cholesky: empty task");
            tk.nrows = (int)a; tk.ncols = (int)b;
            for (i64 q = 0; q < b; q++) {
                const int col = cols[tk.cols_off + q];
                const i64 nk = colptr[col + 1] - colptr[col];
                if (nk < 1 || nk > a) throw std::invalid_argument("kl_cholesky: a column has more entries than its task has rows");
            }
        }
        const long long bad = kl_cholesky_run(device, n, theta, ldt, theta_on_device != 0, tasks, rows, cols, colptr.data(), nnzL, reg, nzval);
        if (bad >= 0) {
            if (info) *info = bad + 1;
            g_create_err = "kl_cholesky: local covariance block of task " + std::to_string(bad) + " is not positive definite";
            return GMRFX_ERR_NOT_POSDEF;
        }
        return GMRFX_OK;
    });
}

// ---- Rao-Blackwellised Monte Carlo marginal variances (include/gmrfx.h; csrc/rbmc_plan.cpp, Device::rbmc_var, csrc/rbmc.hip) --------
static const RbmcPlan &rbmc_plan_for(gmrfx_handle *h, int32_t enclosure_size) {
    if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
    if (h->rplan.enclosure != enclosure_size) rbmc_build_plan(h->rsym, h->S.n, enclosure_size, h->rplan);     // (unchanged when it throws)
    return h->rplan;
}

extern "C" int32_t gmrfx_rbmc_plan(gmrfx_handle *h, int32_t enclosure_size, int32_t index_base, int64_t *counts, int64_t *block_ptr,
                                   int64_t *rows, int64_t *n_interior, int64_t *owner) {
    return guarded(h, [&]() -> int32_t {
        if (!counts) throw std::invalid_argument("rbmc_plan: counts is null");
        if (enclosure_size < 0) throw std::invalid_argument("rbmc_plan: enclosure_size < 0 (the plain estimator has no blocks)");
        check_index_base(index_base, "rbmc_plan: ");
        check_unsharded(h, "rbmc_plan: sharded handles are not supported");
        const RbmcPlan &P = rbmc_plan_for(h, enclosure_size);
        const i64 nb = P.nblocks(), tot = P.block_ptr[nb];
        counts[0] = nb; counts[1] = tot; counts[2] = P.max_block;
        if (block_ptr) for (i64 b = 0; b <= nb; b++) block_ptr[b] = P.block_ptr[b];
        if (rows) for (i64 r = 0; r < tot; r++) rows[r] = (i64)P.rows[r] + index_base;
        if (n_interior) for (i64 b = 0; b < nb; b++) n_interior[b] = P.n_interior[b];
        if (owner) for (i64 r = 0; r < tot; r++) owner[r] = P.owner[r];
        return GMRFX_OK;
    });
}

static int32_t rbmc_var_impl(gmrfx_handle *h, const double *nz, const double *Z, int64_t ldz, int64_t nsamples, int32_t enclosure_size,
                             double *out, bool dev) {
    return guarded(h, [&]() -> int32_t {
        if (!Z || !out) throw std::invalid_argument("rbmc_var: Z/out is null");
        if (nsamples < 2) throw std::invalid_argument("rbmc_var: nsamples < 2 (the corrected sample variance needs two samples)");
        if (ldz < h->S.n) throw std::invalid_argument("rbmc_var: ldz < n");
        if (enclosure_size < -1) throw std::invalid_argument("rbmc_var: enclosure_size < -1");
        check_unsharded(h, "rbmc_var: sharded handles are not supported");
        if (h->con.m > 0 || h->bcon.m > 0) throw std::invalid_argument("rbmc_var: the handle holds a constraint set; the constrained estimator is not implemented");
        if (int32_t e = need_device(h, true)) return e;
        const long long fc = h->D->fail_col();
        if (fc >= 0) {
            h->err = "rbmc_var: the last factorisation failed (non-positive pivot at elimination step " + std::to_string(fc + 1) + ")";
            return GMRFX_ERR_NOT_POSDEF;
        }
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        const RbmcPlan *plan = enclosure_size >= 0 ? &rbmc_plan_for(h, enclosure_size) : nullptr;
        if (dev) { h->D->rbmc_var(h->rsym, plan, nz, Z, ldz, true, nsamples, out, true); return GMRFX_OK; }
        DevBlock bn;
        if (nz) stage_up(h, bn, nz, h->S.nnz_in);
        h->D->rbmc_var(h->rsym, plan, bn, Z, ldz, false, nsamples, out, false);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_rbmc_var(gmrfx_handle *h, const double *nzval, const double *Z, int64_t ldz, int64_t nsamples, int32_t enclosure_size,
                                  double *out) {
    return rbmc_var_impl(h, nzval, Z, ldz, nsamples, enclosure_size, out, false);
}
extern "C" int32_t gmrfx_rbmc_var_dev(gmrfx_handle *h, const double *d_nzval, const double *d_Z, int64_t ldz, int64_t nsamples,
                                      int32_t enclosure_size, double *d_out) {
    return rbmc_var_impl(h, d_nzval, d_Z, ldz, nsamples, enclosure_size, d_out, true);
}
