// api_fisher.cpp -- the C ABI of include/gmrfx.h: the observation likelihood as state of a plain handle and the fused evaluation of a
// Fisher-scoring iterate (Device::obs_set, Device::fisher_eval; csrc/fisher.hip).
#include <cmath>

#include "api_obs.h"

extern "C" int32_t gmrfx_obs_set(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *indices, int32_t index_base, const double *y,
                                 const double *aux, double param) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "obs_set: ";
        obs_check_handle(h, who);
        const int64_t n = h->S.n;
        if (nobs == 0) {        // removes the likelihood, of either form
            if (h->D) h->D->obs_set(ObsHost{});
            h->obs = ObsHost{};
            return GMRFX_OK;
        }
        obs_check_family(who, family);
        if (nobs < 0 || nobs > n) throw std::invalid_argument("obs_set: nobs outside [0, n]");
        check_index_base(index_base, "obs_set: ");
        if (!indices && nobs != n) throw std::invalid_argument("obs_set: indices is null and nobs != n");
        obs_check_operands(who, family, y, aux, param);
        ObsHost o;
        o.idx.resize((size_t)nobs);
        std::vector<unsigned char> seen((size_t)n, 0);
        for (int64_t k = 0; k < nobs; k++) {
            const int64_t i = indices ? indices[k] - index_base : k;
            if (i < 0 || i >= n) throw std::invalid_argument("obs_set: index " + std::to_string(k) + " is outside the range");
            if (seen[(size_t)i]) throw std::invalid_argument("obs_set: node " + std::to_string(i + index_base) + " is observed twice");
            seen[(size_t)i] = 1;
            o.idx[(size_t)k] = i;
        }
        obs_fill_values(o, who, family, nobs, y, aux, param);
        if (h->D) h->D->obs_set(o);
        h->obs = std::move(o);
        return GMRFX_OK;
    });
}

// The likelihood observed through eta = A x + b (A: nobs x n, CSC). The host analysis (fisher_design_plan.cpp) validates A and b and
// builds the Hessian's positions and term lists; the plan replaces a node-form likelihood and the other way round.
extern "C" int32_t gmrfx_obs_set_design(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *colptr, const int64_t *rowval,
                                        const double *nzval, int32_t index_base, const double *offset, const double *y, const double *aux,
                                        double param) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "obs_set_design: ";
        obs_check_handle(h, who);
        const int64_t n = h->S.n;
        obs_check_family(who, family);
        if (nobs <= 0) throw std::invalid_argument(who + "nobs must be positive (gmrfx_obs_set with nobs = 0 removes the likelihood)");
        check_index_base(index_base, who.c_str());
        if (!colptr) throw std::invalid_argument(who + "colptr is null");
        check_compressed_ptr(colptr, n, index_base, "obs_set_design: colptr");
        design_check_sizes(n, nobs, colptr[n] - index_base);        // (before y, aux or A are read at those lengths)
        if (colptr[n] > index_base && (!rowval || !nzval)) throw std::invalid_argument(who + "rowval / nzval is null");
        obs_check_operands(who, family, y, aux, param);
        ObsHost o;
        obs_fill_values(o, who, family, nobs, y, aux, param);
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        auto plan = std::make_shared<DesignPlan>();
        design_build_plan(h->rsym, n, h->S.nnz_in, nobs, colptr, rowval, nzval, index_base, offset, *plan);
        o.design = std::move(plan);
        if (h->D) h->D->obs_set(o);
        h->obs = std::move(o);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_obs_hess_map(const gmrfx_handle *h, int64_t *cnt, int64_t *map) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    return guarded(const_cast<gmrfx_handle *>(h), [&]() -> int32_t {
        if (!h->obs.design) throw std::invalid_argument("obs_hess_map: no design likelihood is set (gmrfx_obs_set_design)");
        const DesignPlan &P = *h->obs.design;
        if (cnt) *cnt = P.cnt;
        if (map) std::copy(P.map.begin(), P.map.end(), map);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_obs_design_info(const gmrfx_handle *h, int64_t *nnz_a, int64_t *cnt, int64_t *terms) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    const DesignPlan *P = h->obs.design.get();
    if (nnz_a) *nnz_a = P ? P->nnz : -1;
    if (cnt) *cnt = P ? P->cnt : -1;
    if (terms) *terms = P ? P->terms : -1;
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_obs_info(const gmrfx_handle *h, int32_t *family, int64_t *nobs, double *loglik_const) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    if (family) *family = h->obs.nobs > 0 ? h->obs.family : -1;
    if (nobs) *nobs = h->obs.nobs;
    if (loglik_const) *loglik_const = h->obs.loglik_const;
    return GMRFX_OK;
}

// entries of the Hessian vector: n in node form, the map's cnt in design form
static int64_t obs_hess_len(const gmrfx_handle *h) { return h->obs.design ? h->obs.design->cnt : h->S.n; }

// ---- score, hess, energy and loglik at a point, one pass over Symmetric(Q_prior) (Device::fisher_eval) --------------------------------
// The per-iterate host work of the reference's loop (src/workspace/gaussian_approximation.jl:191-313: neg_score_k = Q_p x - h - loggrad,
// loghessian, and the line search's merit = energy - loglik, src/arithmetic/condition/gaussian_approximation.jl:231-409).
static int32_t fisher_eval_impl(gmrfx_handle *h, const double *x, const double *mu, double *score, double *hess, double *out, bool dev) {
    return guarded(h, [&]() -> int32_t {
        check_unsharded(h, "fisher_eval: sharded handles are not supported");
        if (h->nbatch > 1) throw std::invalid_argument("fisher_eval: batched handles are not supported");
        if (!x) throw std::invalid_argument("fisher_eval: x is null");
        if (!out) throw std::invalid_argument("fisher_eval: out is null");
        if (h->obs.nobs == 0) throw std::invalid_argument("fisher_eval: no observation likelihood is set (gmrfx_obs_set)");
        if (int32_t e = need_device(h, false)) return e;
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        double res[2] = {0.0, 0.0};
        if (dev) h->D->fisher_eval(h->rsym, x, mu, score, hess, res);
        else {
            const int64_t n = h->S.n, hl = obs_hess_len(h);
            DevBlock bx, bm, bs, bh;
            stage_up(h, bx, x, n);
            if (mu) stage_up(h, bm, mu, n);
            if (score) stage_alloc(h, bs, n);
            if (hess) stage_alloc(h, bh, hl);
            h->D->fisher_eval(h->rsym, bx, mu ? bm.get() : nullptr, score ? bs.get() : nullptr, hess ? bh.get() : nullptr, res);
            if (score) stage_down(h, bs, score, n, n, 1);
            if (hess && hl > 0) stage_down(h, bh, hess, hl, hl, 1);
        }
        out[0] = res[0];
        out[1] = res[1];
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_fisher_eval(gmrfx_handle *h, const double *x, const double *mu, double *score, double *hess, double *out) {
    return fisher_eval_impl(h, x, mu, score, hess, out, false);
}
extern "C" int32_t gmrfx_fisher_eval_dev(gmrfx_handle *h, const double *d_x, const double *d_mu, double *d_score, double *d_hess, double *out) {
    return fisher_eval_impl(h, d_x, d_mu, d_score, d_hess, out, true);
}

// ---- the loop (Device::gaussian_approximation): _workspace_newton_loop, src/workspace/gaussian_approximation.jl:230-313 -------------
static int32_t ga_impl(gmrfx_handle *h, const double *mu, const double *x0, int64_t max_iter, int64_t max_ls, double mean_tol, double dec_tol,
                       int32_t flags, double *x, double *hess, double *result, double *dec_trace, double *alpha_trace, int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        check_unsharded(h, "gaussian_approximation: sharded handles are not supported");
        if (h->nbatch > 1) throw std::invalid_argument("gaussian_approximation: batched handles are not supported");
        if (!x || !result) throw std::invalid_argument("gaussian_approximation: x / result is null");
        if (max_iter < 0 || max_ls < 0) throw std::invalid_argument("gaussian_approximation: max_iter / max_linesearch_iter is negative");
        if (flags < 0 || flags > 15) throw std::invalid_argument("gaussian_approximation: unknown flag bits");
        if (h->obs.nobs == 0) throw std::invalid_argument("gaussian_approximation: no observation likelihood is set (gmrfx_obs_set)");
        if (int32_t e = need_device(h, false)) return e;
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        const Device::GaOpts o{max_iter, max_ls, mean_tol, dec_tol, flags};
        long long inf = 0;
        int rc;
        if (dev) rc = h->D->gaussian_approximation(h->rsym, mu, x0, o, x, hess, result, dec_trace, alpha_trace, &inf);
        else {
            const int64_t n = h->S.n, hl = obs_hess_len(h);
            DevBlock bm, b0, bx, bh;
            if (mu) stage_up(h, bm, mu, n);
            if (x0) stage_up(h, b0, x0, n);
            stage_alloc(h, bx, n);
            if (hess) stage_alloc(h, bh, hl);
            rc = h->D->gaussian_approximation(h->rsym, mu ? bm.get() : nullptr, x0 ? b0.get() : nullptr, o, bx, hess ? bh.get() : nullptr, result,
                                              dec_trace, alpha_trace, &inf);
            stage_down(h, bx, x, n, n, 1);
            if (hess && rc == 0 && hl > 0) stage_down(h, bh, hess, hl, hl, 1);
        }
        if (info) *info = inf;
        if (rc == 1) {
            h->err = "gaussian_approximation: Q_prior - H is not positive definite (non-positive pivot at elimination step " + std::to_string(inf) + ")";
            return GMRFX_ERR_NOT_POSDEF;
        }
        if (rc == 2) {
            h->err = "gaussian_approximation: A Q^-1 A' is not positive definite (rank-deficient constraint matrix)";
            return GMRFX_ERR_NOT_POSDEF;
        }
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_gaussian_approximation(gmrfx_handle *h, const double *mu, const double *x0, int64_t max_iter, int64_t max_linesearch_iter,
                                                double mean_change_tol, double newton_dec_tol, int32_t flags, double *x, double *hess, double *result,
                                                double *dec_trace, double *alpha_trace, int64_t *info) {
    return ga_impl(h, mu, x0, max_iter, max_linesearch_iter, mean_change_tol, newton_dec_tol, flags, x, hess, result, dec_trace, alpha_trace, info, false);
}
extern "C" int32_t gmrfx_gaussian_approximation_dev(gmrfx_handle *h, const double *d_mu, const double *d_x0, int64_t max_iter,
                                                    int64_t max_linesearch_iter, double mean_change_tol, double newton_dec_tol, int32_t flags,
                                                    double *d_x, double *d_hess, double *result, double *dec_trace, double *alpha_trace, int64_t *info) {
    return ga_impl(h, d_mu, d_x0, max_iter, max_linesearch_iter, mean_change_tol, newton_dec_tol, flags, d_x, d_hess, result, dec_trace, alpha_trace, info, true);
}
