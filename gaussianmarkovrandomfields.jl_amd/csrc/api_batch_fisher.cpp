// api_batch_fisher.cpp -- the C ABI of include/gmrfx.h: Fisher scoring and the Gaussian approximation for every member of a batched
// handle (Device::bobs_set, Device::batch_fisher_eval, Device::batch_gaussian_approximation; csrc/fisher.hip, csrc/fisher_design.hip),
// in node form (gmrfx_batch_obs_set) or through a design matrix (gmrfx_batch_obs_set_design). A plain handle is a batch of one to
// these calls, as to every gmrfx_batch_* call; gmrfx_obs_set and its family keep refusing batched handles.
#include "api_obs.h"

// what every call here refuses about the handle itself, before anything else is looked at
// (bcon_ok: the calls that work with a batch constraint held -- the prior's values and the constrained loop; a plain constraint
// stays refused everywhere. The unconstrained loop and the evaluation refuse both: they would silently ignore the constraint.)
static void bf_check_handle(const gmrfx_handle *h, const std::string &who, bool bcon_ok = false) {
    check_unsharded(h, (who + "sharded handles are not supported").c_str());
    if (h->nbatch > kBatchFisherMaxMembers) throw std::invalid_argument(who + "more than 65535 members");
    if (h->obs.design) throw std::invalid_argument(who + "the design form (eta = A x + b, gmrfx_obs_set_design) is not supported");
    if ((h->bcon.m > 0 && !bcon_ok) || h->con.m > 0) throw std::invalid_argument(who + "a constraint set is not supported (clear it first)");
}
// the member's sizes, on plain handles too
static int64_t bf_n(const gmrfx_handle *h) { return h->nbatch > 1 ? h->n_member : h->S.n; }
static int64_t bf_nnz(const gmrfx_handle *h) { return h->nbatch > 1 ? h->nnz_member : h->S.nnz_in; }
// entries of a member's Hessian vector: n in node form, the plan's cnt in design form
static int64_t bf_hess_len(const gmrfx_handle *h) { return h->bobs.design ? h->bobs.design->cnt : bf_n(h); }
// a plain handle's batch buffers, on its first batch call (need_batch without the NO_DEVICE answer: symbolic_only handles pass)
static void bf_ensure_batch(gmrfx_handle *h) {
    if (h->D && !h->D->batched()) h->D->set_batch(1, h->S.n, h->S.nnz_in);
}
static void bf_check_stride(const std::string &who, const char *what, int64_t s, int64_t n, bool zero_ok = false, const char *len = "n") {
    if (zero_ok && s == 0) return;
    if (s < n) throw std::invalid_argument(who + what + ": member stride smaller than " + len);
}

// nobs = 0 of either form: the batch likelihood is dropped, on the device and on the host
static int32_t bf_clear(gmrfx_handle *h) {
    if (h->D) h->D->bobs_set(h->rsym, BObsHost{});
    h->bobs = BObsHost{};
    return GMRFX_OK;
}
// Every check of gmrfx_obs_set (or gmrfx_obs_set_design) on the values, member by member, with the member's loglik_const in long double
// each; o (its family and nobs set) takes the parameters, the constants and the one data set.
static void bf_fill_members(BObsHost &o, const std::string &who, int64_t nb, const double *y, const double *aux, const double *param) {
    o.param.resize((size_t)nb); o.loglik_const.resize((size_t)nb);
    for (int64_t k = 0; k < nb; k++) {
        const std::string wk = who + "member " + std::to_string(k) + ": ";
        obs_check_operands(wk, o.family, y, aux, param[k]);
        ObsHost ok;
        obs_fill_values(ok, wk, o.family, o.nobs, y, aux, param[k]);
        o.param[(size_t)k] = param[k];
        o.loglik_const[(size_t)k] = ok.loglik_const;
        if (k == nb - 1) { o.y = std::move(ok.y); o.aux = std::move(ok.aux); }
    }
}

extern "C" int32_t gmrfx_batch_set_prior(gmrfx_handle *h, const double *prior_nzval) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_set_prior: ";
        bf_check_handle(h, who, true);
        if (!prior_nzval) throw std::invalid_argument(who + "prior_nzval is null");
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);       // (refuses a pattern without a stored diagonal)
        if (int32_t e = need_device(h, false)) return e;
        bf_ensure_batch(h);
        // the map of the likelihood in place, member after member: the forest's own diagonal positions (none, or the node form), or
        // the plan's positions in one member's values shifted by k nnz_member (design form)
        std::vector<long long> map;
        if (const DesignPlan *P = h->bobs.design.get()) {
            const int64_t nnz = bf_nnz(h);
            map.reserve((size_t)(P->cnt * h->nbatch));
            for (int64_t k = 0; k < h->nbatch; k++)
                for (i64 p : P->map) map.push_back(p + k * nnz);
        } else map.assign(h->rsym.diag.begin(), h->rsym.diag.end());
        h->D->bset_prior(prior_nzval, map, (bool)h->bobs.design);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_batch_obs_set(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *indices, int32_t index_base, const double *y,
                                       const double *aux, const double *param) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_obs_set: ";
        bf_check_handle(h, who);
        const int64_t n = bf_n(h), nb = h->nbatch;
        if (nobs == 0) return bf_clear(h);
        obs_check_family(who, family);
        if (nobs < 0 || nobs > n) throw std::invalid_argument(who + "nobs outside [0, n]");
        check_index_base(index_base, who.c_str());
        if (!indices && nobs != n) throw std::invalid_argument(who + "indices is null and nobs != n");
        if (!param) throw std::invalid_argument(who + "param is null (one value per member)");
        BObsHost o;
        o.idx.resize((size_t)nobs);
        std::vector<unsigned char> seen((size_t)n, 0);
        for (int64_t k = 0; k < nobs; k++) {
            const int64_t i = indices ? indices[k] - index_base : k;
            if (i < 0 || i >= n) throw std::invalid_argument(who + "index " + std::to_string(k) + " is outside the range");
            if (seen[(size_t)i]) throw std::invalid_argument(who + "node " + std::to_string(i + index_base) + " is observed twice");
            seen[(size_t)i] = 1;
            o.idx[(size_t)k] = i;
        }
        o.family = family; o.nobs = nobs;
        bf_fill_members(o, who, nb, y, aux, param);
        if (h->D) {
            bf_ensure_batch(h);
            if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
            h->D->bobs_set(h->rsym, o);
        }
        h->bobs = std::move(o);
        return GMRFX_OK;
    });
}

// The same likelihood observed through eta = A x + b (A: nobs x n_member, CSC): the checks of gmrfx_obs_set_design and, member by
// member, those of gmrfx_batch_obs_set; the plan (fisher_design_plan.cpp) is built on the MEMBER's pattern, which the forest's first
// n_member rows of Symmetric(Q) are. Either batch form replaces the other.
extern "C" int32_t gmrfx_batch_obs_set_design(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *colptr, const int64_t *rowval,
                                              const double *nzval, int32_t index_base, const double *offset, const double *y, const double *aux,
                                              const double *param) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_obs_set_design: ";
        bf_check_handle(h, who);
        const int64_t n = bf_n(h), nb = h->nbatch;
        if (nobs == 0) return bf_clear(h);
        obs_check_family(who, family);
        if (nobs < 0) throw std::invalid_argument(who + "nobs is negative");
        check_index_base(index_base, who.c_str());
        if (!colptr) throw std::invalid_argument(who + "colptr is null");
        check_compressed_ptr(colptr, n, index_base, "batch_obs_set_design: colptr");
        design_check_sizes(n, nobs, colptr[n] - index_base);        // (before y, aux or A are read at those lengths)
        if (colptr[n] > index_base && (!rowval || !nzval)) throw std::invalid_argument(who + "rowval / nzval is null");
        if (!param) throw std::invalid_argument(who + "param is null (one value per member)");
        BObsHost o;
        o.family = family; o.nobs = nobs;
        bf_fill_members(o, who, nb, y, aux, param);
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        auto plan = std::make_shared<DesignPlan>();
        design_build_plan(h->rsym, n, bf_nnz(h), nobs, colptr, rowval, nzval, index_base, offset, *plan);
        o.design = std::move(plan);
        if (h->D) {
            bf_ensure_batch(h);
            h->D->bobs_set(h->rsym, o);
        }
        h->bobs = std::move(o);
        return GMRFX_OK;
    });
}

// The members' parameters replaced in place, in node or design form: the validation of gmrfx_batch_obs_set on every param[k], loglik_const
// per member in long double from the data the handle keeps (read in place, validated when it was set). Nothing else of the likelihood changes (no data goes up, no plan is
// rebuilt), so it also works while a batch constraint is held.
extern "C" int32_t gmrfx_batch_obs_set_param(gmrfx_handle *h, const double *param) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_obs_set_param: ";
        if (h->bobs.nobs == 0) throw std::invalid_argument(who + "no observation likelihood is set (gmrfx_batch_obs_set)");
        if (!param) throw std::invalid_argument(who + "param is null (one value per member)");
        const int64_t nb = h->nbatch;
        const BObsHost &b = h->bobs;        // (its y and aux were validated when they were set: only the parameters are new)
        for (int64_t k = 0; k < nb; k++) obs_check_param(who + "member " + std::to_string(k) + ": ", b.family, param[k]);
        std::vector<double> p(param, param + nb), c((size_t)nb);
        for (int64_t k = 0; k < nb; k++) c[(size_t)k] = obs_loglik_const(b.family, b.nobs, b.y, b.aux, param[k]);
        if (h->D) h->D->bobs_set_param(p, c);
        h->bobs.param = std::move(p);
        h->bobs.loglik_const = std::move(c);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_batch_obs_hess_map(const gmrfx_handle *h, int64_t *map, int64_t cap, int64_t *cnt) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    return guarded(const_cast<gmrfx_handle *>(h), [&]() -> int32_t {
        const std::string who = "batch_obs_hess_map: ";
        if (!h->bobs.design) throw std::invalid_argument(who + "no design likelihood is set (gmrfx_batch_obs_set_design)");
        const DesignPlan &P = *h->bobs.design;
        if (cnt) *cnt = P.cnt;
        if (map) {
            if (cap < P.cnt) throw std::invalid_argument(who + "cap is smaller than cnt");
            std::copy(P.map.begin(), P.map.end(), map);
        }
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_batch_obs_design_info(const gmrfx_handle *h, int64_t *nnz_a, int64_t *cnt, int64_t *terms) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    const DesignPlan *P = h->bobs.design.get();
    if (nnz_a) *nnz_a = P ? P->nnz : -1;
    if (cnt) *cnt = P ? P->cnt : -1;
    if (terms) *terms = P ? P->terms : -1;
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_batch_obs_info(const gmrfx_handle *h, int32_t *family, int64_t *nobs, double *loglik_const) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    if (family) *family = h->bobs.nobs > 0 ? h->bobs.family : -1;
    if (nobs) *nobs = h->bobs.nobs;
    if (loglik_const)
        for (int64_t k = 0; k < h->nbatch; k++) loglik_const[k] = h->bobs.nobs > 0 ? h->bobs.loglik_const[(size_t)k] : 0.0;
    return GMRFX_OK;
}

static int32_t bf_eval_impl(gmrfx_handle *h, const double *x, int64_t sx, const double *mu, int64_t smu, const uint8_t *active, double *score,
                            double *hess, int64_t ss, double *out, bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_fisher_eval: ";
        bf_check_handle(h, who);
        if (!x) throw std::invalid_argument(who + "x is null");
        if (!out) throw std::invalid_argument(who + "out is null");
        const int64_t n = bf_n(h), nb = h->nbatch;
        bf_check_stride(who, "x", sx, n);
        if (mu) bf_check_stride(who, "mu", smu, n, true);
        const int64_t hl = bf_hess_len(h);
        if (score) bf_check_stride(who, "score", ss, n);
        if (hess) bf_check_stride(who, "hess", ss, hl, false, h->bobs.design ? "cnt" : "n");
        if (h->bobs.nobs == 0) throw std::invalid_argument(who + "no observation likelihood is set (gmrfx_batch_obs_set)");
        if (int32_t e = need_batch(h, false)) return e;
        if (dev) {
            h->D->batch_fisher_eval(Device::BEvalIO{x, sx, mu, smu, active, score, hess, ss, ss}, out);
            return GMRFX_OK;
        }
        DevBlock bx, bm, bs, bh;
        stage_up(h, bx, x, sx, n, 1, sx, nb);
        if (mu) stage_up(h, bm, mu, n, n, 1, smu, smu == 0 ? 1 : nb);
        // the outputs go up first: a member that is masked out keeps what the caller's arrays hold
        if (score) stage_up(h, bs, score, ss, n, 1, ss, nb);
        if (hess && hl > 0) stage_up(h, bh, hess, ss, hl, 1, ss, nb);       // (hl rows per member: n in node form, cnt in design form)
        h->D->batch_fisher_eval(Device::BEvalIO{bx, n, mu ? bm.get() : nullptr, smu == 0 ? 0 : n, active, score ? bs.get() : nullptr,
                                                hess ? bh.get() : nullptr, n, hl}, out);
        if (score) stage_down(h, bs, score, ss, n, 1, ss, nb);
        if (hess && hl > 0) stage_down(h, bh, hess, ss, hl, 1, ss, nb);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_fisher_eval(gmrfx_handle *h, const double *x, int64_t sx, const double *mu, int64_t smu, const uint8_t *active,
                                           double *score, double *hess, int64_t ss, double *out) {
    return bf_eval_impl(h, x, sx, mu, smu, active, score, hess, ss, out, false);
}
extern "C" int32_t gmrfx_batch_fisher_eval_dev(gmrfx_handle *h, const double *d_x, int64_t sx, const double *d_mu, int64_t smu,
                                               const uint8_t *active, double *d_score, double *d_hess, int64_t ss, double *out) {
    return bf_eval_impl(h, d_x, sx, d_mu, smu, active, d_score, d_hess, ss, out, true);
}

static int32_t bf_ga_impl(gmrfx_handle *h, const double *mu, int64_t smu, const double *x0, int64_t sx0, int64_t max_iter, int64_t max_ls,
                          double mean_tol, double dec_tol, int32_t flags, double *x, int64_t sx, double *hess, int64_t sh, double *result,
                          double *totals, double *dec_trace, double *alpha_trace, int64_t *info, bool dev, bool constrained = false,
                          int64_t *cinfo = nullptr, double *residual = nullptr) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = constrained ? "batch_constrained_gaussian_approximation: " : "batch_gaussian_approximation: ";
        if (constrained) {
            if (h->con.m > 0 && h->bcon.m == 0)
                throw std::invalid_argument(who + "the handle holds a plain constraint (gmrfx_constraints_set); set it with gmrfx_batch_constraints_set");
            if (h->bcon.m == 0) throw std::invalid_argument(who + "no batch constraint is held (gmrfx_batch_constraints_set); without one call gmrfx_batch_gaussian_approximation");
        }
        bf_check_handle(h, who, constrained);
        if (!x || !result) throw std::invalid_argument(who + "x / result is null");
        if (max_iter < 0 || max_ls < 0) throw std::invalid_argument(who + "max_iter / max_linesearch_iter is negative");
        if (flags < 0 || flags > 15) throw std::invalid_argument(who + "unknown flag bits");
        const int64_t n = bf_n(h), nb = h->nbatch;
        bf_check_stride(who, "x", sx, n);
        if (mu) bf_check_stride(who, "mu", smu, n, true);
        if (x0) bf_check_stride(who, "x0", sx0, n);
        const int64_t hl = bf_hess_len(h);
        if (hess) bf_check_stride(who, "hess", sh, hl, false, h->bobs.design ? "cnt" : "n");
        if (h->bobs.nobs == 0) throw std::invalid_argument(who + "no observation likelihood is set (gmrfx_batch_obs_set)");
        if (int32_t e = need_batch(h, false)) return e;
        const Device::GaOpts o{max_iter, max_ls, mean_tol, dec_tol, flags};
        std::vector<long long> inf((size_t)nb, 0), cin((size_t)nb, 0);
        int rc;
        if (dev) rc = h->D->batch_gaussian_approximation(Device::BGaIO{mu, smu, x0, sx0, x, sx, hess, sh}, o, result, totals, dec_trace, alpha_trace, inf.data(),
                                                         cin.data(), residual);
        else {
            DevBlock bm, b0, bx, bh;
            if (mu) stage_up(h, bm, mu, n, n, 1, smu, smu == 0 ? 1 : nb);
            if (x0) stage_up(h, b0, x0, n, n, 1, sx0, nb);
            stage_alloc(h, bx, n * nb);
            if (hess && hl > 0) stage_up(h, bh, hess, hl, hl, 1, sh, nb);      // (a failed member's slice keeps what the caller's array holds)
            rc = h->D->batch_gaussian_approximation(Device::BGaIO{mu ? bm.get() : nullptr, smu == 0 ? 0 : n, x0 ? b0.get() : nullptr, n, bx, n,
                                                                  hess ? bh.get() : nullptr, hl}, o, result, totals, dec_trace, alpha_trace, inf.data(),
                                                     cin.data(), residual);
            stage_down(h, bx, x, n, n, 1, sx, nb);
            if (hess && hl > 0) stage_down(h, bh, hess, hl, hl, 1, sh, nb);
        }
        if (info) std::copy(inf.begin(), inf.end(), info);
        if (cinfo) std::copy(cin.begin(), cin.end(), cinfo);
        if (rc & 2) {
            int64_t k = 0;
            while (k < nb && cin[(size_t)k] <= 0) k++;
            h->err = who + "A Q^-1 A' of member " + std::to_string(k) + " is not positive definite (rank-deficient constraint matrix)";
            return GMRFX_ERR_NOT_POSDEF;
        }
        if (rc == 1) {
            int64_t k = 0;
            while (k < nb && inf[(size_t)k] == 0) k++;
            h->err = who + "member " + std::to_string(k) + ": Q_prior - H is not positive definite (non-positive pivot at elimination step " +
                     std::to_string(k < nb ? inf[(size_t)k] : 0) + ")";
            return GMRFX_ERR_NOT_POSDEF;
        }
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_gaussian_approximation(gmrfx_handle *h, const double *mu, int64_t smu, const double *x0, int64_t sx0, int64_t max_iter,
                                                      int64_t max_linesearch_iter, double mean_change_tol, double newton_dec_tol, int32_t flags,
                                                      double *x, int64_t sx, double *hess, int64_t sh, double *result, double *totals,
                                                      double *dec_trace, double *alpha_trace, int64_t *info) {
    return bf_ga_impl(h, mu, smu, x0, sx0, max_iter, max_linesearch_iter, mean_change_tol, newton_dec_tol, flags, x, sx, hess, sh, result, totals,
                      dec_trace, alpha_trace, info, false);
}
extern "C" int32_t gmrfx_batch_gaussian_approximation_dev(gmrfx_handle *h, const double *d_mu, int64_t smu, const double *d_x0, int64_t sx0,
                                                          int64_t max_iter, int64_t max_linesearch_iter, double mean_change_tol,
                                                          double newton_dec_tol, int32_t flags, double *d_x, int64_t sx, double *d_hess, int64_t sh,
                                                          double *result, double *totals, double *dec_trace, double *alpha_trace, int64_t *info) {
    return bf_ga_impl(h, d_mu, smu, d_x0, sx0, max_iter, max_linesearch_iter, mean_change_tol, newton_dec_tol, flags, d_x, sx, d_hess, sh, result,
                      totals, dec_trace, alpha_trace, info, true);
}

// With a batch constraint held (gmrfx_batch_constraints_set): the same loop with every step projected onto A s = 0, as the plain loop
// does under gmrfx_constraints_set. Entry points of their own: the unconstrained calls keep refusing such a handle.
extern "C" int32_t gmrfx_batch_constrained_gaussian_approximation(gmrfx_handle *h, const double *mu, int64_t smu, const double *x0, int64_t sx0,
                                                                  int64_t max_iter, int64_t max_linesearch_iter, double mean_change_tol,
                                                                  double newton_dec_tol, int32_t flags, double *x, int64_t sx, double *hess, int64_t sh,
                                                                  double *result, double *totals, double *dec_trace, double *alpha_trace, int64_t *info,
                                                                  int64_t *cinfo, double *residual) {
    return bf_ga_impl(h, mu, smu, x0, sx0, max_iter, max_linesearch_iter, mean_change_tol, newton_dec_tol, flags, x, sx, hess, sh, result, totals,
                      dec_trace, alpha_trace, info, false, true, cinfo, residual);
}
extern "C" int32_t gmrfx_batch_constrained_gaussian_approximation_dev(gmrfx_handle *h, const double *d_mu, int64_t smu, const double *d_x0, int64_t sx0,
                                                                      int64_t max_iter, int64_t max_linesearch_iter, double mean_change_tol,
                                                                      double newton_dec_tol, int32_t flags, double *d_x, int64_t sx, double *d_hess,
                                                                      int64_t sh, double *result, double *totals, double *dec_trace,
                                                                      double *alpha_trace, int64_t *info, int64_t *cinfo, double *residual) {
    return bf_ga_impl(h, d_mu, smu, d_x0, sx0, max_iter, max_linesearch_iter, mean_change_tol, newton_dec_tol, flags, d_x, sx, d_hess, sh, result,
                      totals, dec_trace, alpha_trace, info, true, true, cinfo, residual);
}

// ---- the pullback of the Gaussian approximation for every member (Device::batch_ga_pullback; csrc/ga_pullback.hip) -------------------
// The middle link of gmrfx_batch_logpdf_grad -> gmrfx_batch_ga_pullback -> gmrfx_batch_pattern_dot: cotangents and outputs dense per
// member, as the two neighbours have them; x and mu with member strides, as gmrfx_batch_fisher_eval.
static int32_t bf_pullback_impl(gmrfx_handle *h, const double *x, int64_t sx, const double *mu, int64_t smu, const double *mubar, const double *Qbar,
                                int32_t flags, double *Qbar_prior, double *mubar_prior, double *lambda, double *out, int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_ga_pullback: ";
        bf_check_handle(h, who, true);
        if (!x) throw std::invalid_argument(who + "x is null");
        if (!out) throw std::invalid_argument(who + "out is null");
        const int64_t n = bf_n(h), nnz = bf_nnz(h), nb = h->nbatch;
        bf_check_stride(who, "x", sx, n);
        if (mu) bf_check_stride(who, "mu", smu, n, true);
        if (flags < 0 || flags > 3) throw std::invalid_argument(who + "unknown flag bits");
        if (!mubar && !Qbar) throw std::invalid_argument(who + "mubar and Qbar are both null");
        if (!Qbar_prior && !mubar_prior && !lambda) throw std::invalid_argument(who + "every output is null");
        if ((flags & 1) && h->bcon.m <= 0)
            throw std::invalid_argument(who + "flag bit 0 (project lambda) needs a batch constraint (gmrfx_batch_constraints_set)");
        if (h->bobs.nobs == 0) throw std::invalid_argument(who + "no observation likelihood is set (gmrfx_batch_obs_set)");
        if (int32_t e = need_batch(h, !(flags & 2))) return e;
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        std::vector<double> res(2 * (size_t)nb, 0.0);
        std::vector<long long> inf((size_t)nb, 0);
        if (dev)
            h->D->batch_ga_pullback(h->rsym, Device::BGapIO{x, sx, mu, smu, mubar, Qbar, flags, Qbar_prior, mubar_prior, lambda}, res.data(), inf.data());
        else {
            DevBlock bx, bm, bb, bq, oq, om, ol;
            stage_up(h, bx, x, n, n, 1, sx, nb);
            if (mu) stage_up(h, bm, mu, n, n, 1, smu, smu == 0 ? 1 : nb);
            if (mubar) stage_up(h, bb, mubar, n * nb);
            if (Qbar) stage_up(h, bq, Qbar, nnz * nb);
            if (Qbar_prior) stage_alloc(h, oq, nnz * nb);
            if (mubar_prior) stage_alloc(h, om, n * nb);
            if (lambda) stage_alloc(h, ol, n * nb);
            h->D->batch_ga_pullback(h->rsym, Device::BGapIO{bx, n, mu ? bm.get() : nullptr, smu == 0 ? 0 : n, mubar ? bb.get() : nullptr,
                                                            Qbar ? bq.get() : nullptr, flags, Qbar_prior ? oq.get() : nullptr,
                                                            mubar_prior ? om.get() : nullptr, lambda ? ol.get() : nullptr},
                                    res.data(), inf.data());
            if (Qbar_prior && nnz > 0) stage_down(h, oq, Qbar_prior, nnz * nb, nnz * nb, 1);
            if (mubar_prior) stage_down(h, om, mubar_prior, n * nb, n * nb, 1);
            if (lambda) stage_down(h, ol, lambda, n * nb, n * nb, 1);
        }
        std::copy(res.begin(), res.end(), out);
        if (info) { std::copy(inf.begin(), inf.end(), info); return GMRFX_OK; }
        // a failed member has NaN in its own outputs; without info the return code says so
        for (int64_t k = 0; k < nb; k++) {
            if (inf[(size_t)k] == 0) continue;
            h->err = who + "member " + std::to_string(k) + ": " +
                     (inf[(size_t)k] < 0 ? "Q_prior - H(x) is not positive definite (its factorisation failed)"
                                         : "A Q^-1 A' is not positive definite (rank-deficient constraint matrix)");
            return GMRFX_ERR_NOT_POSDEF;
        }
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_ga_pullback(gmrfx_handle *h, const double *x, int64_t sx, const double *mu, int64_t smu, const double *mubar,
                                           const double *Qbar, int32_t flags, double *Qbar_prior, double *mubar_prior, double *lambda, double *out,
                                           int64_t *info) {
    return bf_pullback_impl(h, x, sx, mu, smu, mubar, Qbar, flags, Qbar_prior, mubar_prior, lambda, out, info, false);
}
extern "C" int32_t gmrfx_batch_ga_pullback_dev(gmrfx_handle *h, const double *d_x, int64_t sx, const double *d_mu, int64_t smu, const double *d_mubar,
                                               const double *d_Qbar, int32_t flags, double *d_Qbar_prior, double *d_mubar_prior, double *d_lambda,
                                               double *out, int64_t *info) {
    return bf_pullback_impl(h, d_x, sx, d_mu, smu, d_mubar, d_Qbar, flags, d_Qbar_prior, d_mubar_prior, d_lambda, out, info, true);
}
