// api_predictive.cpp -- the C ABI of include/gmrfx.h: the marginals of the linear predictor, the predictive scores over them and the
// per-observation constants of the log density (Device::predictor_marginals, Device::predictive_scores; csrc/predictive.hip).
#include <cmath>

#include "api_common.h"

static void pred_check_handle(const gmrfx_handle *h, const std::string &who) {
    check_unsharded(h, (who + "sharded handles are not supported").c_str());
    if (h->nbatch > 1) throw std::invalid_argument(who + "batched handles are not supported");
    if (h->obs.nobs == 0) throw std::invalid_argument(who + "no observation likelihood is set (gmrfx_obs_set)");
}

extern "C" int32_t gmrfx_obs_pointwise_const(const gmrfx_handle *h, double *out) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    return guarded(const_cast<gmrfx_handle *>(h), [&]() -> int32_t {
        if (h->obs.nobs == 0) throw std::invalid_argument("obs_pointwise_const: no observation likelihood is set (gmrfx_obs_set)");
        if (!out) throw std::invalid_argument("obs_pointwise_const: out is null");
        obs_pointwise_const(h->obs, out);
        return GMRFX_OK;
    });
}

static int32_t marginals_impl(gmrfx_handle *h, const double *x, int32_t flags, double *mu_eta, double *v_eta, double *pll, bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "predictor_marginals: ";
        if (!x) throw std::invalid_argument(who + "x is null");
        if (!mu_eta && !v_eta && !pll) throw std::invalid_argument(who + "every output is null");
        if (flags < 0 || flags > 1) throw std::invalid_argument(who + "unknown flag bits");
        if ((flags & 1) && h->con.m <= 0) throw std::invalid_argument(who + "flag bit 0 (constraint correction) needs a constraint (gmrfx_constraints_set)");
        pred_check_handle(h, who);
        if (int32_t e = need_device(h, v_eta != nullptr)) return e;
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        int rc;
        if (dev) rc = h->D->predictor_marginals(h->rsym, h->obs, Device::PredIO{x, flags, mu_eta, v_eta, pll});
        else {
            const int64_t n = h->S.n, nobs = h->obs.nobs;
            DevBlock bx, bm, bv, bp;
            stage_up(h, bx, x, n);
            if (mu_eta) stage_alloc(h, bm, nobs);
            if (v_eta) stage_alloc(h, bv, nobs);
            if (pll) stage_alloc(h, bp, nobs);
            rc = h->D->predictor_marginals(h->rsym, h->obs, Device::PredIO{bx, flags, mu_eta ? bm.get() : nullptr, v_eta ? bv.get() : nullptr,
                                                                           pll ? bp.get() : nullptr});
            if (rc == 0) {
                if (mu_eta) stage_down(h, bm, mu_eta, nobs, nobs, 1);
                if (v_eta) stage_down(h, bv, v_eta, nobs, nobs, 1);
                if (pll) stage_down(h, bp, pll, nobs, nobs, 1);
            }
        }
        if (rc == 2) {
            h->err = "predictor_marginals: A Q^-1 A' is not positive definite (rank-deficient constraint matrix)";
            return GMRFX_ERR_NOT_POSDEF;
        }
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_predictor_marginals(gmrfx_handle *h, const double *x, int32_t flags, double *mu_eta, double *v_eta, double *pll) {
    return marginals_impl(h, x, flags, mu_eta, v_eta, pll, false);
}
extern "C" int32_t gmrfx_predictor_marginals_dev(gmrfx_handle *h, const double *d_x, int32_t flags, double *d_mu_eta, double *d_v_eta, double *d_pll) {
    return marginals_impl(h, d_x, flags, d_mu_eta, d_v_eta, d_pll, true);
}

static int32_t scores_impl(gmrfx_handle *h, const double *mu_eta, const double *v_eta, int64_t K, const double *z, const double *w, double *lpd,
                           double *lcpo, double *elp, double *vlp, double *out, bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "predictive_scores: ";
        if (!mu_eta || !v_eta) throw std::invalid_argument(who + "mu_eta / v_eta is null");
        if (!out) throw std::invalid_argument(who + "out is null");
        if (K < 1 || K > 64) throw std::invalid_argument(who + "K must be 1 .. 64");
        if (!z || !w) throw std::invalid_argument(who + "the quadrature nodes / weights are null");
        for (int64_t k = 0; k < K; k++) {
            if (!std::isfinite(z[k]) || !std::isfinite(w[k])) throw std::invalid_argument(who + "a quadrature node or weight is not finite");
            if (!(w[k] > 0.0)) throw std::invalid_argument(who + "the quadrature weights must be positive");
        }
        pred_check_handle(h, who);
        if (int32_t e = need_device(h, false)) return e;
        double res[4] = {0.0, 0.0, 0.0, 0.0};
        if (dev) h->D->predictive_scores(h->obs, Device::ScoreIO{mu_eta, v_eta, (int)K, z, w, lpd, lcpo, elp, vlp}, res);
        else {
            const int64_t nobs = h->obs.nobs;
            DevBlock bm, bv, o0, o1, o2, o3;
            stage_up(h, bm, mu_eta, nobs);
            stage_up(h, bv, v_eta, nobs);
            if (lpd) stage_alloc(h, o0, nobs);
            if (lcpo) stage_alloc(h, o1, nobs);
            if (elp) stage_alloc(h, o2, nobs);
            if (vlp) stage_alloc(h, o3, nobs);
            h->D->predictive_scores(h->obs, Device::ScoreIO{bm, bv, (int)K, z, w, lpd ? o0.get() : nullptr, lcpo ? o1.get() : nullptr,
                                                            elp ? o2.get() : nullptr, vlp ? o3.get() : nullptr}, res);
            if (lpd) stage_down(h, o0, lpd, nobs, nobs, 1);
            if (lcpo) stage_down(h, o1, lcpo, nobs, nobs, 1);
            if (elp) stage_down(h, o2, elp, nobs, nobs, 1);
            if (vlp) stage_down(h, o3, vlp, nobs, nobs, 1);
        }
        std::copy(res, res + 4, out);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_predictive_scores(gmrfx_handle *h, const double *mu_eta, const double *v_eta, int64_t K, const double *z, const double *w,
                                           double *lpd, double *lcpo, double *elp, double *vlp, double *out) {
    return scores_impl(h, mu_eta, v_eta, K, z, w, lpd, lcpo, elp, vlp, out, false);
}
extern "C" int32_t gmrfx_predictive_scores_dev(gmrfx_handle *h, const double *d_mu_eta, const double *d_v_eta, int64_t K, const double *z,
                                               const double *w, double *d_lpd, double *d_lcpo, double *d_elp, double *d_vlp, double *out) {
    return scores_impl(h, d_mu_eta, d_v_eta, K, z, w, d_lpd, d_lcpo, d_elp, d_vlp, out, true);
}

// ---- the same for every member of a batched handle (Device::batch_predictor_marginals, Device::batch_predictive_scores) and the
// mixture over the members (Device::batch_predictive_mixture). A plain handle that holds a batch likelihood is a batch of one. -----------
// what the batch calls refuse about the handle itself (the rules of gmrfx_batch_ga_pullback: a batch constraint may be held)
static void bpred_check_handle(const gmrfx_handle *h, const std::string &who) {
    check_unsharded(h, (who + "sharded handles are not supported").c_str());
    if (h->nbatch > kBatchFisherMaxMembers) throw std::invalid_argument(who + "more than 65535 members");
    if (h->obs.design) throw std::invalid_argument(who + "the design form (eta = A x + b, gmrfx_obs_set_design) is not supported");
    if (h->con.m > 0) throw std::invalid_argument(who + "a constraint set is not supported (clear it first)");
    if (h->bobs.nobs == 0) throw std::invalid_argument(who + "no observation likelihood is set (gmrfx_batch_obs_set)");
}
static int64_t bpred_n(const gmrfx_handle *h) { return h->nbatch > 1 ? h->n_member : h->S.n; }
static void bpred_check_rule(const std::string &who, int64_t K, const double *z, const double *w) {
    if (K < 1 || K > 64) throw std::invalid_argument(who + "K must be 1 .. 64");
    if (!z || !w) throw std::invalid_argument(who + "the quadrature nodes / weights are null");
    for (int64_t k = 0; k < K; k++) {
        if (!std::isfinite(z[k]) || !std::isfinite(w[k])) throw std::invalid_argument(who + "a quadrature node or weight is not finite");
        if (!(w[k] > 0.0)) throw std::invalid_argument(who + "the quadrature weights must be positive");
    }
}

extern "C" int32_t gmrfx_batch_obs_pointwise_const(const gmrfx_handle *h, double *out) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    return guarded(const_cast<gmrfx_handle *>(h), [&]() -> int32_t {
        if (h->bobs.nobs == 0) throw std::invalid_argument("batch_obs_pointwise_const: no observation likelihood is set (gmrfx_batch_obs_set)");
        if (!out) throw std::invalid_argument("batch_obs_pointwise_const: out is null");
        bobs_pointwise_const(h->bobs, out);
        return GMRFX_OK;
    });
}

static int32_t bmarginals_impl(gmrfx_handle *h, const double *x, int64_t sx, int32_t flags, double *mu_eta, double *v_eta, double *pll, int64_t *info,
                               bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_predictor_marginals: ";
        if (!x) throw std::invalid_argument(who + "x is null");
        if (!mu_eta && !v_eta && !pll) throw std::invalid_argument(who + "every output is null");
        if (flags < 0 || flags > 1) throw std::invalid_argument(who + "unknown flag bits");
        if ((flags & 1) && h->bcon.m <= 0)
            throw std::invalid_argument(who + "flag bit 0 (constraint correction) needs a batch constraint (gmrfx_batch_constraints_set)");
        bpred_check_handle(h, who);
        const int64_t n = bpred_n(h), nobs = h->bobs.nobs, nb = h->nbatch;
        if (sx < n) throw std::invalid_argument(who + "x: member stride smaller than n");
        if (int32_t e = need_batch(h, v_eta != nullptr)) return e;
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        std::vector<long long> inf((size_t)nb, 0);
        if (dev) h->D->batch_predictor_marginals(h->rsym, h->bobs, Device::BPredIO{x, sx, flags, mu_eta, v_eta, pll}, inf.data());
        else {
            DevBlock bx, bm, bv, bp;
            stage_up(h, bx, x, n, n, 1, sx, nb);
            if (mu_eta) stage_alloc(h, bm, nobs * nb);
            if (v_eta) stage_alloc(h, bv, nobs * nb);
            if (pll) stage_alloc(h, bp, nobs * nb);
            h->D->batch_predictor_marginals(h->rsym, h->bobs, Device::BPredIO{bx, n, flags, mu_eta ? bm.get() : nullptr, v_eta ? bv.get() : nullptr,
                                                                               pll ? bp.get() : nullptr}, inf.data());
            if (mu_eta) stage_down(h, bm, mu_eta, nobs * nb, nobs * nb, 1);
            if (v_eta) stage_down(h, bv, v_eta, nobs * nb, nobs * nb, 1);
            if (pll) stage_down(h, bp, pll, nobs * nb, nobs * nb, 1);
        }
        if (info) std::copy(inf.begin(), inf.end(), info);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_predictor_marginals(gmrfx_handle *h, const double *x, int64_t sx, int32_t flags, double *mu_eta, double *v_eta, double *pll,
                                                   int64_t *info) {
    return bmarginals_impl(h, x, sx, flags, mu_eta, v_eta, pll, info, false);
}
extern "C" int32_t gmrfx_batch_predictor_marginals_dev(gmrfx_handle *h, const double *d_x, int64_t sx, int32_t flags, double *d_mu_eta, double *d_v_eta,
                                                       double *d_pll, int64_t *info) {
    return bmarginals_impl(h, d_x, sx, flags, d_mu_eta, d_v_eta, d_pll, info, true);
}

static int32_t bscores_impl(gmrfx_handle *h, const double *mu_eta, const double *v_eta, int64_t K, const double *z, const double *w, double *lpd,
                            double *lcpo, double *elp, double *vlp, double *out, int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_predictive_scores: ";
        if (!mu_eta || !v_eta) throw std::invalid_argument(who + "mu_eta / v_eta is null");
        if (!out) throw std::invalid_argument(who + "out is null");
        bpred_check_rule(who, K, z, w);
        bpred_check_handle(h, who);
        if (int32_t e = need_batch(h, false)) return e;
        const int64_t nobs = h->bobs.nobs, nb = h->nbatch, len = nobs * nb;
        std::vector<double> res(4 * (size_t)nb, 0.0);
        std::vector<long long> inf((size_t)nb, 0);
        if (dev) h->D->batch_predictive_scores(h->bobs, Device::ScoreIO{mu_eta, v_eta, (int)K, z, w, lpd, lcpo, elp, vlp}, res.data(), inf.data());
        else {
            DevBlock bm, bv, o0, o1, o2, o3;
            stage_up(h, bm, mu_eta, len);
            stage_up(h, bv, v_eta, len);
            if (lpd) stage_alloc(h, o0, len);
            if (lcpo) stage_alloc(h, o1, len);
            if (elp) stage_alloc(h, o2, len);
            if (vlp) stage_alloc(h, o3, len);
            h->D->batch_predictive_scores(h->bobs, Device::ScoreIO{bm, bv, (int)K, z, w, lpd ? o0.get() : nullptr, lcpo ? o1.get() : nullptr,
                                                                   elp ? o2.get() : nullptr, vlp ? o3.get() : nullptr}, res.data(), inf.data());
            if (lpd) stage_down(h, o0, lpd, len, len, 1);
            if (lcpo) stage_down(h, o1, lcpo, len, len, 1);
            if (elp) stage_down(h, o2, elp, len, len, 1);
            if (vlp) stage_down(h, o3, vlp, len, len, 1);
        }
        std::copy(res.begin(), res.end(), out);
        if (info) std::copy(inf.begin(), inf.end(), info);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_predictive_scores(gmrfx_handle *h, const double *mu_eta, const double *v_eta, int64_t K, const double *z, const double *w,
                                                 double *lpd, double *lcpo, double *elp, double *vlp, double *out, int64_t *info) {
    return bscores_impl(h, mu_eta, v_eta, K, z, w, lpd, lcpo, elp, vlp, out, info, false);
}
extern "C" int32_t gmrfx_batch_predictive_scores_dev(gmrfx_handle *h, const double *d_mu_eta, const double *d_v_eta, int64_t K, const double *z,
                                                     const double *w, double *d_lpd, double *d_lcpo, double *d_elp, double *d_vlp, double *out,
                                                     int64_t *info) {
    return bscores_impl(h, d_mu_eta, d_v_eta, K, z, w, d_lpd, d_lcpo, d_elp, d_vlp, out, info, true);
}

// omega_k = exp(logw_k - max) / sum and log omega_k = (logw_k - max) - log sum, in long double, each rounded to double once; an
// excluded member (logw = -inf) gets omega = 0 and log omega = -inf, which is how the kernel knows it. w: nbatch omegas, then the logs.
static void mixture_weights(const std::string &who, const double *logw, int64_t nb, std::vector<double> &w) {
    long double mx = -INFINITY;
    for (int64_t k = 0; k < nb; k++) {
        if (std::isnan(logw[k]) || logw[k] == INFINITY) throw std::invalid_argument(who + "a log weight is NaN or +inf");
        mx = std::max(mx, (long double)logw[k]);
    }
    if (mx == -INFINITY) throw std::invalid_argument(who + "every member is excluded (all log weights are -inf)");
    long double sum = 0.0L;
    for (int64_t k = 0; k < nb; k++)
        if (logw[k] != -INFINITY) sum += std::exp((long double)logw[k] - mx);
    const long double lsum = std::log(sum);
    w.assign(2 * (size_t)nb, 0.0);
    for (int64_t k = 0; k < nb; k++) {
        const bool in = logw[k] != -INFINITY;
        w[(size_t)k] = in ? (double)(std::exp((long double)logw[k] - mx) / sum) : 0.0;
        w[(size_t)(nb + k)] = in ? (double)(((long double)logw[k] - mx) - lsum) : -INFINITY;
    }
}

static int32_t bmixture_impl(gmrfx_handle *h, const double *logw, const double *mu_eta, const double *v_eta, const double *lpd, double *mix_mu,
                             double *mix_v, double *mix_lpd, double *out, bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "batch_predictive_mixture: ";
        if (!logw) throw std::invalid_argument(who + "logw is null");
        if (!mu_eta || !v_eta) throw std::invalid_argument(who + "mu_eta / v_eta is null");
        if (!mix_mu && !mix_v && !mix_lpd && !(lpd && out)) throw std::invalid_argument(who + "every output is null");
        if (mix_lpd && !lpd) throw std::invalid_argument(who + "mix_lpd needs lpd");
        bpred_check_handle(h, who);
        const int64_t nobs = h->bobs.nobs, nb = h->nbatch, len = nobs * nb;
        std::vector<double> w;
        mixture_weights(who, logw, nb, w);
        if (int32_t e = need_batch(h, false)) return e;
        double total = 0.0;
        if (dev) h->D->batch_predictive_mixture(h->bobs, w, Device::MixIO{mu_eta, v_eta, lpd, mix_mu, mix_v, mix_lpd}, &total);
        else {
            // an excluded member's columns are never read on the device; they go up with the rest, as they are
            DevBlock bm, bv, bl, o0, o1, o2;
            stage_up(h, bm, mu_eta, len);
            stage_up(h, bv, v_eta, len);
            if (lpd) stage_up(h, bl, lpd, len);
            if (mix_mu) stage_alloc(h, o0, nobs);
            if (mix_v) stage_alloc(h, o1, nobs);
            if (mix_lpd) stage_alloc(h, o2, nobs);
            h->D->batch_predictive_mixture(h->bobs, w, Device::MixIO{bm, bv, lpd ? bl.get() : nullptr, mix_mu ? o0.get() : nullptr,
                                                                     mix_v ? o1.get() : nullptr, mix_lpd ? o2.get() : nullptr}, &total);
            if (mix_mu) stage_down(h, o0, mix_mu, nobs, nobs, 1);
            if (mix_v) stage_down(h, o1, mix_v, nobs, nobs, 1);
            if (mix_lpd) stage_down(h, o2, mix_lpd, nobs, nobs, 1);
        }
        if (out) *out = total;
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_predictive_mixture(gmrfx_handle *h, const double *logw, const double *mu_eta, const double *v_eta, const double *lpd,
                                                  double *mix_mu, double *mix_v, double *mix_lpd, double *out) {
    return bmixture_impl(h, logw, mu_eta, v_eta, lpd, mix_mu, mix_v, mix_lpd, out, false);
}
extern "C" int32_t gmrfx_batch_predictive_mixture_dev(gmrfx_handle *h, const double *logw, const double *d_mu_eta, const double *d_v_eta,
                                                      const double *d_lpd, double *d_mix_mu, double *d_mix_v, double *d_mix_lpd, double *out) {
    return bmixture_impl(h, logw, d_mu_eta, d_v_eta, d_lpd, d_mix_mu, d_mix_v, d_mix_lpd, out, true);
}
