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
