// api_ga_pullback.cpp -- the C ABI of include/gmrfx.h: the pullback of gaussian_approximation (Device::ga_pullback; csrc/ga_pullback.hip),
// the same for a composite likelihood (Device::ga_pullback_composite) and the read-out of the design plan's transposed term table.
#include "api_common.h"

static int32_t ga_pullback_impl(gmrfx_handle *h, const double *x, const double *mu, const double *mubar, const double *Qbar, int32_t flags,
                                double *Qbar_prior, double *mubar_prior, double *lambda, double *out, bool dev) {
    return guarded(h, [&]() -> int32_t {
        check_unsharded(h, "ga_pullback: sharded handles are not supported");
        if (h->nbatch > 1) throw std::invalid_argument("ga_pullback: batched handles are not supported");
        if (!x) throw std::invalid_argument("ga_pullback: x is null");
        if (!out) throw std::invalid_argument("ga_pullback: out is null");
        if (h->obs.nobs == 0) throw std::invalid_argument("ga_pullback: no observation likelihood is set (gmrfx_obs_set)");
        if (!h->obs.comp.empty())
            throw std::invalid_argument("ga_pullback: composite likelihoods are not supported (one parameter cotangent per component is needed; gmrfx_obs_set_composite)");
        if (flags < 0 || flags > 3) throw std::invalid_argument("ga_pullback: unknown flag bits");
        if (!mubar && !Qbar) throw std::invalid_argument("ga_pullback: mubar and Qbar are both null");
        if (!Qbar_prior && !mubar_prior && !lambda) throw std::invalid_argument("ga_pullback: every output is null");
        if ((flags & 1) && h->con.m <= 0) throw std::invalid_argument("ga_pullback: flag bit 0 (project lambda) needs a constraint (gmrfx_constraints_set)");
        if (int32_t e = need_device(h, !(flags & 2))) return e;
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        double res[2] = {0.0, 0.0};
        long long inf = 0;
        int rc;
        if (dev) rc = h->D->ga_pullback(h->rsym, Device::GapIO{x, mu, mubar, Qbar, flags, Qbar_prior, mubar_prior, lambda}, res, &inf);
        else {
            const int64_t n = h->S.n, nnz = h->S.nnz_in;
            DevBlock bx, bm, bb, bq, oq, om, ol;
            stage_up(h, bx, x, n);
            if (mu) stage_up(h, bm, mu, n);
            if (mubar) stage_up(h, bb, mubar, n);
            if (Qbar) stage_up(h, bq, Qbar, nnz);
            if (Qbar_prior) stage_alloc(h, oq, nnz);
            if (mubar_prior) stage_alloc(h, om, n);
            if (lambda) stage_alloc(h, ol, n);
            rc = h->D->ga_pullback(h->rsym, Device::GapIO{bx, mu ? bm.get() : nullptr, mubar ? bb.get() : nullptr, Qbar ? bq.get() : nullptr, flags,
                                                          Qbar_prior ? oq.get() : nullptr, mubar_prior ? om.get() : nullptr, lambda ? ol.get() : nullptr},
                                   res, &inf);
            if (rc == 0) {
                if (Qbar_prior && nnz > 0) stage_down(h, oq, Qbar_prior, nnz, nnz, 1);
                if (mubar_prior) stage_down(h, om, mubar_prior, n, n, 1);
                if (lambda) stage_down(h, ol, lambda, n, n, 1);
            }
        }
        if (rc == 1) {
            h->err = "ga_pullback: Q_prior - H(x) is not positive definite (non-positive pivot at elimination step " + std::to_string(inf) + ")";
            return GMRFX_ERR_NOT_POSDEF;
        }
        if (rc == 2) {
            h->err = "ga_pullback: A Q^-1 A' is not positive definite (rank-deficient constraint matrix)";
            return GMRFX_ERR_NOT_POSDEF;
        }
        out[0] = res[0];
        out[1] = res[1];
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_ga_pullback(gmrfx_handle *h, const double *x, const double *mu, const double *mubar, const double *Qbar, int32_t flags,
                                     double *Qbar_prior, double *mubar_prior, double *lambda, double *out) {
    return ga_pullback_impl(h, x, mu, mubar, Qbar, flags, Qbar_prior, mubar_prior, lambda, out, false);
}
extern "C" int32_t gmrfx_ga_pullback_dev(gmrfx_handle *h, const double *d_x, const double *d_mu, const double *d_mubar, const double *d_Qbar,
                                         int32_t flags, double *d_Qbar_prior, double *d_mubar_prior, double *d_lambda, double *out) {
    return ga_pullback_impl(h, d_x, d_mu, d_mubar, d_Qbar, flags, d_Qbar_prior, d_mubar_prior, d_lambda, out, true);
}

// The same rule for a composite likelihood (gmrfx_obs_set_composite): one parameter cotangent per component.
static int32_t ga_pullback_composite_impl(gmrfx_handle *h, const double *x, const double *mu, const double *mubar, const double *Qbar, int32_t flags,
                                          double *Qbar_prior, double *mubar_prior, double *lambda, double *param_bar, double *check, bool dev) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "ga_pullback_composite: ";
        check_unsharded(h, "ga_pullback_composite: sharded handles are not supported");
        if (h->nbatch > 1) throw std::invalid_argument(who + "batched handles are not supported");
        if (h->obs.comp.empty())
            throw std::invalid_argument(who + "no composite likelihood is set (gmrfx_obs_set_composite; gmrfx_ga_pullback serves single-family likelihoods)");
        if (!x) throw std::invalid_argument(who + "x is null");
        if (!param_bar) throw std::invalid_argument(who + "param_bar is null");
        if (flags < 0 || flags > 3) throw std::invalid_argument(who + "unknown flag bits");
        if (!mubar && !Qbar) throw std::invalid_argument(who + "mubar and Qbar are both null");
        if (!Qbar_prior && !mubar_prior && !lambda) throw std::invalid_argument(who + "every output is null");
        if ((flags & 1) && h->con.m <= 0) throw std::invalid_argument(who + "flag bit 0 (project lambda) needs a constraint (gmrfx_constraints_set)");
        if (int32_t e = need_device(h, !(flags & 2))) return e;
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        std::vector<double> res(h->obs.comp.size(), 0.0);
        double chk = 0.0;
        long long inf = 0;
        int rc;
        if (dev)
            rc = h->D->ga_pullback_composite(h->rsym, Device::GapIO{x, mu, mubar, Qbar, flags, Qbar_prior, mubar_prior, lambda}, res.data(), &chk, &inf);
        else {
            const int64_t n = h->S.n, nnz = h->S.nnz_in;
            DevBlock bx, bm, bb, bq, oq, om, ol;
            stage_up(h, bx, x, n);
            if (mu) stage_up(h, bm, mu, n);
            if (mubar) stage_up(h, bb, mubar, n);
            if (Qbar) stage_up(h, bq, Qbar, nnz);
            if (Qbar_prior) stage_alloc(h, oq, nnz);
            if (mubar_prior) stage_alloc(h, om, n);
            if (lambda) stage_alloc(h, ol, n);
            rc = h->D->ga_pullback_composite(h->rsym,
                                             Device::GapIO{bx, mu ? bm.get() : nullptr, mubar ? bb.get() : nullptr, Qbar ? bq.get() : nullptr, flags,
                                                           Qbar_prior ? oq.get() : nullptr, mubar_prior ? om.get() : nullptr, lambda ? ol.get() : nullptr},
                                             res.data(), &chk, &inf);
            if (rc == 0) {
                if (Qbar_prior && nnz > 0) stage_down(h, oq, Qbar_prior, nnz, nnz, 1);
                if (mubar_prior) stage_down(h, om, mubar_prior, n, n, 1);
                if (lambda) stage_down(h, ol, lambda, n, n, 1);
            }
        }
        if (rc == 1) {
            h->err = who + "Q_prior - H(x) is not positive definite (non-positive pivot at elimination step " + std::to_string(inf) + ")";
            return GMRFX_ERR_NOT_POSDEF;
        }
        if (rc == 2) {
            h->err = who + "A Q^-1 A' is not positive definite (rank-deficient constraint matrix)";
            return GMRFX_ERR_NOT_POSDEF;
        }
        std::copy(res.begin(), res.end(), param_bar);
        if (check) *check = chk;
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_ga_pullback_composite(gmrfx_handle *h, const double *x, const double *mu, const double *mubar, const double *Qbar,
                                               int32_t flags, double *Qbar_prior, double *mubar_prior, double *lambda, double *param_bar,
                                               double *check) {
    return ga_pullback_composite_impl(h, x, mu, mubar, Qbar, flags, Qbar_prior, mubar_prior, lambda, param_bar, check, false);
}
extern "C" int32_t gmrfx_ga_pullback_composite_dev(gmrfx_handle *h, const double *d_x, const double *d_mu, const double *d_mubar,
                                                   const double *d_Qbar, int32_t flags, double *d_Qbar_prior, double *d_mubar_prior,
                                                   double *d_lambda, double *param_bar, double *check) {
    return ga_pullback_composite_impl(h, d_x, d_mu, d_mubar, d_Qbar, flags, d_Qbar_prior, d_mubar_prior, d_lambda, param_bar, check, true);
}

// the plan's transposed term table: per observation the pairs of its row as (position in nzval, weight), positions ascending
extern "C" int32_t gmrfx_obs_design_rows(const gmrfx_handle *h, int64_t *ptr, int64_t *pos, double *w) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    return guarded(const_cast<gmrfx_handle *>(h), [&]() -> int32_t {
        if (!h->obs.design) throw std::invalid_argument("obs_design_rows: no design likelihood is set (gmrfx_obs_set_design)");
        const DesignPlan &P = *h->obs.design;
        if (ptr) std::copy(P.optr.begin(), P.optr.end(), ptr);
        if (pos)
            for (size_t t = 0; t < P.oidx.size(); t++) pos[t] = P.map[(size_t)P.oidx[t]];
        if (w) std::copy(P.ow.begin(), P.ow.end(), w);
        return GMRFX_OK;
    });
}
