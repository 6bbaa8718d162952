// fisher_point.h -- the pointwise functions of the six observation families, shared by fisher.hip (eta_i = x_i) and fisher_design.hip
// (eta = A x + b). Device code only.
// STABLE FORMS. Every exponential takes a non-positive argument or the linear predictor itself: logistic(t) = 1 / (1 + e^-t) for
// t >= 0 and e^t / (1 + e^t) below, log(1 + e^t) = max(t, 0) + log1p(e^-|t|), 1 - logistic(t) = logistic(-t) (no cancellation), the
// negative binomial through s = mu / (r + mu) = logistic(eta + aux - log r), log(r + mu) = max(log r, eta + aux) + log1p(e^-|..|).
// Finite for every eta where the mathematics is (Bernoulli / binomial everywhere; the log links up to the overflow of mu itself).
#pragma once
#include <hip/hip_runtime.h>

namespace gmrfx {

__device__ __forceinline__ double fisher_logistic(double t) {
    if (t >= 0.0) return 1.0 / (1.0 + exp(-t));
    const double e = exp(t);
    return e / (1.0 + e);
}
__device__ __forceinline__ double fisher_log1pexp(double t) { return fmax(t, 0.0) + log1p(exp(-fabs(t))); }

// g, d and the x-dependent part of the log-likelihood of one observed node
__device__ __forceinline__ void fisher_point(int family, double eta, double y, double aux, double param, double logparam, double &g, double &d,
                                             double &ll) {
#pragma clang fp contract(off)
    switch (family) {
        case 0: {       // Normal / identity, param = sigma
            const double inv = 1.0 / (param * param), r = y - eta;
            g = r * inv; d = -inv; ll = -0.5 * inv * (r * r);
            break;
        }
        case 1: {       // Poisson / log, aux = log exposure
            const double e = eta + aux, m = exp(e);
            g = y - m; d = -m; ll = y * e - m;
            break;
        }
        case 2:         // Bernoulli / logit (one trial)
        case 3: {       // Binomial / logit, aux = trials
            const double nt = family == 3 ? aux : 1.0, m = fisher_logistic(eta), q = fisher_logistic(-eta);
            g = y - nt * m; d = -(nt * m * q); ll = y * eta - nt * fisher_log1pexp(eta);
            break;
        }
        case 4: {       // NegativeBinomial / log, aux = log exposure, param = r
            const double e = eta + aux, t = e - logparam, s = fisher_logistic(t), q = fisher_logistic(-t);
            g = y * q - param * s; d = -((param + y) * s * q);
            ll = y * e - (param + y) * (fmax(logparam, e) + log1p(exp(-fabs(t))));
            break;
        }
        default: {      // 5: Gamma / log, param = phi
            const double w = y * exp(-eta);
            g = param * (w - 1.0); d = -(param * w); ll = -(param * eta) - param * w;
            break;
        }
    }
}

}  // namespace gmrfx
