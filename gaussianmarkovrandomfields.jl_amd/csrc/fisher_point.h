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

// What the pullback of the Gaussian approximation needs besides (gmrfx_ga_pullback): d3 = dd/deta, and the derivatives of g and d with
// respect to the family's parameter (sigma, r, phi), gp and dp; both 0 for the families without one. The same stable forms: q - s and
// q - m are differences of two numbers in [0, 1], each good to a few ulps of 1 -- the absolute error the bounds of the tests count.
__device__ __forceinline__ void fisher_point_pullback(int family, double eta, double y, double aux, double param, double logparam, double &d3,
                                                      double &gp, double &dp) {
#pragma clang fp contract(off)
    gp = 0.0; dp = 0.0;
    switch (family) {
        case 0: {       // g = (y - eta) / sigma^2, d = -1 / sigma^2
            const double inv3 = 1.0 / (param * param * param);
            d3 = 0.0; gp = -(2.0 * (y - eta) * inv3); dp = 2.0 * inv3;
            break;
        }
        case 1:         // d = -m
            d3 = -exp(eta + aux);
            break;
        case 2:
        case 3: {       // d = -nt m q, (m q)' = m q (q - m)
            const double nt = family == 3 ? aux : 1.0, m = fisher_logistic(eta), q = fisher_logistic(-eta);
            d3 = -(nt * m * q * (q - m));
            break;
        }
        case 4: {       // s = logistic(t), t = eta + aux - log r: ds/dr = -s q / r
            const double t = (eta + aux) - logparam, s = fisher_logistic(t), q = fisher_logistic(-t);
            const double c = (param + y) * s * q * (q - s);
            d3 = -c;
            gp = s * ((param + y) * q / param - 1.0);
            dp = c / param - s * q;
            break;
        }
        default: {      // 5: w = y e^-eta, g = phi (w - 1), d = -phi w
            const double w = y * exp(-eta);
            d3 = param * w; gp = w - 1.0; dp = -w;
            break;
        }
    }
}

}  // namespace gmrfx
