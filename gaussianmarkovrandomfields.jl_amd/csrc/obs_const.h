// obs_const.h -- the term of one observation's log density that does not depend on x (canonical_implementations.jl:18-119,
// Distributions' logpdf), in long double. Host only. gmrfx_obs_set sums these into ObsHost::loglik_const (api_fisher.cpp: the
// accumulation is its own); gmrfx_predictor_marginals adds them observation by observation to l_i(eta_i) (pointwise_loglik of the
// reference, src/observation_models/exponential_family/pointwise_implementations.jl), rounded to double.
//   Normal  -1/2 log 2 pi - log sigma          Poisson  -lgamma(y + 1)          Bernoulli  0
//   Binomial  lgamma(n + 1) - lgamma(y + 1) - lgamma(n - y + 1)
//   NegBin  lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log r          Gamma  phi log phi - lgamma(phi) + (phi - 1) log y
#pragma once
#include <cmath>

namespace gmrfx {

// the part every observation of a Normal (sigma = p) or Gamma (phi = p) likelihood shares
inline long double obs_const_shared(int family, long double p) {
    if (family == 0) return -0.5L * std::log(2.0L * std::acos(-1.0L)) - std::log(p);
    if (family == 5) return p * std::log(p) - std::lgamma(p);
    return 0.0L;
}
// the part that goes with y (and aux = the number of trials of a binomial observation)
inline long double obs_const_own(int family, long double y, long double aux, long double p) {
    switch (family) {
        case 1: return -std::lgamma(y + 1.0L);
        case 3: return std::lgamma(aux + 1.0L) - std::lgamma(y + 1.0L) - std::lgamma(aux - y + 1.0L);
        case 4: return std::lgamma(y + p) - std::lgamma(p) - std::lgamma(y + 1.0L) + p * std::log(p);
        case 5: return (p - 1.0L) * std::log(y);
        default: return 0.0L;
    }
}
inline long double obs_const_term(int family, long double y, long double aux, long double p) {
    return obs_const_shared(family, p) + obs_const_own(family, y, aux, p);
}

}  // namespace gmrfx
