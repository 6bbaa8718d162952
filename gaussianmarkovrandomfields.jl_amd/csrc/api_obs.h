// api_obs.h -- what the entry points that set an observation likelihood share (api_fisher.cpp: gmrfx_obs_set, gmrfx_obs_set_design;
// api_composite.cpp: gmrfx_obs_set_composite; api_batch_fisher.cpp: gmrfx_batch_obs_set): the checks of family, operands and values, and the constant of the log-likelihood.
#pragma once
#include <cmath>

#include "api_common.h"
#include "obs_const.h"

// The terms of loglik that do not depend on x (canonical_implementations.jl:18-119, Distributions' logpdf), summed in long double
// (the terms themselves: obs_const.h, shared with gmrfx_obs_pointwise_const):
//   Normal  nobs (-1/2 log 2 pi - log sigma)          Poisson  -sum lgamma(y + 1)          Bernoulli  0
//   Binomial  sum lgamma(n + 1) - lgamma(y + 1) - lgamma(n - y + 1)
//   NegBin  sum lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log r          Gamma  nobs (phi log phi - lgamma(phi)) + (phi - 1) sum log y
// over the nobs observations at ys (aux: read by the binomial family alone), before the rounding to double: a composite likelihood
// (gmrfx_obs_set_composite) adds its components' in long double
inline long double obs_loglik_const_ld(int f, long long nobs_, const double *ys, const double *aux /* null: the family has none */, double param) {
    long double c = 0.0L;
    const long double p = (long double)param, nobs = (long double)nobs_;
    switch (f) {
        case 0: c = nobs * obs_const_shared(f, p); break;
        case 1: for (long long k = 0; k < nobs_; k++) c += obs_const_own(f, ys[k], 0.0L, p); break;
        case 3:
            for (long long k = 0; k < nobs_; k++) c += obs_const_own(f, ys[k], aux[k], p);
            break;
        case 4: for (long long k = 0; k < nobs_; k++) c += obs_const_own(f, ys[k], 0.0L, p); break;
        case 5:
            c = nobs * obs_const_shared(f, p);
            for (long long k = 0; k < nobs_; k++) c += obs_const_own(f, ys[k], 0.0L, p);
            break;
        default: break;
    }
    return c;
}
inline double obs_loglik_const(int f, long long nobs_, const std::vector<double> &ys, const std::vector<double> &aux, double param) {
    return (double)obs_loglik_const_ld(f, (long long)ys.size(), ys.data(), aux.data(), param);
}
inline double obs_loglik_const(const ObsHost &o) { return obs_loglik_const(o.family, o.nobs, o.y, o.aux, o.param); }

// ---- what gmrfx_obs_set and gmrfx_obs_set_design check alike (who: the prefix of the messages) -------------------------------------------
inline void obs_check_handle(const gmrfx_handle *h, const std::string &who) {
    check_unsharded(h, (who + "sharded handles are not supported").c_str());
    if (h->nbatch > 1) throw std::invalid_argument(who + "batched handles are not supported");
}
inline void obs_check_family(const std::string &who, int32_t family) {
    if (family < 0 || family >= kObsFamilies) throw std::invalid_argument(who + "unknown family (0 Normal, 1 Poisson, 2 Bernoulli, 3 Binomial, 4 NegativeBinomial, 5 Gamma)");
}
inline void obs_check_param(const std::string &who, int32_t family, double param) {
    if ((family == 0 || family == 4 || family == 5) && !(param > 0.0 && std::isfinite(param)))
        throw std::invalid_argument(who + "sigma / r / phi must be positive and finite");
}
inline void obs_check_operands(const std::string &who, int32_t family, const double *y, const double *aux, double param) {
    if (!y) throw std::invalid_argument(who + "y is null");
    if (family == 3 && !aux) throw std::invalid_argument(who + "the binomial family needs aux (the number of trials)");
    obs_check_param(who, family, param);
}
inline bool obs_family_reads_aux(int32_t family) { return family == 1 || family == 3 || family == 4; }      // (the others have no auxiliary number)
// one observation's values under its family (aux: null when none is held; at: where, for the message)
inline void obs_check_value(const std::string &who, int32_t family, double yk, const double *aux, const std::string &at) {
    if (!std::isfinite(yk)) throw std::invalid_argument(who + "y is not finite" + at);
    if (aux && !std::isfinite(*aux)) throw std::invalid_argument(who + "aux is not finite" + at);
    if (family >= 1 && family <= 4 && yk < 0.0) throw std::invalid_argument(who + "negative count" + at);
    if (family == 2 && yk > 1.0) throw std::invalid_argument(who + "a Bernoulli observation above 1" + at);
    if (family == 3 && !(*aux >= 0.0 && yk <= *aux)) throw std::invalid_argument(who + "y exceeds the number of trials" + at);
    if (family == 5 && !(yk > 0.0)) throw std::invalid_argument(who + "a Gamma observation must be positive" + at);
}
// y, aux, param and loglik_const of o, observation by observation
inline void obs_fill_values(ObsHost &o, const std::string &who, int32_t family, int64_t nobs, const double *y, const double *aux, double param) {
    o.family = family; o.nobs = nobs; o.param = param;
    o.y.assign(y, y + nobs);
    if (aux && obs_family_reads_aux(family)) o.aux.assign(aux, aux + nobs);
    for (int64_t k = 0; k < nobs; k++)
        obs_check_value(who, family, o.y[(size_t)k], o.aux.empty() ? nullptr : &o.aux[(size_t)k], " (observation " + std::to_string(k) + ")");
    o.loglik_const = obs_loglik_const(o);
}
