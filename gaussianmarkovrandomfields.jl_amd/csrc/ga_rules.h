// ga_rules.h -- the decisions of the Fisher-scoring loop as plain functions (host only, no HIP): what the reference decides in
// src/workspace/gaussian_approximation.jl:230-313 and in _ga_line_search, _predict_converged and _frozen_finish of
// src/arithmetic/condition/gaussian_approximation.jl:231-409. Device::gaussian_approximation drives one GaMember through them,
// Device::batch_gaussian_approximation a vector of them: a member of a batch takes the decisions of its own plain loop because both
// call the same functions. Every constant of the loop is here and nowhere else.
#pragma once
#include <algorithm>
#include <cmath>

namespace gmrfx {

// flags: bit 0 adaptive_stepsize, 1 retry_full, 2 predictive_convergence, 3 leave the handle factorised at Q_prior - H(x_final)
struct GaOpts {
    long long max_iter, max_ls;
    double mean_tol, dec_tol;
    int flags;
    bool adaptive() const { return flags & 1; }
    bool retry_full() const { return flags & 2; }
    bool predictive() const { return flags & 4; }
    bool refactor_final() const { return flags & 8; }
};

// _merit_atol (condition/gaussian_approximation.jl:245): the line search's slack on the merit
inline double merit_atol(double scale) { return 64.0 * 2.220446049250313e-16 * std::max(scale, 1.0); }

// One member's loop state (a plain handle is one member).
enum GaStatus { kGaRun, kGaConverged, kGaMaxIter, kGaFailed };
struct GaMember {
    double alpha = 1.0, alpha_prev = 1.0, dec_prev = 0.0, dec = std::nan(""), nfact = 0, nsolve = 0, nmerit = 0;
    long long iters = 0;
    bool frozen = false;
    int status = kGaRun;
};

// an iterate's refactorize_update_solve has run for the member: the step length of the previous iterate is what _predict_converged asks for
inline void ga_iterate_begun(GaMember &m) { m.nfact += 1; m.nsolve += 1; m.alpha_prev = m.alpha; }
inline void ga_stop(GaMember &m, int status, long long iters, bool frozen) { m.status = status; m.iters = iters; m.frozen = frozen; }

// ---- _ga_line_search. e = {energy, loglik} of an evaluation, the merit is their difference. -----------------------------------------
inline double ga_merit(const double *e) { return e[0] - e[1]; }
// the largest merit a candidate is accepted with, from the evaluation at the current iterate
inline double ga_line_search_bound(const double *e) { return (e[0] - e[1]) + merit_atol(std::fabs(e[0]) + std::fabs(e[1])); }
// the search opens with the full step when the last iterate ended below it
inline bool ga_line_search_retries_full(const GaOpts &o, const GaMember &m) { return o.retry_full() && m.alpha < 1.0; }
// ... and the search is over when that step is accepted
inline bool ga_line_search_full_step(GaMember &m, double merit, double bound) {
    if (!(merit <= bound)) return false;
    m.alpha = 1.0;
    return true;
}
// a probe at x - alpha step: accepted (the next iterate starts from sqrt(alpha)) or backtracked
inline bool ga_line_search_probe(GaMember &m, double merit, double bound) {
    if (merit <= bound) { m.alpha = std::sqrt(m.alpha); return true; }
    m.alpha *= 0.1;
    return false;
}
// after a backtrack: the step has become too small to matter and is taken as it is (step_inf = |step|_inf)
inline bool ga_line_search_tiny_step(const GaOpts &o, const GaMember &m, double step_inf) { return m.alpha * step_inf < o.dec_tol / 1000; }

// ---- the verdict on an iterate, from its four reductions st = {score' step, |x_new - x|^2, |x|^2, (unused)} ------------------------------
// _predict_converged: the Newton decrement extrapolated one quadratically convergent step ahead, after two full steps
inline bool predict_converged(const GaOpts &o, const GaMember &m, long long iter) {
    return o.predictive() && iter > 1 && m.alpha == 1.0 && m.alpha_prev == 1.0 && m.dec * (m.dec / m.dec_prev) * (m.dec / m.dec_prev) < o.dec_tol;
}
enum GaVerdict { kGaContinue, kGaConverges, kGaLooksAhead };
// records dec; dec_prev is the caller's, at the end of an iterate that continues
inline GaVerdict ga_iterate_verdict(const GaOpts &o, GaMember &m, long long iter, const double *st) {
    m.dec = st[0];
    const double mean_change = std::sqrt(st[1]), mean_change_rel = mean_change / std::max(std::sqrt(st[2]), 1.0e-10);
    if (m.dec < o.dec_tol || mean_change < o.mean_tol || mean_change_rel < o.mean_tol) return kGaConverges;
    return predict_converged(o, m, iter) ? kGaLooksAhead : kGaContinue;
}
// _frozen_finish: the first chord step decides with its own decrement (a NaN does not converge); true records it
inline bool frozen_finish_decides(const GaOpts &o, GaMember &m, double dec) {
    if (!(dec < o.dec_tol)) return false;
    m.dec = dec;
    return true;
}
constexpr int kFrozenFinishSteps = 3;

// the eight numbers a loop reports per member
inline void ga_result_row(const GaMember &m, double *r) {
    const double row[8] = {(double)m.iters, m.status == kGaConverged ? 1.0 : 0.0, m.alpha, m.dec, m.nfact, m.nsolve, m.nmerit, m.frozen ? 1.0 : 0.0};
    std::copy(row, row + 8, r);
}

}  // namespace gmrfx
