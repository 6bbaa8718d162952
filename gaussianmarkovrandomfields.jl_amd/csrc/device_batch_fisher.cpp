// device_batch_fisher.cpp -- Fisher scoring for every member of a batched handle (include/gmrfx.h: gmrfx_batch_obs_set,
// gmrfx_batch_obs_set_design, gmrfx_batch_fisher_eval, gmrfx_batch_gaussian_approximation; kernels in fisher.hip and fisher_design.hip).
// The handle is the forest diag(Q_1 .. Q_B): the priors' values (set_prior on the forest) are the members' one after the other,
// refactorize_update_solve factors and solves all members in one pass, batch_diag reports per member. The likelihood's state, its
// builder and the evaluation are those of device_fisher.cpp with a member count; what is added here is the members' control words and
// the loop that lets every member take its own line search and stop at its own iterate.
// THE LOCKSTEP INVARIANT. Member k sees exactly the sequence of operations Device::gaussian_approximation performs on a plain handle
// of Q_p,k and param[k]: the same evaluations at the same points, the same factorisations and solves, the same reductions, the same
// decisions. The decisions are the same by construction: both loops drive GaMember through the functions of ga_rules.h. What is kept
// by hand is the ORDER of operations: each named step below issues, for the members it concerns, what the plain loop issues at that
// place. A step is ONE forest-wide launch masked to those members; a member that has stopped is masked out of every launch that
// writes its slices, its hess slice above all: every later forest factorisation then reproduces its factor bit for bit (a member's
// factor depends on its own values only), so it ends holding the factor of its own last iterate.
// CONSTRAINTS (gmrfx_batch_constrained_gaussian_approximation). With a batch constraint held every step is projected,
// s_k <- s_k - At_k W_k^-1 (A s_k), where the plain loop projects it: after the refactorize_update_solve of an iterate and after each
// chord solve of the frozen finish, by the masked launches of constraint.hip (bcon_project). bcon_prepare runs once per iterate, forest
// wide: a stopped member's factor is reproduced bit for bit, so its At_k, W_k and B_k are too, and it ends holding the operands of its
// own last iterate. A member whose W_k fails is read on the host and masked out before any correction launch; it stops alone.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>

#include "device.h"
#include "kernels.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

void Device::bobs_set(const RbmcSym &sym, const BObsHost &o) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("batch_obs_set: sharded handles are not supported");
    FisherDev f;        // built aside: a failed upload leaves the previous likelihood in place
    if (o.nobs > 0) {
        const size_t n = (size_t)nmember_, nb = (size_t)nbatch_;
        if (n == 0 || n > (size_t)INT_MAX || o.param.size() != nb) throw std::invalid_argument("batch_obs_set: the likelihood does not belong to this handle");
        if (o.design && ((long long)n != o.design->n || o.y.size() != (size_t)o.design->nobs))
            throw std::invalid_argument("batch_obs_set_design: the plan does not belong to this handle");
        const ObsByNode b = o.design ? ObsByNode{} : obs_by_node(n, o.nobs, o.idx, o.y, o.aux);
        f = fisher_build(FisherSource{o.family, &b, &o.y, &o.aux, o.design, o.param, o.loglik_const}, n, &sym);
    }
    HC(hipStreamSynchronize(stream));
    bfisher_ = std::move(f);
    bgap_ = GapDev{};        // (the batched pullback's tables belong to the likelihood: rebuilt on its next call)
    bpred_ = PredDev{};      // (and so do the batched predictive calls')
    bprior_map_ok_ = -1;
}

void Device::bobs_set_param(const std::vector<double> &param, const std::vector<double> &loglik_const) {
    HC(hipSetDevice(device));
    const size_t nb = (size_t)nbatch_;
    if (!bobs_held() || param.size() != nb || loglik_const.size() != nb) throw std::invalid_argument("batch_obs_set_param: the parameters do not belong to this handle");
    std::vector<double> lp(nb);
    for (size_t k = 0; k < nb; k++) lp[k] = fisher_logparam(bfisher_.family, param[k]);
    HC(hipStreamSynchronize(stream));      // nothing in flight may still read the previous values
    HC(hipMemcpy(bfisher_.param_k, param.data(), nb * sizeof(double), hipMemcpyHostToDevice));
    HC(hipMemcpy(bfisher_.logparam_k, lp.data(), nb * sizeof(double), hipMemcpyHostToDevice));
    bfisher_.loglik_const = loglik_const;
    bpred_ = PredDev{};      // (the constants of the pointwise log density belong to the parameters: rebuilt on the next predictive call)
}

void Device::bset_prior(const double *prior_nzval, const std::vector<long long> &map, bool design) {
    set_prior(prior_nzval, map.data(), (long long)map.size());
    bprior_design_ = design;
}

// the map of set_prior must be the one the likelihood in place needs, member after member (what gmrfx_batch_set_prior installs): the
// forest's diagonal in node form, the plan's map shifted by k nnz_member in design form
void Device::bfisher_check_prior() {
    if (!d_prior_) throw std::invalid_argument("batch_fisher_eval: gmrfx_batch_set_prior has not been called");
    if (!bobs_held()) throw std::invalid_argument("batch_fisher_eval: no observation likelihood is set (gmrfx_batch_obs_set)");
    if (bfisher_.design) {
        const DesignPlan &P = *bfisher_.design;
        if (bprior_map_ok_ < 0)
            bprior_map_ok_ = (bprior_design_ && hmap_cnt_ == P.cnt * nbatch_ && std::equal(P.map.begin(), P.map.end(), h_hmap_.begin())) ? 1 : 0;
        if (!bprior_map_ok_)
            throw std::invalid_argument("batch_fisher_eval: the map of the prior is not the one of the design likelihood in place (call "
                                        "gmrfx_batch_set_prior again after changing the likelihood's form)");
    } else if (bprior_design_ || hmap_cnt_ != S_->n)
        throw std::invalid_argument("batch_fisher_eval: the map of the prior is not the members' diagonals (call gmrfx_batch_set_prior again after "
                                    "changing the likelihood's form; it installs the map)");
}

// the control words of the next launches: nbatch step lengths (nullable: kept), then the mask bytes. The pinned copy is rewritten
// only behind a synchronisation: a copy enqueued earlier may still be reading it.
void Device::bfisher_ctl(const std::vector<double> *alpha, const std::vector<unsigned char> &mask) {
    const size_t nb = (size_t)nbatch_;
    HC(hipStreamSynchronize(stream));
    unsigned char *hm = reinterpret_cast<unsigned char *>(bfisher_.h_ctl + nb);
    std::copy(mask.begin(), mask.end(), hm);
    if (alpha) {
        std::copy(alpha->begin(), alpha->end(), (double *)bfisher_.h_ctl);
        HC(hipMemcpyAsync(bfisher_.ctl, bfisher_.h_ctl, nb * sizeof(double) + nb, hipMemcpyHostToDevice, stream));
    } else HC(hipMemcpyAsync(bfisher_.ctl.get() + nb, hm, nb, hipMemcpyHostToDevice, stream));
}

void Device::batch_fisher_eval(const BEvalIO &io, double *out_host) {
    HC(hipSetDevice(device));
    if (!io.d_x || !out_host) throw std::invalid_argument("batch_fisher_eval: x / out is null");
    bfisher_check_prior();
    const unsigned char *d_act = nullptr;
    if (io.active) {
        bfisher_ctl(nullptr, std::vector<unsigned char>(io.active, io.active + nbatch_));
        d_act = reinterpret_cast<const unsigned char *>(bfisher_.ctl.get() + nbatch_);
    }
    fisher_launch(bfisher_, FisherRows{bfisher_.rp, bfisher_.col, bfisher_.pos},
                  FisherIO{io.d_x, io.sx, io.d_mu, io.smu, io.d_score, io.d_hess, io.ss, io.sh, d_act}, io.active, out_host);
}

int Device::batch_gaussian_approximation(const BGaIO &io, const GaOpts &o, double *result, double *totals, double *dec_trace, double *alpha_trace,
                                         long long *info, long long *cinfo, double *residual) {
    HC(hipSetDevice(device));
    if (!io.d_x || !result) throw std::invalid_argument("batch_gaussian_approximation: x / result is null");
    if (o.max_iter < 0 || o.max_ls < 0) throw std::invalid_argument("batch_gaussian_approximation: max_iter / max_linesearch_iter is negative");
    bfisher_check_prior();
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    const long long n = nmember_, N = S_->n;
    const size_t nb = (size_t)nbatch_;
    const size_t nbytes = (size_t)n * sizeof(double);
    // a member's Hessian vector: n entries in node form, the plan's cnt in design form (bobs_set drops the work area with the likelihood,
    // so it is sized for the form in place)
    const long long hl = bhess_len();
    if (!bfisher_.work) bfisher_.work.alloc(5 * (size_t)N + (size_t)hl * nb, &bytes_total, kTableMinBytes);
    // xk: the iterates; cand: every candidate of the line search, so the accepted iterate of every member; xf: the frozen finish's
    // points. The chord steps of the look-ahead are solved into xk, which nobody reads between an iterate's reductions and the copy
    // cand -> xk that ends it: the steps and iterates of the members that did not fire stay as they are.
    double *xk = bfisher_.work, *cand = xk + N, *xf = xk + 2 * N, *step = xk + 3 * N, *score = xk + 4 * N, *hess = xk + 5 * N;
    for (size_t k = 0; k < nb; k++) {
        double *dst = xk + k * n;
        if (io.d_x0) HC(hipMemcpyAsync(dst, io.d_x0 + k * io.sx0, nbytes, hipMemcpyDeviceToDevice, stream));
        else if (io.d_mu) HC(hipMemcpyAsync(dst, io.d_mu + k * io.smu, nbytes, hipMemcpyDeviceToDevice, stream));
        else HC(hipMemsetAsync(dst, 0, nbytes, stream));
        if (info) info[k] = 0;
        if (cinfo) cinfo[k] = 0;
        if (residual) residual[k] = std::nan("");
    }
    const bool constrained = bcon_.m > 0;
    const size_t tl = (size_t)o.max_iter + 1;
    for (size_t q = 0; q < tl * nb; q++) {
        if (dec_trace) dec_trace[q] = std::nan("");
        if (alpha_trace) alpha_trace[q] = std::nan("");
    }
    using Mask = std::vector<unsigned char>;
    std::vector<GaMember> m(nb);
    double tot_fact = 0, tot_solve = 0, tot_eval = 0;
    bool wfail = false;      // some member's W_k = A Q_k^-1 A' was not positive definite
    std::vector<double> ev(2 * nb), ek, st(4 * nb), al(nb, 1.0), bound(nb), stepinf(nb);
    std::vector<long long> binfo(nb);
    Mask run(nb, 1), mask(nb), fire(nb);
    const unsigned char *d_mask = reinterpret_cast<const unsigned char *>(bfisher_.ctl.get() + nb);
    const double *d_alpha = bfisher_.ctl;
    const FisherMembers masked{(int)n, (int)nb, n, d_mask};      // the loop's vectors: member k's at + k n, the members of the mask on the device
    const FisherRows rows{bfisher_.rp, bfisher_.col, bfisher_.pos};
    auto any = [](const Mask &v) { return std::find(v.begin(), v.end(), (unsigned char)1) != v.end(); };
    auto each = [&](const Mask &sel, auto &&f) { for (size_t k = 0; k < nb; k++) if (sel[k]) f(k); };
    // out_k = x_k - alpha_k s_k with the step lengths of the control words
    auto candidate = [&](const double *x, const double *s, double *out) { launch_fisher_candidate(stream, masked, x, s, 0.0, d_alpha, out); };
    // an evaluation over the members of `sel` (already on the device): their pairs to ev
    auto eval = [&](const double *x, long long sx, double *sc, double *hs, const Mask &sel) {
        fisher_launch(bfisher_, rows, FisherIO{x, sx, io.d_mu, io.smu, sc, hs, n, hl, d_mask}, sel.data(), ev.data());
        tot_eval += 1;
    };
    // the four reductions over the members of `sel`, to st
    auto stats = [&](const double *a, const double *b, const double *c, const double *d, const Mask &sel) {
        bfisher_ctl(nullptr, sel);
        fisher_stats(bfisher_, masked, a, b, c, d, sel.data(), st.data());
    };
    // candidates x_k - al[k] step_k into cand and the merit there, for the members of `sel`: merit to ev
    auto probe = [&](const Mask &sel) {
        bfisher_ctl(&al, sel);
        candidate(xk, step, cand);
        eval(cand, n, nullptr, nullptr, sel);
        each(sel, [&](size_t k) { m[k].nmerit += 1; });
    };
    auto trace = [&](size_t k, long long at) {
        if (dec_trace) dec_trace[k * tl + at] = m[k].dec;
        if (alpha_trace) alpha_trace[k * tl + at] = m[k].alpha;
    };
    auto stop = [&](size_t k, int status, const double *x, long long iters, bool frozen) {
        ga_stop(m[k], status, iters, frozen);
        run[k] = 0;
        HC(hipMemcpyAsync(io.d_x + k * io.sx, x + k * n, nbytes, hipMemcpyDeviceToDevice, stream));
    };
    // a member's constraint status: -1 beside a failed factorisation, 1 + the failing pivot of its W_k
    auto con_failed = [&](size_t k, long long c) { if (cinfo) cinfo[k] = c; };

    // ---- the steps of an iterate, for the members of `run` -----------------------------------------------------------------------------
    auto evaluate_factor_solve = [&](long long iter) {
        bfisher_ctl(nullptr, run);
        eval(xk, n, score, hess, run);
        ek = ev;
        refactorize_update_solve(hess, true, score, N, 1, step, N, true);
        tot_fact += 1; tot_solve += 1;
        batch_diag(nullptr, binfo.data());
        each(run, [&](size_t k) {
            ga_iterate_begun(m[k]);
            if (binfo[k] == 0) return;
            if (info) info[k] = binfo[k];
            con_failed(k, -1);
            stop(k, kGaFailed, xk, iter - 1, false);
        });
    };
    // the step - At_k W_k^-1 (A step) of _workspace_constrain_with_matrix, on the operands of the factor in hand. The status words are
    // read before any correction is launched: a member whose W_k failed stops alone, masked out before k_con_apply can see its NaN
    // L_c^-1 (cinfo = -1 is a failed factorisation: the pivot report above has dealt with it)
    auto project = [&](long long iter) {
        const std::vector<long long> &ci = bcon_prepare_members();
        each(run, [&](size_t k) {
            if (ci[k] <= 0) return;
            con_failed(k, ci[k]);
            stop(k, kGaFailed, xk, iter - 1, false);
            wfail = true;
        });
        if (!any(run)) return;
        bfisher_ctl(nullptr, run);
        bcon_project(step, n, d_mask);
    };
    // _ga_line_search per member, in rounds: a round forms the candidates of the members still searching and evaluates them
    auto line_search = [&]() {
        bool have_inf = false;
        Mask searching = run, exhausted(nb, 0);
        std::vector<long long> ls(nb, 0);
        for (size_t k = 0; k < nb; k++) {       // round 0: the full step, for the members that retry it
            bound[k] = ga_line_search_bound(&ek[2 * k]);
            mask[k] = run[k] && ga_line_search_retries_full(o, m[k]);
            al[k] = 1.0;
        }
        if (any(mask)) {
            probe(mask);
            each(mask, [&](size_t k) { if (ga_line_search_full_step(m[k], ga_merit(&ev[2 * k]), bound[k])) searching[k] = 0; });
        }
        for (;;) {
            for (size_t k = 0; k < nb; k++) {
                if (searching[k] && ls[k] >= o.max_ls) { searching[k] = 0; exhausted[k] = 1; }
                al[k] = m[k].alpha;
            }
            if (!any(searching)) break;
            probe(searching);
            bool backtracked = false;
            each(searching, [&](size_t k) {
                ls[k] += 1;
                if (ga_line_search_probe(m[k], ga_merit(&ev[2 * k]), bound[k])) searching[k] = 0;
                else backtracked = true;
            });
            if (!backtracked) continue;
            if (!have_inf) {        // |step_k|_inf, once per iterate
                stats(nullptr, step, nullptr, nullptr, run);
                for (size_t k = 0; k < nb; k++) stepinf[k] = st[4 * k + 3];
                have_inf = true;
            }
            each(searching, [&](size_t k) { if (ga_line_search_tiny_step(o, m[k], stepinf[k])) searching[k] = 0; });
        }
        if (any(exhausted)) {
            bfisher_ctl(&al, exhausted);
            candidate(xk, step, cand);
        }
    };
    auto full_step = [&]() {
        std::fill(al.begin(), al.end(), 1.0);
        bfisher_ctl(&al, run);
        candidate(xk, step, cand);
    };
    // the verdict on every member's iterate: converged members stop, `fire` gets those whose look-ahead fires
    auto iterate_verdicts = [&](long long iter) {
        stats(score, step, cand, xk, run);
        std::fill(fire.begin(), fire.end(), (unsigned char)0);
        each(run, [&](size_t k) {
            const GaVerdict v = ga_iterate_verdict(o, m[k], iter, &st[4 * k]);
            trace(k, iter - 1);
            if (v == kGaConverges) stop(k, kGaConverged, cand, iter, false);
            else if (v == kGaLooksAhead) fire[k] = 1;
        });
    };
    // _predict_converged has fired, _frozen_finish for those members: chord steps on the factorisation in hand, only the first
    // decides, per member
    auto frozen_finish = [&](long long iter) {
        each(fire, [&](size_t k) { HC(hipMemcpyAsync(xf + k * n, cand + k * n, nbytes, hipMemcpyDeviceToDevice, stream)); });
        std::fill(al.begin(), al.end(), 1.0);
        for (int j = 1; j <= kFrozenFinishSteps && any(fire); j++) {
            bfisher_ctl(&al, fire);
            eval(xf, n, score, nullptr, fire);
            solve(score, N, 1, xk, N, true, 0);
            tot_solve += 1;
            if (constrained) bcon_project(xk, n, d_mask);      // (the same factor: the operands of this iterate; the mask is `fire`)
            each(fire, [&](size_t k) { m[k].nsolve += 1; });
            if (j == 1) {
                stats(score, xk, nullptr, nullptr, fire);
                each(fire, [&](size_t k) {
                    if (frozen_finish_decides(o, m[k], st[4 * k])) trace(k, iter);
                    else fire[k] = 0;
                });
                if (!any(fire)) break;
                bfisher_ctl(&al, fire);
            }
            candidate(xf, xk, xf);
        }
        each(fire, [&](size_t k) { stop(k, kGaConverged, xf, iter + 1, true); });
    };
    // energy, loglik and H at every member's x (_workspace_build_result), the final factorisation and the residuals; the stopped
    // members' hess slices may be written now: the only factorisation still to come is the one that wants them
    auto final_readouts = [&]() {
        std::fill(mask.begin(), mask.end(), (unsigned char)1);
        bfisher_ctl(nullptr, mask);
        eval(io.d_x, io.sx, nullptr, hess, mask);
        int rc = 0;
        for (size_t k = 0; k < nb; k++) {
            mask[k] = m[k].status != kGaFailed;
            if (!mask[k]) rc = 1;
            else if (io.d_hess && hl > 0) HC(hipMemcpyAsync(io.d_hess + k * io.sh, hess + k * hl, (size_t)hl * sizeof(double), hipMemcpyDeviceToDevice, stream));
        }
        if (o.refactor_final() && any(mask)) {
            refactorize_update(hess, true);
            tot_fact += 1;
            batch_diag(nullptr, binfo.data());
            each(mask, [&](size_t k) {
                m[k].nfact += 1;
                if (binfo[k] != 0) { if (info) info[k] = binfo[k]; con_failed(k, -1); rc = 1; }
            });
        }
        if (constrained && residual && any(mask)) {
            bfisher_ctl(nullptr, mask);
            bcon_residual(io.d_x, io.sx, d_mask, mask.data(), residual);
        }
        return rc;
    };

    for (long long iter = 1; iter <= o.max_iter && any(run); iter++) {
        evaluate_factor_solve(iter);
        if (constrained && any(run)) project(iter);
        if (!any(run)) break;
        if (o.adaptive()) line_search();
        else full_step();
        iterate_verdicts(iter);
        if (any(fire)) frozen_finish(iter);
        each(run, [&](size_t k) {
            m[k].dec_prev = m[k].dec;
            HC(hipMemcpyAsync(xk + k * n, cand + k * n, nbytes, hipMemcpyDeviceToDevice, stream));
        });
    }
    each(run, [&](size_t k) { stop(k, kGaMaxIter, xk, o.max_iter, false); });
    const int rc = final_readouts();
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    for (size_t k = 0; k < nb; k++) {      // the plain loop's eight, then energy and loglik at the member's x
        ga_result_row(m[k], result + 10 * k);
        result[10 * k + 8] = ev[2 * k];
        result[10 * k + 9] = ev[2 * k + 1];
    }
    if (totals) { totals[0] = tot_fact; totals[1] = tot_solve; totals[2] = tot_eval; }
    return wfail ? (rc | 2) : rc;
}

}  // namespace gmrfx
