// device_batch_fisher.cpp -- Fisher scoring for every member of a batched handle (include/gmrfx.h: gmrfx_batch_obs_set,
// gmrfx_batch_obs_set_design, gmrfx_batch_fisher_eval, gmrfx_batch_gaussian_approximation; kernels in fisher.hip and fisher_design.hip). The handle is the forest diag(Q_1 .. Q_B):
// the priors' values (set_prior on the forest) are the members' one after the other, refactorize_update_solve factors and solves all
// members in one pass, batch_diag reports per member. What is added here is the likelihood evaluation with per-member reductions and
// the loop that lets every member take its own line search and stop at its own iterate.
// THE LOCKSTEP INVARIANT. Member k sees exactly the sequence of operations Device::gaussian_approximation performs on a plain handle
// of Q_p,k and param[k]: the same evaluations at the same points, the same factorisations and solves, the same reductions, the same
// decisions. A step of the loop is ONE forest-wide launch masked to the members it concerns; a member that has stopped is masked out
// of every launch that writes its slices, its hess slice above all: every later forest factorisation then reproduces its factor bit
// for bit (a member's factor depends on its own values only), so it ends holding the factor of its own last iterate.
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

// dst = a device copy of cnt entries of src, on the handle's books
template <class B, class T> static void bf_up(B &dst, const T *src, size_t cnt, double *ledger) {
    dst.alloc(cnt, ledger, kTableMinBytes);
    if (cnt > 0) hip_check(hipMemcpy(dst, src, cnt * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
}

void Device::bobs_set(const RbmcSym &sym, const BObsHost &o) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("batch_obs_set: sharded handles are not supported");
    BFisherDev f;        // built aside: a failed upload leaves the previous likelihood in place
    if (o.nobs > 0) {
        const size_t n = (size_t)nmember_, nb = (size_t)nbatch_;
        if (n == 0 || n > (size_t)INT_MAX || o.param.size() != nb) throw std::invalid_argument("batch_obs_set: the likelihood does not belong to this handle");
        // what both forms hold: the members' parameters, the member's rows (the forest's first n: columns and positions of member 0
        // are the member's own), the loop's reductions, results and control words
        std::vector<double> lp(nb);
        for (size_t k = 0; k < nb; k++) lp[k] = fisher_logparam(o.family, o.param[k]);
        const size_t ne = (size_t)sym.rowptr[n];
        std::vector<int> pos(ne);
        for (size_t q = 0; q < ne; q++) pos[q] = (int)sym.pos[q];
        bf_up(f.param, o.param.data(), nb, &bytes_total);
        bf_up(f.logparam, lp.data(), nb, &bytes_total);
        bf_up(f.rp, reinterpret_cast<const long long *>(sym.rowptr.data()), n + 1, &bytes_total);
        bf_up(f.col, sym.col.data(), ne, &bytes_total);
        bf_up(f.pos, pos.data(), ne, &bytes_total);
        f.spart.alloc(4 * nb * (size_t)fisher_stat_blocks((int)n), &bytes_total, kTableMinBytes);
        f.out.alloc(6 * nb, &bytes_total, kTableMinBytes);
        f.ctl.alloc(2 * nb, &bytes_total, kTableMinBytes);
        f.h_out.alloc(6 * (long long)nb);
        f.h_ctl.alloc(2 * (long long)nb);
        f.family = o.family;
        f.loglik_const = o.loglik_const;
        if (o.design) bobs_set_design(o, f);
        else {          // node form: the data set by node, one (energy, loglik) pair per workgroup and member
            const ObsByNode b = obs_by_node(n, o.nobs, o.idx, o.y, o.aux);
            bf_up(f.y, b.y.data(), n, &bytes_total);
            bf_up(f.mask, b.mask.data(), n, &bytes_total);
            if (!b.aux.empty()) bf_up(f.aux, b.aux.data(), n, &bytes_total);
            f.part.alloc(2 * nb * (size_t)fisher_blocks((int)n), &bytes_total, kTableMinBytes);
        }
    }
    HC(hipStreamSynchronize(stream));
    bfisher_ = std::move(f);
    bprior_map_ok_ = -1;
}

void Device::bobs_set_param(const std::vector<double> &param, const std::vector<double> &loglik_const) {
    HC(hipSetDevice(device));
    const size_t nb = (size_t)nbatch_;
    if (!bobs_held() || param.size() != nb || loglik_const.size() != nb) throw std::invalid_argument("batch_obs_set_param: the parameters do not belong to this handle");
    std::vector<double> lp(nb);
    for (size_t k = 0; k < nb; k++) lp[k] = fisher_logparam(bfisher_.family, param[k]);
    HC(hipStreamSynchronize(stream));      // nothing in flight may still read the previous values
    HC(hipMemcpy(bfisher_.param, param.data(), nb * sizeof(double), hipMemcpyHostToDevice));
    HC(hipMemcpy(bfisher_.logparam, lp.data(), nb * sizeof(double), hipMemcpyHostToDevice));
    bfisher_.loglik_const = loglik_const;
}

// Design form, what it adds to bobs_set: the tables of design_upload once, ONE data set by observation, and every member's work:
// g, d (nobs), chunk sums (ncc + nct), energy and loglik partials (design_blocks of n and of nobs)
void Device::bobs_set_design(const BObsHost &o, BFisherDev &f) {
    const DesignPlan &P = *o.design;
    const size_t n = (size_t)nmember_, nb = (size_t)nbatch_, nobs = (size_t)P.nobs;
    if ((long long)n != P.n || o.y.size() != nobs) throw std::invalid_argument("batch_obs_set_design: the plan does not belong to this handle");
    bf_up(f.y, o.y.data(), nobs, &bytes_total);
    if (!o.aux.empty()) bf_up(f.aux, o.aux.data(), nobs, &bytes_total);
    design_upload(o.design, f);
    f.g.alloc(nobs * nb, &bytes_total, kTableMinBytes);
    f.d.alloc(nobs * nb, &bytes_total, kTableMinBytes);
    f.cpart.alloc((size_t)(f.ncc + f.nct) * nb, &bytes_total, kTableMinBytes);
    f.lpart.alloc((size_t)design_blocks((long long)nobs) * nb, &bytes_total, kTableMinBytes);
    f.part.alloc((size_t)design_blocks((long long)n) * nb, &bytes_total, kTableMinBytes);
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

void Device::bfisher_eval(const double *d_x, long long sx, const double *d_mu, long long smu, const unsigned char *d_active, double *d_score,
                          double *d_hess, long long ss, long long sh) {
    if (bfisher_.design) {
        const DesignPlan &P = *bfisher_.design;
        const BFisherDev &f = bfisher_;
        const FisherDesign a{(int)P.n, (int)P.nobs, (int)P.cnt, f.family, f.rp, f.col, f.pos, d_prior_, d_x, d_mu,
                             f.arp, f.acol, f.aval, f.offset.get(), f.acp, f.arow, f.acv, f.tptr, f.tobs, f.tw, f.cchoff, f.tchoff, f.chs, f.chl,
                             f.ncc, f.nct, f.y, f.aux.get(), 0.0, 0.0, f.g, f.d, f.cpart, d_score, d_hess, f.part, f.lpart,
                             nnz_member_, sx, smu, ss, sh, f.param, f.logparam, d_active};
        launch_fisher_design(stream, a, nbatch_, f.out);
        HC(hipMemcpyAsync(bfisher_.h_out, bfisher_.out, 2 * (size_t)nbatch_ * sizeof(double), hipMemcpyDeviceToHost, stream));
        HC(hipStreamSynchronize(stream));
        return;
    }
    const FisherEval a{(int)nmember_, bfisher_.family, bfisher_.rp, bfisher_.col, bfisher_.pos, d_prior_, d_x, d_mu, bfisher_.y,
                       bfisher_.aux.get(), bfisher_.mask, 0.0, 0.0, d_score, d_hess, bfisher_.part, nnz_member_, sx, smu, ss,
                       bfisher_.param, bfisher_.logparam, d_active};
    launch_fisher_eval(stream, a, nbatch_, bfisher_.out);
    HC(hipMemcpyAsync(bfisher_.h_out, bfisher_.out, 2 * (size_t)nbatch_ * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
}

void Device::batch_fisher_eval(const BEvalIO &io, double *out_host) {
    HC(hipSetDevice(device));
    if (!io.d_x || !out_host) throw std::invalid_argument("batch_fisher_eval: x / out is null");
    bfisher_check_prior();
    const int nb = nbatch_;
    const unsigned char *d_act = nullptr;
    if (io.active) {
        bfisher_ctl(nullptr, std::vector<unsigned char>(io.active, io.active + nb));
        d_act = reinterpret_cast<const unsigned char *>(bfisher_.ctl.get() + nb);
    }
    bfisher_eval(io.d_x, io.sx, io.d_mu, io.smu, d_act, io.d_score, io.d_hess, io.ss, io.sh);
    HC(hipGetLastError());
    for (int k = 0; k < nb; k++) {
        if (io.active && !io.active[k]) continue;
        out_host[2 * k] = bfisher_.h_out[2 * k];
        out_host[2 * k + 1] = bfisher_.h_out[2 * k + 1] + bfisher_.loglik_const[(size_t)k];
    }
}

int Device::batch_gaussian_approximation(const BGaIO &io, const GaOpts &o, double *result, double *totals, double *dec_trace, double *alpha_trace,
                                         long long *info, long long *cinfo, double *residual) {
    HC(hipSetDevice(device));
    if (!io.d_x || !result) throw std::invalid_argument("batch_gaussian_approximation: x / result is null");
    if (o.max_iter < 0 || o.max_ls < 0) throw std::invalid_argument("batch_gaussian_approximation: max_iter / max_linesearch_iter is negative");
    bfisher_check_prior();
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    const long long n = nmember_, N = S_->n;
    const int nb = nbatch_;
    const size_t nbytes = (size_t)n * sizeof(double);
    const bool adaptive = o.flags & 1, retry_full = o.flags & 2, predictive = o.flags & 4, refactor_final = o.flags & 8;
    // a member's Hessian vector: n entries in node form, the plan's cnt in design form (bobs_set drops the work area with the likelihood,
    // so it is sized for the form in place)
    const long long hl = bhess_len();
    if (!bfisher_.work) bfisher_.work.alloc(5 * (size_t)N + (size_t)hl * (size_t)nb, &bytes_total, kTableMinBytes);
    // xk: the iterates; cand: every candidate of the line search, so the accepted iterate of every member; xf: the frozen finish's
    // points. The chord steps of the look-ahead are solved into xk, which nobody reads between an iterate's reductions and the copy
    // cand -> xk that ends it: the steps and iterates of the members that did not fire stay as they are.
    double *xk = bfisher_.work, *cand = xk + N, *xf = xk + 2 * N, *step = xk + 3 * N, *score = xk + 4 * N, *hess = xk + 5 * N;
    for (int k = 0; k < nb; k++) {
        double *dst = xk + k * n;
        if (io.d_x0) HC(hipMemcpyAsync(dst, io.d_x0 + k * io.sx0, nbytes, hipMemcpyDeviceToDevice, stream));
        else if (io.d_mu) HC(hipMemcpyAsync(dst, io.d_mu + k * io.smu, nbytes, hipMemcpyDeviceToDevice, stream));
        else HC(hipMemsetAsync(dst, 0, nbytes, stream));
        if (info) info[k] = 0;
        if (cinfo) cinfo[k] = 0;
        if (residual) residual[k] = std::nan("");
    }
    const bool constrained = bcon_.m > 0;
    const long long tl = o.max_iter + 1;
    for (long long q = 0; q < tl * nb; q++) {
        if (dec_trace) dec_trace[q] = std::nan("");
        if (alpha_trace) alpha_trace[q] = std::nan("");
    }
    enum { kRun, kConverged, kMaxIter, kFailed };
    struct Member { int status = kRun; double alpha = 1.0, alpha_prev = 1.0, dec_prev = 0.0, dec = std::nan(""), nfact = 0, nsolve = 0, nmerit = 0;
                    long long iters = 0; bool frozen = false; };
    std::vector<Member> m((size_t)nb);
    double tot_fact = 0, tot_solve = 0, tot_eval = 0;
    bool wfail = false;      // some member's W_k = A Q_k^-1 A' was not positive definite
    std::vector<double> ev(2 * (size_t)nb), st(4 * (size_t)nb), al((size_t)nb, 1.0), obj_accept((size_t)nb), stepinf((size_t)nb);
    std::vector<long long> binfo((size_t)nb);
    const unsigned char *d_mask = reinterpret_cast<const unsigned char *>(bfisher_.ctl.get() + nb);
    const double *d_alpha = bfisher_.ctl;
    const FisherMembers masked{(int)n, nb, n, d_mask};      // the loop's vectors: member k's at + k n, the members of the mask on the device
    // out_k = x_k - alpha_k s_k with the step lengths of the control words
    auto candidate = [&](const double *x, const double *s, double *out) { launch_fisher_candidate(stream, masked, x, s, 0.0, d_alpha, out); };
    auto any = [](const std::vector<unsigned char> &v) { return std::find(v.begin(), v.end(), (unsigned char)1) != v.end(); };
    // an evaluation over the members of `mask` (already on the device): their pairs to ev
    auto eval = [&](const double *x, long long sx, double *sc, double *hs, const std::vector<unsigned char> &mask) {
        bfisher_eval(x, sx, io.d_mu, io.smu, d_mask, sc, hs, n, hl);
        tot_eval += 1;
        for (int k = 0; k < nb; k++)
            if (mask[(size_t)k]) { ev[2 * k] = bfisher_.h_out[2 * k]; ev[2 * k + 1] = bfisher_.h_out[2 * k + 1] + bfisher_.loglik_const[(size_t)k]; }
    };
    // the four reductions over the members of `mask`, to st
    auto stats = [&](const double *a, const double *b, const double *c, const double *d, const std::vector<unsigned char> &mask) {
        bfisher_ctl(nullptr, mask);
        launch_fisher_stats(stream, masked, a, b, c, d, bfisher_.spart, bfisher_.out.get() + 2 * nb);
        HC(hipMemcpyAsync(bfisher_.h_out + 2 * nb, bfisher_.out.get() + 2 * nb, 4 * (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
        HC(hipStreamSynchronize(stream));
        for (int k = 0; k < nb; k++)
            if (mask[(size_t)k]) std::copy(bfisher_.h_out + 2 * nb + 4 * k, bfisher_.h_out + 2 * nb + 4 * k + 4, st.begin() + 4 * k);
    };
    // candidates x_k - al[k] step_k into cand and the merit there, for the members of `mask`: merit to ev
    auto probe = [&](const std::vector<unsigned char> &mask) {
        bfisher_ctl(&al, mask);
        candidate(xk, step, cand);
        eval(cand, n, nullptr, nullptr, mask);
        for (int k = 0; k < nb; k++)
            if (mask[(size_t)k]) m[(size_t)k].nmerit += 1;
    };
    auto stop = [&](int k, int status, const double *x, long long iters, bool frozen) {
        Member &mk = m[(size_t)k];
        mk.status = status; mk.iters = iters; mk.frozen = frozen;
        HC(hipMemcpyAsync(io.d_x + k * io.sx, x + k * n, nbytes, hipMemcpyDeviceToDevice, stream));
    };
    // a member's constraint status: -1 beside a failed factorisation, 1 + the failing pivot of its W_k
    auto con_failed = [&](int k, long long c) { if (cinfo) cinfo[k] = c; };
    std::vector<unsigned char> run((size_t)nb, 1), mask((size_t)nb);
    for (long long iter = 1; iter <= o.max_iter && any(run); iter++) {
        bfisher_ctl(nullptr, run);
        eval(xk, n, score, hess, run);
        std::vector<double> ek = ev;
        refactorize_update_solve(hess, true, score, N, 1, step, N, true);
        tot_fact += 1; tot_solve += 1;
        batch_diag(nullptr, binfo.data());
        for (int k = 0; k < nb; k++) {
            if (!run[(size_t)k]) continue;
            Member &mk = m[(size_t)k];
            mk.nfact += 1; mk.nsolve += 1;
            if (binfo[(size_t)k] != 0) {
                if (info) info[k] = binfo[(size_t)k];
                con_failed(k, -1);
                stop(k, kFailed, xk, iter - 1, false);
                run[(size_t)k] = 0;
            }
            mk.alpha_prev = mk.alpha;
        }
        if (!any(run)) break;
        if (constrained) {
            // the step - At_k W_k^-1 (A step) of _workspace_constrain_with_matrix, on the operands of the factor in hand. The status
            // words are read before any correction is launched: a member whose W_k failed stops alone, masked out before
            // k_con_apply can see its NaN L_c^-1 (cinfo = -1 is a failed factorisation: the pivot report above has dealt with it)
            const std::vector<long long> &ci = bcon_prepare_members();
            for (int k = 0; k < nb; k++)
                if (run[(size_t)k] && ci[(size_t)k] > 0) {
                    con_failed(k, ci[(size_t)k]);
                    stop(k, kFailed, xk, iter - 1, false);
                    run[(size_t)k] = 0;
                    wfail = true;
                }
            if (!any(run)) break;
            bfisher_ctl(nullptr, run);
            bcon_project(step, n, d_mask);
        }
        if (adaptive) {
            // _ga_line_search per member, in rounds: a round forms the candidates of the members still searching and evaluates them
            bool have_inf = false;
            std::vector<unsigned char> searching = run, exhausted((size_t)nb, 0);
            std::vector<long long> ls((size_t)nb, 0);
            for (int k = 0; k < nb; k++)
                obj_accept[(size_t)k] = (ek[2 * k] - ek[2 * k + 1]) + merit_atol(std::fabs(ek[2 * k]) + std::fabs(ek[2 * k + 1]));
            if (retry_full) {       // round 0: the full step, for the members whose alpha is below 1
                for (int k = 0; k < nb; k++) { mask[(size_t)k] = run[(size_t)k] && m[(size_t)k].alpha < 1.0; al[(size_t)k] = 1.0; }
                if (any(mask)) {
                    probe(mask);
                    for (int k = 0; k < nb; k++)
                        if (mask[(size_t)k] && ev[2 * k] - ev[2 * k + 1] <= obj_accept[(size_t)k]) { m[(size_t)k].alpha = 1.0; searching[(size_t)k] = 0; }
                }
            }
            for (;;) {
                for (int k = 0; k < nb; k++) {
                    if (searching[(size_t)k] && ls[(size_t)k] >= o.max_ls) { searching[(size_t)k] = 0; exhausted[(size_t)k] = 1; }
                    al[(size_t)k] = m[(size_t)k].alpha;
                }
                if (!any(searching)) break;
                probe(searching);
                bool backtracked = false;
                for (int k = 0; k < nb; k++) {
                    if (!searching[(size_t)k]) continue;
                    Member &mk = m[(size_t)k];
                    ls[(size_t)k] += 1;
                    if (ev[2 * k] - ev[2 * k + 1] <= obj_accept[(size_t)k]) { mk.alpha = std::sqrt(mk.alpha); searching[(size_t)k] = 0; }
                    else { mk.alpha *= 0.1; backtracked = true; }
                }
                if (backtracked) {
                    if (!have_inf) {        // |step_k|_inf, once per iterate
                        stats(nullptr, step, nullptr, nullptr, run);
                        for (int k = 0; k < nb; k++) stepinf[(size_t)k] = st[4 * k + 3];
                        have_inf = true;
                    }
                    for (int k = 0; k < nb; k++)
                        if (searching[(size_t)k] && m[(size_t)k].alpha * stepinf[(size_t)k] < o.dec_tol / 1000) searching[(size_t)k] = 0;
                }
            }
            if (any(exhausted)) {
                bfisher_ctl(&al, exhausted);
                candidate(xk, step, cand);
            }
        } else {
            std::fill(al.begin(), al.end(), 1.0);
            bfisher_ctl(&al, run);
            candidate(xk, step, cand);
        }
        stats(score, step, cand, xk, run);
        std::vector<unsigned char> fire((size_t)nb, 0);
        for (int k = 0; k < nb; k++) {
            if (!run[(size_t)k]) continue;
            Member &mk = m[(size_t)k];
            mk.dec = st[4 * k];
            const double mean_change = std::sqrt(st[4 * k + 1]), mean_change_rel = mean_change / std::max(std::sqrt(st[4 * k + 2]), 1.0e-10);
            if (dec_trace) dec_trace[k * tl + iter - 1] = mk.dec;
            if (alpha_trace) alpha_trace[k * tl + iter - 1] = mk.alpha;
            if (mk.dec < o.dec_tol || mean_change < o.mean_tol || mean_change_rel < o.mean_tol) {
                stop(k, kConverged, cand, iter, false);
                run[(size_t)k] = 0;
            } else if (predictive && iter > 1 && mk.alpha == 1.0 && mk.alpha_prev == 1.0 &&
                       mk.dec * (mk.dec / mk.dec_prev) * (mk.dec / mk.dec_prev) < o.dec_tol)
                fire[(size_t)k] = 1;
        }
        // _predict_converged, then _frozen_finish for the members that fired: three chord steps on the factorisation in hand, only the
        // first decides, per member
        if (any(fire)) {
            for (int k = 0; k < nb; k++)
                if (fire[(size_t)k]) HC(hipMemcpyAsync(xf + k * n, cand + k * n, nbytes, hipMemcpyDeviceToDevice, stream));
            std::fill(al.begin(), al.end(), 1.0);
            for (int j = 1; j <= 3 && any(fire); j++) {
                bfisher_ctl(&al, fire);
                eval(xf, n, score, nullptr, fire);
                solve(score, N, 1, xk, N, true, 0);
                tot_solve += 1;
                if (constrained) bcon_project(xk, n, d_mask);      // (the same factor: the operands of this iterate; the mask is `fire`)
                for (int k = 0; k < nb; k++)
                    if (fire[(size_t)k]) m[(size_t)k].nsolve += 1;
                if (j == 1) {
                    stats(score, xk, nullptr, nullptr, fire);
                    for (int k = 0; k < nb; k++) {
                        if (!fire[(size_t)k]) continue;
                        if (!(st[4 * k] < o.dec_tol)) { fire[(size_t)k] = 0; continue; }
                        m[(size_t)k].dec = st[4 * k];
                        if (dec_trace) dec_trace[k * tl + iter] = st[4 * k];
                        if (alpha_trace) alpha_trace[k * tl + iter] = m[(size_t)k].alpha;
                    }
                    if (!any(fire)) break;
                    bfisher_ctl(&al, fire);
                }
                candidate(xf, xk, xf);
            }
            for (int k = 0; k < nb; k++)
                if (fire[(size_t)k]) { stop(k, kConverged, xf, iter + 1, true); run[(size_t)k] = 0; }
        }
        for (int k = 0; k < nb; k++)
            if (run[(size_t)k]) {
                m[(size_t)k].dec_prev = m[(size_t)k].dec;
                HC(hipMemcpyAsync(xk + k * n, cand + k * n, nbytes, hipMemcpyDeviceToDevice, stream));
            }
    }
    for (int k = 0; k < nb; k++)
        if (run[(size_t)k]) stop(k, kMaxIter, xk, o.max_iter, false);
    // energy, loglik and H at every member's x (_workspace_build_result); the stopped members' hess slices may be written now: the
    // only factorisation still to come is the one that wants them
    std::fill(mask.begin(), mask.end(), (unsigned char)1);
    bfisher_ctl(nullptr, mask);
    eval(io.d_x, io.sx, nullptr, hess, mask);
    int rc = 0;
    bool any_ok = false;
    for (int k = 0; k < nb; k++) {
        if (m[(size_t)k].status == kFailed) { rc = 1; continue; }
        any_ok = true;
        if (io.d_hess && hl > 0) HC(hipMemcpyAsync(io.d_hess + k * io.sh, hess + k * hl, (size_t)hl * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    if (refactor_final && any_ok) {
        refactorize_update(hess, true);
        tot_fact += 1;
        batch_diag(nullptr, binfo.data());
        for (int k = 0; k < nb; k++) {
            if (m[(size_t)k].status == kFailed) continue;
            m[(size_t)k].nfact += 1;
            if (binfo[(size_t)k] != 0) { if (info) info[k] = binfo[(size_t)k]; con_failed(k, -1); rc = 1; }
        }
    }
    if (constrained && residual && any_ok) {
        for (int k = 0; k < nb; k++) mask[(size_t)k] = m[(size_t)k].status != kFailed;
        bfisher_ctl(nullptr, mask);
        bcon_residual(io.d_x, io.sx, d_mask, mask.data(), residual);
    }
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    for (int k = 0; k < nb; k++) {
        const Member &mk = m[(size_t)k];
        const double r[10] = {(double)mk.iters, mk.status == kConverged ? 1.0 : 0.0, mk.alpha, mk.dec, mk.nfact, mk.nsolve, mk.nmerit,
                              mk.frozen ? 1.0 : 0.0, ev[2 * k], ev[2 * k + 1]};
        std::copy(r, r + 10, result + 10 * k);
    }
    if (totals) { totals[0] = tot_fact; totals[1] = tot_solve; totals[2] = tot_eval; }
    return wfail ? (rc | 2) : rc;
}

}  // namespace gmrfx
