// device_fisher.cpp -- the Device's side of Fisher scoring on the device (include/gmrfx.h: gmrfx_obs_set, gmrfx_fisher_eval; kernels in
// fisher.hip). The reference's loop (src/workspace/gaussian_approximation.jl:191-313) computes loggrad, loghessian, loglik and
// Q_p x - h on the host at every iterate; here the likelihood is state of the handle, expanded to one value per node, and one pass over
// Symmetric(Q_prior) (the values gmrfx_set_prior keeps) gives all four. Only two numbers reach the host.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>

#include "device.h"
#include "kernels.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

ObsByNode obs_by_node(size_t n, long long nobs, const std::vector<long long> &idx, const std::vector<double> &y, const std::vector<double> &aux) {
    ObsByNode b{std::vector<double>(n, 0.0), std::vector<double>(aux.empty() ? 0 : n, 0.0), std::vector<unsigned char>(n, 0)};
    for (long long k = 0; k < nobs; k++) {
        const size_t i = (size_t)idx[(size_t)k];
        b.y[i] = y[(size_t)k];
        if (!aux.empty()) b.aux[i] = aux[(size_t)k];
        b.mask[i] = 1;
    }
    return b;
}

void Device::obs_set(const ObsHost &o) {
    HC(hipSetDevice(device));
    if (sharded() || many_members()) throw std::invalid_argument("obs_set: batched and sharded handles are not supported");
    FisherDev f;         // built aside: a failed upload leaves the previous likelihood in place
    if (o.nobs > 0 && o.design) obs_set_design(o, f);
    else if (o.nobs > 0) {
        const size_t n = (size_t)S_->n;
        const ObsByNode b = obs_by_node(n, o.nobs, o.idx, o.y, o.aux);
        f.y.alloc(n, &bytes_total, kTableMinBytes);
        f.mask.alloc(n, &bytes_total, kTableMinBytes);
        HC(hipMemcpy(f.y, b.y.data(), n * sizeof(double), hipMemcpyHostToDevice));
        HC(hipMemcpy(f.mask, b.mask.data(), n, hipMemcpyHostToDevice));
        if (!b.aux.empty()) {
            f.aux.alloc(n, &bytes_total, kTableMinBytes);
            HC(hipMemcpy(f.aux, b.aux.data(), n * sizeof(double), hipMemcpyHostToDevice));
        }
        f.part.alloc(2 * (size_t)fisher_blocks((int)n), &bytes_total, kTableMinBytes);
        f.out.alloc(6, &bytes_total, kTableMinBytes);        // 2 of the evaluation, 4 of the reductions
        f.spart.alloc(4 * (size_t)fisher_stat_blocks((int)n), &bytes_total, kTableMinBytes);
        f.h_out.alloc(6);
        f.family = o.family;
        f.param = o.param;
        f.loglik_const = o.loglik_const;
    }
    HC(hipStreamSynchronize(stream));        // (an evaluation in flight on an external stream still reads the old arrays)
    fisher_ = std::move(f);
    gap_ = GapDev{};         // (the pullback's tables belong to the likelihood: rebuilt on its next call)
    pred_ = PredDev{};       // (and so do the predictive calls')
    prior_design_ = -1;
}

// dst = a device copy of src, on the handle's books (i64 and long long: the same 8 bytes)
template <class T, class U> static void fd_up(DevBuf<T> &dst, const std::vector<U> &src, double *ledger) {
    static_assert(sizeof(T) == sizeof(U), "fd_up copies bytes");
    dst.alloc(src.size(), ledger, kTableMinBytes);
    if (!src.empty()) hip_check(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
}

// The plan's tables as they are and the chunk tables of the segments longer than kDesignChunk, for a plain or a batched likelihood
void Device::design_upload(const std::shared_ptr<const DesignPlan> &plan, DesignTables &t) {
    const DesignPlan &P = *plan;
    fd_up(t.arp, P.rptr, &bytes_total);
    fd_up(t.acol, P.rcol, &bytes_total);
    fd_up(t.aval, P.rval, &bytes_total);
    fd_up(t.acp, P.cptr, &bytes_total);
    fd_up(t.arow, P.crow, &bytes_total);
    fd_up(t.acv, P.cval, &bytes_total);
    fd_up(t.tptr, P.tptr, &bytes_total);
    fd_up(t.tobs, P.tobs, &bytes_total);
    fd_up(t.tw, P.tw, &bytes_total);
    if (!P.offset.empty()) fd_up(t.offset, P.offset, &bytes_total);
    std::vector<int> cchoff((size_t)P.n + 1, 0), tchoff((size_t)P.cnt + 1, 0), chl;
    std::vector<long long> chs;
    auto cut = [&](const std::vector<i64> &ptr, std::vector<int> &choff) {
        for (size_t s = 0; s + 1 < ptr.size(); s++) {
            const long long len = ptr[s + 1] - ptr[s];
            const int nch = design_chunks(len);
            for (int c = 0; c < nch; c++) {
                chs.push_back(ptr[s] + (long long)c * kDesignChunk);
                chl.push_back((int)std::min<long long>(kDesignChunk, len - (long long)c * kDesignChunk));
            }
            choff[s + 1] = (int)chs.size();
        }
    };
    cut(P.cptr, cchoff);
    t.ncc = (int)chs.size();
    tchoff[0] = t.ncc;
    cut(P.tptr, tchoff);
    t.nct = (int)chs.size() - t.ncc;
    fd_up(t.cchoff, cchoff, &bytes_total);
    fd_up(t.tchoff, tchoff, &bytes_total);
    fd_up(t.chs, chs, &bytes_total);
    fd_up(t.chl, chl, &bytes_total);
    t.design = plan;
}

// Design form: the tables of design_upload, y / aux by observation, and one member's work
void Device::obs_set_design(const ObsHost &o, FisherDev &f) {
    const DesignPlan &P = *o.design;
    const size_t n = (size_t)S_->n, nobs = (size_t)P.nobs;
    if ((long long)n != P.n || n > (size_t)INT_MAX) throw std::invalid_argument("obs_set_design: the plan does not belong to this handle");
    fd_up(f.y, o.y, &bytes_total);
    if (!o.aux.empty()) fd_up(f.aux, o.aux, &bytes_total);
    design_upload(o.design, f);
    f.g.alloc(nobs, &bytes_total, kTableMinBytes);
    f.d.alloc(nobs, &bytes_total, kTableMinBytes);
    f.cpart.alloc((size_t)(f.ncc + f.nct), &bytes_total, kTableMinBytes);
    f.lpart.alloc((size_t)design_blocks((long long)nobs), &bytes_total, kTableMinBytes);
    f.part.alloc((size_t)design_blocks((long long)n), &bytes_total, kTableMinBytes);
    f.out.alloc(6, &bytes_total, kTableMinBytes);
    f.spart.alloc(4 * (size_t)fisher_stat_blocks((int)n), &bytes_total, kTableMinBytes);
    f.h_out.alloc(6);
    f.family = o.family;
    f.param = o.param;
    f.loglik_const = o.loglik_const;
}

void Device::fisher_eval_design(const RbmcSym &sym, const double *d_x, const double *d_mu, double *d_score, double *d_hess, double *out_host) {
    const DesignPlan &P = *fisher_.design;
    if (prior_design_ < 0) prior_design_ = (hmap_cnt_ == P.cnt && std::equal(P.map.begin(), P.map.end(), h_hmap_.begin())) ? 1 : 0;
    if (!prior_design_)
        throw std::invalid_argument("fisher_eval: the map of gmrfx_set_prior is not the map of gmrfx_obs_hess_map (the positions of A' D A, design form)");
    sym_rows_upload(sym);
    const FisherDesign a{(int)P.n, (int)P.nobs, (int)P.cnt, fisher_.family, sym_rows_.rp, sym_rows_.col, sym_rows_.pos, d_prior_, d_x, d_mu,
                         fisher_.arp, fisher_.acol, fisher_.aval, fisher_.offset.get(), fisher_.acp, fisher_.arow, fisher_.acv,
                         fisher_.tptr, fisher_.tobs, fisher_.tw, fisher_.cchoff, fisher_.tchoff, fisher_.chs, fisher_.chl, fisher_.ncc, fisher_.nct,
                         fisher_.y, fisher_.aux.get(), fisher_.param, fisher_logparam(fisher_.family, fisher_.param),
                         fisher_.g, fisher_.d, fisher_.cpart, d_score, d_hess, fisher_.part, fisher_.lpart};      // (one member: the rest stays zero)
    launch_fisher_design(stream, a, 1, fisher_.out);
    HC(hipMemcpyAsync(fisher_.h_out, fisher_.out, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    out_host[0] = fisher_.h_out[0];
    out_host[1] = fisher_.h_out[1] + fisher_.loglik_const;
}

void Device::fisher_eval(const RbmcSym &sym, const double *d_x, const double *d_mu, double *d_score, double *d_hess, double *out_host) {
    HC(hipSetDevice(device));
    if (sharded() || many_members()) throw std::invalid_argument("fisher_eval: batched and sharded handles are not supported");
    if (!d_x || !out_host) throw std::invalid_argument("fisher_eval: x / out is null");
    if (!d_prior_) throw std::invalid_argument("fisher_eval: gmrfx_set_prior has not been called");
    const long long n = S_->n;
    if (n > INT_MAX) throw std::invalid_argument("fisher_eval: more than 2^31 - 1 nodes");
    if (fisher_.design) return fisher_eval_design(sym, d_x, d_mu, d_score, d_hess, out_host);
    if (prior_diag_ < 0) {
        prior_diag_ = hmap_cnt_ == n ? 1 : 0;
        for (long long i = 0; i < n && prior_diag_; i++)
            if (h_hmap_[(size_t)i] != sym.diag[(size_t)i]) prior_diag_ = 0;
    }
    if (!prior_diag_) throw std::invalid_argument("fisher_eval: the map of gmrfx_set_prior is not the position of (i, i) for every i (diagonal Hessians only)");
    if (!obs_held()) throw std::invalid_argument("fisher_eval: no observation likelihood is set (gmrfx_obs_set)");
    sym_rows_upload(sym);
    // one member: the member fields stay zero (strides 0, the parameter by value, nobody masked)
    const FisherEval a{(int)n, fisher_.family, sym_rows_.rp, sym_rows_.col, sym_rows_.pos, d_prior_, d_x, d_mu, fisher_.y, fisher_.aux.get(),
                       fisher_.mask, fisher_.param, fisher_logparam(fisher_.family, fisher_.param), d_score, d_hess, fisher_.part};
    launch_fisher_eval(stream, a, 1, fisher_.out);
    HC(hipMemcpyAsync(fisher_.h_out, fisher_.out, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    out_host[0] = fisher_.h_out[0];
    out_host[1] = fisher_.h_out[1] + fisher_.loglik_const;
}

// ---- the loop ------------------------------------------------------------------------------------------------------------------------
int Device::gaussian_approximation(const RbmcSym &sym, const double *d_mu, const double *d_x0, const GaOpts &o, double *d_x, double *d_hess,
                                   double *result, double *dec_trace, double *alpha_trace, long long *info) {
    HC(hipSetDevice(device));
    if (!d_x || !result) throw std::invalid_argument("gaussian_approximation: x / result is null");
    if (o.max_iter < 0 || o.max_ls < 0) throw std::invalid_argument("gaussian_approximation: max_iter / max_linesearch_iter is negative");
    const long long n = S_->n;
    const size_t nb = (size_t)n * sizeof(double);
    const bool adaptive = o.flags & 1, retry_full = o.flags & 2, predictive = o.flags & 4, refactor_final = o.flags & 8;
    if (!d_prior_ || !obs_held()) {       // (the evaluation's own refusals, with its messages, before anything is allocated or written)
        double ev[2];
        fisher_eval(sym, d_x, d_mu, nullptr, nullptr, ev);
    }
    const long long hlen = hess_len();      // n in node form, the map's cnt in design form
    if (!fisher_.work) fisher_.work.alloc(5 * (size_t)n + (size_t)hlen, &bytes_total, kTableMinBytes);
    double *xk = fisher_.work, *xnew = xk + n, *cand = xk + 2 * n, *step = xk + 3 * n, *score = xk + 4 * n, *hess = xk + 5 * n;
    if (d_x0) HC(hipMemcpyAsync(xk, d_x0, nb, hipMemcpyDeviceToDevice, stream));
    else if (d_mu) HC(hipMemcpyAsync(xk, d_mu, nb, hipMemcpyDeviceToDevice, stream));
    else HC(hipMemsetAsync(xk, 0, nb, stream));
    if (info) *info = 0;
    for (long long k = 0; k <= o.max_iter; k++) {
        if (dec_trace) dec_trace[k] = std::nan("");
        if (alpha_trace) alpha_trace[k] = std::nan("");
    }
    double nfact = 0, nsolve = 0, nmerit = 0, alpha = 1.0, dec_prev = 0.0, dec = std::nan("");
    const FisherMembers one{(int)n, 1, 0, nullptr};       // the loop's vectors are one member's
    // out = x - al step (al changes between launches: by value, nothing goes up)
    auto candidate = [&](const double *x, double al, double *out) { launch_fisher_candidate(stream, one, x, step, al, nullptr, out); };
    // the four reductions of the loop, to the host: {sum a b, sum (c - d)^2, sum d^2, max |b|}
    auto stats = [&](const double *a, const double *b, const double *c, const double *d, double *out4) {
        launch_fisher_stats(stream, one, a, b, c, d, fisher_.spart, fisher_.out.get() + 2);
        HC(hipMemcpyAsync(fisher_.h_out + 2, fisher_.out.get() + 2, 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
        HC(hipStreamSynchronize(stream));
        for (int q = 0; q < 4; q++) out4[q] = fisher_.h_out[2 + q];
    };
    auto merit = [&](const double *x) {
        double e[2];
        fisher_eval(sym, x, d_mu, nullptr, nullptr, e);
        nmerit += 1;
        return e[0] - e[1];
    };
    // the step - A~' W^-1 (A step) of _workspace_constrain_with_matrix; false: W is not positive definite
    auto project = [&](double *s) {
        if (con_.m <= 0) return true;
        if (!con_prepare()) return false;
        con_correct(s, n, 1, nullptr, true);
        return true;
    };
    auto finish = [&](const double *xfinal, long long iters, bool converged, bool frozen, bool failed = false) -> int {
        HC(hipMemcpyAsync(d_x, xfinal, nb, hipMemcpyDeviceToDevice, stream));
        int rc = 0;
        if (!failed && (d_hess || refactor_final)) {
            double e[2];
            fisher_eval(sym, xfinal, d_mu, nullptr, hess, e);      // the final H(x_final) (_workspace_build_result)
            if (d_hess && hlen > 0) HC(hipMemcpyAsync(d_hess, hess, (size_t)hlen * sizeof(double), hipMemcpyDeviceToDevice, stream));
            if (refactor_final) {
                refactorize_update(hess, true);
                nfact += 1;
                const long long fc = fail_col();
                if (fc >= 0) { if (info) *info = fc + 1; rc = 1; }
            }
        }
        HC(hipStreamSynchronize(stream));
        const double r[8] = {(double)iters, converged ? 1.0 : 0.0, alpha, dec, nfact, nsolve, nmerit, frozen ? 1.0 : 0.0};
        std::copy(r, r + 8, result);
        return rc;
    };
    for (long long iter = 1; iter <= o.max_iter; iter++) {
        double ek[2], st[4];
        fisher_eval(sym, xk, d_mu, score, hess, ek);
        refactorize_update_solve(hess, true, score, n, 1, step, n, true);
        nfact += 1; nsolve += 1;
        const long long fc = fail_col();
        if (fc >= 0) {
            if (info) *info = fc + 1;
            finish(xk, iter - 1, false, false, true);
            return 1;
        }
        if (!project(step)) { finish(xk, iter - 1, false, false, true); return 2; }
        const double alpha_prev = alpha;
        const double *xn = xnew;
        if (adaptive) {
            // _ga_line_search, line by line
            const double obj_current = ek[0] - ek[1];
            const double obj_accept = obj_current + merit_atol(std::fabs(ek[0]) + std::fabs(ek[1]));
            bool done = false;
            if (retry_full && alpha < 1.0) {
                candidate(xk, 1.0, xnew);
                if (merit(xnew) <= obj_accept) { alpha = 1.0; done = true; }
            }
            if (!done) {
                bool accept = false;
                for (long long ls = 1; ls <= o.max_ls; ls++) {
                    candidate(xk, alpha, cand);
                    if (merit(cand) <= obj_accept) {
                        alpha = std::sqrt(alpha);
                        accept = true;
                        break;
                    }
                    alpha *= 0.1;
                    stats(nullptr, step, nullptr, nullptr, st);
                    if (alpha * st[3] < o.dec_tol / 1000) { accept = true; break; }
                }
                if (accept) xn = cand;
                else candidate(xk, alpha, xnew);
            }
        } else candidate(xk, 1.0, xnew);
        stats(score, step, xn, xk, st);
        dec = st[0];
        const double mean_change = std::sqrt(st[1]), mean_change_rel = mean_change / std::max(std::sqrt(st[2]), 1.0e-10);
        if (dec_trace) dec_trace[iter - 1] = dec;
        if (alpha_trace) alpha_trace[iter - 1] = alpha;
        if (dec < o.dec_tol || mean_change < o.mean_tol || mean_change_rel < o.mean_tol) return finish(xn, iter, true, false);
        // _predict_converged, then _frozen_finish: three chord steps on the factorisation in hand, only the first decides
        if (predictive && iter > 1 && alpha == 1.0 && alpha_prev == 1.0 && dec * (dec / dec_prev) * (dec / dec_prev) < o.dec_tol) {
            double *xf = xn == cand ? xnew : cand;          // (the accepted iterate stays where it is until the look-ahead has decided)
            HC(hipMemcpyAsync(xf, xn, nb, hipMemcpyDeviceToDevice, stream));
            bool ok = true;
            for (int j = 1; j <= 3 && ok; j++) {
                double e[2];
                fisher_eval(sym, xf, d_mu, score, nullptr, e);
                solve(score, n, 1, step, n, true, 0);
                nsolve += 1;
                if (!project(step)) { finish(xn, iter, false, false, true); return 2; }
                if (j == 1) {
                    stats(score, step, nullptr, nullptr, st);
                    if (!(st[0] < o.dec_tol)) { ok = false; break; }
                    dec = st[0];
                    if (dec_trace) dec_trace[iter] = dec;
                    if (alpha_trace) alpha_trace[iter] = alpha;
                }
                candidate(xf, 1.0, xf);
            }
            if (ok) return finish(xf, iter + 1, true, true);
        }
        dec_prev = dec;
        if (xn != xk) HC(hipMemcpyAsync(xk, xn, nb, hipMemcpyDeviceToDevice, stream));
    }
    return finish(xk, o.max_iter, false, false);
}

}  // namespace gmrfx
