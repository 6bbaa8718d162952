// device_fisher.cpp -- the Device's side of Fisher scoring on the device (include/gmrfx.h: gmrfx_obs_set, gmrfx_fisher_eval; kernels in
// fisher.hip and fisher_design.hip). The reference's loop (src/workspace/gaussian_approximation.jl:191-313) computes loggrad, loghessian,
// loglik and Q_p x - h on the host at every iterate; here the likelihood is state of the handle, expanded to one value per node, and one
// pass over Symmetric(Q_prior) (the values gmrfx_set_prior keeps) gives all four. Only two numbers reach the host.
// What the plain and the batched likelihood share is here: the one state (FisherDev) with its builder, the one evaluation routine that
// fills the kernels' arguments, and the read-back of the loop's reductions. device_batch_fisher.cpp adds the members' side.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>
#include <string>

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

// The plan's tables as they are and the chunk tables of the segments longer than kDesignChunk, for a plain or a batched likelihood
void Device::design_upload(const std::shared_ptr<const DesignPlan> &plan, DesignTables &t) {
    const DesignPlan &P = *plan;
    dev_upload(t.arp, P.rptr, &bytes_total);
    dev_upload(t.acol, P.rcol, &bytes_total);
    dev_upload(t.aval, P.rval, &bytes_total);
    dev_upload(t.acp, P.cptr, &bytes_total);
    dev_upload(t.arow, P.crow, &bytes_total);
    dev_upload(t.acv, P.cval, &bytes_total);
    dev_upload(t.tptr, P.tptr, &bytes_total);
    dev_upload(t.tobs, P.tobs, &bytes_total);
    dev_upload(t.tw, P.tw, &bytes_total);
    if (!P.offset.empty()) dev_upload(t.offset, P.offset, &bytes_total);
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
    dev_upload(t.cchoff, cchoff, &bytes_total);
    dev_upload(t.tchoff, tchoff, &bytes_total);
    dev_upload(t.chs, chs, &bytes_total);
    dev_upload(t.chl, chl, &bytes_total);
    t.design = plan;
}

// A likelihood for src.param.size() members of n nodes, built aside (the caller moves it into its slot): the data set once, the
// evaluation's and the loop's work per member. The batch slot (rows non-null) adds what a plain likelihood passes by value or takes
// from the handle: the members' parameters and their logs, the member's rows (the forest's first n: columns and positions of member 0
// are the member's own) and the control words.
static std::vector<double> fisher_comp_params(const ObsComponents &C);
Device::FisherDev Device::fisher_build(const FisherSource &src, size_t n, const RbmcSym *rows) {
    FisherDev f;
    const size_t nb = src.param.size();
    f.family = src.family;
    f.members = (int)nb;
    f.n = (int)n;
    f.loglik_const = src.loglik_const;
    if (rows) {
        std::vector<double> lp(nb);
        for (size_t k = 0; k < nb; k++) lp[k] = fisher_logparam(src.family, src.param[k]);
        const size_t ne = (size_t)rows->rowptr[n];
        dev_upload(f.param_k, src.param, &bytes_total);
        dev_upload(f.logparam_k, lp, &bytes_total);
        dev_upload(f.rp, rows->rowptr.data(), n + 1, &bytes_total);
        dev_upload(f.col, rows->col.data(), ne, &bytes_total);
        dev_upload(f.pos, std::vector<int>(rows->pos.begin(), rows->pos.begin() + (std::ptrdiff_t)ne), &bytes_total);
        f.ctl.alloc(2 * nb, &bytes_total, kTableMinBytes);
        f.h_ctl.alloc(2 * (long long)nb);
        f.nnz = nnz_member_;
    } else {
        f.param = src.param[0];
        f.logparam = fisher_logparam(src.family, f.param);
    }
    f.spart.alloc(4 * nb * (size_t)fisher_stat_blocks((int)n), &bytes_total, kTableMinBytes);
    f.out.alloc(6 * nb, &bytes_total, kTableMinBytes);
    f.h_out.alloc(6 * (long long)nb);
    if (src.design) {
        const size_t nobs = (size_t)src.design->nobs;
        dev_upload(f.y, *src.y, &bytes_total);
        if (!src.aux->empty()) dev_upload(f.aux, *src.aux, &bytes_total);
        design_upload(src.design, f);
        if (src.comp) {
            const ObsComponents &C = *src.comp;
            std::vector<unsigned char> comp(nobs);
            for (size_t c = 0; c < C.size(); c++) std::fill(comp.begin() + C.rowptr[c], comp.begin() + C.rowptr[c + 1], (unsigned char)c);
            f.ncomp = (int)C.size();
            f.crowptr = C.rowptr;
            f.cfam = C.family;
            dev_upload(f.comp, comp, &bytes_total);
            dev_upload(f.cfamily, C.family, &bytes_total);
            dev_upload(f.cpar, fisher_comp_params(C), &bytes_total);
        }
        f.g.alloc(nobs * nb, &bytes_total, kTableMinBytes);
        f.d.alloc(nobs * nb, &bytes_total, kTableMinBytes);
        f.cpart.alloc((size_t)(f.ncc + f.nct) * nb, &bytes_total, kTableMinBytes);
        f.lpart.alloc((size_t)design_blocks((long long)nobs) * nb, &bytes_total, kTableMinBytes);
        f.part.alloc((size_t)design_blocks((long long)n) * nb, &bytes_total, kTableMinBytes);
    } else {
        const ObsByNode &b = *src.by_node;
        dev_upload(f.y, b.y, &bytes_total);
        dev_upload(f.mask, b.mask, &bytes_total);
        if (!b.aux.empty()) dev_upload(f.aux, b.aux, &bytes_total);
        f.part.alloc(2 * nb * (size_t)fisher_blocks((int)n), &bytes_total, kTableMinBytes);
    }
    return f;
}

// the component table's parameters as the device holds them: the ncomp parameters, then their logs (fisher_logparam)
static std::vector<double> fisher_comp_params(const ObsComponents &C) {
    std::vector<double> p(C.param);
    for (size_t c = 0; c < C.size(); c++) p.push_back(fisher_logparam(C.family[c], C.param[c]));
    return p;
}
ObsComp Device::FisherDev::comp_table() const { return ObsComp{comp, cfamily, cpar.get(), cpar.get() + ncomp}; }

void Device::obs_set(const ObsHost &o) {
    HC(hipSetDevice(device));
    if (sharded() || many_members()) throw std::invalid_argument("obs_set: batched and sharded handles are not supported");
    FisherDev f;         // built aside: a failed upload leaves the previous likelihood in place
    if (o.nobs > 0) {
        const size_t n = (size_t)S_->n;
        if (o.design && ((long long)n != o.design->n || n > (size_t)INT_MAX)) throw std::invalid_argument("obs_set_design: the plan does not belong to this handle");
        const ObsByNode b = o.design ? ObsByNode{} : obs_by_node(n, o.nobs, o.idx, o.y, o.aux);
        const std::vector<double> param{o.param}, loglik_const{o.loglik_const};
        if (!o.comp.empty() && (!o.design || o.comp.rowptr.size() != o.comp.size() + 1 || o.comp.rowptr.back() != o.nobs))
            throw std::invalid_argument("obs_set_composite: the components do not belong to this likelihood");
        f = fisher_build(FisherSource{o.family, &b, &o.y, &o.aux, o.design, param, loglik_const, o.comp.empty() ? nullptr : &o.comp}, n, nullptr);
    }
    HC(hipStreamSynchronize(stream));        // (an evaluation in flight on an external stream still reads the old arrays)
    fisher_ = std::move(f);
    gap_ = GapDev{};         // (the pullback's tables belong to the likelihood: rebuilt on its next call)
    pred_ = PredDev{};       // (and so do the predictive calls')
    prior_design_ = -1;
}

// The parameters of the composite in place: the table's 2 ncomp doubles and the constant. The plan, the component bytes and every
// other table stay; the cached pointwise constants belong to the parameters and are rebuilt on the next predictive call.
void Device::obs_composite_set_param(const ObsComponents &C, double loglik_const) {
    HC(hipSetDevice(device));
    if (fisher_.ncomp <= 0 || (size_t)fisher_.ncomp != C.size()) throw std::invalid_argument("obs_composite_set_param: no composite likelihood is set");
    const std::vector<double> p = fisher_comp_params(C);
    HC(hipStreamSynchronize(stream));      // nothing in flight may still read the previous values
    HC(hipMemcpy(fisher_.cpar, p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice));
    fisher_.loglik_const.assign(1, loglik_const);
    pred_ = PredDev{};
}

void Device::fisher_launch(FisherDev &f, const FisherRows &rows, const FisherIO &io, const unsigned char *active, double *out_host) {
    if (f.design) {
        const DesignPlan &P = *f.design;
        auto a = FisherDesign{};      // (every field zero, then by name)
        a.n = (int)P.n; a.nobs = (int)P.nobs; a.cnt = (int)P.cnt; a.family = f.family;
        a.rp = rows.rp; a.col = rows.col; a.pos = rows.pos;
        a.val = d_prior_; a.x = io.d_x; a.mu = io.d_mu;
        a.arp = f.arp; a.acol = f.acol; a.aval = f.aval; a.offset = f.offset;
        a.acp = f.acp; a.arow = f.arow; a.acv = f.acv;
        a.tptr = f.tptr; a.tobs = f.tobs; a.tw = f.tw;
        a.cchoff = f.cchoff; a.tchoff = f.tchoff; a.chs = f.chs; a.chl = f.chl; a.ncc = f.ncc; a.nct = f.nct;
        a.y = f.y; a.aux = f.aux;
        a.param = f.param; a.logparam = f.logparam;
        a.g = f.g; a.d = f.d; a.cpart = f.cpart;
        a.score = io.d_score; a.hess = io.d_hess;
        a.epart = f.part; a.lpart = f.lpart;
        a.nnz = f.nnz; a.sx = io.sx; a.smu = io.smu; a.ss = io.ss; a.sh = io.sh;
        a.param_k = f.param_k; a.logparam_k = f.logparam_k; a.active = io.d_active;
        if (f.ncomp > 0) launch_fisher_design_comp(stream, a, f.comp_table(), f.members, f.out);
        else launch_fisher_design(stream, a, f.members, f.out);
    } else {
        auto a = FisherEval{};
        a.n = f.n; a.family = f.family;
        a.rp = rows.rp; a.col = rows.col; a.pos = rows.pos;
        a.val = d_prior_; a.x = io.d_x; a.mu = io.d_mu;
        a.y = f.y; a.aux = f.aux; a.mask = f.mask;
        a.param = f.param; a.logparam = f.logparam;
        a.score = io.d_score; a.hess = io.d_hess;
        a.part = f.part;
        a.nnz = f.nnz; a.sx = io.sx; a.smu = io.smu; a.ss = io.ss;
        a.param_k = f.param_k; a.logparam_k = f.logparam_k; a.active = io.d_active;
        launch_fisher_eval(stream, a, f.members, f.out);
    }
    const size_t nb = (size_t)f.members;
    HC(hipMemcpyAsync(f.h_out, f.out, 2 * nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    for (size_t k = 0; k < nb; k++) {
        if (active && !active[k]) continue;
        out_host[2 * k] = f.h_out[2 * k];
        out_host[2 * k + 1] = f.h_out[2 * k + 1] + f.loglik_const[k];
    }
}

void Device::fisher_stats(FisherDev &f, const FisherMembers &m, const double *a, const double *b, const double *c, const double *d,
                          const unsigned char *active, double *out4) {
    const size_t nb = (size_t)f.members;
    launch_fisher_stats(stream, m, a, b, c, d, f.spart, f.out.get() + 2 * nb);
    HC(hipMemcpyAsync(f.h_out + 2 * nb, f.out.get() + 2 * nb, 4 * nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    for (size_t k = 0; k < nb; k++)
        if (!active || active[k]) std::copy(f.h_out + 2 * nb + 4 * k, f.h_out + 2 * nb + 4 * k + 4, out4 + 4 * k);
}

// What an evaluation of the plain likelihood refuses about the prior and its map, for fisher_eval and the pullback (who: the caller's
// name in the message)
void Device::fisher_check_map(const RbmcSym &sym, const char *who) {
    const std::string w = std::string(who) + ": ";
    if (!d_prior_) throw std::invalid_argument(w + "gmrfx_set_prior has not been called");
    const long long n = S_->n;
    if (fisher_.design) {
        const DesignPlan &P = *fisher_.design;
        if (prior_design_ < 0) prior_design_ = (hmap_cnt_ == P.cnt && std::equal(P.map.begin(), P.map.end(), h_hmap_.begin())) ? 1 : 0;
        if (!prior_design_)
            throw std::invalid_argument(w + "the map of gmrfx_set_prior is not the map of gmrfx_obs_hess_map (the positions of A' D A, design form)");
        return;
    }
    if (prior_diag_ < 0) {
        prior_diag_ = hmap_cnt_ == n ? 1 : 0;
        for (long long i = 0; i < n && prior_diag_; i++)
            if (h_hmap_[(size_t)i] != sym.diag[(size_t)i]) prior_diag_ = 0;
    }
    if (!prior_diag_) throw std::invalid_argument(w + "the map of gmrfx_set_prior is not the position of (i, i) for every i (diagonal Hessians only)");
}

void Device::fisher_eval(const RbmcSym &sym, const double *d_x, const double *d_mu, double *d_score, double *d_hess, double *out_host) {
    HC(hipSetDevice(device));
    if (sharded() || many_members()) throw std::invalid_argument("fisher_eval: batched and sharded handles are not supported");
    if (!d_x || !out_host) throw std::invalid_argument("fisher_eval: x / out is null");
    if (!d_prior_) throw std::invalid_argument("fisher_eval: gmrfx_set_prior has not been called");
    if (S_->n > INT_MAX) throw std::invalid_argument("fisher_eval: more than 2^31 - 1 nodes");
    fisher_check_map(sym, "fisher_eval");
    if (!obs_held()) throw std::invalid_argument("fisher_eval: no observation likelihood is set (gmrfx_obs_set)");
    sym_rows_upload(sym);
    // one member on the handle's own rows: no strides, nobody masked
    fisher_launch(fisher_, FisherRows{sym_rows_.rp, sym_rows_.col, sym_rows_.pos}, FisherIO{d_x, 0, d_mu, 0, d_score, d_hess, 0, 0, nullptr}, nullptr,
                  out_host);
}

// ---- the loop ------------------------------------------------------------------------------------------------------------------------
// One GaMember through the decisions of ga_rules.h. (Known difference from the batched loop, which takes the same decisions: |step|_inf
// is recomputed at every backtrack here, once per iterate there -- one launch per further backtrack, left for a performance change.)
int Device::gaussian_approximation(const RbmcSym &sym, const double *d_mu, const double *d_x0, const GaOpts &o, double *d_x, double *d_hess,
                                   double *result, double *dec_trace, double *alpha_trace, long long *info) {
    HC(hipSetDevice(device));
    if (!d_x || !result) throw std::invalid_argument("gaussian_approximation: x / result is null");
    if (o.max_iter < 0 || o.max_ls < 0) throw std::invalid_argument("gaussian_approximation: max_iter / max_linesearch_iter is negative");
    const long long n = S_->n;
    const size_t nb = (size_t)n * sizeof(double);
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
    GaMember m;
    const FisherMembers one{(int)n, 1, 0, nullptr};       // the loop's vectors are one member's
    // out = x - al step (al changes between launches: by value, nothing goes up)
    auto candidate = [&](const double *x, double al, double *out) { launch_fisher_candidate(stream, one, x, step, al, nullptr, out); };
    auto stats = [&](const double *a, const double *b, const double *c, const double *d, double *out4) {
        fisher_stats(fisher_, one, a, b, c, d, nullptr, out4);
    };
    auto merit = [&](const double *x) {
        double e[2];
        fisher_eval(sym, x, d_mu, nullptr, nullptr, e);
        m.nmerit += 1;
        return ga_merit(e);
    };
    auto trace = [&](long long at) {
        if (dec_trace) dec_trace[at] = m.dec;
        if (alpha_trace) alpha_trace[at] = m.alpha;
    };
    // the step - A~' W^-1 (A step) of _workspace_constrain_with_matrix; false: W is not positive definite
    auto project = [&](double *s) {
        if (con_.m <= 0) return true;
        if (!con_prepare()) return false;
        con_correct(s, n, 1, nullptr, true);
        return true;
    };
    auto finish = [&](const double *xfinal, long long iters, int status, bool frozen) -> int {
        HC(hipMemcpyAsync(d_x, xfinal, nb, hipMemcpyDeviceToDevice, stream));
        int rc = 0;
        if (status != kGaFailed && (d_hess || o.refactor_final())) {
            double e[2];
            fisher_eval(sym, xfinal, d_mu, nullptr, hess, e);      // the final H(x_final) (_workspace_build_result)
            if (d_hess && hlen > 0) HC(hipMemcpyAsync(d_hess, hess, (size_t)hlen * sizeof(double), hipMemcpyDeviceToDevice, stream));
            if (o.refactor_final()) {
                refactorize_update(hess, true);
                m.nfact += 1;
                const long long fc = fail_col();
                if (fc >= 0) { if (info) *info = fc + 1; rc = 1; }
            }
        }
        HC(hipStreamSynchronize(stream));
        ga_stop(m, status, iters, frozen);
        ga_result_row(m, result);
        return rc;
    };
    for (long long iter = 1; iter <= o.max_iter; iter++) {
        double ek[2], st[4];
        fisher_eval(sym, xk, d_mu, score, hess, ek);
        refactorize_update_solve(hess, true, score, n, 1, step, n, true);
        ga_iterate_begun(m);
        const long long fc = fail_col();
        if (fc >= 0) {
            if (info) *info = fc + 1;
            finish(xk, iter - 1, kGaFailed, false);
            return 1;
        }
        if (!project(step)) { finish(xk, iter - 1, kGaFailed, false); return 2; }
        const double *xn = xnew;
        if (o.adaptive()) {
            // _ga_line_search, line by line
            const double bound = ga_line_search_bound(ek);
            bool done = false;
            if (ga_line_search_retries_full(o, m)) {
                candidate(xk, 1.0, xnew);
                done = ga_line_search_full_step(m, merit(xnew), bound);
            }
            if (!done) {
                bool accept = false;
                for (long long ls = 1; ls <= o.max_ls && !accept; ls++) {
                    candidate(xk, m.alpha, cand);
                    if (ga_line_search_probe(m, merit(cand), bound)) accept = true;
                    else {
                        stats(nullptr, step, nullptr, nullptr, st);
                        accept = ga_line_search_tiny_step(o, m, st[3]);
                    }
                }
                if (accept) xn = cand;
                else candidate(xk, m.alpha, xnew);
            }
        } else candidate(xk, 1.0, xnew);
        stats(score, step, xn, xk, st);
        const GaVerdict verdict = ga_iterate_verdict(o, m, iter, st);
        trace(iter - 1);
        if (verdict == kGaConverges) return finish(xn, iter, kGaConverged, false);
        // _predict_converged, then _frozen_finish: chord steps on the factorisation in hand, only the first decides
        if (verdict == kGaLooksAhead) {
            double *xf = xn == cand ? xnew : cand;          // (the accepted iterate stays where it is until the look-ahead has decided)
            HC(hipMemcpyAsync(xf, xn, nb, hipMemcpyDeviceToDevice, stream));
            bool ok = true;
            for (int j = 1; j <= kFrozenFinishSteps && ok; j++) {
                double e[2];
                fisher_eval(sym, xf, d_mu, score, nullptr, e);
                solve(score, n, 1, step, n, true, 0);
                m.nsolve += 1;
                if (!project(step)) { finish(xn, iter, kGaFailed, false); return 2; }
                if (j == 1) {
                    stats(score, step, nullptr, nullptr, st);
                    if (!frozen_finish_decides(o, m, st[0])) { ok = false; break; }
                    trace(iter);
                }
                candidate(xf, 1.0, xf);
            }
            if (ok) return finish(xf, iter + 1, kGaConverged, true);
        }
        m.dec_prev = m.dec;
        if (xn != xk) HC(hipMemcpyAsync(xk, xn, nb, hipMemcpyDeviceToDevice, stream));
    }
    return finish(xk, o.max_iter, kGaMaxIter, false);
}

}  // namespace gmrfx
