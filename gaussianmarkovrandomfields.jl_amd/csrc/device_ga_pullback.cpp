// device_ga_pullback.cpp -- the Device's side of the pullback of gaussian_approximation (include/gmrfx.h: gmrfx_ga_pullback; kernels in
// ga_pullback.hip). The reference's rule (src/workspace/autodiff.jl:140-202) pulls the precision cotangent back through loghessian,
// solves once with the posterior factor and takes a vector-Jacobian product through Q_p (x - mu) - loggrad(x), all on the host. Here the
// factor of Q_prior - H(x*), the likelihood, the prior's values, the Hessian map, the symmetric row structure and the constraint's
// operands are where the Fisher-scoring loop left them; the call adds the arithmetic around one solve and returns two numbers.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>

#include "device.h"
#include "kernels.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

// The plan's transposed term table on the device (design form; 12 B per term, ONE copy whatever the number of members): uploaded by
// whichever of the pullback and gmrfx_predictor_marginals needs it first, kept until the likelihood's setter drops the pullback's state.
void Device::gap_term_table(const FisherDev &f, GapDev &g) {
    const DesignPlan *P = f.design.get();
    if (!P || g.optr) return;
    DevBuf<long long> optr;      // built aside: an upload that fails half-way leaves nothing behind
    DevBuf<int> oidx;
    DevBuf<double> ow;
    dev_upload(optr, P->optr, &bytes_total);
    dev_upload(oidx, P->oidx, &bytes_total);
    dev_upload(ow, P->ow, &bytes_total);
    g.optr = std::move(optr); g.oidx = std::move(oidx); g.ow = std::move(ow);
}
void Device::gap_term_table() { gap_term_table(fisher_, gap_); }

// The first pullback for a likelihood: the plan's transposed term table goes up (design form), the work arrays are allocated.
// O(n + nobs) doubles per member beside the table.
void Device::gap_tables(const FisherDev &f, GapDev &g) {
    if (g.work) return;
    const size_t n = (size_t)f.n, nb = (size_t)f.members;
    const DesignPlan *P = f.design.get();
    const size_t nobs = P ? (size_t)P->nobs : 0;
    gap_term_table(f, g);
    DevBuf<double> work, part, out;      // built aside, as the table
    PinnedBuf<double> h_out;
    // a composite: the component tiling's workgroups and one result per component (kernels.h: GapTiles)
    DevBuf<int> bptr;
    DevBuf<long long> crow;
    size_t nblk = (size_t)gap_obs_blocks(P != nullptr, (long long)n, (long long)nobs), nout = 1;
    if (f.ncomp > 0) {
        std::vector<int> b((size_t)f.ncomp + 1);
        nblk = (size_t)gap_comp_tiles(f.crowptr.data(), f.ncomp, b.data());
        nout = (size_t)f.ncomp;
        dev_upload(bptr, b, &bytes_total);
        dev_upload(crow, f.crowptr, &bytes_total);
    }
    work.alloc(nb * (2 * n + nobs), &bytes_total, kTableMinBytes);
    part.alloc(2 * nb * nblk, &bytes_total, kTableMinBytes);
    out.alloc(nb * nout, &bytes_total, kTableMinBytes);
    h_out.alloc((long long)(nb * nout));
    g.bptr = std::move(bptr); g.crow = std::move(crow); g.nblk = (int)nblk;
    g.part = std::move(part); g.out = std::move(out); g.h_out = std::move(h_out); g.work = std::move(work);
}

void Device::gap_launch(FisherDev &f, GapDev &g, const GapRun &r, const GapIO &io, double *out_host) {
    const long long n = f.n, nnz = f.nnz;
    const int nb = f.members;
    const DesignPlan *P = f.design.get();
    const bool design = P != nullptr;
    const long long nobs = design ? P->nobs : n;
    const int nblk = gap_obs_blocks(design, n, nobs);
    const bool has_param = f.family == 0 || f.family == 4 || f.family == 5;
    const unsigned char *act = r.d_active;
    bool any = false;
    for (int k = 0; k < nb; k++) any = any || !r.active || r.active[k];
    if (any) {
        gap_tables(f, g);
        double *xbar = g.work, *lam = xbar + n * nb, *t = lam + n * nb;
        double *gpart = g.part, *ppart = gpart + (long long)nblk * nb;
        // ---- xbar = mubar - A' (c . d3) ---------------------------------------------------------------------------------------------
        if (io.d_Qbar) {
            auto a = GapPoint{};      // (every field zero, then by name)
            a.n = (int)n; a.nobs = (int)nobs; a.family = f.family;
            a.G = io.d_Qbar; a.hmap = r.hmap; a.x = io.d_x; a.mubar = io.d_mubar;
            a.y = f.y; a.aux = f.aux; a.mask = f.mask;
            a.arp = f.arp; a.acol = f.acol; a.aval = f.aval; a.offset = f.offset;
            a.optr = g.optr; a.oidx = g.oidx; a.ow = g.ow;
            a.param = f.param; a.logparam = f.logparam;
            a.t = t; a.xbar = xbar; a.ppart = ppart;
            a.sg = nnz; a.sx = r.sx; a.sm = n; a.sw = n;
            a.param_k = f.param_k; a.logparam_k = f.logparam_k; a.active = act;
            launch_gap_point(stream, a, design, nb);
            if (design) {
                const GapGather b{(int)n, f.ncc, f.acp, f.arow, f.acv, f.cchoff, f.chs, f.chl, t, io.d_mubar, f.cpart, xbar,
                                  nobs, n, (long long)(f.ncc + f.nct), n, act};
                launch_gap_gather(stream, b, nb);
            }
        } else launch_gap_copy(stream, n, io.d_mubar, n, xbar, n, act, nb);
        // ---- lam = Q_post^-1 xbar: ONE solve for all members, projected under bit 0 -------------------------------------------------
        launch_gap_copy(stream, n, xbar, n, lam, n, act, nb);
        solve(lam, n * nb, 1, lam, n * nb, true, 0);
        if (r.project == 1) con_correct(lam, n, 1, nullptr, true);
        else if (r.project == 2) bcon_project(lam, n, act);
        // ---- the outputs ------------------------------------------------------------------------------------------------------------
        if (io.d_Qbar_prior) {
            const GapPattern a{(int)n, r.colptr, r.row, io.d_Qbar, lam, io.d_x, io.d_mu, io.d_Qbar_prior, nnz, n, r.sx, r.smu, act};
            launch_gap_pattern(stream, a, nb);
        }
        if (io.d_mubar_prior) {
            const GapMean a{(int)n, r.rows.rp, r.rows.col, r.rows.pos, d_prior_, lam, io.d_mubar_prior, nnz, n, n, act};
            launch_gap_mean(stream, a, nb);
        }
        if (io.d_lambda) launch_gap_copy(stream, n, lam, n, io.d_lambda, n, act, nb);
        if (has_param) {
            auto a = GapParam{};
            a.n = (int)n; a.nobs = (int)nobs; a.family = f.family;
            a.lam = lam; a.x = io.d_x;
            a.y = f.y; a.aux = f.aux; a.mask = f.mask;
            a.arp = f.arp; a.acol = f.acol; a.aval = f.aval; a.offset = f.offset;
            a.param = f.param; a.logparam = f.logparam;
            a.gpart = gpart;
            a.sw = n; a.sx = r.sx;
            a.param_k = f.param_k; a.logparam_k = f.logparam_k; a.active = act;
            launch_gap_param(stream, a, design, nb);
            launch_gap_final(stream, gpart, nblk, ppart, io.d_Qbar ? nblk : 0, act, nb, g.out);
            HC(hipMemcpyAsync(g.h_out, g.out, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
        }
        // lam' xbar by the loop's own reduction (sum a b of launch_fisher_stats)
        launch_fisher_stats(stream, FisherMembers{(int)n, nb, n, act}, lam, xbar, nullptr, nullptr, f.spart, f.out.get() + 2 * nb);
        HC(hipMemcpyAsync(f.h_out + 2 * nb, f.out.get() + 2 * nb, 4 * (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    // ---- a member that takes no part: NaN in what was asked of it, nothing else of it is touched ----------------------------------------
    if (act) {
        if (io.d_Qbar_prior) launch_gap_fill_failed(stream, nnz, io.d_Qbar_prior, nnz, act, nb);
        if (io.d_mubar_prior) launch_gap_fill_failed(stream, n, io.d_mubar_prior, n, act, nb);
        if (io.d_lambda) launch_gap_fill_failed(stream, n, io.d_lambda, n, act, nb);
    }
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    for (int k = 0; k < nb; k++) {
        const bool on = !r.active || r.active[k];
        out_host[2 * k] = !on ? std::nan("") : (has_param ? g.h_out[k] : 0.0);
        out_host[2 * k + 1] = !on ? std::nan("") : f.h_out[2 * nb + 4 * k];
    }
}

int Device::gap_prepare(const RbmcSym &sym, const GapIO &io, long long *info, const char *who) {
    const std::string w = std::string(who) + ": ";
    if (sharded() || many_members()) throw std::invalid_argument(w + "batched and sharded handles are not supported");
    if (!io.d_x) throw std::invalid_argument(w + "x / out is null");
    if (!obs_held()) throw std::invalid_argument(w + "no observation likelihood is set (gmrfx_obs_set)");
    const long long n = S_->n;
    if (n > INT_MAX) throw std::invalid_argument(w + "more than 2^31 - 1 nodes");
    const bool project = io.flags & 1, refactor = io.flags & 2;
    if (!io.d_mubar && !io.d_Qbar) throw std::invalid_argument(w + "mubar and Qbar are both null");
    if (project && con_.m <= 0) throw std::invalid_argument(w + "flag bit 0 (project lambda) needs a constraint (gmrfx_constraints_set)");
    fisher_check_map(sym, who);
    if (info) *info = 0;
    if (refactor) {
        // Q_prior - H(x): the evaluation's Hessian values, then the update the loop's last step does under its flag bit 3
        const long long hlen = hess_len();
        if (!fisher_.work) fisher_.work.alloc(5 * (size_t)n + (size_t)hlen, &bytes_total, kTableMinBytes);
        double *hess = fisher_.work.get() + 5 * n, e[2];
        fisher_eval(sym, io.d_x, io.d_mu, nullptr, hess, e);
        refactorize_update(hess, true);
        const long long fc = fail_col();
        if (fc >= 0) { if (info) *info = fc + 1; return 1; }
    }
    if (project && !con_prepare()) return 2;      // (the operands of the factor in hand: nothing of the rule has been launched yet)
    if (io.d_Qbar_prior) prepare_quadform(0);     // (the pattern of Q on the device)
    if (io.d_mubar_prior) sym_rows_upload(sym);
    return 0;
}

int Device::ga_pullback(const RbmcSym &sym, const GapIO &io, double *out_host, long long *info) {
    HC(hipSetDevice(device));
    if (!out_host) throw std::invalid_argument("ga_pullback: x / out is null");
    if (fisher_.ncomp > 0) throw std::invalid_argument("ga_pullback: composite likelihoods take gmrfx_ga_pullback_composite");
    if (const int rc = gap_prepare(sym, io, info, "ga_pullback")) return rc;
    // one member on the handle's own map, pattern and rows: no strides, nobody masked
    gap_launch(fisher_, gap_, GapRun{d_hmap_, d_in_colptr_, d_in_row_, FisherRows{sym_rows_.rp, sym_rows_.col, sym_rows_.pos}, 0, 0, (io.flags & 1) ? 1 : 0,
                                     nullptr, nullptr}, io, out_host);
    return 0;
}

// The launch sequence of gap_launch for ONE member of a composite (the batched path is gap_launch's alone): the three kernels that
// read a family are the composite's, on the component tiling; everything else is launched as there.
int Device::ga_pullback_composite(const RbmcSym &sym, const GapIO &io, double *param_bar_host, double *check_host, long long *info) {
    HC(hipSetDevice(device));
    if (!param_bar_host) throw std::invalid_argument("ga_pullback_composite: param_bar is null");
    if (fisher_.ncomp <= 0) throw std::invalid_argument("ga_pullback_composite: no composite likelihood is set (gmrfx_obs_set_composite)");
    if (const int rc = gap_prepare(sym, io, info, "ga_pullback_composite")) return rc;
    FisherDev &f = fisher_;
    GapDev &g = gap_;
    const DesignPlan &P = *f.design;
    const long long n = f.n, nnz = f.nnz, nobs = P.nobs;
    const int nc = f.ncomp;
    bool has_param = false;
    for (int c = 0; c < nc; c++) has_param = has_param || f.cfam[c] == 0 || f.cfam[c] == 4 || f.cfam[c] == 5;
    gap_tables(f, g);
    const ObsComp tab = f.comp_table();
    const GapTiles tiles{nc, g.bptr, g.crow};
    double *xbar = g.work, *lam = xbar + n, *t = lam + n;
    double *gpart = g.part, *ppart = gpart + g.nblk;
    // ---- xbar = mubar - A' (c . d3) -------------------------------------------------------------------------------------------------
    if (io.d_Qbar) {
        auto a = GapPoint{};      // (every field zero, then by name)
        a.n = (int)n; a.nobs = (int)nobs; a.family = f.family;
        a.G = io.d_Qbar; a.hmap = d_hmap_; a.x = io.d_x; a.mubar = io.d_mubar;
        a.y = f.y; a.aux = f.aux;
        a.arp = f.arp; a.acol = f.acol; a.aval = f.aval; a.offset = f.offset;
        a.optr = g.optr; a.oidx = g.oidx; a.ow = g.ow;
        a.t = t; a.xbar = xbar; a.ppart = ppart;
        a.sg = nnz; a.sm = n; a.sw = n;
        launch_gap_point_comp(stream, a, tab, tiles, g.nblk, 1);
        const GapGather b{(int)n, f.ncc, f.acp, f.arow, f.acv, f.cchoff, f.chs, f.chl, t, io.d_mubar, f.cpart, xbar,
                          nobs, n, (long long)(f.ncc + f.nct), n, nullptr};
        launch_gap_gather(stream, b, 1);
    } else launch_gap_copy(stream, n, io.d_mubar, n, xbar, n, nullptr, 1);
    // ---- lam = Q_post^-1 xbar, projected under bit 0 --------------------------------------------------------------------------------
    launch_gap_copy(stream, n, xbar, n, lam, n, nullptr, 1);
    solve(lam, n, 1, lam, n, true, 0);
    if (io.flags & 1) con_correct(lam, n, 1, nullptr, true);
    // ---- the outputs ----------------------------------------------------------------------------------------------------------------
    if (io.d_Qbar_prior) {
        const GapPattern a{(int)n, d_in_colptr_, d_in_row_, io.d_Qbar, lam, io.d_x, io.d_mu, io.d_Qbar_prior, nnz, n, 0, 0, nullptr};
        launch_gap_pattern(stream, a, 1);
    }
    if (io.d_mubar_prior) {
        const GapMean a{(int)n, sym_rows_.rp, sym_rows_.col, sym_rows_.pos, d_prior_, lam, io.d_mubar_prior, nnz, n, n, nullptr};
        launch_gap_mean(stream, a, 1);
    }
    if (io.d_lambda) launch_gap_copy(stream, n, lam, n, io.d_lambda, n, nullptr, 1);
    if (has_param) {
        auto a = GapParam{};
        a.n = (int)n; a.nobs = (int)nobs; a.family = f.family;
        a.lam = lam; a.x = io.d_x;
        a.y = f.y; a.aux = f.aux;
        a.arp = f.arp; a.acol = f.acol; a.aval = f.aval; a.offset = f.offset;
        a.gpart = gpart;
        a.sw = n;
        launch_gap_param_comp(stream, a, tab, tiles, g.nblk, 1);
        launch_gap_final_comp(stream, gpart, ppart, io.d_Qbar != nullptr, tiles, g.nblk, nullptr, 1, g.out);
        HC(hipMemcpyAsync(g.h_out, g.out, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    // lam' xbar by the loop's own reduction (sum a b of launch_fisher_stats)
    launch_fisher_stats(stream, FisherMembers{(int)n, 1, n, nullptr}, lam, xbar, nullptr, nullptr, f.spart, f.out.get() + 2);
    HC(hipMemcpyAsync(f.h_out + 2, f.out.get() + 2, 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    for (int c = 0; c < nc; c++) {
        const bool par = f.cfam[c] == 0 || f.cfam[c] == 4 || f.cfam[c] == 5;
        param_bar_host[c] = par ? g.h_out[c] : 0.0;
    }
    if (check_host) *check_host = f.h_out[2];
    return 0;
}

int Device::batch_ga_pullback(const RbmcSym &, const BGapIO &io, double *out_host, long long *info_host) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("batch_ga_pullback: sharded handles are not supported");
    if (!io.d_x || !out_host) throw std::invalid_argument("batch_ga_pullback: x / out is null");
    bfisher_check_prior();
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    if (!io.d_mubar && !io.d_Qbar) throw std::invalid_argument("batch_ga_pullback: mubar and Qbar are both null");
    if (!io.d_Qbar_prior && !io.d_mubar_prior && !io.d_lambda) throw std::invalid_argument("batch_ga_pullback: every output is null");
    if (io.flags < 0 || io.flags > 3) throw std::invalid_argument("batch_ga_pullback: unknown flag bits");
    const bool project = io.flags & 1, refactor = io.flags & 2;
    if (project && bcon_.m <= 0)
        throw std::invalid_argument("batch_ga_pullback: flag bit 0 (project lambda) needs a batch constraint (gmrfx_batch_constraints_set)");
    const long long n = nmember_, N = S_->n;
    const size_t nb = (size_t)nbatch_;
    if (refactor) {
        // every member's Q_prior,k - H(x_k): one batched evaluation into the loop's hess area, then the loop's final update
        const long long hl = bhess_len();
        if (!bfisher_.work) bfisher_.work.alloc(5 * (size_t)N + (size_t)hl * nb, &bytes_total, kTableMinBytes);
        double *hess = bfisher_.work.get() + 5 * N;
        std::vector<double> ev(2 * nb);
        fisher_launch(bfisher_, FisherRows{bfisher_.rp, bfisher_.col, bfisher_.pos}, FisherIO{io.d_x, io.sx, io.d_mu, io.smu, nullptr, hess, n, hl, nullptr},
                      nullptr, ev.data());
        refactorize_update(hess, true);
    }
    // the members that take part: a failed factor (of this call or held) masks its member out for the rest of the call, and so does a
    // failed W_k under bit 0, read on the host BEFORE any correction is launched (its L_ck^-1 is NaN)
    std::vector<long long> inf(nb, 0);
    std::vector<unsigned char> mask(nb, 1);
    batch_diag(nullptr, inf.data());
    bool failed = false;
    for (size_t k = 0; k < nb; k++)
        if (inf[k] != 0) { inf[k] = -1; mask[k] = 0; failed = true; }
    const bool any = std::find(mask.begin(), mask.end(), (unsigned char)1) != mask.end();
    if (project && any) {
        const std::vector<long long> &ci = bcon_prepare_members();
        for (size_t k = 0; k < nb; k++)
            if (mask[k] && ci[k] > 0) { inf[k] = ci[k]; mask[k] = 0; failed = true; }
    }
    const unsigned char *d_mask = nullptr;
    if (failed) {
        bfisher_ctl(nullptr, mask);
        d_mask = reinterpret_cast<const unsigned char *>(bfisher_.ctl.get() + nb);
    }
    // every member on ONE copy of the member's map slice, pattern and rows
    gap_launch(bfisher_, bgap_, GapRun{d_hmap_, d_bin_colptr_, d_bin_row_, FisherRows{bfisher_.rp, bfisher_.col, bfisher_.pos}, io.sx, io.smu,
                                       project ? 2 : 0, d_mask, failed ? mask.data() : nullptr},
               GapIO{io.d_x, io.d_mu, io.d_mubar, io.d_Qbar, io.flags, io.d_Qbar_prior, io.d_mubar_prior, io.d_lambda}, out_host);
    if (info_host) std::copy(inf.begin(), inf.end(), info_host);
    return failed ? 1 : 0;
}

}  // namespace gmrfx
