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

// The plan's transposed term table on the device (design form; 12 B per term): uploaded by whichever of gmrfx_ga_pullback and
// gmrfx_predictor_marginals needs it first, kept until obs_set drops the pullback's state.
void Device::gap_term_table() {
    const DesignPlan *P = fisher_.design.get();
    if (!P || gap_.optr) return;
    DevBuf<long long> optr;      // built aside: an upload that fails half-way leaves nothing behind
    DevBuf<int> oidx;
    DevBuf<double> ow;
    dev_upload(optr, P->optr, &bytes_total);
    dev_upload(oidx, P->oidx, &bytes_total);
    dev_upload(ow, P->ow, &bytes_total);
    gap_.optr = std::move(optr); gap_.oidx = std::move(oidx); gap_.ow = std::move(ow);
}

// The first pullback for a likelihood: the plan's transposed term table goes up (design form), the work arrays are allocated.
// O(n + nobs) doubles beside the table.
void Device::gap_tables() {
    if (gap_.work) return;
    const size_t n = (size_t)S_->n;
    const DesignPlan *P = fisher_.design.get();
    const size_t nobs = P ? (size_t)P->nobs : 0;
    gap_term_table();
    DevBuf<double> work, part, out;      // built aside, as the table
    PinnedBuf<double> h_out;
    work.alloc(2 * n + nobs, &bytes_total, kTableMinBytes);
    part.alloc(2 * (size_t)gap_obs_blocks(P != nullptr, (long long)n, (long long)nobs), &bytes_total, kTableMinBytes);
    out.alloc(1, &bytes_total, kTableMinBytes);
    h_out.alloc(1);
    gap_.part = std::move(part); gap_.out = std::move(out); gap_.h_out = std::move(h_out); gap_.work = std::move(work);
}

int Device::ga_pullback(const RbmcSym &sym, const GapIO &io, double *out_host, long long *info) {
    HC(hipSetDevice(device));
    if (sharded() || many_members()) throw std::invalid_argument("ga_pullback: batched and sharded handles are not supported");
    if (!io.d_x || !out_host) throw std::invalid_argument("ga_pullback: x / out is null");
    if (!obs_held()) throw std::invalid_argument("ga_pullback: no observation likelihood is set (gmrfx_obs_set)");
    const long long n = S_->n;
    if (n > INT_MAX) throw std::invalid_argument("ga_pullback: more than 2^31 - 1 nodes");
    const bool project = io.flags & 1, refactor = io.flags & 2;
    if (!io.d_mubar && !io.d_Qbar) throw std::invalid_argument("ga_pullback: mubar and Qbar are both null");
    if (project && con_.m <= 0) throw std::invalid_argument("ga_pullback: flag bit 0 (project lambda) needs a constraint (gmrfx_constraints_set)");
    fisher_check_map(sym, "ga_pullback");
    if (info) *info = 0;
    const size_t nb = (size_t)n * sizeof(double);
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
    gap_tables();
    const DesignPlan *P = fisher_.design.get();
    const bool design = P != nullptr;
    const long long nobs = design ? P->nobs : n;
    const int nblk = gap_obs_blocks(design, n, nobs);
    double *xbar = gap_.work, *lam = xbar + n, *t = lam + n;
    double *gpart = gap_.part, *ppart = gpart + nblk;
    const double logparam = fisher_logparam(fisher_.family, fisher_.param);
    const bool has_param = fisher_.family == 0 || fisher_.family == 4 || fisher_.family == 5;
    // ---- xbar = mubar - A' (c . d3) -------------------------------------------------------------------------------------------------
    if (io.d_Qbar) {
        const GapPoint a{(int)n, (int)nobs, fisher_.family, io.d_Qbar, d_hmap_, io.d_x, io.d_mubar, fisher_.y, fisher_.aux.get(), fisher_.mask.get(),
                         fisher_.arp.get(), fisher_.acol.get(), fisher_.aval.get(), fisher_.offset.get(), gap_.optr.get(), gap_.oidx.get(), gap_.ow.get(),
                         fisher_.param, logparam, t, xbar, ppart};
        launch_gap_point(stream, a, design);
        if (design) {
            const GapGather b{(int)n, fisher_.ncc, fisher_.acp, fisher_.arow, fisher_.acv, fisher_.cchoff, fisher_.chs, fisher_.chl, t, io.d_mubar,
                              fisher_.cpart, xbar};
            launch_gap_gather(stream, b);
        }
    } else HC(hipMemcpyAsync(xbar, io.d_mubar, nb, hipMemcpyDeviceToDevice, stream));
    // ---- lam = Q_post^-1 xbar, projected under bit 0 --------------------------------------------------------------------------------
    HC(hipMemcpyAsync(lam, xbar, nb, hipMemcpyDeviceToDevice, stream));
    solve(lam, n, 1, lam, n, true, 0);
    if (project) {
        if (!con_prepare()) return 2;
        con_correct(lam, n, 1, nullptr, true);
    }
    // ---- the outputs ------------------------------------------------------------------------------------------------------------------
    if (io.d_Qbar_prior) {
        prepare_quadform(0);          // (the pattern of Q on the device)
        const GapPattern a{(int)n, d_in_colptr_, d_in_row_, io.d_Qbar, lam, io.d_x, io.d_mu, io.d_Qbar_prior};
        launch_gap_pattern(stream, a);
    }
    if (io.d_mubar_prior) {
        sym_rows_upload(sym);
        launch_gap_mean(stream, (int)n, sym_rows_.rp, sym_rows_.col, sym_rows_.pos, d_prior_, lam, io.d_mubar_prior);
    }
    if (io.d_lambda) HC(hipMemcpyAsync(io.d_lambda, lam, nb, hipMemcpyDeviceToDevice, stream));
    if (has_param) {
        const GapParam a{(int)n, (int)nobs, fisher_.family, lam, io.d_x, fisher_.y, fisher_.aux.get(), fisher_.mask.get(), fisher_.arp.get(),
                         fisher_.acol.get(), fisher_.aval.get(), fisher_.offset.get(), fisher_.param, logparam, gpart};
        launch_gap_param(stream, a, design);
        launch_gap_final(stream, gpart, nblk, ppart, io.d_Qbar ? nblk : 0, gap_.out);
        HC(hipMemcpyAsync(gap_.h_out, gap_.out, sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    // lam' xbar by the loop's own reduction (sum a b of launch_fisher_stats)
    launch_fisher_stats(stream, FisherMembers{(int)n, 1, 0, nullptr}, lam, xbar, nullptr, nullptr, fisher_.spart, fisher_.out.get() + 2);
    HC(hipMemcpyAsync(fisher_.h_out + 2, fisher_.out.get() + 2, sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    out_host[0] = has_param ? gap_.h_out[0] : 0.0;
    out_host[1] = fisher_.h_out[2];
    return 0;
}

}  // namespace gmrfx
