// device_predictive.cpp -- the Device's side of the linear predictor's marginals and the predictive scores (include/gmrfx.h:
// gmrfx_predictor_marginals, gmrfx_predictive_scores; kernels in predictive.hip). The reference forms both on the host from the whole
// posterior (src/linear_predictor_marginals.jl:58-195, pointwise_loglik); here the factor of Q_post, the selected inverse, the
// likelihood, the design plan's term table and the constraint's B are where the Fisher-scoring loop and its pullback left them, and
// only what the caller asks for leaves the device.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>

#include "device.h"
#include "kernels.h"
#include "obs_const.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

void obs_pointwise_const(const ObsHost &o, double *out) {
    const long double p = (long double)o.param;
    for (long long k = 0; k < o.nobs; k++)
        out[k] = (double)obs_const_term(o.family, o.y[(size_t)k], o.aux.empty() ? 0.0 : o.aux[(size_t)k], p);
}

// The first predictive call for a likelihood: the observation order (node form), the constants and the plan's map (design form) go
// up, the scores' buffers are allocated. 4 nobs (node form) + 8 nobs + 8 cnt bytes beside the plan's transposed term table (gap_term_table).
void Device::pred_tables(const ObsHost &o) {
    if (pred_.c) return;
    const size_t nobs = (size_t)o.nobs;
    PredDev p;       // built aside: an upload that fails half-way leaves nothing behind
    std::vector<double> c(nobs);
    obs_pointwise_const(o, c.data());
    dev_upload(p.c, c, &bytes_total);
    if (o.design) dev_upload(p.hmap, o.design->map, &bytes_total);
    else {
        std::vector<int> idx(nobs);
        for (size_t k = 0; k < nobs; k++) idx[k] = (int)o.idx[k];
        dev_upload(p.idx, idx, &bytes_total);
    }
    p.part.alloc(4 * (size_t)design_blocks((long long)nobs), &bytes_total, kTableMinBytes);
    p.out.alloc(4, &bytes_total, kTableMinBytes);
    p.quad.alloc(2 * kPredMaxNodes, &bytes_total, kTableMinBytes);
    p.h_out.alloc(4);
    p.h_quad.alloc(2 * kPredMaxNodes);
    std::fill(p.h_quad + 0, p.h_quad + 2 * kPredMaxNodes, 0.0);
    pred_ = std::move(p);
}

int Device::predictor_marginals(const RbmcSym &sym, const ObsHost &o, const PredIO &io) {
    HC(hipSetDevice(device));
    if (sharded() || many_members()) throw std::invalid_argument("predictor_marginals: batched and sharded handles are not supported");
    if (!io.d_x) throw std::invalid_argument("predictor_marginals: x is null");
    if (!io.d_mu_eta && !io.d_v_eta && !io.d_pll) throw std::invalid_argument("predictor_marginals: every output is null");
    if (!obs_held() || o.nobs <= 0) throw std::invalid_argument("predictor_marginals: no observation likelihood is set (gmrfx_obs_set)");
    const long long n = S_->n;
    if (n > INT_MAX || o.nobs > INT_MAX) throw std::invalid_argument("predictor_marginals: more than 2^31 - 1 nodes or observations");
    const bool correct = io.flags & 1;
    if (correct && con_.m <= 0) throw std::invalid_argument("predictor_marginals: flag bit 0 (constraint correction) needs a constraint (gmrfx_constraints_set)");
    const bool design = (bool)fisher_.design;
    if (io.d_v_eta) {
        if (!factorized) throw std::invalid_argument("predictor_marginals: the variance needs a factorisation");
        if (correct && !con_prepare()) return 2;
        selinv_compute();
        grad_tables();
        if (design) gap_term_table();
        else sym_rows_upload(sym);
    }
    pred_tables(o);
    const int m = io.d_v_eta && correct ? con_.m : 0;
    const PredMarg a{(int)n, (int)o.nobs, m, fisher_.family, io.d_x, pred_.idx.get(), sym_rows_.dpos.get(), fisher_.arp.get(), fisher_.acol.get(),
                     fisher_.aval.get(), fisher_.offset.get(), gap_.optr.get(), gap_.oidx.get(), gap_.ow.get(), pred_.hmap.get(),
                     io.d_v_eta ? grad_.zoff.get() : nullptr, d_Z_, m > 0 ? con_.B.get() : nullptr, fisher_.y.get(), fisher_.aux.get(), pred_.c.get(),
                     fisher_.param, fisher_logparam(fisher_.family, fisher_.param), io.d_mu_eta, io.d_v_eta, io.d_pll};
    launch_pred_marginals(stream, a, design);
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    return 0;
}

void Device::predictive_scores(const ObsHost &o, const ScoreIO &io, double *out4_host) {
    HC(hipSetDevice(device));
    if (sharded() || many_members()) throw std::invalid_argument("predictive_scores: batched and sharded handles are not supported");
    if (!io.d_mu || !io.d_v || !out4_host) throw std::invalid_argument("predictive_scores: mu_eta / v_eta / out is null");
    if (!obs_held() || o.nobs <= 0) throw std::invalid_argument("predictive_scores: no observation likelihood is set (gmrfx_obs_set)");
    if (io.K < 1 || io.K > kPredMaxNodes || !io.z || !io.w) throw std::invalid_argument("predictive_scores: K must be 1 .. 64, with nodes and weights");
    if (o.nobs > INT_MAX) throw std::invalid_argument("predictive_scores: more than 2^31 - 1 observations");
    pred_tables(o);
    std::copy(io.z, io.z + io.K, pred_.h_quad + 0);
    std::copy(io.w, io.w + io.K, pred_.h_quad + kPredMaxNodes);
    HC(hipMemcpyAsync(pred_.quad, pred_.h_quad, 2 * kPredMaxNodes * sizeof(double), hipMemcpyHostToDevice, stream));
    const PredScores a{(int)o.nobs, io.K, fisher_.family, io.d_mu, io.d_v, pred_.idx.get(), fisher_.y.get(), fisher_.aux.get(), pred_.c.get(),
                       pred_.quad.get(), pred_.quad.get() + kPredMaxNodes, fisher_.param, fisher_logparam(fisher_.family, fisher_.param),
                       io.d_lpd, io.d_lcpo, io.d_elp, io.d_vlp, pred_.part.get()};
    launch_pred_scores(stream, a, pred_.out);
    HC(hipMemcpyAsync(pred_.h_out, pred_.out, 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    std::copy(pred_.h_out + 0, pred_.h_out + 4, out4_host);
}

}  // namespace gmrfx
