// device_predictive.cpp -- the Device's side of the linear predictor's marginals and the predictive scores (include/gmrfx.h:
// gmrfx_predictor_marginals, gmrfx_predictive_scores, their gmrfx_batch_* forms and gmrfx_batch_predictive_mixture; kernels in
// predictive.hip). The reference forms both on the host from the whole posterior (src/linear_predictor_marginals.jl:58-195,
// pointwise_loglik); here the factor of Q_post, the selected inverse, the likelihood, the design plan's term table and the constraint's
// B are where the Fisher-scoring loop and its pullback left them, and only what the caller asks for leaves the device.
// What the plain and the batched calls share is here: the one state (PredDev) with its builder and the two launch routines that fill
// the kernels' arguments (pred_marg_launch, pred_score_launch). A plain handle is one member with every stride zero, its parameter by
// value and nobody masked; the batch adds the members' strides, their parameters on the device and the mask of the members that failed.
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
    for (size_t c = 0; c < o.comp.size(); c++) {        // a composite: every row under its own component
        const long double p = (long double)o.comp.param[c];
        for (long long k = o.comp.rowptr[c]; k < o.comp.rowptr[c + 1]; k++)
            out[k] = (double)obs_const_term(o.comp.family[c], o.y[(size_t)k], o.aux.empty() ? 0.0 : o.aux[(size_t)k], p);
    }
    if (!o.comp.empty()) return;
    const long double p = (long double)o.param;
    for (long long k = 0; k < o.nobs; k++)
        out[k] = (double)obs_const_term(o.family, o.y[(size_t)k], o.aux.empty() ? 0.0 : o.aux[(size_t)k], p);
}

static bool family_has_param(int family) { return family == 0 || family == 4 || family == 5; }
// column k of the members' constants: the plain rule at param[k]
static void bobs_const_column(const BObsHost &o, size_t k, double *out) {
    const long double p = (long double)o.param[k];
    for (long long i = 0; i < o.nobs; i++)
        out[i] = (double)obs_const_term(o.family, o.y[(size_t)i], o.aux.empty() ? 0.0 : o.aux[(size_t)i], p);
}
void bobs_pointwise_const(const BObsHost &o, double *out) {
    for (size_t k = 0; k < o.param.size(); k++) bobs_const_column(o, k, out + (long long)k * o.nobs);
}

// The observation order (node form) or the plan's map (design form), the constants and the work of `members` members, built aside: an
// upload that fails half-way leaves nothing behind. 4 nobs (node form) + 8 nobs per column of c + 8 cnt bytes beside the plan's
// transposed term table (gap_term_table), and 32 bytes per workgroup and member of partial sums.
Device::PredDev Device::pred_build(long long nobs_, const std::vector<long long> &idx_host, const DesignPlan *plan, const std::vector<double> &c,
                                   int members) {
    const size_t nobs = (size_t)nobs_, nb = (size_t)members;
    PredDev p;
    p.nobs = nobs_;
    p.members = members;
    p.sc = c.size() > nobs ? nobs_ : 0;       // (one column: every member reads it)
    dev_upload(p.c, c, &bytes_total);
    if (plan) dev_upload(p.hmap, plan->map, &bytes_total);
    else {
        std::vector<int> idx(nobs);
        for (size_t k = 0; k < nobs; k++) idx[k] = (int)idx_host[k];
        dev_upload(p.idx, idx, &bytes_total);
    }
    p.part.alloc(4 * nb * (size_t)design_blocks(nobs_), &bytes_total, kTableMinBytes);
    p.out.alloc(4 * nb, &bytes_total, kTableMinBytes);
    p.quad.alloc(2 * kPredMaxNodes, &bytes_total, kTableMinBytes);
    p.h_out.alloc(4 * (long long)nb);
    p.h_quad.alloc(2 * kPredMaxNodes);
    std::fill(p.h_quad + 0, p.h_quad + 2 * kPredMaxNodes, 0.0);
    return p;
}

// The first predictive call for a likelihood
void Device::pred_tables(const ObsHost &o) {
    if (pred_.c) return;
    std::vector<double> c((size_t)o.nobs);
    obs_pointwise_const(o, c.data());
    PredDev p = pred_build(o.nobs, o.idx, o.design.get(), c, 1);
    pred_ = std::move(p);
}

// and for a batch likelihood: one column of constants where they do not depend on the parameter, one per member where they do; the
// mixture's weights (2 per member) with their pinned copy
void Device::bpred_tables(const BObsHost &o) {
    if (bpred_.c) return;
    const size_t nb = (size_t)nbatch_, cols = family_has_param(o.family) ? nb : 1;
    std::vector<double> c((size_t)o.nobs * cols);
    for (size_t k = 0; k < cols; k++) bobs_const_column(o, k, c.data() + k * (size_t)o.nobs);
    PredDev p = pred_build(o.nobs, o.idx, o.design.get(), c, (int)nb);
    p.mixw.alloc(2 * nb, &bytes_total, kTableMinBytes);
    p.h_mixw.alloc(2 * (long long)nb);
    bpred_ = std::move(p);
}

void Device::pred_marg_launch(const FisherDev &f, const GapDev &g, const PredDev &p, const PredRun &r, const PredIO &io) {
    auto a = PredMarg{};      // (every field zero, then by name)
    a.n = f.n; a.nobs = (int)p.nobs; a.m = r.m; a.family = f.family;
    a.x = io.d_x; a.idx = p.idx; a.dpos = r.dpos;
    a.arp = f.arp; a.acol = f.acol; a.aval = f.aval; a.offset = f.offset;
    a.optr = g.optr; a.oidx = g.oidx; a.ow = g.ow; a.hmap = p.hmap;
    a.zoff = io.d_v_eta ? grad_.zoff.get() : nullptr; a.Z = d_Z_;
    a.B = r.m > 0 ? r.B : nullptr;
    a.y = f.y; a.aux = f.aux; a.c = p.c;
    a.param = f.param; a.logparam = f.logparam;
    a.mu_eta = io.d_mu_eta; a.v_eta = io.d_v_eta; a.pll = io.d_pll;
    a.sx = r.sx; a.sz = r.sz; a.sb = r.sb; a.sc = p.sc; a.so = r.so;
    a.param_k = f.param_k; a.logparam_k = f.logparam_k; a.active = r.d_active;
    if (f.ncomp > 0) launch_pred_marginals_comp(stream, a, f.comp_table(), p.members);
    else launch_pred_marginals(stream, a, (bool)f.design, p.members);
}

void Device::pred_score_launch(const FisherDev &f, PredDev &p, const ScoreIO &io, long long stride, const unsigned char *d_active) {
    std::copy(io.z, io.z + io.K, p.h_quad + 0);
    std::copy(io.w, io.w + io.K, p.h_quad + kPredMaxNodes);
    HC(hipMemcpyAsync(p.quad, p.h_quad, 2 * kPredMaxNodes * sizeof(double), hipMemcpyHostToDevice, stream));
    auto a = PredScores{};
    a.nobs = (int)p.nobs; a.K = io.K; a.family = f.family;
    a.mu = io.d_mu; a.v = io.d_v; a.idx = p.idx;
    a.y = f.y; a.aux = f.aux; a.c = p.c;
    a.z = p.quad.get(); a.w = p.quad.get() + kPredMaxNodes;
    a.param = f.param; a.logparam = f.logparam;
    a.lpd = io.d_lpd; a.lcpo = io.d_lcpo; a.elp = io.d_elp; a.vlp = io.d_vlp;
    a.part = p.part;
    a.sm = stride; a.sc = p.sc; a.so = stride;
    a.param_k = f.param_k; a.logparam_k = f.logparam_k; a.active = d_active;
    if (f.ncomp > 0) launch_pred_scores_comp(stream, a, f.comp_table(), p.members, p.out);
    else launch_pred_scores(stream, a, p.members, p.out);
    HC(hipMemcpyAsync(p.h_out, p.out, 4 * (size_t)p.members * sizeof(double), hipMemcpyDeviceToHost, stream));
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
    // one member on the handle's own diagonal positions and B: no strides, nobody masked
    pred_marg_launch(fisher_, gap_, pred_, PredRun{sym_rows_.dpos, con_.B, io.d_v_eta && correct ? con_.m : 0, 0, 0, 0, 0, nullptr}, io);
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
    pred_score_launch(fisher_, pred_, io, 0, nullptr);
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    std::copy(pred_.h_out + 0, pred_.h_out + 4, out4_host);
}

// ---- every member of a batched handle ------------------------------------------------------------------------------------------------
int Device::batch_predictor_marginals(const RbmcSym &sym, const BObsHost &o, const BPredIO &io, long long *info_host) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("batch_predictor_marginals: sharded handles are not supported");
    if (!io.d_x) throw std::invalid_argument("batch_predictor_marginals: x is null");
    if (!io.d_mu_eta && !io.d_v_eta && !io.d_pll) throw std::invalid_argument("batch_predictor_marginals: every output is null");
    if (!bobs_held() || o.nobs <= 0) throw std::invalid_argument("batch_predictor_marginals: no observation likelihood is set (gmrfx_batch_obs_set)");
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    if (io.flags < 0 || io.flags > 1) throw std::invalid_argument("batch_predictor_marginals: unknown flag bits");
    const bool correct = io.flags & 1;
    if (correct && bcon_.m <= 0)
        throw std::invalid_argument("batch_predictor_marginals: flag bit 0 (constraint correction) needs a batch constraint (gmrfx_batch_constraints_set)");
    const long long n = nmember_, nobs = o.nobs;
    if (n > INT_MAX || nobs > INT_MAX) throw std::invalid_argument("batch_predictor_marginals: more than 2^31 - 1 nodes or observations");
    const size_t nb = (size_t)nbatch_;
    const bool design = (bool)bfisher_.design;
    // the members that take part. The mean and the log density need no factor: without the variance nobody is masked. With it a failed
    // factor masks its member out, and so does a failed W_k under bit 0, read on the host BEFORE any correction is launched (its B_k is NaN).
    std::vector<long long> inf(nb, 0);
    std::vector<unsigned char> mask(nb, 1);
    bool failed = false;
    if (io.d_v_eta) {
        if (!factorized) throw std::invalid_argument("batch_predictor_marginals: the variance needs a factorisation");
        batch_diag(nullptr, inf.data());
        for (size_t k = 0; k < nb; k++)
            if (inf[k] != 0) { inf[k] = -1; mask[k] = 0; failed = true; }
        const bool any = std::find(mask.begin(), mask.end(), (unsigned char)1) != mask.end();
        if (correct && any) {
            const std::vector<long long> &ci = bcon_prepare_members();
            for (size_t k = 0; k < nb; k++)
                if (mask[k] && ci[k] > 0) { inf[k] = ci[k]; mask[k] = 0; failed = true; }
        }
        selinv_compute();
        grad_tables();
        if (design) gap_term_table(bfisher_, bgap_);
    }
    bpred_tables(o);
    if (io.d_v_eta && !design && !bpred_.dpos) {       // the member's diagonal positions: the forest's first n
        DevBuf<int> dpos;
        dev_upload(dpos, std::vector<int>(sym.diag.begin(), sym.diag.begin() + (std::ptrdiff_t)n), &bytes_total);
        bpred_.dpos = std::move(dpos);
    }
    const unsigned char *d_mask = nullptr;
    if (failed) {
        bfisher_ctl(nullptr, mask);
        d_mask = reinterpret_cast<const unsigned char *>(bfisher_.ctl.get() + nb);
    }
    const int m = io.d_v_eta && correct ? bcon_.m : 0;
    // every member on ONE copy of the member's diagonal positions, map slice and tables
    pred_marg_launch(bfisher_, bgap_, bpred_, PredRun{bpred_.dpos, bcon_.B, m, io.sx, nnz_member_, n * (long long)m, nobs, d_mask},
                     PredIO{io.d_x, io.flags, io.d_mu_eta, io.d_v_eta, io.d_pll});
    // a member that takes no part: NaN in what was asked of it, nothing else of it is touched
    if (d_mask) {
        if (io.d_mu_eta) launch_gap_fill_failed(stream, nobs, io.d_mu_eta, nobs, d_mask, (int)nb);
        if (io.d_v_eta) launch_gap_fill_failed(stream, nobs, io.d_v_eta, nobs, d_mask, (int)nb);
        if (io.d_pll) launch_gap_fill_failed(stream, nobs, io.d_pll, nobs, d_mask, (int)nb);
    }
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    if (info_host) std::copy(inf.begin(), inf.end(), info_host);
    return failed ? 1 : 0;
}

int Device::batch_predictive_scores(const BObsHost &o, const ScoreIO &io, double *out_host, long long *info_host) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("batch_predictive_scores: sharded handles are not supported");
    if (!io.d_mu || !io.d_v || !out_host) throw std::invalid_argument("batch_predictive_scores: mu_eta / v_eta / out is null");
    if (!bobs_held() || o.nobs <= 0) throw std::invalid_argument("batch_predictive_scores: no observation likelihood is set (gmrfx_batch_obs_set)");
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    if (io.K < 1 || io.K > kPredMaxNodes || !io.z || !io.w) throw std::invalid_argument("batch_predictive_scores: K must be 1 .. 64, with nodes and weights");
    const long long nobs = o.nobs;
    if (nobs > INT_MAX) throw std::invalid_argument("batch_predictive_scores: more than 2^31 - 1 observations");
    const size_t nb = (size_t)nbatch_;
    // the scores read no factor; a member whose factor (where the handle holds one) failed is reported and masked all the same: its
    // variance is NaN, and so its four would be
    std::vector<long long> inf(nb, 0);
    std::vector<unsigned char> mask(nb, 1);
    bool failed = false;
    if (factorized) {
        batch_diag(nullptr, inf.data());
        for (size_t k = 0; k < nb; k++)
            if (inf[k] != 0) { inf[k] = -1; mask[k] = 0; failed = true; }
    }
    bpred_tables(o);
    const unsigned char *d_mask = nullptr;
    if (failed) {
        bfisher_ctl(nullptr, mask);
        d_mask = reinterpret_cast<const unsigned char *>(bfisher_.ctl.get() + nb);
    }
    pred_score_launch(bfisher_, bpred_, io, nobs, d_mask);
    if (d_mask)
        for (double *p : {io.d_lpd, io.d_lcpo, io.d_elp, io.d_vlp})
            if (p) launch_gap_fill_failed(stream, nobs, p, nobs, d_mask, (int)nb);
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    for (size_t k = 0; k < nb; k++)
        for (int r = 0; r < 4; r++) out_host[4 * k + r] = mask[k] ? bpred_.h_out[4 * k + r] : std::nan("");
    if (info_host) std::copy(inf.begin(), inf.end(), info_host);
    return failed ? 1 : 0;
}

void Device::batch_predictive_mixture(const BObsHost &o, const std::vector<double> &w, const MixIO &io, double *out_host) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("batch_predictive_mixture: sharded handles are not supported");
    if (!bobs_held() || o.nobs <= 0) throw std::invalid_argument("batch_predictive_mixture: no observation likelihood is set (gmrfx_batch_obs_set)");
    const size_t nb = (size_t)nbatch_;
    if (w.size() != 2 * nb) throw std::invalid_argument("batch_predictive_mixture: the weights do not belong to this handle");
    if (o.nobs > INT_MAX) throw std::invalid_argument("batch_predictive_mixture: more than 2^31 - 1 observations");
    bpred_tables(o);
    HC(hipStreamSynchronize(stream));      // (a copy enqueued earlier may still be reading the pinned weights)
    std::copy(w.begin(), w.end(), bpred_.h_mixw + 0);
    HC(hipMemcpyAsync(bpred_.mixw, bpred_.h_mixw, 2 * nb * sizeof(double), hipMemcpyHostToDevice, stream));
    const PredMix a{(int)o.nobs, (int)nb, bpred_.mixw, io.d_mu, io.d_v, io.d_lpd, io.d_mix_mu, io.d_mix_v, io.d_lpd ? io.d_mix_lpd : nullptr, bpred_.part};
    launch_pred_mixture(stream, a, bpred_.out);
    if (io.d_lpd) HC(hipMemcpyAsync(bpred_.h_out, bpred_.out, sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    if (out_host) *out_host = io.d_lpd ? bpred_.h_out[0] : std::nan("");
}

}  // namespace gmrfx
