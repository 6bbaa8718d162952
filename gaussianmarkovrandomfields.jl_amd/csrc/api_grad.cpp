// api_grad.cpp -- the C ABI of include/gmrfx.h: log-density gradients on Q's own pattern, for a plain handle and for the members of a batch.
#include "api_common.h"

// ---- Qbar / mubar of logpdf (+ log_correction) (include/gmrfx.h; Device::logpdf_grad, csrc/grad.hip) --------------------------------
// What the reference's pullbacks form on the host from the whole selected inverse: src/autodiff/logpdf.jl:63-90 with
// src/autodiff/precision_gradient.jl (Qbar = ybar/2 (Sigma - r r'), mubar = ybar Q r), src/workspace/autodiff.jl:14-50 (the same for
// a WorkspaceGMRF, and :24-37 the two constraint terms).
static int32_t grad_impl(gmrfx_handle *h, const double *nz, const double *z, int64_t sz, const double *mu, const double *ybar, double *Qbar,
                         double *mubar, int64_t *info, bool dev, bool batch) {
    return guarded(h, [&]() -> int32_t {
        // the arguments first: they are checked against the handle's sizes, with or without device state
        check_unsharded(h, "logpdf_grad: sharded handles are not supported");
        if (!batch && h->nbatch > 1) throw std::invalid_argument("logpdf_grad: a batched handle takes gmrfx_batch_logpdf_grad");
        if (!z) throw std::invalid_argument("logpdf_grad: z is null");
        if (!ybar) throw std::invalid_argument("logpdf_grad: ybar is null");
        if (!Qbar && !mubar) throw std::invalid_argument("logpdf_grad: Qbar and mubar are both null");
        if (batch && h->nbatch > 1 && sz < h->n_member) throw std::invalid_argument("logpdf_grad: z: member stride smaller than n");
        if (int32_t e = batch ? need_batch(h, true) : need_device(h, true)) return e;
        const int64_t nb = h->nbatch, n = h->n_member, nnz = h->nnz_member;
        const ConHost *A = h->con.m > 0 ? &h->con : (h->bcon.m > 0 ? &h->bcon : nullptr);
        if (mubar && !h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        std::vector<long long> inf((size_t)nb, 0);
        if (dev) h->D->logpdf_grad(h->rsym, A, Device::GradIO{nz, z, sz, mu, ybar, Qbar, mubar}, inf.data());
        else {
            DevBlock bn, bz, bm, bq, bo;
            if (nz && mubar) stage_up(h, bn, nz, nnz * nb);
            stage_up(h, bz, z, n, n, 1, sz, nb);
            if (mu) stage_up(h, bm, mu, n * nb);
            if (Qbar) stage_alloc(h, bq, nnz * nb);
            if (mubar) stage_alloc(h, bo, n * nb);
            h->D->logpdf_grad(h->rsym, A, Device::GradIO{bn, bz, n, bm, ybar, bq, bo}, inf.data());
            if (Qbar) stage_down(h, bq, Qbar, nnz * nb, nnz * nb, 1);
            if (mubar) stage_down(h, bo, mubar, n * nb, n * nb, 1);
        }
        if (info) std::copy(inf.begin(), inf.end(), info);
        // a failed member has NaN in its own outputs; the batch forms say which through info, the others through the return code
        for (int64_t k = 0; k < nb; k++) {
            if (inf[(size_t)k] == 0 || (batch && info)) continue;
            const std::string who = batch ? "member " + std::to_string(k) + ": " : "";
            h->err = "logpdf_grad: " + who + (inf[(size_t)k] < 0 ? "the last factorisation failed (matrix is not positive definite)"
                                                                : "A Q^-1 A' is not positive definite (rank-deficient constraint matrix)");
            return GMRFX_ERR_NOT_POSDEF;
        }
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_logpdf_grad(gmrfx_handle *h, const double *nzval, const double *z, const double *mu, double ybar, double *Qbar, double *mubar) {
    return grad_impl(h, nzval, z, 0, mu, &ybar, Qbar, mubar, nullptr, false, false);
}
extern "C" int32_t gmrfx_logpdf_grad_dev(gmrfx_handle *h, const double *d_nzval, const double *d_z, const double *d_mu, double ybar, double *d_Qbar,
                                         double *d_mubar) {
    return grad_impl(h, d_nzval, d_z, 0, d_mu, &ybar, d_Qbar, d_mubar, nullptr, true, false);
}
extern "C" int32_t gmrfx_batch_logpdf_grad(gmrfx_handle *h, const double *nzval, const double *z, int64_t sz, const double *mu, const double *ybar,
                                           double *Qbar, double *mubar, int64_t *info) {
    return grad_impl(h, nzval, z, sz, mu, ybar, Qbar, mubar, info, false, true);
}
extern "C" int32_t gmrfx_batch_logpdf_grad_dev(gmrfx_handle *h, const double *d_nzval, const double *d_z, int64_t sz, const double *d_mu,
                                               const double *ybar, double *d_Qbar, double *d_mubar, int64_t *info) {
    return grad_impl(h, d_nzval, d_z, sz, d_mu, ybar, d_Qbar, d_mubar, info, true, true);
}

// stored entries of the pattern the handle was created with (per member): the length of Qbar / G, for callers that size buffers
extern "C" int32_t gmrfx_pattern_nnz(const gmrfx_handle *h, int64_t *nnz) {
    if (!h || !nnz) return GMRFX_ERR_INVALID_ARG;
    *nnz = h->nnz_member;
    return GMRFX_OK;
}

// ---- out[k] = sum_e w_e G[e] J[e, k]: dlogpdf/dtheta_k from Qbar and the Jacobian of Q's values (Device::pattern_dot) ---------------
// The contraction the reference's rules leave to the caller's AD (`dot(Qbar, dQ/dtheta)` over the stored pattern, the pullback of
// precision_matrix(model; theta...) in src/workspace/autodiff.jl:259-263), with the Symmetric(Q) weights of gmrfx_quadform.
static int32_t pattern_dot_impl(gmrfx_handle *h, const double *G, const double *J, int64_t ldj, int64_t sj, int64_t p, double *out, bool dev,
                                bool batch) {
    return guarded(h, [&]() -> int32_t {
        check_unsharded(h, "pattern_dot: sharded handles are not supported");
        if (!batch && h->nbatch > 1) throw std::invalid_argument("pattern_dot: a batched handle takes gmrfx_batch_pattern_dot");
        if (!G || !J || !out) throw std::invalid_argument("pattern_dot: G / J / out is null");
        if (p < 1) throw std::invalid_argument("pattern_dot: p < 1");
        if (ldj < std::max<int64_t>(h->nnz_member, 1)) throw std::invalid_argument("pattern_dot: ldj < nnz");
        if (batch && h->nbatch > 1 && (sj < 0 || sj / ldj < p)) throw std::invalid_argument("pattern_dot: J: member stride smaller than ldj * p");
        if (int32_t e = batch ? need_batch(h, false) : need_device(h, false)) return e;
        if (dev) { h->D->pattern_dot(G, J, ldj, sj, p, out); return GMRFX_OK; }
        const int64_t nb = h->nbatch, nnz = h->nnz_member;
        DevBlock bg, bj;
        stage_up(h, bg, G, nnz * nb);
        stage_up(h, bj, J, ldj, nnz, p, sj, nb);
        h->D->pattern_dot(bg, bj, nnz, nnz * p, p, out);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_pattern_dot(gmrfx_handle *h, const double *G, const double *J, int64_t ldj, int64_t p, double *out) {
    return pattern_dot_impl(h, G, J, ldj, 0, p, out, false, false);
}
extern "C" int32_t gmrfx_pattern_dot_dev(gmrfx_handle *h, const double *d_G, const double *d_J, int64_t ldj, int64_t p, double *out) {
    return pattern_dot_impl(h, d_G, d_J, ldj, 0, p, out, true, false);
}
extern "C" int32_t gmrfx_batch_pattern_dot(gmrfx_handle *h, const double *G, const double *J, int64_t ldj, int64_t sj, int64_t p, double *out) {
    return pattern_dot_impl(h, G, J, ldj, sj, p, out, false, true);
}
extern "C" int32_t gmrfx_batch_pattern_dot_dev(gmrfx_handle *h, const double *d_G, const double *d_J, int64_t ldj, int64_t sj, int64_t p, double *out) {
    return pattern_dot_impl(h, d_G, d_J, ldj, sj, p, out, true, true);
}
