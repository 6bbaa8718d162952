// api_batch.cpp -- the C ABI of include/gmrfx.h: batched handles and their numeric calls.
#include <chrono>

#include "api_common.h"

// ---- batched handles (include/gmrfx.h) ------------------------------------------------------------------------------------------
// The member's pattern and order are analysed once; the handle itself is an ordinary handle of the block-diagonal forest
// diag(Q_1 .. Q_B): pattern and elimination order replicated with offsets k n. Copies of the member's tree fall on the same levels
// (levels are numbered by depth below each root), so every level launch does B times the work of one member.
extern "C" int32_t gmrfx_create_batched(int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t index_base, const int64_t *perm,
                                        int64_t nbatch, const gmrfx_opts *opts, gmrfx_handle **out) {
    if (!out) { g_create_err = "out is null"; return GMRFX_ERR_INVALID_ARG; }
    *out = nullptr;
    // everything that can be refused is refused before anything is allocated
    if (!colptr || !rowval) { g_create_err = "colptr/rowval is null"; return GMRFX_ERR_INVALID_ARG; }
    if (nbatch < 1) { g_create_err = "nbatch must be >= 1"; return GMRFX_ERR_INVALID_ARG; }
    if (n <= 0) { g_create_err = "n must be positive"; return GMRFX_ERR_INVALID_ARG; }
    if (n > (int64_t)INT32_MAX / nbatch) { g_create_err = "nbatch * n exceeds INT32_MAX (32-bit node indices of the forest)"; return GMRFX_ERR_INVALID_ARG; }
    gmrfx_opts o;
    if (!read_opts(opts, o)) return GMRFX_ERR_INVALID_ARG;
    if (o.shard_world > 1 || o.shard_min_top > 0) { g_create_err = "batched handles cannot be sharded (shard_world > 1 / shard_min_top > 0)"; return GMRFX_ERR_INVALID_ARG; }
    const int64_t nnz = colptr[n] - index_base;
    if (nnz < 0 || nnz > INT64_MAX / nbatch) { g_create_err = "colptr[n] out of range"; return GMRFX_ERR_INVALID_ARG; }
    std::unique_ptr<gmrfx_handle> h(new gmrfx_handle());
    h->opts = o;
    if (int32_t e = create_guarded(true, [&]() -> int32_t {
        const auto t0 = std::chrono::steady_clock::now();
        SymOptions so;
        sym_options(h->opts, so);
        Symbolic M;             // the member: its ordering (user perm, or nested dissection on its own coords) + postorder
        analyze(n, colptr, rowval, index_base, perm, so, M);
        const int64_t N = nbatch * n;
        std::vector<i64> fcol((size_t)N + 1), frow((size_t)(nbatch * nnz)), fperm((size_t)N);
        for (int64_t k = 0; k < nbatch; k++) {
            for (int64_t j = 0; j < n; j++) fcol[k * n + j] = k * nnz + (colptr[j] - index_base);
            for (int64_t p = 0; p < nnz; p++) frow[k * nnz + p] = k * n + (rowval[p] - index_base);
            for (int64_t i = 0; i < n; i++) fperm[k * n + i] = k * n + M.perm[i];
        }
        fcol[N] = nbatch * nnz;
        // the member's order is a postorder of its tree, so the forest's (copies one after the other, roots ascending) is one of the
        // forest: the analysis keeps it as it is
        so.coords = nullptr; so.coord_dim = 0;
        analyze(N, fcol.data(), frow.data(), 0, fperm.data(), so, h->S);
        h->S.flops = (double)nbatch * M.flops;      // the same sum, without the rounding of B copies added one by one
        h->S.ms_symbolic = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        h->opts.coords = nullptr;
        h->nbatch = nbatch; h->n_member = n; h->nnz_member = nnz;
        return GMRFX_OK;
    })) return e;
    if (int32_t e = attach_device(h.get(), true)) return e;
    *out = h.release();
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_batch_size(const gmrfx_handle *h, int64_t *nbatch, int64_t *n_member) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    if (nbatch) *nbatch = h->nbatch;
    if (n_member) *n_member = h->n_member;
    return GMRFX_OK;
}

static int32_t batch_refactorize_impl(gmrfx_handle *h, const double *nz, int64_t *info, bool dev) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_batch(h, false)) return e;
        if (!nz) throw std::invalid_argument("nzval is null");
        h->D->refactorize(nz, dev);
        std::vector<int64_t> inf((size_t)h->nbatch);
        h->D->batch_diag(nullptr, (long long *)inf.data());
        if (info) std::copy(inf.begin(), inf.end(), info);
        return batch_status(h, inf);
    });
}
extern "C" int32_t gmrfx_batch_refactorize(gmrfx_handle *h, const double *nzval, int64_t *info) { return batch_refactorize_impl(h, nzval, info, false); }
extern "C" int32_t gmrfx_batch_refactorize_dev(gmrfx_handle *h, const double *d_nzval, int64_t *info) { return batch_refactorize_impl(h, d_nzval, info, true); }

extern "C" int32_t gmrfx_batch_logdet(gmrfx_handle *h, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = need_batch(h, true)) return e;
        if (!out) throw std::invalid_argument("out is null");
        h->D->batch_diag(out, nullptr);
        return GMRFX_OK;
    });
}

static int32_t batch_solve_impl(gmrfx_handle *h, const double *B, int64_t ldb, int64_t sb, int64_t nrhs, double *X, int64_t ldx, int64_t sx,
                                bool dev, int mode) {
    return guarded(h, [&]() -> int32_t {
        // the arguments first: they are checked against the handle's sizes, with or without device state
        check_block(h, B && X ? B : nullptr, ldb, nrhs, "nrhs", "B/X", &sb, "B");
        check_block(h, X, ldx, nrhs, "nrhs", "B/X", &sx, "X");
        if (int32_t e = need_batch(h, true)) return e;
        if (nrhs == 0) return GMRFX_OK;
        const int64_t n = h->n_member, nb = h->nbatch, N = h->S.n;
        if (dev) {
            const Device::MemberLayout ml{n, sb, sx};
            h->D->solve(B, ldb, nrhs, X, ldx, true, mode, &ml);
            return GMRFX_OK;
        }
        // host arrays: the members stacked into the forest's N x nrhs array (a host copy), the plain host path, and back
        std::vector<double> buf((size_t)(N * nrhs));
        for (int64_t j = 0; j < nrhs; j++)
            for (int64_t k = 0; k < nb; k++) std::memcpy(&buf[(size_t)(j * N + k * n)], B + k * sb + j * ldb, (size_t)n * sizeof(double));
        h->D->solve(buf.data(), N, nrhs, buf.data(), N, false, mode);
        for (int64_t j = 0; j < nrhs; j++)
            for (int64_t k = 0; k < nb; k++) std::memcpy(X + k * sx + j * ldx, &buf[(size_t)(j * N + k * n)], (size_t)n * sizeof(double));
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_solve(gmrfx_handle *h, const double *B, int64_t ldb, int64_t sb, int64_t nrhs, double *X, int64_t ldx, int64_t sx) {
    return batch_solve_impl(h, B, ldb, sb, nrhs, X, ldx, sx, false, 0);
}
extern "C" int32_t gmrfx_batch_solve_dev(gmrfx_handle *h, const double *d_B, int64_t ldb, int64_t sb, int64_t nrhs, double *d_X, int64_t ldx,
                                         int64_t sx) {
    return batch_solve_impl(h, d_B, ldb, sb, nrhs, d_X, ldx, sx, true, 0);
}
extern "C" int32_t gmrfx_batch_backward_solve(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t sz, int64_t nrhs, double *X, int64_t ldx,
                                              int64_t sx) {
    return batch_solve_impl(h, Z, ldz, sz, nrhs, X, ldx, sx, false, 1);
}
extern "C" int32_t gmrfx_batch_backward_solve_dev(gmrfx_handle *h, const double *d_Z, int64_t ldz, int64_t sz, int64_t nrhs, double *d_X,
                                                  int64_t ldx, int64_t sx) {
    return batch_solve_impl(h, d_Z, ldz, sz, nrhs, d_X, ldx, sx, true, 1);
}

static int32_t batch_quadform_impl(gmrfx_handle *h, const double *nz, const double *X, int64_t ldx, int64_t sx, int64_t nvec,
                                   const double *mu, double *quad, bool dev) {
    return guarded(h, [&]() -> int32_t {
        check_batch_quadform(h, X, ldx, sx, nvec, quad);
        if (int32_t e = need_batch(h, false)) return e;
        if (nvec == 0) return GMRFX_OK;
        if (dev) { h->D->batch_quadform(nz, X, ldx, sx, nvec, mu, quad); return GMRFX_OK; }
        // host operands: the members packed on the host (ld = n, stride = n nvec), then staged as one array
        const int64_t n = h->n_member, nb = h->nbatch;
        DevBlock bx, bm, bn;
        std::vector<double> xs((size_t)(n * nvec * nb));
        for (int64_t k = 0; k < nb; k++)
            for (int64_t v = 0; v < nvec; v++) std::memcpy(&xs[(size_t)((k * nvec + v) * n)], X + k * sx + v * ldx, (size_t)n * sizeof(double));
        stage_up(h, bx, xs.data(), (int64_t)xs.size());
        if (mu) stage_up(h, bm, mu, n * nb);
        if (nz) stage_up(h, bn, nz, h->S.nnz_in);
        h->D->batch_quadform(bn, bx, n, n * nvec, nvec, bm, quad);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_quadform(gmrfx_handle *h, const double *nzval, const double *X, int64_t ldx, int64_t sx, int64_t nvec,
                                        const double *mu, double *quad) {
    return batch_quadform_impl(h, nzval, X, ldx, sx, nvec, mu, quad, false);
}
extern "C" int32_t gmrfx_batch_quadform_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t sx, int64_t nvec,
                                            const double *d_mu, double *quad) {
    return batch_quadform_impl(h, d_nzval, d_X, ldx, sx, nvec, d_mu, quad, true);
}

extern "C" int32_t gmrfx_batch_refactorize_logpdf_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t sx,
                                                      int64_t nvec, const double *d_mu, double *quad, double *logdet, int64_t *info) {
    return guarded(h, [&]() -> int32_t {
        if (!d_nzval) throw std::invalid_argument("nzval is null");
        check_batch_quadform(h, d_X, ldx, sx, nvec, quad);
        if (int32_t e = need_batch(h, false)) return e;
        std::vector<int64_t> inf((size_t)h->nbatch);
        h->D->batch_refactorize_logpdf(d_nzval, d_X, ldx, sx, nvec, d_mu, quad, logdet, (long long *)inf.data());
        if (info) std::copy(inf.begin(), inf.end(), info);
        return batch_status(h, inf);
    });
}
