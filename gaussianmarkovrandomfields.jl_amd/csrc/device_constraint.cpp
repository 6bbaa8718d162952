// device_constraint.cpp -- the Device's side of linear equality constraints A x = e (include/gmrfx.h: gmrfx_constraints_*,
// gmrfx_sample; kernels in constraint.hip). What the reference builds in ConstraintInfo (src/workspace/workspace_gmrf.jl:22-56)
// is built here once per factorisation and kept in HBM:
//   At = Q^-1 A'    n x m, column-major: zero + scatter of the CSR rows, then ONE blocked solve in place (the existing sweeps)
//   W  = A At       m x m, by the deterministic sparse-rows-times-dense reduction
//   L_c, L_c^-1     host, plain C++ (m <= 64), L_c^-1 uploaded row-major
//   B  = At L_c^-T  n x m, kept BESIDE At (2 x 8 n m bytes: 1 GB at n = 10^6, m = 64; the getter is a plain copy)
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <stdexcept>

#include "device.h"
#include "kernels.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

void *Device::con_alloc(size_t bytes) {
    void *p = nullptr;
    bytes = std::max<size_t>(bytes, 8) + 16;       // 16 bytes of slack, as dalloc
    HC(hipMalloc(&p, bytes));
    allocs_.push_back({p, bytes});
    bytes_total += (double)bytes;
    return p;
}

void Device::con_release(void *p) {
    if (!p) return;
    for (size_t k = 0; k < allocs_.size(); k++)
        if (allocs_[k].first == p) {
            bytes_total -= (double)allocs_[k].second;
            allocs_.erase(allocs_.begin() + (long)k);
            break;
        }
    (void)hipFree(p);
}

void Device::con_drop() {
    HC(hipSetDevice(device));
    HC(hipDeviceSynchronize());        // nothing in flight may still read the buffers
    for (void *p : {(void *)con_.rowptr, (void *)con_.col, (void *)con_.choff, (void *)con_.val, (void *)con_.e, (void *)con_.At, (void *)con_.B,
                    (void *)con_.Linv, (void *)con_.R, (void *)con_.amu, (void *)con_.part, (void *)con_.sig})
        con_release(p);
    const hipEvent_t e0 = con_.ev0, e1 = con_.ev1;
    con_ = ConDev();
    con_.ev0 = e0; con_.ev1 = e1;
}

void Device::con_set(const ConHost &c) {
    con_drop();
    if (c.m <= 0) return;
    if (sharded() || batched()) throw std::invalid_argument("constraints need a plain (unsharded, unbatched) handle");
    const int m = c.m;
    const long long n = S_->n, nnz = c.rowptr[m];
    std::vector<int> choff((size_t)m + 1, 0);
    long long maxlen = 0;
    int maxchunks = 0;
    for (int r = 0; r < m; r++) {
        const long long len = c.rowptr[r + 1] - c.rowptr[r];
        const int ch = (int)((len + kConChunk - 1) / kConChunk);
        choff[r + 1] = choff[r] + ch;
        maxlen = std::max(maxlen, len);
        maxchunks = std::max(maxchunks, ch);
    }
    try {
        con_.rowptr = (long long *)con_alloc((size_t)(m + 1) * sizeof(long long));
        con_.col = (int *)con_alloc((size_t)nnz * sizeof(int));
        con_.val = (double *)con_alloc((size_t)nnz * sizeof(double));
        con_.e = (double *)con_alloc((size_t)m * sizeof(double));
        con_.choff = (int *)con_alloc((size_t)(m + 1) * sizeof(int));
        con_.At = (double *)con_alloc((size_t)n * m * sizeof(double));
        con_.B = (double *)con_alloc((size_t)n * m * sizeof(double));
        con_.Linv = (double *)con_alloc((size_t)m * m * sizeof(double));
        con_.amu = (double *)con_alloc((size_t)m * sizeof(double));
        con_.sig = (double *)con_alloc((size_t)n * sizeof(double));
        HC(hipMemcpy(con_.rowptr, c.rowptr.data(), (size_t)(m + 1) * sizeof(long long), hipMemcpyHostToDevice));
        HC(hipMemcpy(con_.col, c.col.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
        HC(hipMemcpy(con_.val, c.val.data(), (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
        HC(hipMemcpy(con_.e, c.e.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice));
        HC(hipMemcpy(con_.choff, choff.data(), (size_t)(m + 1) * sizeof(int), hipMemcpyHostToDevice));
        if (!con_.ev0) { HC(hipEventCreate(&con_.ev0)); HC(hipEventCreate(&con_.ev1)); }
    } catch (...) {
        con_drop();
        throw;
    }
    con_.m = m; con_.nnz = nnz; con_.maxlen = maxlen; con_.maxchunks = maxchunks; con_.totchunks = choff[m];
}

// column capacity of the reduction's buffers (R: m x cols, part: totchunks x cols); wider blocks go through in pieces
static constexpr long long kConColBatch = 1024;

bool Device::con_prepare() {
    HC(hipSetDevice(device));
    const int m = con_.m;
    if (m <= 0 || con_.serial == factor_serial_) return true;
    const long long n = S_->n;
    con_.serial = 0;
    if (con_.colcap < m) {       // W is an m-column product
        const long long cap = 64;
        void *R = con_alloc((size_t)m * cap * sizeof(double)), *part = con_alloc((size_t)con_.totchunks * cap * sizeof(double));
        HC(hipDeviceSynchronize());
        con_release(con_.R); con_release(con_.part);
        con_.R = (double *)R; con_.part = (double *)part; con_.colcap = cap;
    }
    HC(hipEventRecord(con_.ev0, stream));
    HC(hipMemsetAsync(con_.At, 0, (size_t)n * m * sizeof(double), stream));
    launch_con_scatter(stream, con_.rowptr, con_.col, con_.val, (int)n, m, con_.maxlen, con_.At);
    solve(con_.At, n, m, con_.At, n, true, 0);          // one pass of the sweeps (m <= 64): in place
    launch_con_ax(stream, con_.rowptr, con_.col, con_.val, con_.choff, con_.maxchunks, m, con_.At, n, m, con_.part, nullptr, nullptr, con_.R);
    std::vector<double> W((size_t)m * m);
    HC(hipMemcpyAsync(W.data(), con_.R, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    // L_c from the lower triangle of W (column-major W[r + j m] = (A At)[r, j]). A pivot within rounding of zero relative to its
    // diagonal entry is a failure: two equal rows of A leave a pivot of a few ulps of either sign
    std::vector<double> L((size_t)m * m, 0.0), Li((size_t)m * m, 0.0);
    double ld = 0.0;
    for (int j = 0; j < m; j++) {
        double d = W[(size_t)j + (size_t)j * m];
        for (int q = 0; q < j; q++) d -= L[(size_t)j * m + q] * L[(size_t)j * m + q];
        if (!(d > 16.0 * m * DBL_EPSILON * std::fabs(W[(size_t)j + (size_t)j * m])) || !std::isfinite(d)) return false;
        const double dj = std::sqrt(d);
        L[(size_t)j * m + j] = dj;      // row-major
        ld += 2.0 * std::log(dj);
        for (int i = j + 1; i < m; i++) {
            double s = W[(size_t)i + (size_t)j * m];
            for (int q = 0; q < j; q++) s -= L[(size_t)i * m + q] * L[(size_t)j * m + q];
            L[(size_t)i * m + j] = s / dj;
        }
    }
    for (int j = 0; j < m; j++) {       // column j of L_c^-1 by forward substitution
        Li[(size_t)j * m + j] = 1.0 / L[(size_t)j * m + j];
        for (int i = j + 1; i < m; i++) {
            double s = 0.0;
            for (int q = j; q < i; q++) s -= L[(size_t)i * m + q] * Li[(size_t)q * m + j];
            Li[(size_t)i * m + j] = s / L[(size_t)i * m + i];
        }
    }
    HC(hipMemcpyAsync(con_.Linv, Li.data(), (size_t)m * m * sizeof(double), hipMemcpyHostToDevice, stream));
    launch_con_trsm(stream, con_.At, con_.Linv, (int)n, m, con_.B);
    HC(hipEventRecord(con_.ev1, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms = 0;
    HC(hipEventElapsedTime(&ms, con_.ev0, con_.ev1));
    con_.ms = ms;
    con_.h_w = W; con_.h_linv = Li; con_.logdet_w = ld;
    con_.serial = factor_serial_;
    return true;
}

void Device::con_get(double *At_host, long long ld, double *W_host) {
    HC(hipSetDevice(device));
    const int m = con_.m;
    const long long n = S_->n;
    if (m <= 0) return;
    if (At_host) HC(hipMemcpy2D(At_host, (size_t)ld * sizeof(double), con_.At, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)m,
                                hipMemcpyDeviceToHost));
    if (W_host) std::copy(con_.h_w.begin(), con_.h_w.end(), W_host);
}

void Device::con_correct(double *d_X, long long ldx, long long nvec, const double *d_mu) {
    HC(hipSetDevice(device));
    const int m = con_.m;
    const long long n = S_->n;
    if (nvec <= 0) return;
    if (m <= 0) {
        if (!d_mu) return;
        for (long long j0 = 0; j0 < nvec; j0 += kConColBatch)
            launch_con_apply(stream, nullptr, nullptr, nullptr, d_mu, d_X + j0 * ldx, ldx, (int)n, 0, (int)std::min(kConColBatch, nvec - j0));
        HC(hipStreamSynchronize(stream));
        HC(hipGetLastError());
        return;
    }
    const long long want = std::min(kConColBatch, nvec);
    if (con_.colcap < want) {
        void *R = con_alloc((size_t)m * want * sizeof(double)), *part = con_alloc((size_t)con_.totchunks * want * sizeof(double));
        HC(hipDeviceSynchronize());
        con_release(con_.R); con_release(con_.part);
        con_.R = (double *)R; con_.part = (double *)part; con_.colcap = want;
    }
    HC(hipEventRecord(con_.ev0, stream));
    // with a mean: A (X + mu) - e = A X + (A mu - e), the second term once
    if (d_mu) launch_con_ax(stream, con_.rowptr, con_.col, con_.val, con_.choff, con_.maxchunks, m, d_mu, n, 1, con_.part, con_.e, nullptr, con_.amu);
    for (long long j0 = 0; j0 < nvec; j0 += kConColBatch) {
        const int k = (int)std::min(kConColBatch, nvec - j0);
        double *X = d_X + j0 * ldx;
        launch_con_ax(stream, con_.rowptr, con_.col, con_.val, con_.choff, con_.maxchunks, m, X, ldx, k, con_.part, d_mu ? nullptr : con_.e,
                      d_mu ? con_.amu : nullptr, con_.R);
        launch_con_apply(stream, con_.B, con_.Linv, con_.R, d_mu, X, ldx, (int)n, m, k);
    }
    HC(hipEventRecord(con_.ev1, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms = 0;
    HC(hipEventElapsedTime(&ms, con_.ev0, con_.ev1));
    ms_con_correct = ms;
}

void Device::con_residual(double *out_host) {
    HC(hipSetDevice(device));
    if (con_.m > 0) HC(hipMemcpy(out_host, con_.R, (size_t)con_.m * sizeof(double), hipMemcpyDeviceToHost));
}

void Device::con_var(double *out_host) {
    selinv_compute();
    if (con_.m <= 0) { selinv_diag(out_host); return; }
    const long long n = S_->n;
    launch_gather_diag(stream, d_Z_, ds_.diagoff, ds_.perm, (int)n, con_.sig);
    launch_con_var(stream, con_.B, (int)n, con_.m, con_.sig);
    HC(hipMemcpyAsync(out_host, con_.sig, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
}

}  // namespace gmrfx
