// device_constraint.cpp -- the Device's side of linear equality constraints A x = e (include/gmrfx.h: gmrfx_constraints_*,
// gmrfx_sample; kernels in constraint.hip). What the reference builds in ConstraintInfo (src/workspace/workspace_gmrf.jl:22-56)
// is built here once per factorisation and kept in HBM:
//   At = Q^-1 A'    n x m, column-major: zero + scatter of the CSR rows, then ONE blocked solve in place (the existing sweeps)
//   W  = A At       m x m, by the deterministic sparse-rows-times-dense reduction
//   L_c, L_c^-1     host, plain C++ (m <= 64), L_c^-1 uploaded row-major
//   B  = At L_c^-T  n x m, kept BESIDE At (2 x 8 n m bytes: 1 GB at n = 10^6, m = 64; the getter is a plain copy)
// Batched handles (bcon_*, at the end of this file): one A and e, the same operands per member in member-strided blocks, and L_c,
// L_c^-1 on the device (k_batch_con_chol) -- no download of W, no host loop over the members.
#include <new>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <stdexcept>

#include "device.h"
#include "kernels.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

// A's rows, e and the chunk offsets of the reduction on the device (c.m > 0)
Device::ConRows Device::con_rows_upload(const ConHost &c) {
    ConRows a;
    const int m = c.m;
    const long long nnz = c.rowptr[m];
    std::vector<int> choff((size_t)m + 1, 0);
    for (int r = 0; r < m; r++) {
        const long long len = c.rowptr[r + 1] - c.rowptr[r];
        const int ch = (int)((len + kConChunk - 1) / kConChunk);
        choff[r + 1] = choff[r] + ch;
        a.maxlen = std::max(a.maxlen, len);
        a.maxchunks = std::max(a.maxchunks, ch);
    }
    a.rowptr.alloc((size_t)m + 1, &bytes_total, kTableMinBytes);
    a.col.alloc((size_t)nnz, &bytes_total, kTableMinBytes);
    a.val.alloc((size_t)nnz, &bytes_total, kTableMinBytes);
    a.e.alloc((size_t)m, &bytes_total, kTableMinBytes);
    a.choff.alloc((size_t)m + 1, &bytes_total, kTableMinBytes);
    HC(hipMemcpy(a.rowptr, c.rowptr.data(), (size_t)(m + 1) * sizeof(long long), hipMemcpyHostToDevice));
    HC(hipMemcpy(a.col, c.col.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HC(hipMemcpy(a.val, c.val.data(), (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    HC(hipMemcpy(a.e, c.e.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice));
    HC(hipMemcpy(a.choff, choff.data(), (size_t)(m + 1) * sizeof(int), hipMemcpyHostToDevice));
    a.m = m; a.nnz = nnz; a.totchunks = choff[m];
    return a;
}

void Device::con_drop() {
    HC(hipSetDevice(device));
    HC(hipDeviceSynchronize());        // nothing in flight may still read the buffers
    con_ = ConDev();
    grad_drop_constraint();
}

void Device::con_set(const ConHost &c) {
    con_drop();
    if (c.m <= 0) return;
    if (sharded() || nbatch_ > 1) throw std::invalid_argument("constraints need a plain (unsharded, unbatched) handle");
    const int m = c.m;
    const long long n = S_->n;
    ConDev d;        // a failure half-way leaves the handle without constraints
    static_cast<ConRows &>(d) = con_rows_upload(c);
    d.At.alloc((size_t)n * m, &bytes_total, kTableMinBytes);
    d.B.alloc((size_t)n * m, &bytes_total, kTableMinBytes);
    d.Linv.alloc((size_t)m * m, &bytes_total, kTableMinBytes);
    d.amu.alloc((size_t)m, &bytes_total, kTableMinBytes);
    d.sig.alloc((size_t)n, &bytes_total, kTableMinBytes);
    for (Event &e : con_ev_) e.ensure();
    con_ = std::move(d);
}

// column capacity of the reduction's buffers (R: m x cols, part: totchunks x cols); wider blocks go through in pieces
static constexpr long long kConColBatch = 1024;

// the reduction's buffers for `cols` columns: the new pair first (released again if either does not fit), the old pair goes
// once nothing in flight can still read it
void Device::con_reserve_cols(ConRows &a, long long cols, int members) {
    if (a.colcap >= cols) return;
    DevBuf<double> R, part;
    R.alloc((size_t)a.m * cols * members, &bytes_total, kTableMinBytes);
    part.alloc((size_t)a.totchunks * cols * members, &bytes_total, kTableMinBytes);
    HC(hipDeviceSynchronize());
    a.R = std::move(R); a.part = std::move(part); a.colcap = cols;
}

bool Device::con_prepare() {
    HC(hipSetDevice(device));
    const int m = con_.m;
    if (m <= 0 || con_.serial == factor_serial_) return true;
    const long long n = S_->n;
    con_.serial = 0;
    if (con_.colcap < m) con_reserve_cols(con_, 64, 1);       // W is an m-column product
    HC(hipEventRecord(con_ev_[0], stream));
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
    HC(hipEventRecord(con_ev_[1], stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms = 0;
    HC(hipEventElapsedTime(&ms, con_ev_[0], con_ev_[1]));
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

void Device::con_correct(double *d_X, long long ldx, long long nvec, const double *d_mu, bool homogeneous) {
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
    con_reserve_cols(con_, std::min(kConColBatch, nvec), 1);
    HC(hipEventRecord(con_ev_[0], stream));
    // with a mean: A (X + mu) - e = A X + (A mu - e), the second term once
    if (d_mu) launch_con_ax(stream, con_.rowptr, con_.col, con_.val, con_.choff, con_.maxchunks, m, d_mu, n, 1, con_.part, con_.e, nullptr, con_.amu);
    for (long long j0 = 0; j0 < nvec; j0 += kConColBatch) {
        const int k = (int)std::min(kConColBatch, nvec - j0);
        double *X = d_X + j0 * ldx;
        launch_con_ax(stream, con_.rowptr, con_.col, con_.val, con_.choff, con_.maxchunks, m, X, ldx, k, con_.part, (d_mu || homogeneous) ? nullptr : con_.e.get(),
                      d_mu ? con_.amu.get() : nullptr, con_.R);
        launch_con_apply(stream, con_.B, con_.Linv, con_.R, d_mu, X, ldx, (int)n, m, k);
    }
    HC(hipEventRecord(con_ev_[1], stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms = 0;
    HC(hipEventElapsedTime(&ms, con_ev_[0], con_ev_[1]));
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

// ---- batched handles: the constraint of every member (include/gmrfx.h: gmrfx_batch_constraints_*, gmrfx_batch_sample) -------------
// Columns of X per piece of a correction (capacity of R: m x piece x B and of the chunk sums: totchunks x piece x B): the plain
// handle's 1024 for one member, fewer for many -- 64 from B = 128 on, so that R stays at 4 MB for B = 128, m = 64. Columns are
// independent of each other: the piece changes no bits.
static long long bcon_piece(int nbatch) {
    return std::min<long long>(kConColBatch, std::max<long long>(64, (8192 / std::max(nbatch, 1)) / 64 * 64));
}

void Device::bcon_set(const ConHost &c) {
    HC(hipSetDevice(device));
    if (c.m <= 0) {
        HC(hipDeviceSynchronize());
        bcon_ = BConDev();
        grad_drop_constraint();
        return;
    }
    if (sharded() || !batched()) throw std::invalid_argument("batch constraints need an unsharded handle with its batch buffers");
    if (nbatch_ > 65535) throw std::invalid_argument("batch constraints: more than 65535 members");
    const int m = c.m, nb = nbatch_;
    const long long n = nmember_;
    BConDev b;      // built aside: a failure leaves the handle's state as it was
    // the two big arrays first, and quietly: that they do not fit is an answer (GMRFX_ERR_ALLOC), not a failure of the device
    if (!b.At.try_alloc((size_t)n * nb * m, &bytes_total) || !b.B.try_alloc((size_t)n * nb * m, &bytes_total)) throw std::bad_alloc();
    static_cast<ConRows &>(b) = con_rows_upload(c);
    b.W.alloc((size_t)m * m * nb, &bytes_total, kTableMinBytes);
    b.Linv.alloc((size_t)m * m * nb, &bytes_total, kTableMinBytes);
    b.amu.alloc((size_t)m * nb, &bytes_total, kTableMinBytes);
    b.sig.alloc((size_t)n * nb, &bytes_total, kTableMinBytes);
    b.stat.alloc(2 * (size_t)nb, &bytes_total, kTableMinBytes);
    b.cinfo.alloc((size_t)nb, &bytes_total, kTableMinBytes);
    for (Event &e : bcon_ev_) e.ensure();
    b.piece = bcon_piece(nb);
    HC(hipDeviceSynchronize());        // nothing in flight may still read the previous buffers
    bcon_ = std::move(b);
    grad_drop_constraint();
}

bool Device::bcon_prepare() {
    HC(hipSetDevice(device));
    BConDev &b = bcon_;
    const int m = b.m, nb = nbatch_;
    if (m <= 0) return true;
    if (b.serial == factor_serial_) return b.ok;
    const long long n = nmember_;
    b.serial = 0;
    con_reserve_cols(bcon_, 64, nbatch_);       // W_k is an m-column product
    if (bdiag_for_ != factor_serial_) enqueue_batch_diag(stream);       // the members' factorisation status, for k_batch_con_chol
    HC(hipEventRecord(bcon_ev_[0], stream));
    HC(hipMemsetAsync(b.At, 0, (size_t)n * nb * m * sizeof(double), stream));
    launch_con_scatter(stream, b.rowptr, b.col, b.val, (int)n, m, b.maxlen, b.At, nb);
    const MemberLayout ml{n, n * m, n * m};
    solve(b.At, n, m, b.At, n, true, 0, &ml);         // ONE pass of the forest's sweeps for all members (m <= 64): in place
    launch_con_ax(stream, b.rowptr, b.col, b.val, b.choff, b.maxchunks, m, b.At, n, m, b.part, nullptr, nullptr, b.W, nb, n * m);
    launch_batch_con_chol(stream, b.W, m, nb, reinterpret_cast<const long long *>(d_bdiag_ + nbatch_), b.Linv, b.stat, b.cinfo);
    launch_batch_con_void(stream, b.cinfo, b.At, n * m, b.W, m * m, nb);
    launch_con_trsm(stream, b.At, b.Linv, (int)n, m, b.B, nb);
    HC(hipEventRecord(bcon_ev_[1], stream));
    b.h_logdet.assign((size_t)nb, 0.0);
    b.h_cinfo.assign((size_t)nb, 0);
    HC(hipMemcpyAsync(b.h_logdet.data(), b.stat, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipMemcpyAsync(b.h_cinfo.data(), b.cinfo, (size_t)nb * sizeof(long long), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms = 0;
    HC(hipEventElapsedTime(&ms, bcon_ev_[0], bcon_ev_[1]));
    b.ms = ms;
    b.ok = true;
    for (int k = 0; k < nb; k++) b.ok = b.ok && b.h_cinfo[(size_t)k] <= 0;
    b.serial = factor_serial_;
    return b.ok;
}

void Device::bcon_get(int member, double *At_host, long long ld, double *W_host) {
    HC(hipSetDevice(device));
    const int m = bcon_.m;
    const long long n = nmember_;
    if (m <= 0) return;
    if (At_host) HC(hipMemcpy2D(At_host, (size_t)ld * sizeof(double), bcon_.At + (size_t)member * n * m, (size_t)n * sizeof(double),
                                (size_t)n * sizeof(double), (size_t)m, hipMemcpyDeviceToHost));
    if (W_host) HC(hipMemcpy(W_host, bcon_.W + (size_t)member * m * m, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost));
}

void Device::bcon_correct(double *d_X, long long ldx, long long sx, long long nvec, const double *d_mu) {
    HC(hipSetDevice(device));
    BConDev &b = bcon_;
    const int m = b.m, nb = nbatch_;
    const long long n = nmember_;
    if (nvec <= 0 || (m <= 0 && !d_mu)) return;
    const long long piece = m > 0 ? b.piece : bcon_piece(nb);
    if (m > 0) con_reserve_cols(bcon_, std::min(piece, nvec), nbatch_);
    // with a mean: A (X + mu) - e = A X + (A mu - e), the second term once
    if (m > 0 && d_mu) launch_con_ax(stream, b.rowptr, b.col, b.val, b.choff, b.maxchunks, m, d_mu, n, 1, b.part, b.e, nullptr, b.amu, nb, n);
    for (long long j0 = 0; j0 < nvec; j0 += piece) {
        const int k = (int)std::min(piece, nvec - j0);
        double *X = d_X + j0 * ldx;
        if (m > 0)
            launch_con_ax(stream, b.rowptr, b.col, b.val, b.choff, b.maxchunks, m, X, ldx, k, b.part, d_mu ? nullptr : b.e.get(), d_mu ? b.amu.get() : nullptr, b.R,
                          nb, sx);
        launch_con_apply(stream, b.B, b.Linv, b.R, d_mu, X, ldx, (int)n, m, k, nb, sx, n);
    }
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
}

void Device::bcon_project(double *d_S, long long stride, const unsigned char *d_active) {
    HC(hipSetDevice(device));
    BConDev &b = bcon_;
    const int m = b.m, nb = nbatch_;
    const long long n = nmember_;
    if (m <= 0) return;
    con_reserve_cols(bcon_, 1, nbatch_);        // (bcon_prepare has reserved more)
    launch_con_ax(stream, b.rowptr, b.col, b.val, b.choff, b.maxchunks, m, d_S, n, 1, b.part, nullptr, nullptr, b.R, nb, stride, d_active);
    launch_con_apply(stream, b.B, b.Linv, b.R, nullptr, d_S, n, (int)n, m, 1, nb, stride, n, d_active);
}

void Device::bcon_residual(const double *d_x, long long sx, const unsigned char *d_active, const unsigned char *active_host, double *out_host) {
    HC(hipSetDevice(device));
    BConDev &b = bcon_;
    const int m = b.m, nb = nbatch_;
    if (m <= 0) return;
    con_reserve_cols(bcon_, 1, nbatch_);
    launch_con_ax(stream, b.rowptr, b.col, b.val, b.choff, b.maxchunks, m, d_x, nmember_, 1, b.part, b.e, nullptr, b.R, nb, sx, d_active);
    launch_batch_con_maxabs(stream, b.R, m, nb, d_active, b.stat + nb);
    std::vector<double> r((size_t)nb);
    HC(hipMemcpyAsync(r.data(), b.stat + nb, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    for (int k = 0; k < nb; k++)
        if (!active_host || active_host[k]) out_host[k] = r[(size_t)k];
}

void Device::bcon_quad(const double *d_x, double *quad_host) {
    HC(hipSetDevice(device));
    BConDev &b = bcon_;
    const int m = b.m, nb = nbatch_;
    const long long n = nmember_;
    if (m <= 0) { std::fill(quad_host, quad_host + nb, 0.0); return; }
    con_reserve_cols(bcon_, 1, nbatch_);
    if (!d_x) HC(hipMemsetAsync(b.sig, 0, (size_t)n * sizeof(double), stream));       // a zero mean, shared by the members
    launch_con_ax(stream, b.rowptr, b.col, b.val, b.choff, b.maxchunks, m, d_x ? d_x : b.sig, n, 1, b.part, b.e, nullptr, b.R, nb, d_x ? n : 0);
    launch_batch_con_quad(stream, b.Linv, b.R, m, m, nb, b.stat + nb);
    HC(hipMemcpyAsync(quad_host, b.stat + nb, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
}

void Device::bcon_var(double *out_host) {
    selinv_compute();
    if (bcon_.m <= 0) { selinv_diag(out_host); return; }
    const long long N = S_->n;
    launch_gather_diag(stream, d_Z_, ds_.diagoff, ds_.perm, (int)N, bcon_.sig);
    launch_con_var(stream, bcon_.B, (int)nmember_, bcon_.m, bcon_.sig, nbatch_);
    HC(hipMemcpyAsync(out_host, bcon_.sig, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
}

}  // namespace gmrfx
