// device_grad.cpp -- the Device's side of the log-density gradients on Q's own pattern (include/gmrfx.h: gmrfx_logpdf_grad,
// gmrfx_pattern_dot and their batch forms; kernels in grad.hip). The pullbacks of the reference (src/autodiff/logpdf.jl:63-90,
// src/autodiff/logdetcov.jl:14-18, src/workspace/autodiff.jl:14-50) download the whole selected inverse and form
//   Qbar = ybar/2 (Sigma - r r') - ybar/2 At (W^-1 - w w') At',   mubar = ybar Q r - ybar A' W^-1 (e - A mu)
// on the host; only the entries on pattern(Q) are ever used. Here they are formed where Sigma's panels, B = At L_c^-T and L_c^-1
// already are, per member of a batch, and only pattern(Q)-sized arrays (or p contracted numbers) leave the device.
#include <algorithm>
#include <climits>
#include <new>
#include <stdexcept>

#include "device.h"
#include "kernels.h"
#include "selinv_offsets.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

// The tables that depend on the symbolic structure only: built on the first call, kept for the handle's life, on its books.
void Device::grad_tables() {
    if (grad_.zoff) return;
    const Symbolic &S = *S_;
    // pattern(Q) is inside pattern(L + L'): every stored entry has a place in the panels
    const std::vector<long long> off = z_offsets_csc(S, S.n, S.in_colptr.data(), S.in_row.data(), 0);
    for (long long o : off)
        if (o < 0 || o >= l_size_) throw std::runtime_error("logpdf_grad: a stored entry of Q has no place in the selected-inverse panels (internal error)");
    // the weights k_quadform applies, for the member's pattern (the forest's first columns)
    const long long nm = batched() ? nmember_ : S.n, nnz = batched() ? nnz_member_ : S.nnz_in;
    std::vector<unsigned char> w((size_t)nnz);
    for (long long j = 0; j < nm; j++)
        for (long long p = S.in_colptr[j]; p < S.in_colptr[j + 1]; p++) {
            const long long i = S.in_row[p];
            w[(size_t)p] = i == j ? 1 : ((S.in_use ? i > j : i < j) ? 2 : 0);
        }
    GradDev g;        // built aside: an upload that fails half-way leaves nothing behind
    dev_upload(g.zoff, off, &bytes_total);
    dev_upload(g.wgt, w, &bytes_total);
    const size_t nb = batched() ? (size_t)nbatch_ : 1;
    g.r.alloc((size_t)nm * nb, &bytes_total, kTableMinBytes);
    g.ybar.alloc(nb, &bytes_total, kTableMinBytes);
    g.bad.alloc(nb, &bytes_total, kTableMinBytes);
    grad_ = std::move(g);
}

// What a constraint adds: the work vectors u, tw, R and a zero mean (sizes of the handle alone: allocated on the first constrained
// call, kept), A by columns (the mean kernel gathers, nothing is scattered) and Bt = B' per member for the current factorisation
// (both dropped when the constraint changes: grad_drop_constraint).
void Device::grad_constraint_tables(const ConHost &A, int m, const double *d_B, int nb, long long n) {
    if (!grad_.u) {
        DevBuf<double> u, tw, R, zero;
        u.alloc((size_t)n * nb, &bytes_total, kTableMinBytes);
        tw.alloc((size_t)128 * nb, &bytes_total, kTableMinBytes);       // t and w, m <= 64 each
        R.alloc((size_t)64 * nb, &bytes_total, kTableMinBytes);
        zero.alloc((size_t)n, &bytes_total, kTableMinBytes);
        HC(hipMemset(zero, 0, (size_t)n * sizeof(double)));
        grad_.tw = std::move(tw); grad_.R = std::move(R); grad_.zero = std::move(zero); grad_.u = std::move(u);
    }
    if (!grad_.acolptr) {
        std::vector<long long> cp((size_t)n + 1, 0);
        for (int c : A.col) cp[(size_t)c + 1]++;
        for (long long j = 0; j < n; j++) cp[(size_t)j + 1] += cp[(size_t)j];
        std::vector<int> ar(A.col.size());
        std::vector<double> av(A.col.size());
        std::vector<long long> fill(cp.begin(), cp.end() - 1);
        for (int r = 0; r < A.m; r++)          // rows ascending: a column's entries are in row order
            for (long long p = A.rowptr[r]; p < A.rowptr[r + 1]; p++) {
                const long long q = fill[(size_t)A.col[p]]++;
                ar[(size_t)q] = r; av[(size_t)q] = A.val[p];
            }
        DevBuf<long long> dcp;
        DevBuf<int> dar;
        DevBuf<double> dav;
        dev_upload(dcp, cp, &bytes_total);
        dev_upload(dar, ar, &bytes_total);
        dev_upload(dav, av, &bytes_total);
        grad_.acolptr = std::move(dcp); grad_.arow = std::move(dar); grad_.aval = std::move(dav);
        grad_.bt_serial = 0;
    }
    if (grad_.bt_serial == factor_serial_) return;
    if (!grad_.Bt && !grad_.Bt.try_alloc((size_t)n * m * nb, &bytes_total)) throw std::bad_alloc();
    launch_grad_bt(stream, (int)n, m, nb, d_B, grad_.Bt);
    grad_.bt_serial = factor_serial_;
}

void Device::logpdf_grad(const RbmcSym &sym, const ConHost *A, const GradIO &io, long long *info_host) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("logpdf_grad: sharded handles are not supported");
    const Symbolic &S = *S_;
    const bool bt = batched();
    const int nb = bt ? nbatch_ : 1;
    const long long n = bt ? nmember_ : S.n, nnz = bt ? nnz_member_ : S.nnz_in;
    if (!io.d_z || !io.ybar_host) throw std::invalid_argument("logpdf_grad: z / ybar is null");
    if (n > INT_MAX || nb > 65535) throw std::invalid_argument("logpdf_grad: more than 65535 members");
    const double *d_nz = io.d_nz;
    if (io.d_mubar && !d_nz) {
        if (!nz_held_) throw std::invalid_argument("logpdf_grad: the handle does not hold Q's values (last refactorisation read a caller device buffer, or the handle is a clone): pass them");
        d_nz = d_nz_;
    }
    const int kind = con_.m > 0 ? 1 : (bcon_.m > 0 ? 2 : 0);
    const int m = kind == 1 ? con_.m : (kind == 2 ? bcon_.m : 0);
    if (m > 0 && !A) throw std::invalid_argument("logpdf_grad: the constraint's rows are missing");
    // ---- what the call ensures: the members' status, the constraint operands, the selected inverse --------------------------------
    std::vector<long long> bad((size_t)nb, 0);
    if (bt) {
        batch_diag(nullptr, bad.data());
        for (long long &b : bad) b = b != 0 ? -1 : 0;
    } else if (fail_col() >= 0) bad[0] = -1;
    if (kind == 1 && !con_prepare() && bad[0] == 0) bad[0] = 1;
    if (kind == 2) {
        bcon_prepare();
        const std::vector<long long> &ci = bcon_cinfo();
        for (int k = 0; k < nb; k++)
            if (bad[(size_t)k] == 0 && ci[(size_t)k] != 0) bad[(size_t)k] = ci[(size_t)k];
    }
    if (io.d_Qbar) selinv_compute();
    grad_tables();
    if (io.d_mubar) sym_rows_upload(sym);
    if (!bt) prepare_quadform(0);          // (the pattern of Q on the device)
    const double *d_B = kind == 1 ? con_.B.get() : bcon_.B.get(), *d_Linv = kind == 1 ? con_.Linv.get() : bcon_.Linv.get();
    if (m > 0) grad_constraint_tables(*A, m, d_B, nb, n);
    // ---- the kernels --------------------------------------------------------------------------------------------------------------
    HC(hipMemcpyAsync(grad_.ybar, io.ybar_host, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, stream));
    HC(hipMemcpyAsync(grad_.bad, bad.data(), (size_t)nb * sizeof(long long), hipMemcpyHostToDevice, stream));
    launch_grad_residual(stream, (int)n, nb, io.d_z, io.sz, io.d_mu, grad_.r);
    if (m > 0) {
        ConRows &cr = kind == 1 ? static_cast<ConRows &>(con_) : static_cast<ConRows &>(bcon_);
        con_reserve_cols(cr, 1, nb);
        // R = A mu - e by the constraint's own chunked reduction, then t, w (m x m work per member) and u = B t
        launch_con_ax(stream, cr.rowptr, cr.col, cr.val, cr.choff, cr.maxchunks, m, io.d_mu ? io.d_mu : grad_.zero.get(), n, 1, cr.part, cr.e, nullptr,
                      grad_.R, nb, io.d_mu ? n : 0);
        launch_grad_tw(stream, m, nb, d_Linv, grad_.R, grad_.tw);
        launch_grad_u(stream, (int)n, m, nb, d_B, grad_.tw, grad_.u);
    }
    if (io.d_Qbar) {
        const GradPattern a{(int)n, m, nnz, bt ? d_bin_colptr_ : d_in_colptr_, bt ? d_bin_row_ : d_in_row_, grad_.zoff, d_Z_, grad_.r, grad_.ybar,
                            m > 0 ? grad_.Bt.get() : grad_.r.get(), m > 0 ? grad_.u.get() : grad_.r.get(), grad_.bad, io.d_Qbar};
        launch_grad_pattern(stream, a, nb);
    }
    if (io.d_mubar) {
        const GradMean a{(int)n, m, nnz, sym_rows_.rp, sym_rows_.col, sym_rows_.pos, d_nz, grad_.r, grad_.ybar, m > 0 ? grad_.acolptr.get() : nullptr,
                         grad_.arow, grad_.aval, grad_.tw, grad_.bad, io.d_mubar};
        launch_grad_mubar(stream, a, nb);
    }
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    if (info_host) std::copy(bad.begin(), bad.end(), info_host);
}

void Device::pattern_dot(const double *d_G, const double *d_J, long long ldj, long long sj, long long p, double *out_host) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("pattern_dot: sharded handles are not supported");
    const bool bt = batched();
    const int nb = bt ? nbatch_ : 1;
    const long long nnz = bt ? nnz_member_ : S_->nnz_in;
    if (!d_G || !d_J || !out_host) throw std::invalid_argument("pattern_dot: G / J / out is null");
    if (p < 1 || p > 65535 || nb > 65535 || p * nb > INT_MAX) throw std::invalid_argument("pattern_dot: p must be 1 .. 65535 (and p * nbatch below 2^31)");
    if (ldj < nnz) throw std::invalid_argument("pattern_dot: ldj < nnz");
    if (nnz == 0) { std::fill(out_host, out_host + p * nb, 0.0); return; }       // (no stored entry: nothing is launched)
    grad_tables();
    const long long nchunks = choose_grad_dot(nnz, (int)p, nb).gx, need = std::max<long long>(nchunks * p * nb, 1);
    if (need > grad_.dot_cap) {
        DevBuf<double> fresh;
        fresh.alloc((size_t)need, &bytes_total);
        HC(hipDeviceSynchronize());
        grad_.dpart = std::move(fresh); grad_.dot_cap = need;
    }
    if (p * nb > grad_.out_cap) {
        DevBuf<double> fresh;
        fresh.alloc((size_t)(p * nb), &bytes_total);
        HC(hipDeviceSynchronize());
        grad_.dout = std::move(fresh); grad_.out_cap = p * nb;
    }
    launch_grad_dot(stream, nnz, grad_.wgt, d_G, d_J, ldj, sj, (int)p, nb, grad_.dpart, grad_.dout);
    HC(hipMemcpyAsync(out_host, grad_.dout, (size_t)(p * nb) * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
}

}  // namespace gmrfx
