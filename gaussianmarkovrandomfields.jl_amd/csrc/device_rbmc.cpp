// device_rbmc.cpp -- the Device's side of the Rao-Blackwellised Monte Carlo marginal variances (include/gmrfx.h: gmrfx_rbmc_var;
// kernels in rbmc.hip, host analysis in rbmc_plan.cpp). What the reference does on the host (src/solvers/rbmc.jl: k single-vector
// rand! calls, a host SpMM, one CHOLMOD factorisation per block) runs here per block of kRbmcW samples:
//   Xc = P' L^-T Z[:, j0 : j0 + w]      the existing backward sweep, one pass
//   Xt = Xc'                            row-major n x kRbmcW, what the estimator kernels read
//   plain: one wave per row of symmetric Q;  block: one workgroup per block of the plan, by size class
// with the rows' (mean, M2) merged block by block in HBM and the variances written by the last block.
#include <algorithm>
#include <climits>
#include <stdexcept>

#include "device.h"
#include "kernels.h"

namespace gmrfx {

#define HC(x) hip_check((x), #x)

template <class T, class U> static T *rb_up(void *dst, const std::vector<U> &src) {
    std::vector<T> tmp(src.begin(), src.end());
    if (!tmp.empty()) HC(hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice));
    return (T *)dst;
}

void Device::rbmc_upload_sym(const RbmcSym &sym) {
    if (rb_.rp) return;
    const long long n = S_->n;
    if (S_->nnz_in > INT_MAX || (long long)sym.col.size() > (1ll << 40)) throw std::invalid_argument("rbmc: Q has too many stored entries for 32-bit positions");
    long long *rp = (long long *)con_alloc((size_t)(n + 1) * sizeof(long long));
    rb_.col = rb_up<int>(con_alloc(sym.col.size() * sizeof(int)), sym.col);
    rb_.pos = rb_up<int>(con_alloc(sym.pos.size() * sizeof(int)), sym.pos);
    rb_.dpos = rb_up<int>(con_alloc((size_t)n * sizeof(int)), sym.diag);
    rb_.Xc = (double *)con_alloc((size_t)n * kRbmcW * sizeof(double));
    rb_.Xt = (double *)con_alloc((size_t)n * kRbmcW * sizeof(double));
    rb_.mean = (double *)con_alloc((size_t)n * sizeof(double));
    rb_.m2 = (double *)con_alloc((size_t)n * sizeof(double));
    rb_.base = (double *)con_alloc((size_t)n * sizeof(double));
    rb_.out = (double *)con_alloc((size_t)n * sizeof(double));
    if (!rb_.ev0) HC(hipEventCreate(&rb_.ev0));
    if (!rb_.ev1) HC(hipEventCreate(&rb_.ev1));
    rb_.rp = rb_up<long long>(rp, sym.rowptr);       // set last: marks the upload complete
}

void Device::rbmc_upload_plan(const RbmcPlan &plan) {
    if (rb_.plan_serial == plan.serial && rb_.plan_enclosure == plan.enclosure) return;
    HC(hipDeviceSynchronize());        // nothing in flight may still read the old tables
    for (void *p : {(void *)rb_.bptr, (void *)rb_.eptr, (void *)rb_.rows, (void *)rb_.ns, (void *)rb_.loc, (void *)rb_.owner, (void *)rb_.scrM,
                    (void *)rb_.scrR, (void *)rb_.order[0], (void *)rb_.order[1], (void *)rb_.order[2], (void *)rb_.order[3]})
        con_release(p);
    rb_.bptr = rb_.eptr = nullptr; rb_.rows = rb_.ns = rb_.loc = nullptr; rb_.owner = nullptr; rb_.scrM = rb_.scrR = nullptr;
    for (int c = 0; c < kRbmcClasses; c++) { rb_.order[c] = nullptr; rb_.cnt[c] = 0; }
    rb_.plan_enclosure = -2; rb_.plan_serial = 0;
    if (plan.loc.size() > (size_t)1 << 40) throw std::invalid_argument("rbmc: plan too large");
    rb_.bptr = rb_up<long long>(con_alloc(plan.block_ptr.size() * sizeof(long long)), plan.block_ptr);
    rb_.eptr = rb_up<long long>(con_alloc(plan.eptr.size() * sizeof(long long)), plan.eptr);
    rb_.rows = rb_up<int>(con_alloc(plan.rows.size() * sizeof(int)), plan.rows);
    rb_.ns = rb_up<int>(con_alloc(plan.n_interior.size() * sizeof(int)), plan.n_interior);
    rb_.loc = rb_up<int>(con_alloc(plan.loc.size() * sizeof(int)), plan.loc);
    rb_.owner = rb_up<unsigned char>(con_alloc(plan.owner.size()), plan.owner);
    for (int c = 0; c < kRbmcClasses; c++) {
        rb_.cnt[c] = (int)plan.order[c].size();
        if (rb_.cnt[c]) rb_.order[c] = rb_up<int>(con_alloc(plan.order[c].size() * sizeof(int)), plan.order[c]);
    }
    // global scratch of the two large classes, by workgroup of a launch: Q_BB (512 x 512) and R (rows x kRbmcW)
    const size_t wg3 = (size_t)std::min(rb_.cnt[3], rbmc_class_chunk(3)), wg2 = (size_t)std::min(rb_.cnt[2], rbmc_class_chunk(2));
    if (wg3) rb_.scrM = (double *)con_alloc(wg3 * kRbmcMaxBlock * kRbmcMaxBlock * sizeof(double));
    const size_t rdoubles = std::max(wg3 * kRbmcMaxBlock * kRbmcW, wg2 * 128 * kRbmcW);
    if (rdoubles) rb_.scrR = (double *)con_alloc(rdoubles * sizeof(double));
    rb_.plan_enclosure = plan.enclosure; rb_.plan_serial = plan.serial;
}

void Device::rbmc_var(const RbmcSym &sym, const RbmcPlan *plan, const double *d_nz, const double *Z, long long ldz, bool z_on_device, long long k,
                      double *out, bool out_on_device) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("rbmc_var: sharded handles are not supported");
    const long long n = S_->n;
    if (k < 2) throw std::invalid_argument("rbmc_var: nsamples < 2");
    if (ldz < n) throw std::invalid_argument("rbmc_var: ldz < n");
    if (!d_nz) {
        if (!nz_held_) throw std::invalid_argument("rbmc_var: the handle does not hold Q's values (last refactorisation read a caller device buffer, or the handle is a clone): pass them");
        d_nz = d_nz_;
    }
    rbmc_upload_sym(sym);
    if (plan) rbmc_upload_plan(*plan);
    const RbmcDev P{rb_.rp, rb_.col, rb_.pos, rb_.dpos, rb_.bptr, rb_.rows, rb_.ns, rb_.owner, rb_.eptr, rb_.loc};
    double *d_out = out_on_device ? out : rb_.out;
    double bs = 0;
    HC(hipEventRecord(rb_.ev0, stream));
    for (long long j0 = 0; j0 < k; j0 += kRbmcW) {
        const int w = (int)std::min<long long>(kRbmcW, k - j0);
        const bool first = j0 == 0, last = j0 + w == k;
        if (z_on_device) solve(Z + j0 * ldz, ldz, w, rb_.Xc, n, true, 1);
        else {
            HC(hipMemcpy2DAsync(rb_.Xc, (size_t)n * sizeof(double), Z + j0 * ldz, (size_t)ldz * sizeof(double), (size_t)n * sizeof(double), (size_t)w,
                                hipMemcpyHostToDevice, stream));
            solve(rb_.Xc, n, w, rb_.Xc, n, true, 1);
        }
        bs += ms_bsolve;
        launch_rbmc_transpose(stream, rb_.Xc, n, w, rb_.Xt);
        if (!plan) launch_rbmc_plain(stream, P, n, d_nz, rb_.Xt, j0, w, last, k, rb_.mean, rb_.m2, d_out);
        else
            for (int c = 0; c < kRbmcClasses; c++)
                if (rb_.cnt[c])
                    launch_rbmc_blocks(stream, P, c, rb_.order[c], rb_.cnt[c], d_nz, rb_.Xt, j0, w, first, last, k, rb_.mean, rb_.m2, rb_.base, d_out,
                                       rb_.scrM, rb_.scrR);
        HC(hipGetLastError());
    }
    HC(hipEventRecord(rb_.ev1, stream));
    if (!out_on_device) HC(hipMemcpyAsync(out, rb_.out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms = 0;
    HC(hipEventElapsedTime(&ms, rb_.ev0, rb_.ev1));
    ms_rbmc = ms; ms_rbmc_bsolve = bs;
}

}  // namespace gmrfx
