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

void Device::sym_rows_upload(const RbmcSym &sym) {
    if (sym_rows_.rp) return;
    if (S_->nnz_in > INT_MAX || (long long)sym.col.size() > (1ll << 40)) throw std::invalid_argument("rbmc: Q has too many stored entries for 32-bit positions");
    SymRowsDev d;        // built aside: an upload that fails half-way leaves nothing behind
    dev_upload(d.rp, sym.rowptr, &bytes_total);      // n + 1
    dev_upload(d.col, sym.col, &bytes_total);
    dev_upload(d.pos, std::vector<int>(sym.pos.begin(), sym.pos.end()), &bytes_total);        // (32-bit positions: checked above)
    dev_upload(d.dpos, std::vector<int>(sym.diag.begin(), sym.diag.end()), &bytes_total);     // n
    sym_rows_ = std::move(d);
}

void Device::rbmc_upload_sym(const RbmcSym &sym) {
    sym_rows_upload(sym);
    if (rb_.sym.Xc) return;
    const size_t n = (size_t)S_->n;
    RbmcSymDev d;
    d.Xc.alloc(n * kRbmcW, &bytes_total, kTableMinBytes);
    d.Xt.alloc(n * kRbmcW, &bytes_total, kTableMinBytes);
    d.mean.alloc(n, &bytes_total, kTableMinBytes);
    d.m2.alloc(n, &bytes_total, kTableMinBytes);
    d.base.alloc(n, &bytes_total, kTableMinBytes);
    d.out.alloc(n, &bytes_total, kTableMinBytes);
    for (Event &e : rb_ev_) e.ensure();
    rb_.sym = std::move(d);
}

void Device::rbmc_upload_plan(const RbmcPlan &plan) {
    if (rb_.plan.serial == plan.serial && rb_.plan.enclosure == plan.enclosure) return;
    HC(hipDeviceSynchronize());        // nothing in flight may still read the old tables
    rb_.plan = RbmcPlanDev();
    if (plan.loc.size() > (size_t)1 << 40) throw std::invalid_argument("rbmc: plan too large");
    RbmcPlanDev d;
    dev_upload(d.bptr, plan.block_ptr, &bytes_total);
    dev_upload(d.eptr, plan.eptr, &bytes_total);
    dev_upload(d.rows, plan.rows, &bytes_total);
    dev_upload(d.ns, plan.n_interior, &bytes_total);
    dev_upload(d.loc, plan.loc, &bytes_total);
    dev_upload(d.owner, plan.owner, &bytes_total);
    for (int c = 0; c < kRbmcClasses; c++) {
        d.cnt[c] = (int)plan.order[c].size();
        if (d.cnt[c]) dev_upload(d.order[c], plan.order[c], &bytes_total);
    }
    // global scratch of the two large classes, by workgroup of a launch: Q_BB (512 x 512) and R (rows x kRbmcW)
    const size_t wg3 = (size_t)std::min(d.cnt[3], rbmc_class_chunk(3)), wg2 = (size_t)std::min(d.cnt[2], rbmc_class_chunk(2));
    if (wg3) d.scrM.alloc(wg3 * kRbmcMaxBlock * kRbmcMaxBlock, &bytes_total, kTableMinBytes);
    const size_t rdoubles = std::max(wg3 * kRbmcMaxBlock * kRbmcW, wg2 * 128 * kRbmcW);
    if (rdoubles) d.scrR.alloc(rdoubles, &bytes_total, kTableMinBytes);
    d.enclosure = plan.enclosure; d.serial = plan.serial;
    rb_.plan = std::move(d);
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
    const RbmcSymDev &sy = rb_.sym;
    const RbmcPlanDev &pl = rb_.plan;
    const RbmcDev P{sym_rows_.rp, sym_rows_.col, sym_rows_.pos, sym_rows_.dpos, pl.bptr, pl.rows, pl.ns, pl.owner, pl.eptr, pl.loc};
    double *d_out = out_on_device ? out : sy.out;
    double bs = 0;
    HC(hipEventRecord(rb_ev_[0], stream));
    for (long long j0 = 0; j0 < k; j0 += kRbmcW) {
        const int w = (int)std::min<long long>(kRbmcW, k - j0);
        const bool first = j0 == 0, last = j0 + w == k;
        if (z_on_device) solve(Z + j0 * ldz, ldz, w, sy.Xc, n, true, 1);
        else {
            HC(hipMemcpy2DAsync(sy.Xc, (size_t)n * sizeof(double), Z + j0 * ldz, (size_t)ldz * sizeof(double), (size_t)n * sizeof(double), (size_t)w,
                                hipMemcpyHostToDevice, stream));
            solve(sy.Xc, n, w, sy.Xc, n, true, 1);
        }
        bs += ms_bsolve;
        launch_rbmc_transpose(stream, sy.Xc, n, w, sy.Xt);
        if (!plan) launch_rbmc_plain(stream, P, n, d_nz, sy.Xt, j0, w, last, k, sy.mean, sy.m2, d_out);
        else
            for (int c = 0; c < kRbmcClasses; c++)
                if (pl.cnt[c])
                    launch_rbmc_blocks(stream, P, c, pl.order[c], pl.cnt[c], d_nz, sy.Xt, j0, w, first, last, k, sy.mean, sy.m2, sy.base, d_out,
                                       pl.scrM, pl.scrR);
        HC(hipGetLastError());
    }
    HC(hipEventRecord(rb_ev_[1], stream));
    if (!out_on_device) HC(hipMemcpyAsync(out, sy.out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms = 0;
    HC(hipEventElapsedTime(&ms, rb_ev_[0], rb_ev_[1]));
    ms_rbmc = ms; ms_rbmc_bsolve = bs;
}

}  // namespace gmrfx
