// rbmc.hip -- Rao-Blackwellised Monte Carlo marginal variances (gmrfx_rbmc_var; reference: src/solvers/rbmc.jl).
//
//   plain (:71-87)    out_i = 1 / D_i + Var_s( (sum_{j != i} Q_ij X_js) / D_i ),  D = diag(Q)
//   block (:124-158)  for the rows i of a block's subset S (B = S + enclosure):
//                     out_i = (Q_BB^-1)_ii + Var_s( [Q_BB^-1 Q_{B,out} X_out]_i ), written by the LAST block whose subset holds i
//
// X = P' L^-T Z are the centred samples, formed by the existing backward sweep in blocks of kRbmcW = 64 columns (one sweep
// pass) and handed to these kernels TRANSPOSED (row-major n x 64: lane s of a wave reads sample s of a row, one 512-byte
// line per row of X). A wave holds one row of the product for all 64 samples, one per lane; Var_s is a butterfly over the
// wave (the same association in every lane, a function of the lane numbers only), and the per-row state (mean, M2) of the
// sample blocks is merged with Chan's update in block order. No atomics: every sum's order depends on indices only.
//
// Block kernel: one workgroup per block, by size class (<= 32 / 64 / 128 rows: Q_BB in LDS; <= 512: global scratch, as
// k_kl_chol). The block is factored with S LAST (local row l = plan row nb - 1 - l): Q_BB = L L', so (Q_BB^-1)_SS =
// L_SS^-T L_SS^-1 and the S rows of a solve are L_SS^-T (L^-1 R)_S -- one forward substitution over the whole block, a back
// substitution over |S| rows; (Q_BB^-1)_ii = |L^-1 e_i|^2 comes from the same forward substitution on unit vectors (first
// sample block only). Substitutions are right-looking with one barrier per column, the 64 samples across the lanes, the rows
// across the four waves. A non-positive pivot (impossible for a principal block of a positive definite Q short of rounding)
// turns the block's outputs into NaN.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_common.h"

namespace gmrfx {

namespace {

constexpr int W = kRbmcW;
static_assert(W == 64, "one sample per lane of a wave");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (mean, M2) of the w live lanes of y, merged into the row's state of na earlier samples (Chan et al.); the last block writes
// out = base + M2 / (k - 1). Every lane computes the same values; lane 0 stores.
__device__ __forceinline__ void merge_row(double y, int lane, int w, long long na, bool last, long long k, double base, long long i,
                                          double *__restrict__ mean, double *__restrict__ m2, double *__restrict__ out) {
    const double v = lane < w ? y : 0.0;
    const double mb = wave_sum(v) / (double)w;
    const double d = lane < w ? y - mb : 0.0;
    const double m2b = wave_sum(d * d);
    double mn = mb, M = m2b;
    if (na > 0) {
        const double ma = mean[i], Ma = m2[i], dl = mb - ma, nt = (double)(na + w);
        mn = ma + dl * ((double)w / nt);
        M = Ma + m2b + dl * dl * ((double)na * (double)w / nt);
    }
    if (lane == 0) {
        if (last) out[i] = base + M / (double)(k - 1);
        else { mean[i] = mn; m2[i] = M; }
    }
}

}  // namespace

// Xc: column-major n x w (leading dimension n) -> Xt: row-major n x 64, zeros in the columns from w on
__global__ __launch_bounds__(256) void k_rbmc_transpose(const double *__restrict__ Xc, long long n, int w, double *__restrict__ Xt) {
    __shared__ double t[W][W + 1];
    const long long i0 = (long long)blockIdx.x * W;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c = ty; c < W; c += 4) t[c][tx] = (c < w && i0 + tx < n) ? Xc[i0 + tx + (long long)c * n] : 0.0;
    __syncthreads();
    for (int r = ty; r < W; r += 4)
        if (i0 + r < n) Xt[(i0 + r) * W + tx] = t[tx][r];
}

// one wave per row of symmetric Q
__global__ __launch_bounds__(256) void k_rbmc_plain(long long n, const long long *__restrict__ rp, const int *__restrict__ col,
                                                    const int *__restrict__ pos, const int *__restrict__ dpos,
                                                    const double *__restrict__ val, const double *__restrict__ Xt, long long na, int w,
                                                    int last, long long k, double *__restrict__ mean, double *__restrict__ m2,
                                                    double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const double D = val[dpos[i]];
    double acc = 0.0;
    for (long long p = rp[i]; p < rp[i + 1]; p++) {
        const int j = col[p];
        if (j != i) acc += val[pos[p]] * Xt[(long long)j * W + lane];
    }
    merge_row(acc / D, lane, w, na, last != 0, k, 1.0 / D, i, mean, m2, out);
}

namespace {

// forward substitution L Y = R on rows / columns j0 .. nb-1, right-looking; on return row l holds y_l L_ll (the division is left
// to the reader of the row, so nobody writes a row that others read between two barriers)
__device__ __forceinline__ void fwd_subst(const double *M, int ldm, double *R, int j0, int nb, int wave, int lane) {
    for (int j = j0; j < nb; j++) {
        const double yj = R[j * W + lane] / M[j + j * ldm];
        for (int i = j + 1 + wave; i < nb; i += 4) R[i * W + lane] -= M[i + j * ldm] * yj;
        __syncthreads();
    }
}

}  // namespace

template <int NMAX, bool M_LDS, bool R_LDS>
__global__ __launch_bounds__(256) void k_rbmc_block(RbmcDev P, const int *__restrict__ order, const double *__restrict__ val,
                                                    const double *__restrict__ Xt, long long na, int w, int first, int last, long long k,
                                                    double *__restrict__ mean, double *__restrict__ m2, double *__restrict__ base,
                                                    double *__restrict__ out, double *__restrict__ scrM, double *__restrict__ scrR) {
    extern __shared__ double smem[];
    __shared__ int bad;
    const int b = order[blockIdx.x];
    const long long r0 = P.bptr[b];
    const int nb = (int)(P.bptr[b + 1] - r0), ns = P.ns[b], s0 = nb - ns;
    double *M = M_LDS ? smem : scrM + (long long)blockIdx.x * NMAX * NMAX;
    const int ldm = M_LDS ? NMAX + 1 : nb;
    double *R = R_LDS ? smem + (M_LDS ? NMAX * (NMAX + 1) : 0) : scrR + (long long)blockIdx.x * NMAX * W;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) bad = 0;
    for (int idx = tid; idx < nb * nb; idx += 256) {
        const int i = idx % nb, j = idx / nb;
        if (i >= j) M[i + j * ldm] = 0.0;
    }
    __syncthreads();
    // Q_BB from the sparse values, through the plan's local columns
    for (int l = wave; l < nb; l += 4) {
        const long long pr = r0 + (nb - 1 - l);
        const int g = P.rows[pr];
        const long long p0 = P.rp[g], e0 = P.eptr[pr];
        const int len = (int)(P.rp[g + 1] - p0);
        for (int t = lane; t < len; t += 64) {
            const int lc = P.loc[e0 + t];
            if (lc >= 0 && lc <= l) M[l + lc * ldm] = val[P.pos[p0 + t]];
        }
    }
    __syncthreads();
    // Cholesky, right-looking, two barriers per column (as k_kl_chol): the diagonal keeps the pivots until the loop is done
    for (int j = 0; j < nb; j++) {
        const double d = M[j + j * ldm];
        if (!(d > 0.0) && tid == 0) bad = 1;
        const double inv = 1.0 / sqrt(d);
        for (int i = j + 1 + tid; i < nb; i += 256) M[i + j * ldm] *= inv;
        __syncthreads();
        const int m = nb - j - 1;
        for (int idx = tid; idx < m * m; idx += 256) {
            const int i = j + 1 + idx % m, c = j + 1 + idx / m;
            if (i >= c) M[i + c * ldm] -= M[i + j * ldm] * M[c + j * ldm];
        }
        __syncthreads();
    }
    for (int j = tid; j < nb; j += 256) M[j + j * ldm] = sqrt(M[j + j * ldm]);
    __syncthreads();
    const bool isbad = bad != 0;
    // (Q_BB^-1)_ii = |L^-1 e_i|^2 for the owned rows of S, 64 unit vectors at a time (only rows s0 .. nb-1 are touched)
    if (first) {
        for (int c0 = 0; c0 < ns; c0 += W) {
            const int mine = s0 + c0 + lane;          // this lane's unit vector
            for (int l = s0 + wave; l < nb; l += 4) R[l * W + lane] = (l == mine) ? 1.0 : 0.0;
            __syncthreads();
            fwd_subst(M, ldm, R, s0, nb, wave, lane);
            if (wave == 0 && mine < nb) {
                const long long pr = r0 + (nb - 1 - mine);
                if (P.owner[pr]) {
                    double s = 0.0;
                    for (int l = mine; l < nb; l++) {
                        const double z = R[l * W + lane] / M[l + l * ldm];
                        s += z * z;
                    }
                    base[P.rows[pr]] = isbad ? NAN : s;
                }
            }
            __syncthreads();
        }
    }
    // R = Q_{B,out} X_out: the entries of the block's rows whose column lies outside the block
    for (int l = wave; l < nb; l += 4) {
        const long long pr = r0 + (nb - 1 - l);
        const int g = P.rows[pr];
        const long long p0 = P.rp[g], e0 = P.eptr[pr];
        const int len = (int)(P.rp[g + 1] - p0);
        double acc = 0.0;
        for (int t = 0; t < len; t++)
            if (P.loc[e0 + t] < 0) acc += val[P.pos[p0 + t]] * Xt[(long long)P.col[p0 + t] * W + lane];
        R[l * W + lane] = acc;
    }
    __syncthreads();
    fwd_subst(M, ldm, R, 0, nb, wave, lane);
    // y_S, then L_SS' x = y_S from the last row up (same convention: the row keeps x_l L_ll)
    for (int l = s0 + wave; l < nb; l += 4) R[l * W + lane] /= M[l + l * ldm];
    __syncthreads();
    for (int j = nb - 1; j > s0; j--) {
        const double xj = R[j * W + lane] / M[j + j * ldm];
        for (int i = s0 + wave; i < j; i += 4) R[i * W + lane] -= M[j + i * ldm] * xj;
        __syncthreads();
    }
    for (int l = s0 + wave; l < nb; l += 4) {
        const long long pr = r0 + (nb - 1 - l);
        if (!P.owner[pr]) continue;
        const long long g = P.rows[pr];
        const double x = isbad ? NAN : R[l * W + lane] / M[l + l * ldm];
        merge_row(x, lane, w, na, last != 0, k, last ? base[g] : 0.0, g, mean, m2, out);
    }
}

void launch_rbmc_transpose(hipStream_t st, const double *Xc, long long n, int w, double *Xt) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rbmc_transpose, dim3((unsigned)((n + W - 1) / W)), dim3(256), 0, st, Xc, n, w, Xt);
}

void launch_rbmc_plain(hipStream_t st, const RbmcDev &P, long long n, const double *val, const double *Xt, long long na, int w, bool last,
                       long long k, double *mean, double *m2, double *out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rbmc_plain, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, P.rp, P.col, P.pos, P.dpos, val, Xt, na, w, last ? 1 : 0, k,
                       mean, m2, out);
}

namespace {
template <int NMAX, bool M_LDS, bool R_LDS>
void launch_block_class(hipStream_t st, const RbmcDev &P, const int *order, int cnt, const double *val, const double *Xt, long long na, int w,
                        bool first, bool last, long long k, double *mean, double *m2, double *base, double *out, double *scrM, double *scrR) {
    const size_t lds = ((M_LDS ? (size_t)NMAX * (NMAX + 1) : 0) + (R_LDS ? (size_t)NMAX * W : 0)) * sizeof(double);
    if (lds > 48 * 1024)
        hip_check(hipFuncSetAttribute((const void *)k_rbmc_block<NMAX, M_LDS, R_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                  "hipFuncSetAttribute");
    hipLaunchKernelGGL((k_rbmc_block<NMAX, M_LDS, R_LDS>), dim3(cnt), dim3(256), lds, st, P, order, val, Xt, na, w, first ? 1 : 0, last ? 1 : 0, k,
                       mean, m2, base, out, scrM, scrR);
}
}  // namespace

// one size class: cnt blocks of `order`, at most rbmc_class_chunk(cls) per launch (the scratch is indexed by workgroup)
void launch_rbmc_blocks(hipStream_t st, const RbmcDev &P, int cls, const int *order, int cnt, const double *val, const double *Xt, long long na,
                        int w, bool first, bool last, long long k, double *mean, double *m2, double *base, double *out, double *scrM,
                        double *scrR) {
    const int chunk = rbmc_class_chunk(cls);
    for (int b0 = 0; b0 < cnt; b0 += chunk) {
        const int c = cnt - b0 < chunk ? cnt - b0 : chunk;
        if (cls == 0) launch_block_class<32, true, true>(st, P, order + b0, c, val, Xt, na, w, first, last, k, mean, m2, base, out, scrM, scrR);
        else if (cls == 1) launch_block_class<64, true, true>(st, P, order + b0, c, val, Xt, na, w, first, last, k, mean, m2, base, out, scrM, scrR);
        else if (cls == 2) launch_block_class<128, true, false>(st, P, order + b0, c, val, Xt, na, w, first, last, k, mean, m2, base, out, scrM, scrR);
        else launch_block_class<512, false, false>(st, P, order + b0, c, val, Xt, na, w, first, last, k, mean, m2, base, out, scrM, scrR);
    }
}

}  // namespace gmrfx
