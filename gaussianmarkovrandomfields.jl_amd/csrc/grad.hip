// grad.hip -- the array arithmetic of the log-density pullbacks, on the pattern of Q (gmrfx_logpdf_grad, gmrfx_pattern_dot). What the
// reference's rules do on the host with the whole selected inverse in hand (src/autodiff/logpdf.jl:63-90,
// src/autodiff/precision_gradient.jl, src/workspace/autodiff.jl:14-50) is done here entry by entry of pattern(Q):
//   Qbar[e] = c (Z[off[e]] - r_i r_j) - c (sum_q Bt[i, q] Bt[j, q] - u_i u_j),   e = (i, j),  c = ybar / 2,  r = z - mu
//   mubar_i = ybar (Q r)_i - ybar (A' w)_i
//   out[k]  = sum_e w_e G[e] J[e, k]
// with Z the selected-inverse panels, B = Q^-1 A' L_c^-T (constraint.hip), t = L_c^-1 (e - A mu), u = B t, w = L_c^-T t. The second
// terms exist only with a constraint (m > 0).
//   k_grad_residual  r = z - mu, packed per member (whatever stride or alignment z came with)
//   k_grad_bt        Bt = B', one contiguous row of m values per node: the dots of the pattern kernel read 8 m contiguous bytes per
//                    operand instead of m loads with stride 8 n. Made once per factorisation and constraint.
//   k_grad_tw        t and w of every member from L_c^-1 (row-major) and A mu - e: one workgroup per member
//   k_grad_u         u = B t, one thread per node (B column-major: coalesced)
//   k_grad_pattern   a lane group of kGradLanes lanes per column, kGradCols columns per workgroup; the column's row of Bt sits in LDS
//   k_grad_mubar     a lane group per row of Symmetric(Q) (the row structure RBMC uses: a gather, nothing is scattered) and per
//                    column of A (its CSC image)
//   k_grad_dot_part / k_grad_dot_final   chunks of kGradDotChunk entries, then the chunk sums
// MEMBERS. Every kernel takes a member index from its grid: member k's values at + k nnz, vectors at + k n, Bt at + k n m, J at + k sj.
// A member listed in `bad` (its factorisation or its W failed) gets NaN in its own outputs and touches nobody else's.
// DETERMINISM. No atomics. A lane adds its entries p0 + l, p0 + l + 16, ... in that order, the 16 lane sums meet in a fixed xor
// butterfly; dots over m run in ascending q; chunk sums meet in a fixed LDS tree and are added by a fixed strided loop + tree. Products
// and differences that the interface pins (c (Z - r_i r_j)) are written with contraction off.
#include <hip/hip_runtime.h>

#include "kernel_common.h"

namespace gmrfx {

__global__ __launch_bounds__(256) void k_grad_residual(int n, const double *__restrict__ z, long long sz, const double *__restrict__ mu,
                                                       double *__restrict__ r) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, mb = blockIdx.y;
    if (i < n) r[mb * n + i] = z[mb * sz + i] - (mu ? mu[mb * n + i] : 0.0);
}

// Bt[(k n + j) m + q] = B[k n m + j + q n]: 64 nodes per workgroup through LDS (reads run along j, writes along q)
__global__ __launch_bounds__(256) void k_grad_bt(int n, int m, const double *__restrict__ B, double *__restrict__ Bt) {
    __shared__ double tile[64][65];
    const long long mb = blockIdx.y, j0 = (long long)blockIdx.x * 64;
    B += mb * n * m;
    Bt += mb * n * m;
    for (int idx = threadIdx.x; idx < 64 * m; idx += 256) {
        const int jj = idx & 63, q = idx >> 6;
        if (j0 + jj < n) tile[q][jj] = B[j0 + jj + (long long)q * n];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * m; idx += 256) {
        const int jj = idx / m, q = idx - jj * m;
        if (j0 + jj < n) Bt[(j0 + jj) * m + q] = tile[q][jj];
    }
}

// tw[k 2m + l] = t_l = -(L_c^-1 R)_l, tw[k 2m + m + l] = w_l = (L_c^-T t)_l; R = A mu - e (m values per member)
__global__ __launch_bounds__(64) void k_grad_tw(int m, const double *__restrict__ Linv, const double *__restrict__ R, double *__restrict__ tw) {
    __shared__ double ts[64];
    const int mb = blockIdx.x, l = threadIdx.x;
    Linv += (long long)mb * m * m;
    R += (long long)mb * m;
    tw += (long long)mb * 2 * m;
    if (l < m) {
        double s = 0.0;
        for (int q = 0; q <= l; q++) s = __builtin_fma(Linv[l * m + q], R[q], s);
        ts[l] = -s;
        tw[l] = -s;
    }
    __syncthreads();
    if (l < m) {
        double s = 0.0;
        for (int q = l; q < m; q++) s = __builtin_fma(Linv[q * m + l], ts[q], s);
        tw[m + l] = s;
    }
}

__global__ __launch_bounds__(256) void k_grad_u(int n, int m, const double *__restrict__ B, const double *__restrict__ tw, double *__restrict__ u) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x, mb = blockIdx.y;
    if (j >= n) return;
    B += mb * n * m;
    tw += mb * 2 * m;
    double s = 0.0;
    for (int q = 0; q < m; q++) s = __builtin_fma(B[j + (long long)q * n], tw[q], s);
    u[mb * n + j] = s;
}

__global__ __launch_bounds__(256) void k_grad_pattern(const GradPattern a) {
    __shared__ double bj[256 / kGradLanes][65];      // 65: the four lane groups of a wave read their rows from different banks
    const int g = threadIdx.x / kGradLanes, l = threadIdx.x % kGradLanes, n = a.n, m = a.m;
    const long long mb = blockIdx.y;
    const bool bad = a.bad && a.bad[mb] != 0;
    const double c = 0.5 * a.ybar[mb], nan = __builtin_nan("");
    const double *r = a.r + mb * n, *u = a.u + mb * n, *Bt = a.Bt + mb * n * m;
    const long long *zoff = a.zoff + mb * a.nnz;
    double *Qbar = a.Qbar + mb * a.nnz;
    for (int t = 0; t < kGradColsPerGroup; t++) {
        const int j = blockIdx.x * kGradCols + t * (256 / kGradLanes) + g;      // neighbouring groups walk neighbouring columns
        if (m > 0) {
            __syncthreads();       // (m is uniform: every thread of the workgroup takes both barriers, kGradColsPerGroup times)
            if (j < n)
                for (int q = l; q < m; q += kGradLanes) bj[g][q] = Bt[(long long)j * m + q];
            __syncthreads();
        }
        if (j >= n) continue;
        const long long p0 = a.colptr[j], p1 = a.colptr[j + 1];
        const double rj = r[j], uj = m > 0 ? u[j] : 0.0;
        for (long long p = p0 + l; p < p1; p += kGradLanes) {
            const int i = a.row[p];
            double v;
            {
#pragma clang fp contract(off)
                v = c * (a.Z[zoff[p]] - r[i] * rj);
                if (m > 0) {
                    const double *bi = Bt + (long long)i * m;
                    double dot = 0.0;
                    for (int q = 0; q < m; q++) dot = __builtin_fma(bi[q], bj[g][q], dot);
                    v = v - c * (dot - u[i] * uj);
                }
            }
            Qbar[p] = bad ? nan : v;
        }
    }
}

__global__ __launch_bounds__(256) void k_grad_mubar(const GradMean a) {
    const int g = threadIdx.x / kGradLanes, l = threadIdx.x % kGradLanes, n = a.n;
    const long long mb = blockIdx.y;
    const int i = blockIdx.x * kGradRows + g;
    if (i >= n) return;            // (a whole lane group leaves together)
    const double *val = a.val + mb * a.nnz, *r = a.r + mb * n;
    double s = 0.0;
    for (long long q = a.rp[i] + l; q < a.rp[i + 1]; q += kGradLanes) s = __builtin_fma(val[a.pos[q]], r[a.col[q]], s);
#pragma unroll
    for (int sh = kGradLanes / 2; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, kGradLanes);
    double t = 0.0;
    if (a.acolptr) {
        const double *w = a.tw + mb * 2 * a.m + a.m;
        for (long long q = a.acolptr[i] + l; q < a.acolptr[i + 1]; q += kGradLanes) t = __builtin_fma(a.aval[q], w[a.arow[q]], t);
#pragma unroll
        for (int sh = kGradLanes / 2; sh > 0; sh >>= 1) t += __shfl_xor(t, sh, kGradLanes);
    }
    if (l == 0) {
        const double yb = a.ybar[mb];
        double v;
        {
#pragma clang fp contract(off)
            v = yb * s;
            if (a.acolptr) v = v - yb * t;
        }
        a.mubar[mb * n + i] = (a.bad && a.bad[mb] != 0) ? __builtin_nan("") : v;
    }
}

// grid (chunks, columns of J, members): part[(k p + c) nchunks + chunk]
__global__ __launch_bounds__(256) void k_grad_dot_part(long long nnz, const unsigned char *__restrict__ wgt, const double *__restrict__ G,
                                                       const double *__restrict__ J, long long ldj, long long sj, double *__restrict__ part) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const long long mb = blockIdx.z, e0 = (long long)blockIdx.x * kGradDotChunk;
    G += mb * nnz;
    J += mb * sj + (long long)blockIdx.y * ldj;
    double acc = 0.0;
    for (int t = tid; t < kGradDotChunk; t += 256) {
        const long long e = e0 + t;
        if (e < nnz) acc = __builtin_fma((double)wgt[e] * G[e], J[e], acc);
    }
    sh[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) sh[tid] += sh[tid + st];
        __syncthreads();
    }
    if (tid == 0) part[(mb * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void k_grad_dot_final(const double *__restrict__ part, int nchunks, double *__restrict__ out) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const double *p = part + (long long)blockIdx.x * nchunks;
    double acc = 0.0;
    for (int i = tid; i < nchunks; i += 256) acc += p[i];
    sh[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) sh[tid] += sh[tid + st];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = sh[0];
}

void launch_grad_residual(hipStream_t st, int n, int nb, const double *z, long long sz, const double *mu, double *r) {
    if (n <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_grad_residual, dim3((unsigned)cdiv(n, 256), (unsigned)nb), dim3(256), 0, st, n, z, sz, mu, r);
}
void launch_grad_bt(hipStream_t st, int n, int m, int nb, const double *B, double *Bt) {
    if (n <= 0 || m <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_grad_bt, dim3((unsigned)cdiv(n, 64), (unsigned)nb), dim3(256), 0, st, n, m, B, Bt);
}
void launch_grad_tw(hipStream_t st, int m, int nb, const double *Linv, const double *R, double *tw) {
    if (m <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_grad_tw, dim3((unsigned)nb), dim3(64), 0, st, m, Linv, R, tw);
}
void launch_grad_u(hipStream_t st, int n, int m, int nb, const double *B, const double *tw, double *u) {
    if (n <= 0 || m <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_grad_u, dim3((unsigned)cdiv(n, 256), (unsigned)nb), dim3(256), 0, st, n, m, B, tw, u);
}
void launch_grad_pattern(hipStream_t st, const GradPattern &a, int nb) {
    const Launch c = choose_grad_pattern(a.n, nb);
    if (c.variant == kGradPattern) GMRFX_LAUNCH(k_grad_pattern, c, st, a);
}
void launch_grad_mubar(hipStream_t st, const GradMean &a, int nb) {
    const Launch c = choose_grad_mubar(a.n, nb);
    if (c.variant == kGradMubar) GMRFX_LAUNCH(k_grad_mubar, c, st, a);
}
void launch_grad_dot(hipStream_t st, long long nnz, const unsigned char *wgt, const double *G, const double *J, long long ldj, long long sj, int p,
                     int nb, double *part, double *out) {
    const Launch c = choose_grad_dot(nnz, p, nb);
    if (c.variant != kGradDot) return;
    GMRFX_LAUNCH(k_grad_dot_part, c, st, nnz, wgt, G, J, ldj, sj, part);
    hipLaunchKernelGGL(k_grad_dot_final, dim3((unsigned)(p * nb)), dim3(256), 0, st, part, (int)c.gx, out);
}

}  // namespace gmrfx
