// ga_pullback.hip -- the array arithmetic of the pullback of gaussian_approximation (gmrfx_ga_pullback): the implicit-function rule of
// the reference (src/workspace/autodiff.jl:140-202; src/autodiff/gaussian_approximation.jl:278-347), which it forms on the host with
// dense intermediates. With G the cotangent of the posterior precision on Q's pattern, mubar that of the mode, r = x - mu:
//   c_i   = a_i' G a_i                      node form: G[position of (i, i)]; design form: sum over the pairs of row i of A
//   t_i   = c_i d3_i(eta_i)                 d3 = dd/deta (fisher_point.h)
//   xbar  = mubar - A' t
//   lam   = Q_post^-1 xbar                  the handle's own solve (and the constraint's correction): no kernel of this file
//   Qbar_prior[e = (i, j)] = G[e] - 0.5 (lam_i r_j + lam_j r_i)
//   mubar_prior = Q_p lam
//   out[0] = sum_i (A lam)_i gp_i - sum_i c_i dp_i        gp, dp: the derivatives of g and d by sigma / r / phi
//   k_gap_point_node   one thread per node: c, t, xbar and the partial of sum c dp
//   k_gap_point        a lane group per row of A: eta as k_design_eta forms it, c over the row's transposed term list, t, the partial
//   k_gap_chunks       one workgroup per chunk of a long column of A: sum A_ij t_i
//   k_gap_gather       a lane group per node: xbar_j = mubar_j - sum_i A_ij t_i (short column: entry by entry; long: its chunk sums)
//   k_gap_pattern      a lane group per column of the pattern
//   k_gap_mean         a lane group per row of Symmetric(Q_p)
//   k_gap_param_node / k_gap_param   (A lam)_i gp_i (eta_i formed again in the same pass) and its partial per workgroup;  k_gap_final   the two sums
// DETERMINISM. No atomics. A lane adds entries q0 + l, q0 + l + 16, ... in that order, the 16 lane sums meet in a fixed xor butterfly;
// a chunk's thread adds entries t, t + 256 and the 256 sums meet in a fixed LDS tree; workgroup partials are added by a fixed strided
// loop and tree. Every operand is read and written one double at a time: nothing depends on alignment. Contraction is off in the
// whole file; every fused multiply-add is written as one.
// SELECTION MATRICES. With A = rows of the identity and no offset every sum has one term of weight 1: eta, t and xbar have the bits
// of the node form, and so has everything behind the solve.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "fisher_point.h"

namespace gmrfx {

#pragma clang fp contract(off)

__device__ __forceinline__ double gap_group_sum(double s) {
#pragma unroll
    for (int sh = kDesignLanes / 2; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, kDesignLanes);
    return s;
}

// the workgroup's sum of one value per thread (cnt of them, a power of two, in sh), by thread 0 into *dst
__device__ __forceinline__ void gap_block_sum(double *sh, int cnt, double *dst) {
    __syncthreads();
    for (int st = cnt / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = sh[0];
}

__global__ __launch_bounds__(kGapNode) void k_gap_point_node(const GapPoint a) {
    __shared__ double sp[kGapNode];
    const long long i = (long long)blockIdx.x * kGapNode + threadIdx.x;
    double p = 0.0;
    if (i < a.n) {
        double t = 0.0;
        if (a.mask[i]) {
            const double c = a.G[a.hmap[i]];
            double d3, gp, dp;
            fisher_point_pullback(a.family, a.x[i], a.y[i], a.aux ? a.aux[i] : 0.0, a.param, a.logparam, d3, gp, dp);
            t = c * d3;
            p = c * dp;
        }
        a.xbar[i] = (a.mubar ? a.mubar[i] : 0.0) - t;
    }
    sp[threadIdx.x] = p;
    gap_block_sum(sp, kGapNode, a.ppart + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_gap_point(const GapPoint a) {
    __shared__ double sp[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double p = 0.0;
    if (i < a.nobs) {           // (a whole lane group takes the branch together)
        double s = 0.0, c = 0.0;
        const long long q1 = a.arp[i + 1], o1 = a.optr[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], a.x[a.acol[q]], s);
        for (long long q = a.optr[i] + l; q < o1; q += kDesignLanes) c = __builtin_fma(a.ow[q], a.G[a.hmap[a.oidx[q]]], c);
        s = gap_group_sum(s);
        c = gap_group_sum(c);
        if (l == 0) {
            const double eta = a.offset ? s + a.offset[i] : s;
            double d3, gp, dp;
            fisher_point_pullback(a.family, eta, a.y[i], a.aux ? a.aux[i] : 0.0, a.param, a.logparam, d3, gp, dp);
            a.t[i] = c * d3;
            p = c * dp;
        }
    }
    if (l == 0) sp[g] = p;
    gap_block_sum(sp, kDesignRows, a.ppart + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_gap_chunks(const GapGather a) {
    __shared__ double sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long p0 = a.chs[b];
    const int len = a.chl[b];
    double s = 0.0;
    for (int t = tid; t < len; t += 256) s = __builtin_fma(a.acv[p0 + t], a.t[a.arow[p0 + t]], s);
    sh[tid] = s;
    gap_block_sum(sh, 256, a.cpart + b);
}

__global__ __launch_bounds__(256) void k_gap_gather(const GapGather a) {
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long j = (long long)blockIdx.x * kDesignRows + g;
    if (j >= a.n) return;       // (a whole lane group leaves together)
    const long long p0 = a.acp[j], p1 = a.acp[j + 1];
    double s = 0.0;
    if (p1 - p0 <= kDesignChunk)
        for (long long q = p0 + l; q < p1; q += kDesignLanes) s = __builtin_fma(a.acv[q], a.t[a.arow[q]], s);
    else
        for (int c = a.cchoff[j] + l; c < a.cchoff[j + 1]; c += kDesignLanes) s += a.cpart[c];
    s = gap_group_sum(s);
    if (l == 0) a.xbar[j] = (a.mubar ? a.mubar[j] : 0.0) - s;
}

__global__ __launch_bounds__(256) void k_gap_pattern(const GapPattern a) {
    const int g = threadIdx.x / kGradLanes, l = threadIdx.x % kGradLanes, n = a.n;
    for (int t = 0; t < kGradColsPerGroup; t++) {
        const long long j = (long long)blockIdx.x * kGradCols + t * (256 / kGradLanes) + g;      // neighbouring groups walk neighbouring columns
        if (j >= n) continue;
        const double lj = a.lam[j], rj = a.x[j] - (a.mu ? a.mu[j] : 0.0);
        const long long p1 = a.colptr[j + 1];
        for (long long p = a.colptr[j] + l; p < p1; p += kGradLanes) {
            const int i = a.row[p];
            const double ri = a.x[i] - (a.mu ? a.mu[i] : 0.0);
            a.out[p] = (a.G ? a.G[p] : 0.0) - 0.5 * (a.lam[i] * rj + lj * ri);
        }
    }
}

__global__ __launch_bounds__(256) void k_gap_mean(int n, const long long *__restrict__ rp, const int *__restrict__ col, const int *__restrict__ pos,
                                                  const double *__restrict__ val, const double *__restrict__ lam, double *__restrict__ out) {
    const int g = threadIdx.x / kGradLanes, l = threadIdx.x % kGradLanes;
    const long long i = (long long)blockIdx.x * kGradRows + g;
    if (i >= n) return;         // (a whole lane group leaves together)
    double s = 0.0;
    const long long q1 = rp[i + 1];
    for (long long q = rp[i] + l; q < q1; q += kGradLanes) s = __builtin_fma(val[pos[q]], lam[col[q]], s);
#pragma unroll
    for (int sh = kGradLanes / 2; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, kGradLanes);
    if (l == 0) out[i] = s;
}

__global__ __launch_bounds__(kGapNode) void k_gap_param_node(const GapParam a) {
    __shared__ double sp[kGapNode];
    const long long i = (long long)blockIdx.x * kGapNode + threadIdx.x;
    double p = 0.0;
    if (i < a.n && a.mask[i]) {
        double d3, gp, dp;
        fisher_point_pullback(a.family, a.x[i], a.y[i], a.aux ? a.aux[i] : 0.0, a.param, a.logparam, d3, gp, dp);
        p = a.lam[i] * gp;
    }
    sp[threadIdx.x] = p;
    gap_block_sum(sp, kGapNode, a.gpart + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_gap_param(const GapParam a) {
    __shared__ double sp[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double p = 0.0;
    if (i < a.nobs) {
        double s = 0.0, e = 0.0;
        const long long q1 = a.arp[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) {
            const int k = a.acol[q];
            e = __builtin_fma(a.aval[q], a.x[k], e);
            s = __builtin_fma(a.aval[q], a.lam[k], s);
        }
        e = gap_group_sum(e);
        s = gap_group_sum(s);
        if (l == 0) {
            const double eta = a.offset ? e + a.offset[i] : e;
            double d3, gp, dp;
            fisher_point_pullback(a.family, eta, a.y[i], a.aux ? a.aux[i] : 0.0, a.param, a.logparam, d3, gp, dp);
            p = s * gp;
        }
    }
    if (l == 0) sp[g] = p;
    gap_block_sum(sp, kDesignRows, a.gpart + blockIdx.x);
}

__global__ __launch_bounds__(kFisherFinal) void k_gap_final(const double *__restrict__ gpart, int ng, const double *__restrict__ ppart, int np,
                                                            double *__restrict__ out) {
    __shared__ double sg[kFisherFinal], sp[kFisherFinal];
    const int tid = threadIdx.x;
    double g = 0.0, p = 0.0;
    for (int b = tid; b < ng; b += kFisherFinal) g += gpart[b];
    for (int b = tid; b < np; b += kFisherFinal) p += ppart[b];
    sg[tid] = g; sp[tid] = p;
    __syncthreads();
    for (int st = kFisherFinal / 2; st > 0; st >>= 1) {
        if (tid < st) { sg[tid] += sg[tid + st]; sp[tid] += sp[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) out[0] = sg[0] - sp[0];
}

void launch_gap_point(hipStream_t st, const GapPoint &a, bool design) {
    if (a.n <= 0 || a.nobs <= 0) return;
    const unsigned nb = (unsigned)gap_obs_blocks(design, a.n, a.nobs);
    if (design) hipLaunchKernelGGL(k_gap_point, dim3(nb), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_gap_point_node, dim3(nb), dim3(kGapNode), 0, st, a);
}
void launch_gap_gather(hipStream_t st, const GapGather &a) {
    if (a.n <= 0) return;
    if (a.ncc > 0) hipLaunchKernelGGL(k_gap_chunks, dim3((unsigned)a.ncc), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_gap_gather, dim3((unsigned)design_blocks(a.n)), dim3(256), 0, st, a);
}
void launch_gap_pattern(hipStream_t st, const GapPattern &a) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_gap_pattern, dim3((unsigned)cdiv(a.n, kGradCols)), dim3(256), 0, st, a);
}
void launch_gap_mean(hipStream_t st, int n, const long long *rp, const int *col, const int *pos, const double *val, const double *lam, double *out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_gap_mean, dim3((unsigned)cdiv(n, kGradRows)), dim3(256), 0, st, n, rp, col, pos, val, lam, out);
}
void launch_gap_param(hipStream_t st, const GapParam &a, bool design) {
    if (a.n <= 0 || a.nobs <= 0) return;
    const unsigned nb = (unsigned)gap_obs_blocks(design, a.n, a.nobs);
    if (design) hipLaunchKernelGGL(k_gap_param, dim3(nb), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_gap_param_node, dim3(nb), dim3(kGapNode), 0, st, a);
}
void launch_gap_final(hipStream_t st, const double *gpart, int ng, const double *ppart, int np, double *out) {
    hipLaunchKernelGGL(k_gap_final, dim3(1), dim3(kFisherFinal), 0, st, gpart, ng, ppart, np, out);
}

}  // namespace gmrfx
