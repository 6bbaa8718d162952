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
//   k_gap_point_comp / k_gap_param_comp / k_gap_final_comp   a composite likelihood (gmrfx_ga_pullback_composite): out[c] per component;
//                      the observations tiled per component (kernels.h: GapTiles), family and parameter from the component table
// DETERMINISM. No atomics. A lane adds entries q0 + l, q0 + l + 16, ... in that order, the 16 lane sums meet in a fixed xor butterfly;
// a chunk's thread adds entries t, t + 256 and the 256 sums meet in a fixed LDS tree; workgroup partials are added by a fixed strided
// loop and tree. Every operand is read and written one double at a time: nothing depends on alignment. Contraction is off in the
// whole file; every fused multiply-add is written as one.
// MEMBERS (batched handles, gmrfx_batch_ga_pullback). Every kernel takes a member index from its grid (blockIdx.y; blockIdx.x in
// k_gap_final) and member strides: ONE copy of A by rows and columns, the chunk tables, the transposed term table, the data set (y, aux,
// offset, mask), the member's pattern, its symmetric rows and its slice of the Hessian map; member k's G and Qbar_prior at + k sg, its
// point at + k sx, its mean at + k smu (0: one mean), its cotangents, work vectors and outputs at their own strides, t at + k nobs, its
// chunk sums at + k sc, its partial sums at + k gap_obs_blocks(...), its result at out[k]. A per-member scalar is the by-value argument
// unless its device array is non-null. A workgroup never spans two members and a member's sums are formed in the order above whatever
// the other members hold: member k's results have the bits of a plain handle of Q_p,k and param[k]. A plain handle is one member, grid
// (blocks, 1), strides 0, scalars by value. INACTIVE MEMBERS (active non-null and active[k] == 0): every workgroup of the member returns
// on its first statement, uniform over the workgroup and ahead of every barrier and load; nothing of the member is written.
// k_gap_copy carries a vector of every active member (or NaN into those of the inactive ones: the slices of a member whose factor failed).
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
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sp[kGapNode];
    const long long i = (long long)blockIdx.x * kGapNode + threadIdx.x;
    double p = 0.0;
    if (i < a.n) {
        double t = 0.0;
        if (a.mask[i]) {
            const double c = a.G[(long long)k * a.sg + a.hmap[i]];
            double d3, gp, dp;
            fisher_point_pullback(a.family, a.x[(long long)k * a.sx + i], a.y[i], a.aux ? a.aux[i] : 0.0, a.param_k ? a.param_k[k] : a.param,
                                  a.logparam_k ? a.logparam_k[k] : a.logparam, d3, gp, dp);
            t = c * d3;
            p = c * dp;
        }
        a.xbar[(long long)k * a.sw + i] = (a.mubar ? a.mubar[(long long)k * a.sm + i] : 0.0) - t;
    }
    sp[threadIdx.x] = p;
    gap_block_sum(sp, kGapNode, a.ppart + ((long long)k * gridDim.x + blockIdx.x));
}

__global__ __launch_bounds__(256) void k_gap_point(const GapPoint a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sp[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double p = 0.0;
    if (i < a.nobs) {           // (a whole lane group takes the branch together)
        const double *x = a.x + (long long)k * a.sx, *G = a.G + (long long)k * a.sg;
        double s = 0.0, c = 0.0;
        const long long q1 = a.arp[i + 1], o1 = a.optr[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], x[a.acol[q]], s);
        for (long long q = a.optr[i] + l; q < o1; q += kDesignLanes) c = __builtin_fma(a.ow[q], G[a.hmap[a.oidx[q]]], c);
        s = gap_group_sum(s);
        c = gap_group_sum(c);
        if (l == 0) {
            const double eta = a.offset ? s + a.offset[i] : s;
            double d3, gp, dp;
            fisher_point_pullback(a.family, eta, a.y[i], a.aux ? a.aux[i] : 0.0, a.param_k ? a.param_k[k] : a.param,
                                  a.logparam_k ? a.logparam_k[k] : a.logparam, d3, gp, dp);
            a.t[(long long)k * a.nobs + i] = c * d3;
            p = c * dp;
        }
    }
    if (l == 0) sp[g] = p;
    gap_block_sum(sp, kDesignRows, a.ppart + ((long long)k * gridDim.x + blockIdx.x));
}

__global__ __launch_bounds__(256) void k_gap_chunks(const GapGather a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *t_k = a.t + (long long)k * a.st;
    const long long p0 = a.chs[b];
    const int len = a.chl[b];
    double s = 0.0;
    for (int t = tid; t < len; t += 256) s = __builtin_fma(a.acv[p0 + t], t_k[a.arow[p0 + t]], s);
    sh[tid] = s;
    gap_block_sum(sh, 256, a.cpart + ((long long)k * a.sc + b));
}

__global__ __launch_bounds__(256) void k_gap_gather(const GapGather a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long j = (long long)blockIdx.x * kDesignRows + g;
    if (j >= a.n) return;       // (a whole lane group leaves together)
    const double *t_k = a.t + (long long)k * a.st, *cpart = a.cpart + (long long)k * a.sc;
    const long long p0 = a.acp[j], p1 = a.acp[j + 1];
    double s = 0.0;
    if (p1 - p0 <= kDesignChunk)
        for (long long q = p0 + l; q < p1; q += kDesignLanes) s = __builtin_fma(a.acv[q], t_k[a.arow[q]], s);
    else
        for (int c = a.cchoff[j] + l; c < a.cchoff[j + 1]; c += kDesignLanes) s += cpart[c];
    s = gap_group_sum(s);
    if (l == 0) a.xbar[(long long)k * a.sw + j] = (a.mubar ? a.mubar[(long long)k * a.sm + j] : 0.0) - s;
}

__global__ __launch_bounds__(256) void k_gap_pattern(const GapPattern a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    const int g = threadIdx.x / kGradLanes, l = threadIdx.x % kGradLanes, n = a.n;
    const double *lam = a.lam + (long long)k * a.sw, *x = a.x + (long long)k * a.sx;
    const double *mu = a.mu ? a.mu + (long long)k * a.smu : nullptr, *G = a.G ? a.G + (long long)k * a.sg : nullptr;
    double *out = a.out + (long long)k * a.sg;
    for (int t = 0; t < kGradColsPerGroup; t++) {
        const long long j = (long long)blockIdx.x * kGradCols + t * (256 / kGradLanes) + g;      // neighbouring groups walk neighbouring columns
        if (j >= n) continue;
        const double lj = lam[j], rj = x[j] - (mu ? mu[j] : 0.0);
        const long long p1 = a.colptr[j + 1];
        for (long long p = a.colptr[j] + l; p < p1; p += kGradLanes) {
            const int i = a.row[p];
            const double ri = x[i] - (mu ? mu[i] : 0.0);
            out[p] = (G ? G[p] : 0.0) - 0.5 * (lam[i] * rj + lj * ri);
        }
    }
}

__global__ __launch_bounds__(256) void k_gap_mean(const GapMean a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    const int g = threadIdx.x / kGradLanes, l = threadIdx.x % kGradLanes;
    const long long i = (long long)blockIdx.x * kGradRows + g;
    if (i >= a.n) return;       // (a whole lane group leaves together)
    const double *__restrict__ val = a.val + (long long)k * a.nnz, *__restrict__ lam = a.lam + (long long)k * a.sw;
    double s = 0.0;
    const long long q1 = a.rp[i + 1];
    for (long long q = a.rp[i] + l; q < q1; q += kGradLanes) s = __builtin_fma(val[a.pos[q]], lam[a.col[q]], s);
#pragma unroll
    for (int sh = kGradLanes / 2; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, kGradLanes);
    if (l == 0) a.out[(long long)k * a.so + i] = s;
}

__global__ __launch_bounds__(kGapNode) void k_gap_param_node(const GapParam a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sp[kGapNode];
    const long long i = (long long)blockIdx.x * kGapNode + threadIdx.x;
    double p = 0.0;
    if (i < a.n && a.mask[i]) {
        double d3, gp, dp;
        fisher_point_pullback(a.family, a.x[(long long)k * a.sx + i], a.y[i], a.aux ? a.aux[i] : 0.0, a.param_k ? a.param_k[k] : a.param,
                              a.logparam_k ? a.logparam_k[k] : a.logparam, d3, gp, dp);
        p = a.lam[(long long)k * a.sw + i] * gp;
    }
    sp[threadIdx.x] = p;
    gap_block_sum(sp, kGapNode, a.gpart + ((long long)k * gridDim.x + blockIdx.x));
}

__global__ __launch_bounds__(256) void k_gap_param(const GapParam a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sp[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double p = 0.0;
    if (i < a.nobs) {
        const double *x = a.x + (long long)k * a.sx, *lam = a.lam + (long long)k * a.sw;
        double s = 0.0, e = 0.0;
        const long long q1 = a.arp[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) {
            const int c = a.acol[q];
            e = __builtin_fma(a.aval[q], x[c], e);
            s = __builtin_fma(a.aval[q], lam[c], s);
        }
        e = gap_group_sum(e);
        s = gap_group_sum(s);
        if (l == 0) {
            const double eta = a.offset ? e + a.offset[i] : e;
            double d3, gp, dp;
            fisher_point_pullback(a.family, eta, a.y[i], a.aux ? a.aux[i] : 0.0, a.param_k ? a.param_k[k] : a.param,
                                  a.logparam_k ? a.logparam_k[k] : a.logparam, d3, gp, dp);
            p = s * gp;
        }
    }
    if (l == 0) sp[g] = p;
    gap_block_sum(sp, kDesignRows, a.gpart + ((long long)k * gridDim.x + blockIdx.x));
}

__global__ __launch_bounds__(kFisherFinal) void k_gap_final(const double *__restrict__ gpart, int ng, const double *__restrict__ ppart, int np,
                                                            const unsigned char *__restrict__ active, double *__restrict__ out) {
    const int k = blockIdx.x;
    if (active && !active[k]) return;
    __shared__ double sg[kFisherFinal], sp[kFisherFinal];
    const int tid = threadIdx.x;
    gpart += (long long)k * ng;
    ppart += (long long)k * np;
    double g = 0.0, p = 0.0;
    for (int b = tid; b < ng; b += kFisherFinal) g += gpart[b];
    for (int b = tid; b < np; b += kFisherFinal) p += ppart[b];
    sg[tid] = g; sp[tid] = p;
    __syncthreads();
    for (int st = kFisherFinal / 2; st > 0; st >>= 1) {
        if (tid < st) { sg[tid] += sg[tid + st]; sp[tid] += sp[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) out[k] = sg[0] - sp[0];
}

// ---- a composite likelihood (gmrfx_ga_pullback_composite; kernels.h: GapTiles, ObsComp) -----------------------------------------------
// The component of workgroup b: the last c with bptr[c] <= b, by a search over the at most kObsMaxComponents + 1 offsets. Every
// thread reads the same addresses: the loads are the workgroup's, not the lanes'.
__device__ __forceinline__ int gap_tile_comp(const GapTiles &w, int b) {
    int c = 0;
    while (c + 1 < w.ncomp && b >= w.bptr[c + 1]) c++;
    return c;
}

// k_gap_point on the component tiling: the same statements, except the row index and that lane 0 takes (family, param, logparam)
// of the workgroup's component from the table in device memory. KEEP THE TWO IN STEP: the body is written twice because a shared body
// gives the single-family kernel another instruction schedule; the one-component test of
// tests/test_gpu_composite_pullback.py compares their bits.
__global__ __launch_bounds__(256) void k_gap_point_comp(const GapPoint a, const ObsComp t, const GapTiles w) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sp[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const int cm = gap_tile_comp(w, (int)blockIdx.x);
    const long long i = w.rowptr[cm] + (long long)((int)blockIdx.x - w.bptr[cm]) * kDesignRows + g;
    double p = 0.0;
    if (i < w.rowptr[cm + 1]) { // (a whole lane group takes the branch together)
        const double *x = a.x + (long long)k * a.sx, *G = a.G + (long long)k * a.sg;
        double s = 0.0, c = 0.0;
        const long long q1 = a.arp[i + 1], o1 = a.optr[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], x[a.acol[q]], s);
        for (long long q = a.optr[i] + l; q < o1; q += kDesignLanes) c = __builtin_fma(a.ow[q], G[a.hmap[a.oidx[q]]], c);
        s = gap_group_sum(s);
        c = gap_group_sum(c);
        if (l == 0) {
            const double eta = a.offset ? s + a.offset[i] : s;
            double d3, gp, dp;
            fisher_point_pullback(t.family[cm], eta, a.y[i], a.aux ? a.aux[i] : 0.0, t.param[cm], t.logparam[cm], d3, gp, dp);
            a.t[(long long)k * a.nobs + i] = c * d3;
            p = c * dp;
        }
    }
    if (l == 0) sp[g] = p;
    gap_block_sum(sp, kDesignRows, a.ppart + ((long long)k * gridDim.x + blockIdx.x));
}

// k_gap_param the same way. A component whose family has no parameter (gp = 0 on every row) leaves 0 without walking its rows.
__global__ __launch_bounds__(256) void k_gap_param_comp(const GapParam a, const ObsComp t, const GapTiles w) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sp[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const int cm = gap_tile_comp(w, (int)blockIdx.x);
    const int family = t.family[cm];
    if (family != 0 && family != 4 && family != 5) {        // (uniform over the workgroup, ahead of its barriers)
        if (threadIdx.x == 0) a.gpart[(long long)k * gridDim.x + blockIdx.x] = 0.0;
        return;
    }
    const long long i = w.rowptr[cm] + (long long)((int)blockIdx.x - w.bptr[cm]) * kDesignRows + g;
    double p = 0.0;
    if (i < w.rowptr[cm + 1]) {
        const double *x = a.x + (long long)k * a.sx, *lam = a.lam + (long long)k * a.sw;
        double s = 0.0, e = 0.0;
        const long long q1 = a.arp[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) {
            const int c = a.acol[q];
            e = __builtin_fma(a.aval[q], x[c], e);
            s = __builtin_fma(a.aval[q], lam[c], s);
        }
        e = gap_group_sum(e);
        s = gap_group_sum(s);
        if (l == 0) {
            const double eta = a.offset ? e + a.offset[i] : e;
            double d3, gp, dp;
            fisher_point_pullback(family, eta, a.y[i], a.aux ? a.aux[i] : 0.0, t.param[cm], t.logparam[cm], d3, gp, dp);
            p = s * gp;
        }
    }
    if (l == 0) sp[g] = p;
    gap_block_sum(sp, kDesignRows, a.gpart + ((long long)k * gridDim.x + blockIdx.x));
}

// k_gap_final per component: workgroup (c, k) adds the partials of c's workgroups, strided loop then tree as k_gap_final does
__global__ __launch_bounds__(kFisherFinal) void k_gap_final_comp(const double *__restrict__ gpart, const double *__restrict__ ppart, int has_p,
                                                                 const GapTiles w, int nblk, const unsigned char *__restrict__ active,
                                                                 double *__restrict__ out) {
    const int c = blockIdx.x, k = blockIdx.y;
    if (active && !active[k]) return;
    __shared__ double sg[kFisherFinal], sp[kFisherFinal];
    const int tid = threadIdx.x;
    const int b0 = w.bptr[c], nb = w.bptr[c + 1] - b0;
    gpart += (long long)k * nblk + b0;
    ppart += (long long)k * nblk + b0;
    double g = 0.0, p = 0.0;
    for (int b = tid; b < nb; b += kFisherFinal) g += gpart[b];
    if (has_p)
        for (int b = tid; b < nb; b += kFisherFinal) p += ppart[b];
    sg[tid] = g; sp[tid] = p;
    __syncthreads();
    for (int st = kFisherFinal / 2; st > 0; st >>= 1) {
        if (tid < st) { sg[tid] += sg[tid + st]; sp[tid] += sp[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) out[(long long)k * w.ncomp + c] = sg[0] - sp[0];
}

// the active members' vectors copied (src non-null), or the INACTIVE members' filled with NaN (src null)
__global__ __launch_bounds__(256) void k_gap_copy(long long n, const double *__restrict__ src, long long ss, double *__restrict__ dst, long long sd,
                                                  const unsigned char *__restrict__ active) {
    const int k = blockIdx.y;
    const bool on = !active || active[k];
    if (on != (src != nullptr)) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[(long long)k * sd + i] = src ? src[(long long)k * ss + i] : __builtin_nan("");
}

void launch_gap_point(hipStream_t st, const GapPoint &a, bool design, int nbatch) {
    if (a.n <= 0 || a.nobs <= 0 || nbatch <= 0) return;
    const unsigned nb = (unsigned)gap_obs_blocks(design, a.n, a.nobs);
    if (design) hipLaunchKernelGGL(k_gap_point, dim3(nb, (unsigned)nbatch), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_gap_point_node, dim3(nb, (unsigned)nbatch), dim3(kGapNode), 0, st, a);
}
void launch_gap_gather(hipStream_t st, const GapGather &a, int nbatch) {
    if (a.n <= 0 || nbatch <= 0) return;
    if (a.ncc > 0) hipLaunchKernelGGL(k_gap_chunks, dim3((unsigned)a.ncc, (unsigned)nbatch), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_gap_gather, dim3((unsigned)design_blocks(a.n), (unsigned)nbatch), dim3(256), 0, st, a);
}
void launch_gap_pattern(hipStream_t st, const GapPattern &a, int nbatch) {
    if (a.n <= 0 || nbatch <= 0) return;
    hipLaunchKernelGGL(k_gap_pattern, dim3((unsigned)cdiv(a.n, kGradCols), (unsigned)nbatch), dim3(256), 0, st, a);
}
void launch_gap_mean(hipStream_t st, const GapMean &a, int nbatch) {
    if (a.n <= 0 || nbatch <= 0) return;
    hipLaunchKernelGGL(k_gap_mean, dim3((unsigned)cdiv(a.n, kGradRows), (unsigned)nbatch), dim3(256), 0, st, a);
}
void launch_gap_param(hipStream_t st, const GapParam &a, bool design, int nbatch) {
    if (a.n <= 0 || a.nobs <= 0 || nbatch <= 0) return;
    const unsigned nb = (unsigned)gap_obs_blocks(design, a.n, a.nobs);
    if (design) hipLaunchKernelGGL(k_gap_param, dim3(nb, (unsigned)nbatch), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_gap_param_node, dim3(nb, (unsigned)nbatch), dim3(kGapNode), 0, st, a);
}
void launch_gap_final(hipStream_t st, const double *gpart, int ng, const double *ppart, int np, const unsigned char *active, int nbatch, double *out) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(k_gap_final, dim3((unsigned)nbatch), dim3(kFisherFinal), 0, st, gpart, ng, ppart, np, active, out);
}
void launch_gap_point_comp(hipStream_t st, const GapPoint &a, const ObsComp &t, const GapTiles &w, int nblk, int nbatch) {
    if (a.n <= 0 || a.nobs <= 0 || nblk <= 0 || nbatch <= 0) return;
    hipLaunchKernelGGL(k_gap_point_comp, dim3((unsigned)nblk, (unsigned)nbatch), dim3(256), 0, st, a, t, w);
}
void launch_gap_param_comp(hipStream_t st, const GapParam &a, const ObsComp &t, const GapTiles &w, int nblk, int nbatch) {
    if (a.n <= 0 || a.nobs <= 0 || nblk <= 0 || nbatch <= 0) return;
    hipLaunchKernelGGL(k_gap_param_comp, dim3((unsigned)nblk, (unsigned)nbatch), dim3(256), 0, st, a, t, w);
}
void launch_gap_final_comp(hipStream_t st, const double *gpart, const double *ppart, bool has_p, const GapTiles &w, int nblk,
                           const unsigned char *active, int nbatch, double *out) {
    if (w.ncomp <= 0 || nbatch <= 0) return;
    hipLaunchKernelGGL(k_gap_final_comp, dim3((unsigned)w.ncomp, (unsigned)nbatch), dim3(kFisherFinal), 0, st, gpart, ppart, has_p ? 1 : 0, w, nblk,
                       active, out);
}
void launch_gap_copy(hipStream_t st, long long n, const double *src, long long ss, double *dst, long long sd, const unsigned char *active, int nbatch) {
    if (n <= 0 || nbatch <= 0 || !src) return;
    hipLaunchKernelGGL(k_gap_copy, dim3((unsigned)((n + 255) / 256), (unsigned)nbatch), dim3(256), 0, st, n, src, ss, dst, sd, active);
}
void launch_gap_fill_failed(hipStream_t st, long long n, double *dst, long long sd, const unsigned char *active, int nbatch) {
    if (n <= 0 || nbatch <= 0 || !active) return;
    hipLaunchKernelGGL(k_gap_copy, dim3((unsigned)((n + 255) / 256), (unsigned)nbatch), dim3(256), 0, st, n, (const double *)nullptr, 0LL, dst, sd, active);
}

}  // namespace gmrfx
