// fisher.hip -- what one Fisher-scoring iterate of the Gaussian approximation needs besides the factorisation (gmrfx_fisher_eval,
// gmrfx_batch_fisher_eval and the two loops), in ONE pass over Symmetric(Q_prior). The reference forms these on the host, array by array
// (src/workspace/gaussian_approximation.jl:191-313: loggrad, loghessian, loglik, Q_p x - h; the pointwise formulas:
// src/observation_models/exponential_family/canonical_implementations.jl:146-327 with helpers.jl:5-31). For a point x, with h = Q_p mu
// and eta_i = x_i:
//   score_i = ((Q_p x)_i - h_i) - g_i(x_i)            the reference's neg_score_k
//   hess_i  = d_i(x_i)                                 the hvals of gmrfx_refactorize_update under the diagonal map
//   energy  = sum_i (0.5 x_i (Q_p x)_i - x_i h_i)      = 1/2 x' Q_p x - x' h
//   loglik  = sum_i l_i(x_i)                           the terms that depend on x; the rest is the host's loglik_const
// g_i = dl_i/deta, d_i = d2l_i/deta2; a node without an observation has g = d = l = 0 exactly (_embed_grad, _embed_diag).
//   k_fisher_eval         a lane group of kFisherLanes lanes per row of Symmetric(Q_p) (the row structure RBMC and k_grad_mubar use: a
//                         gather, nothing is scattered; the loop itself: fisher_gather.h, shared with fisher_design.hip), kFisherRows
//                         rows per workgroup; one (energy, loglik) pair per workgroup
//   k_fisher_final        the pairs of a member's workgroups, one workgroup of kFisherFinal threads
//   k_fisher_candidate    the line search's candidate out = x - alpha s, contraction off
//   k_fisher_stats        the loop's four reductions over chunks of kFisherStatChunk entries; k_fisher_stats_final: a member's chunks
// STABLE FORMS of the six families: fisher_point.h, shared with fisher_design.hip.
// MEMBERS (batched handles, gmrfx_batch_fisher_eval and the lockstep loop of gmrfx_batch_gaussian_approximation). Every kernel above
// takes a member index from its grid (blockIdx.y; blockIdx.x in the two final kernels) and member strides: ONE copy of the row structure
// (rp, col, pos) and ONE data set by node (y, aux, mask) for all members, member k's prior values at + k nnz, its point at + k sx, its
// mean at + k smu (smu = 0: one mean), its score / hess at + k ss, the loop's vectors (candidate, reductions) at + k ms, its partial
// sums at + 2 k fisher_blocks(n) and + 4 k fisher_stat_blocks(n), its results at out + 2 k and out4 + 4 k. A per-member scalar
// (param, log param, the candidate's alpha) is the by-value argument unless its device array is non-null, then entry k of the array.
// A workgroup never spans two members. A plain handle is one member, strides 0, scalars by value; its arithmetic is what it was.
// ONE MEMBER, NOBODY MASKED (every plain evaluation: 62 500 workgroups of 16 short rows at n = 10^6): k_fisher_eval<false> is the same
// text compiled with k = 0, without the test and with the scalars by value, so a workgroup fetches none of the member fields of
// FisherEval (they lie behind the rest) and forms no member offset ahead of its first load.
// INACTIVE MEMBERS (active non-null and active[k] == 0): every workgroup of the member returns before its first load; its slices,
// partial sums and results keep what they held. The test is uniform over the workgroup, so no barrier is skipped by a part of it.
// DETERMINISM. No atomics. A lane adds its entries q0 + l, q0 + l + 16, ... in that order, the 16 lane sums meet in a fixed xor
// butterfly, the rows of a workgroup in a fixed LDS tree, the workgroups' pairs in a fixed strided loop + tree. The differences and
// products the interface pins are written with contraction off. Nothing depends on the alignment of x, mu, score or hess: all are read
// and written one double at a time. A member's sums are formed in one order whatever the other members hold and whichever of them are
// active: member k's results have the bits of a plain handle of that member.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "fisher_gather.h"
#include "fisher_point.h"

namespace gmrfx {

template <bool kMembers> __global__ __launch_bounds__(256) void k_fisher_eval(const FisherEval a) {
    const int k = kMembers ? blockIdx.y : 0;
    if (kMembers && a.active && !a.active[k]) return;
    __shared__ double se[kFisherRows], sl[kFisherRows];
    const int g = threadIdx.x / kFisherLanes, l = threadIdx.x % kFisherLanes;
    const int i = blockIdx.x * kFisherRows + g;
    const double *x = a.x + (long long)k * a.sx;
    double en = 0.0, ll = 0.0;
    if (i < a.n) {              // (a whole lane group takes the branch together)
        double s = 0.0, t = 0.0;
        fisher_row_gather(i, l, a.rp, a.col, a.pos, a.val + (long long)k * a.nnz, x, a.mu ? a.mu + (long long)k * a.smu : nullptr, s, t);
#pragma unroll
        for (int sh = kFisherLanes / 2; sh > 0; sh >>= 1) {
            s += __shfl_xor(s, sh, kFisherLanes);
            t += __shfl_xor(t, sh, kFisherLanes);
        }
        if (l == 0) {
            const double xi = x[i];
            double gi = 0.0, di = 0.0;
            if (a.mask[i])
                fisher_point(a.family, xi, a.y[i], a.aux ? a.aux[i] : 0.0, kMembers && a.param_k ? a.param_k[k] : a.param,
                             kMembers && a.logparam_k ? a.logparam_k[k] : a.logparam, gi, di, ll);
            {
#pragma clang fp contract(off)
                const double sc = (s - t) - gi;
                en = (0.5 * xi) * s - xi * t;
                if (a.score) a.score[(long long)k * a.ss + i] = sc;
            }
            if (a.hess) a.hess[(long long)k * a.ss + i] = di;
        }
    }
    if (l == 0) { se[g] = en; sl[g] = ll; }
    __syncthreads();
    for (int st = kFisherRows / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) { se[threadIdx.x] += se[threadIdx.x + st]; sl[threadIdx.x] += sl[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *part = a.part + 2 * ((long long)k * gridDim.x + blockIdx.x);
        part[0] = se[0]; part[1] = sl[0];
    }
}

__global__ __launch_bounds__(kFisherFinal) void k_fisher_final(const double *__restrict__ part, int nblocks, const unsigned char *__restrict__ active,
                                                               double *__restrict__ out) {
    const int k = blockIdx.x;
    if (active && !active[k]) return;
    __shared__ double se[kFisherFinal], sl[kFisherFinal];
    const int tid = threadIdx.x;
    part += 2 * (long long)k * nblocks;
    double e = 0.0, l = 0.0;
    for (int b = tid; b < nblocks; b += kFisherFinal) { e += part[2 * (long long)b]; l += part[2 * (long long)b + 1]; }
    se[tid] = e; sl[tid] = l;
    __syncthreads();
    for (int st = kFisherFinal / 2; st > 0; st >>= 1) {
        if (tid < st) { se[tid] += se[tid + st]; sl[tid] += sl[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) { out[2 * (long long)k] = se[0]; out[2 * (long long)k + 1] = sl[0]; }
}

// the line search's candidate: out = x - alpha s (alpha = 1: x - s exactly, the reference's full step)
__global__ __launch_bounds__(256) void k_fisher_candidate(int n, const double *x, const double *__restrict__ s, long long ms, double alpha,
                                                          const double *__restrict__ alpha_k, const unsigned char *__restrict__ active,
                                                          double *out) {      // (out may be x)
#pragma clang fp contract(off)
    const int k = blockIdx.y;
    if (active && !active[k]) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, ki = (long long)k * ms + i;
    if (i < n) out[ki] = x[ki] - (alpha_k ? alpha_k[k] : alpha) * s[ki];
}

// The loop's reductions over chunks of kFisherStatChunk entries: part[4 b ..] = sum a_i b_i (a, b non-null), sum (c_i - d_i)^2 (c, d
// non-null), sum d_i^2 (d non-null), max |b_i| (b non-null); a thread adds entries t, t + 256, ... of its chunk in that order, then the tree.
__global__ __launch_bounds__(256) void k_fisher_stats(int n, const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ c,
                                                      const double *__restrict__ d, long long ms, const unsigned char *__restrict__ active,
                                                      double *__restrict__ part) {
    const int k = blockIdx.y;
    if (active && !active[k]) return;
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kFisherStatChunk, off = (long long)k * ms;
    if (a) a += off;
    if (b) b += off;
    if (c) c += off;
    if (d) d += off;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    for (int t = tid; t < kFisherStatChunk; t += 256) {
        const long long i = base + t;
        if (i >= n) break;
        if (a && b) v0 = __builtin_fma(a[i], b[i], v0);
        if (c && d) { const double r = c[i] - d[i]; v1 = __builtin_fma(r, r, v1); }
        if (d) v2 = __builtin_fma(d[i], d[i], v2);
        if (b) v3 = fmax(v3, fabs(b[i]));
    }
    sh[0][tid] = v0; sh[1][tid] = v1; sh[2][tid] = v2; sh[3][tid] = v3;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            sh[0][tid] += sh[0][tid + st]; sh[1][tid] += sh[1][tid + st]; sh[2][tid] += sh[2][tid + st];
            sh[3][tid] = fmax(sh[3][tid], sh[3][tid + st]);
        }
        __syncthreads();
    }
    if (tid < 4) part[4 * ((long long)k * gridDim.x + blockIdx.x) + tid] = sh[tid][0];
}
__global__ __launch_bounds__(256) void k_fisher_stats_final(const double *__restrict__ part, int nblocks, const unsigned char *__restrict__ active,
                                                            double *__restrict__ out) {
    const int k = blockIdx.x;
    if (active && !active[k]) return;
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    part += 4 * (long long)k * nblocks;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int bk = tid; bk < nblocks; bk += 256) {
        for (int q = 0; q < 3; q++) v[q] += part[4 * (long long)bk + q];
        v[3] = fmax(v[3], part[4 * (long long)bk + 3]);
    }
    for (int q = 0; q < 4; q++) sh[q][tid] = v[q];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            for (int q = 0; q < 3; q++) sh[q][tid] += sh[q][tid + st];
            sh[3][tid] = fmax(sh[3][tid], sh[3][tid + st]);
        }
        __syncthreads();
    }
    if (tid < 4) out[4 * (long long)k + tid] = sh[tid][0];
}

void launch_fisher_eval(hipStream_t st, const FisherEval &a, int nbatch, double *out) {
    if (a.n <= 0 || nbatch <= 0) return;
    const int nblocks = fisher_blocks(a.n);
    if (nbatch == 1 && !a.active && !a.param_k && !a.logparam_k) hipLaunchKernelGGL(k_fisher_eval<false>, dim3((unsigned)nblocks, 1), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_fisher_eval<true>, dim3((unsigned)nblocks, (unsigned)nbatch), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_fisher_final, dim3((unsigned)nbatch), dim3(kFisherFinal), 0, st, a.part, nblocks, a.active, out);
}
void launch_fisher_candidate(hipStream_t st, const FisherMembers &m, const double *x, const double *s, double alpha, const double *alpha_k,
                             double *out) {
    if (m.n <= 0 || m.nbatch <= 0) return;
    hipLaunchKernelGGL(k_fisher_candidate, dim3((unsigned)cdiv(m.n, 256), (unsigned)m.nbatch), dim3(256), 0, st, m.n, x, s, m.stride, alpha, alpha_k,
                       m.active, out);
}
void launch_fisher_stats(hipStream_t st, const FisherMembers &m, const double *a, const double *b, const double *c, const double *d, double *part,
                         double *out4) {
    if (m.n <= 0 || m.nbatch <= 0) return;
    const int nblocks = fisher_stat_blocks(m.n);
    hipLaunchKernelGGL(k_fisher_stats, dim3((unsigned)nblocks, (unsigned)m.nbatch), dim3(256), 0, st, m.n, a, b, c, d, m.stride, m.active, part);
    hipLaunchKernelGGL(k_fisher_stats_final, dim3((unsigned)m.nbatch), dim3(256), 0, st, part, nblocks, m.active, out4);
}

}  // namespace gmrfx
