// batch_fisher.hip -- the kernels of fisher.hip for the members of a batched handle (gmrfx_batch_fisher_eval and the lockstep loop of
// gmrfx_batch_gaussian_approximation): blockIdx.y is the member. The formulas, the lane layout and every reduction order are those of
// fisher.hip; what differs is where a member's operands live:
//   the row structure    ONE copy (the member's rp, col, pos), shared by all members
//   the prior's values   val + k nnz            the point   x + k sx            the mean   mu + k smu (smu = 0: one mean)
//   y, aux, mask         ONE data set, by node  param, log param   one per member, from two small device arrays
//   k_fisher_eval_batch         kFisherRows rows of ONE member per workgroup; one (energy, loglik) pair per workgroup, member k's pairs
//                               at part + 2 k nblocks
//   k_fisher_final_batch        one workgroup per member adds that member's pairs in the order of k_fisher_final
//   k_fisher_candidate_batch    out_k = x_k - alpha[k] s_k, alpha from a device array, contraction off
//   k_fisher_stats_batch        the four reductions over chunks of kFisherStatChunk entries of ONE member; k_fisher_stats_final_batch
//                               one workgroup per member
// INACTIVE MEMBERS (active[k] == 0): every workgroup of the member returns before its first load; its slices, partial sums and results
// keep what they held. The test is uniform over the workgroup, so no barrier is skipped by a part of it.
// DETERMINISM. No atomics; a member's sums are formed in the order fisher.hip forms them for a plain handle of that member, so the
// results have the same bits, whatever the other members hold and whichever of them are active.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "fisher_point.h"

namespace gmrfx {

__global__ __launch_bounds__(256) void k_fisher_eval_batch(const FisherEvalBatch a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double se[kFisherRows], sl[kFisherRows];
    const int g = threadIdx.x / kFisherLanes, l = threadIdx.x % kFisherLanes;
    const int i = blockIdx.x * kFisherRows + g;
    const double *val = a.val + (long long)k * a.nnz, *x = a.x + (long long)k * a.sx;
    const double *mu = a.mu ? a.mu + (long long)k * a.smu : nullptr;
    double en = 0.0, ll = 0.0;
    if (i < a.n) {              // (a whole lane group takes the branch together)
        double s = 0.0, t = 0.0;
        const long long q1 = a.rp[i + 1];
        for (long long q = a.rp[i] + l; q < q1; q += kFisherLanes) {
            const double v = val[a.pos[q]];
            const int c = a.col[q];
            s = __builtin_fma(v, x[c], s);
            if (mu) t = __builtin_fma(v, mu[c], t);
        }
#pragma unroll
        for (int sh = kFisherLanes / 2; sh > 0; sh >>= 1) {
            s += __shfl_xor(s, sh, kFisherLanes);
            t += __shfl_xor(t, sh, kFisherLanes);
        }
        if (l == 0) {
            const double xi = x[i];
            double gi = 0.0, di = 0.0;
            if (a.mask[i]) fisher_point(a.family, xi, a.y[i], a.aux ? a.aux[i] : 0.0, a.param[k], a.logparam[k], gi, di, ll);
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

__global__ __launch_bounds__(kFisherFinal) void k_fisher_final_batch(const double *__restrict__ part, int nblocks, const unsigned char *__restrict__ active,
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

__global__ __launch_bounds__(256) void k_fisher_candidate_batch(int n, const double *x, long long sx, const double *__restrict__ s, long long ss,
                                                                const double *__restrict__ alpha, const unsigned char *__restrict__ active,
                                                                double *out, long long so) {      // (out may be x)
#pragma clang fp contract(off)
    const int k = blockIdx.y;
    if (active && !active[k]) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[(long long)k * so + i] = x[(long long)k * sx + i] - alpha[k] * s[(long long)k * ss + i];
}

__global__ __launch_bounds__(256) void k_fisher_stats_batch(int n, const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ c,
                                                            const double *__restrict__ d, long long s, const unsigned char *__restrict__ active,
                                                            double *__restrict__ part) {
    const int k = blockIdx.y;
    if (active && !active[k]) return;
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kFisherStatChunk, off = (long long)k * s;
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
__global__ __launch_bounds__(256) void k_fisher_stats_final_batch(const double *__restrict__ part, int nblocks, const unsigned char *__restrict__ active,
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

void launch_fisher_eval_batch(hipStream_t st, const FisherEvalBatch &a, int nbatch, double *out) {
    if (a.n <= 0 || nbatch <= 0) return;
    const int nblocks = fisher_blocks(a.n);
    hipLaunchKernelGGL(k_fisher_eval_batch, dim3((unsigned)nblocks, (unsigned)nbatch), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_fisher_final_batch, dim3((unsigned)nbatch), dim3(kFisherFinal), 0, st, a.part, nblocks, a.active, out);
}
void launch_fisher_candidate_batch(hipStream_t st, int n, int nbatch, const double *x, long long sx, const double *s, long long ss,
                                   const double *alpha, const unsigned char *active, double *out, long long so) {
    if (n <= 0 || nbatch <= 0) return;
    hipLaunchKernelGGL(k_fisher_candidate_batch, dim3((unsigned)cdiv(n, 256), (unsigned)nbatch), dim3(256), 0, st, n, x, sx, s, ss, alpha, active,
                       out, so);
}
void launch_fisher_stats_batch(hipStream_t st, int n, int nbatch, const double *a, const double *b, const double *c, const double *d, long long s,
                               const unsigned char *active, double *part, double *out4) {
    if (n <= 0 || nbatch <= 0) return;
    const int nblocks = fisher_stat_blocks(n);
    hipLaunchKernelGGL(k_fisher_stats_batch, dim3((unsigned)nblocks, (unsigned)nbatch), dim3(256), 0, st, n, a, b, c, d, s, active, part);
    hipLaunchKernelGGL(k_fisher_stats_final_batch, dim3((unsigned)nbatch), dim3(256), 0, st, part, nblocks, active, out4);
}

}  // namespace gmrfx
