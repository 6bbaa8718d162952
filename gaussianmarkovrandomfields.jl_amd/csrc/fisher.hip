// fisher.hip -- what one Fisher-scoring iterate of the Gaussian approximation needs besides the factorisation (gmrfx_fisher_eval), in ONE
// pass over Symmetric(Q_prior). The reference forms these on the host, array by array (src/workspace/gaussian_approximation.jl:191-313:
// loggrad, loghessian, loglik, Q_p x - h; the pointwise formulas: src/observation_models/exponential_family/
// canonical_implementations.jl:146-327 with helpers.jl:5-31). For a point x, with h = Q_p mu and eta_i = x_i:
//   score_i = ((Q_p x)_i - h_i) - g_i(x_i)            the reference's neg_score_k
//   hess_i  = d_i(x_i)                                 the hvals of gmrfx_refactorize_update under the diagonal map
//   energy  = sum_i (0.5 x_i (Q_p x)_i - x_i h_i)      = 1/2 x' Q_p x - x' h
//   loglik  = sum_i l_i(x_i)                           the terms that depend on x; the rest is the host's loglik_const
// g_i = dl_i/deta, d_i = d2l_i/deta2; a node without an observation has g = d = l = 0 exactly (_embed_grad, _embed_diag).
//   k_fisher_eval    a lane group of kFisherLanes lanes per row of Symmetric(Q_p) (the row structure RBMC and k_grad_mubar use: a gather,
//                    nothing is scattered), kFisherRows rows per workgroup; one (energy, loglik) pair per workgroup
//   k_fisher_final   the pairs of all workgroups, one workgroup of kFisherFinal threads
// STABLE FORMS of the six families: fisher_point.h, shared with fisher_design.hip.
// DETERMINISM. No atomics. A lane adds its entries q0 + l, q0 + l + 16, ... in that order, the 16 lane sums meet in a fixed xor
// butterfly, the rows of a workgroup in a fixed LDS tree, the workgroups' pairs in a fixed strided loop + tree. The differences and
// products the interface pins are written with contraction off. Nothing depends on the alignment of x, mu, score or hess: all are read
// and written one double at a time.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "fisher_point.h"

namespace gmrfx {

__global__ __launch_bounds__(256) void k_fisher_eval(const FisherEval a) {
    __shared__ double se[kFisherRows], sl[kFisherRows];
    const int g = threadIdx.x / kFisherLanes, l = threadIdx.x % kFisherLanes;
    const int i = blockIdx.x * kFisherRows + g;
    double en = 0.0, ll = 0.0;
    if (i < a.n) {              // (a whole lane group takes the branch together)
        double s = 0.0, t = 0.0;
        const long long q1 = a.rp[i + 1];
        for (long long q = a.rp[i] + l; q < q1; q += kFisherLanes) {
            const double v = a.val[a.pos[q]];
            const int c = a.col[q];
            s = __builtin_fma(v, a.x[c], s);
            if (a.mu) t = __builtin_fma(v, a.mu[c], t);
        }
#pragma unroll
        for (int sh = kFisherLanes / 2; sh > 0; sh >>= 1) {
            s += __shfl_xor(s, sh, kFisherLanes);
            t += __shfl_xor(t, sh, kFisherLanes);
        }
        if (l == 0) {
            const double xi = a.x[i];
            double gi = 0.0, di = 0.0;
            if (a.mask[i]) fisher_point(a.family, xi, a.y[i], a.aux ? a.aux[i] : 0.0, a.param, a.logparam, gi, di, ll);
            {
#pragma clang fp contract(off)
                const double sc = (s - t) - gi;
                en = (0.5 * xi) * s - xi * t;
                if (a.score) a.score[i] = sc;
            }
            if (a.hess) a.hess[i] = di;
        }
    }
    if (l == 0) { se[g] = en; sl[g] = ll; }
    __syncthreads();
    for (int st = kFisherRows / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) { se[threadIdx.x] += se[threadIdx.x + st]; sl[threadIdx.x] += sl[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { a.part[2 * (long long)blockIdx.x] = se[0]; a.part[2 * (long long)blockIdx.x + 1] = sl[0]; }
}

__global__ __launch_bounds__(kFisherFinal) void k_fisher_final(const double *__restrict__ part, int nblocks, double *__restrict__ out) {
    __shared__ double se[kFisherFinal], sl[kFisherFinal];
    const int tid = threadIdx.x;
    double e = 0.0, l = 0.0;
    for (int b = tid; b < nblocks; b += kFisherFinal) { e += part[2 * (long long)b]; l += part[2 * (long long)b + 1]; }
    se[tid] = e; sl[tid] = l;
    __syncthreads();
    for (int st = kFisherFinal / 2; st > 0; st >>= 1) {
        if (tid < st) { se[tid] += se[tid + st]; sl[tid] += sl[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) { out[0] = se[0]; out[1] = sl[0]; }
}

// the line search's candidate: out = x - alpha s (alpha = 1: x - s exactly, the reference's full step)
__global__ __launch_bounds__(256) void k_fisher_candidate(int n, const double *x, const double *__restrict__ s, double alpha, double *out) {      // (out may be x)
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = x[i] - alpha * s[i];
}

// The loop's reductions over chunks of kFisherStatChunk entries: part[4 b ..] = sum a_i b_i (a, b non-null), sum (c_i - d_i)^2 (c, d
// non-null), sum d_i^2 (d non-null), max |b_i| (b non-null); a thread adds entries t, t + 256, ... of its chunk in that order, then the tree.
__global__ __launch_bounds__(256) void k_fisher_stats(int n, const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ c,
                                                      const double *__restrict__ d, double *__restrict__ part) {
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kFisherStatChunk;
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
    if (tid < 4) part[4 * (long long)blockIdx.x + tid] = sh[tid][0];
}
__global__ __launch_bounds__(256) void k_fisher_stats_final(const double *__restrict__ part, int nblocks, double *__restrict__ out) {
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int bk = tid; bk < nblocks; bk += 256) {
        for (int k = 0; k < 3; k++) v[k] += part[4 * (long long)bk + k];
        v[3] = fmax(v[3], part[4 * (long long)bk + 3]);
    }
    for (int k = 0; k < 4; k++) sh[k][tid] = v[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            for (int k = 0; k < 3; k++) sh[k][tid] += sh[k][tid + st];
            sh[3][tid] = fmax(sh[3][tid], sh[3][tid + st]);
        }
        __syncthreads();
    }
    if (tid < 4) out[tid] = sh[tid][0];
}

void launch_fisher_candidate(hipStream_t st, int n, const double *x, const double *s, double alpha, double *out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_fisher_candidate, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, n, x, s, alpha, out);
}
void launch_fisher_stats(hipStream_t st, int n, const double *a, const double *b, const double *c, const double *d, double *part, double *out) {
    if (n <= 0) return;
    const int nblocks = fisher_stat_blocks(n);
    hipLaunchKernelGGL(k_fisher_stats, dim3((unsigned)nblocks), dim3(256), 0, st, n, a, b, c, d, part);
    hipLaunchKernelGGL(k_fisher_stats_final, dim3(1), dim3(256), 0, st, part, nblocks, out);
}

void launch_fisher_eval(hipStream_t st, const FisherEval &a, double *out) {
    if (a.n <= 0) return;
    const int nblocks = fisher_blocks(a.n);
    hipLaunchKernelGGL(k_fisher_eval, dim3((unsigned)nblocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_fisher_final, dim3(1), dim3(kFisherFinal), 0, st, a.part, nblocks, out);
}

}  // namespace gmrfx
