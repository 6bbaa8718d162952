// fisher_design.hip -- the evaluation of a Fisher-scoring iterate for a likelihood observed through a sparse design matrix
// (gmrfx_obs_set_design, gmrfx_fisher_eval in design form; gmrfx_batch_obs_set_design, gmrfx_batch_fisher_eval for the members of a batch). The reference forms these on the host (LinearlyTransformedLikelihood,
// src/observation_models/linearly_transformed.jl:313-340: eta = A x + b, loggrad = A' g, loghessian = Symmetric(A' (D A)); the loop
// subtracts it through _sparse_hessian_map, src/workspace/gaussian_approximation.jl:73-129). For a point x, with h = Q_p mu:
//   eta_i   = sum_k A_ik x_k (+ b_i)
//   score_j = ((Q_p x)_j - h_j) - sum_i A_ij g_i(eta_i)
//   hess[p] = sum_t w_t d_{i_t}(eta_{i_t})             the hvals of gmrfx_refactorize_update under the map of gmrfx_obs_hess_map
//   energy  = sum_j (0.5 x_j (Q_p x)_j - x_j h_j),  loglik = sum_i l_i(eta_i)
//   k_design_eta     a lane group per row of A: eta_i, then g_i, d_i and l_i (fisher_point.h); one loglik partial per workgroup
//   k_design_eta_comp  the same row pass for a composite likelihood (gmrfx_obs_set_composite): the row's family and parameter come from
//                    the component table (ObsComp), one byte per observation naming the component
//   k_design_chunks  one workgroup per chunk of kDesignChunk entries of a long column of A (sum A_ij g_i; when the score is wanted) or
//                    term list (sum w_t d_i; when the Hessian is)
//   k_design_score   a lane group per node: the pass of k_fisher_eval over Symmetric(Q_p) (fisher_gather.h), then the gather over column j of A
//   k_design_hess    a lane group per Hessian position over its term list
//   k_design_final   the energy and loglik partials of all workgroups, one workgroup of kFisherFinal threads
// A short segment is read entry by entry by its lane group; of a long one the lane group adds the chunk sums.
// DETERMINISM. No atomics. A lane adds entries q0 + l, q0 + l + 16, ... (or chunk sums c0 + l, c0 + l + 16, ...) in that order, the 16
// lane sums meet in a fixed xor butterfly; a chunk's thread adds entries t, t + 256 and the 256 sums meet in a fixed LDS tree; rows
// and workgroups as in fisher.hip. Differences and products the interface pins are written with contraction off. Every operand is
// read and written one double at a time: nothing depends on the alignment of x, mu, score or hess.
// MEMBERS (batched handles, gmrfx_batch_obs_set_design). Every kernel takes a member index from its grid (blockIdx.y; blockIdx.x in
// k_design_final) and the member strides of FisherDesign: ONE copy of the plan's tables, the chunk tables, the data set (y, aux, offset)
// and the member's row structure; member k's prior values at + k nnz, its point at + k sx, its mean at + k smu (0: one mean), its score at
// + k ss and hess at + k sh, g and d at + k nobs, its chunk sums at + k (ncc + nct), its partial sums at + k design_blocks(n) and
// + k design_blocks(nobs), its results at out + 2 k. A per-member scalar is the by-value argument unless its device array is non-null.
// A workgroup never spans two members; a member's sums are formed in today's order whatever the other members hold, so member k's
// results have the bits of a plain handle of Q_p,k and param[k]. A plain handle is one member, grid (blocks, 1), strides 0, scalars by
// value. INACTIVE MEMBERS (active non-null and active[k] == 0): every workgroup of the member returns on its first statement, uniform
// over the workgroup and ahead of every barrier and load; nothing of the member is written, its (energy, loglik) pair included.
// SELECTION MATRICES. With A = rows of the identity and no offset every sum above has one term with weight 1: eta, g, d, score and
// energy then have the bits of fisher.hip (the node pass is the same code in the same order).
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "fisher_gather.h"
#include "fisher_point.h"

namespace gmrfx {

#pragma clang fp contract(off)      // (the whole file: every fused multiply-add below is written as one)

__device__ __forceinline__ double design_group_sum(double s) {
#pragma unroll
    for (int sh = kDesignLanes / 2; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, kDesignLanes);
    return s;
}

// sum_q w[q] v[idx[q]] over the segment [p0, p1) by the lane group of lane l; a long segment: its chunk sums part[c0 .. c1)
__device__ __forceinline__ double design_segment(int l, long long p0, long long p1, const int *__restrict__ idx, const double *__restrict__ w,
                                                 const double *__restrict__ v, int c0, int c1, const double *__restrict__ part) {
    double s = 0.0;
    if (p1 - p0 <= kDesignChunk)
        for (long long q = p0 + l; q < p1; q += kDesignLanes) s = __builtin_fma(w[q], v[idx[q]], s);
    else
        for (int c = c0 + l; c < c1; c += kDesignLanes) s += part[c];
    return design_group_sum(s);
}

__global__ __launch_bounds__(256) void k_design_eta(const FisherDesign a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sl[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;       // (nobs may lie within kDesignRows of 2^31)
    double ll = 0.0;
    if (i < a.nobs) {           // (a whole lane group takes the branch together)
        const double *x = a.x + (long long)k * a.sx;
        double s = 0.0;
        const long long q1 = a.arp[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], x[a.acol[q]], s);
        s = design_group_sum(s);
        if (l == 0) {
            const double eta = a.offset ? s + a.offset[i] : s;
            double gi, di;
            fisher_point(a.family, eta, a.y[i], a.aux ? a.aux[i] : 0.0, a.param_k ? a.param_k[k] : a.param,
                         a.logparam_k ? a.logparam_k[k] : a.logparam, gi, di, ll);
            a.g[(long long)k * a.nobs + i] = gi;
            a.d[(long long)k * a.nobs + i] = di;
        }
    }
    if (l == 0) sl[g] = ll;
    __syncthreads();
    for (int st = kDesignRows / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sl[threadIdx.x] += sl[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.lpart[(long long)k * gridDim.x + blockIdx.x] = sl[0];
}

// k_design_eta for a composite likelihood: the same statements, except that lane 0 takes the row's (family, param, logparam) from the
// component table in device memory. KEEP THE TWO IN STEP: the body is written twice because sharing it through an inlined function
// gives k_design_eta another instruction schedule; the one-component test of tests/test_gpu_composite.py compares
// their bits.
__global__ __launch_bounds__(256) void k_design_eta_comp(const FisherDesign a, const ObsComp t) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sl[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double ll = 0.0;
    if (i < a.nobs) {           // (a whole lane group takes the branch together)
        const double *x = a.x + (long long)k * a.sx;
        double s = 0.0;
        const long long q1 = a.arp[i + 1];
        for (long long q = a.arp[i] + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], x[a.acol[q]], s);
        s = design_group_sum(s);
        if (l == 0) {
            const double eta = a.offset ? s + a.offset[i] : s;
            const int c = t.comp[i];
            double gi, di;
            fisher_point(t.family[c], eta, a.y[i], a.aux ? a.aux[i] : 0.0, t.param[c], t.logparam[c], gi, di, ll);
            a.g[(long long)k * a.nobs + i] = gi;
            a.d[(long long)k * a.nobs + i] = di;
        }
    }
    if (l == 0) sl[g] = ll;
    __syncthreads();
    for (int st = kDesignRows / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sl[threadIdx.x] += sl[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.lpart[(long long)k * gridDim.x + blockIdx.x] = sl[0];
}

__global__ __launch_bounds__(256) void k_design_chunks(const FisherDesign a, int chunk0) {       // chunks chunk0 .. chunk0 + gridDim.x
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double sh[256];
    const int b = chunk0 + blockIdx.x, tid = threadIdx.x;
    const bool column = b < a.ncc;
    const int *__restrict__ idx = column ? a.arow : a.tobs;
    const double *__restrict__ w = column ? a.acv : a.tw;
    const double *__restrict__ v = (column ? a.g : a.d) + (long long)k * a.nobs;
    const long long p0 = a.chs[b];
    const int len = a.chl[b];
    double s = 0.0;
    for (int t = tid; t < len; t += 256) s = __builtin_fma(w[p0 + t], v[idx[p0 + t]], s);
    sh[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) sh[tid] += sh[tid + st];
        __syncthreads();
    }
    if (tid == 0) a.cpart[(long long)k * (a.ncc + a.nct) + b] = sh[0];
}

__global__ __launch_bounds__(256) void k_design_score(const FisherDesign a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    __shared__ double se[kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double en = 0.0;
    if (i < a.n) {
        const double *x = a.x + (long long)k * a.sx;
        double s = 0.0, t = 0.0;
        fisher_row_gather(i, l, a.rp, a.col, a.pos, a.val + (long long)k * a.nnz, x, a.mu ? a.mu + (long long)k * a.smu : nullptr, s, t);
        s = design_group_sum(s);
        t = design_group_sum(t);
        double ag = 0.0;
        if (a.score)
            ag = design_segment(l, a.acp[i], a.acp[i + 1], a.arow, a.acv, a.g + (long long)k * a.nobs, a.cchoff[i], a.cchoff[i + 1],
                                a.cpart + (long long)k * (a.ncc + a.nct));
        if (l == 0) {
            const double xi = x[i];
            const double sc = (s - t) - ag;
            en = (0.5 * xi) * s - xi * t;
            if (a.score) a.score[(long long)k * a.ss + i] = sc;
        }
    }
    if (l == 0) se[g] = en;
    __syncthreads();
    for (int st = kDesignRows / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) se[threadIdx.x] += se[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.epart[(long long)k * gridDim.x + blockIdx.x] = se[0];
}

__global__ __launch_bounds__(256) void k_design_hess(const FisherDesign a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long p = (long long)blockIdx.x * kDesignRows + g;
    if (p >= a.cnt) return;      // (a whole lane group leaves together)
    const double s = design_segment(l, a.tptr[p], a.tptr[p + 1], a.tobs, a.tw, a.d + (long long)k * a.nobs, a.tchoff[p], a.tchoff[p + 1],
                                    a.cpart + (long long)k * (a.ncc + a.nct));
    if (l == 0) a.hess[(long long)k * a.sh + p] = s;
}

__global__ __launch_bounds__(kFisherFinal) void k_design_final(const double *__restrict__ epart, int ne, const double *__restrict__ lpart, int nl,
                                                               const unsigned char *__restrict__ active, double *__restrict__ out) {
    const int k = blockIdx.x;
    if (active && !active[k]) return;
    __shared__ double se[kFisherFinal], sl[kFisherFinal];
    const int tid = threadIdx.x;
    epart += (long long)k * ne;
    lpart += (long long)k * nl;
    double e = 0.0, l = 0.0;
    for (int b = tid; b < ne; b += kFisherFinal) e += epart[b];
    for (int b = tid; b < nl; b += kFisherFinal) l += lpart[b];
    se[tid] = e; sl[tid] = l;
    __syncthreads();
    for (int st = kFisherFinal / 2; st > 0; st >>= 1) {
        if (tid < st) { se[tid] += se[tid + st]; sl[tid] += sl[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) { out[2 * (long long)k] = se[0]; out[2 * (long long)k + 1] = sl[0]; }
}

// t null: a single family (k_design_eta); non-null: a composite (k_design_eta_comp)
static void design_launches(hipStream_t st, const FisherDesign &a, const ObsComp *t, int nbatch, double *out) {
    if (a.n <= 0 || a.nobs <= 0 || nbatch <= 0) return;
    const int ne = design_blocks(a.n), nl = design_blocks(a.nobs);
    const unsigned nb = (unsigned)nbatch;
    if (t) hipLaunchKernelGGL(k_design_eta_comp, dim3((unsigned)nl, nb), dim3(256), 0, st, a, *t);
    else hipLaunchKernelGGL(k_design_eta, dim3((unsigned)nl, nb), dim3(256), 0, st, a);
    // the chunk sums of the long columns feed the score only, those of the long term lists the Hessian only
    const int c0 = a.score ? 0 : a.ncc, c1 = a.hess ? a.ncc + a.nct : a.ncc;
    if ((a.score || a.hess) && c1 > c0) hipLaunchKernelGGL(k_design_chunks, dim3((unsigned)(c1 - c0), nb), dim3(256), 0, st, a, c0);
    hipLaunchKernelGGL(k_design_score, dim3((unsigned)ne, nb), dim3(256), 0, st, a);
    if (a.hess && a.cnt > 0) hipLaunchKernelGGL(k_design_hess, dim3((unsigned)design_blocks(a.cnt), nb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_design_final, dim3(nb), dim3(kFisherFinal), 0, st, a.epart, ne, a.lpart, nl, a.active, out);
}
void launch_fisher_design(hipStream_t st, const FisherDesign &a, int nbatch, double *out) { design_launches(st, a, nullptr, nbatch, out); }
void launch_fisher_design_comp(hipStream_t st, const FisherDesign &a, const ObsComp &t, int nbatch, double *out) {
    design_launches(st, a, &t, nbatch, out);
}

}  // namespace gmrfx
