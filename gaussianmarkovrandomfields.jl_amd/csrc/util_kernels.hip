// util_kernels.hip -- small HIP kernels beside the phases: log-determinant, gathers, segment sums, Q's values in assembly order, the
// Newton update of Q's values, the level marker of the profiling runs; their launch wrappers.
#include <algorithm>

#include "kernel_common.h"

namespace gmrfx {

// ------------------------------------------------------------------------------------------
// log det Q = 2 sum_k log L_kk, fixed-order two-stage reduction (bit-reproducible)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_logdet_partial(const double *__restrict__ L, const long long *__restrict__ diagoff,
                                                        const unsigned char *__restrict__ own, int n, double *__restrict__ part) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int k0 = blockIdx.x * per, k1 = min(n, k0 + per);
    double acc = 0.0;
    // own (sharded handles): only the columns of the fronts this rank factored; nullptr = all
    for (int k = k0 + tid; k < k1; k += 256)
        if (!own || own[k]) acc += log(L[diagoff[k]]);
    sh[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) sh[tid] += sh[tid + st];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(256) void k_logdet_final(const double *__restrict__ part, int nparts, double *__restrict__ out) {
    // fixed tree over the (at most 1024) block sums: reproducible, and 4 us instead of 50 for one serial thread
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nparts; i += 256) acc += part[i];
    sh[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) sh[tid] += sh[tid + st];
        __syncthreads();
    }
    if (tid == 0) out[0] = 2.0 * sh[0];
}

// Gather values at precomputed offsets (-1 -> 0.0): selected-inverse extraction.
__global__ __launch_bounds__(256) void k_gather(const double *__restrict__ src, const long long *__restrict__ off,
                                                long long cnt, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < cnt) { const long long o = off[i]; out[i] = (o >= 0) ? src[o] : 0.0; }
}
// out[g] = sum over t in [segptr[g], segptr[g+1]) of w[t] * src[off[t]] (off < 0 -> 0): one wave per segment, lanes
// stride the segment, butterfly sum in a fixed order (reproducible). Consumers of the selected inverse that only
// need contractions (diag(A Sigma A'), tr(Sigma B)) never move Sigma's values to the host.
__global__ __launch_bounds__(64) void k_seg_wsum(const double *__restrict__ src, const long long *__restrict__ segptr,
                                                 const long long *__restrict__ off, const double *__restrict__ w,
                                                 double *__restrict__ out) {
    const long long t0 = segptr[blockIdx.x], t1 = segptr[blockIdx.x + 1];
    double acc = 0.0;
    for (long long t = t0 + threadIdx.x; t < t1; t += 64) {
        const long long o = off[t];
        acc += w[t] * src[o >= 0 ? o : 0] * (o >= 0 ? 1.0 : 0.0);
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}
// The same with the weights formed on the fly from the values of a sparse design matrix: entry t is the pair
// (p, q) of entries of one row, weight = A_p A_q (twice for p != q: Sigma is symmetric and only q <= p is listed).
__global__ __launch_bounds__(64) void k_seg_wsum_pairs(const double *__restrict__ src, const long long *__restrict__ segptr,
                                                       const long long *__restrict__ off, const int *__restrict__ pi,
                                                       const int *__restrict__ qi, const double *__restrict__ vals,
                                                       double *__restrict__ out) {
    const long long t0 = segptr[blockIdx.x], t1 = segptr[blockIdx.x + 1];
    double acc = 0.0;
    for (long long t = t0 + threadIdx.x; t < t1; t += 64) {
        const long long o = off[t];
        const int p = pi[t], q = qi[t];
        acc += (p == q ? 1.0 : 2.0) * vals[p] * vals[q] * src[o >= 0 ? o : 0] * (o >= 0 ? 1.0 : 0.0);
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void k_gather_diag(const double *__restrict__ src, const long long *__restrict__ diagoff,
                                                     const int *__restrict__ perm, int n, double *__restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[perm[k]] = src[diagoff[k]];
}

// nzp[q] = nzval[qsrc[q]]: Q's values in the order the assembly reads them (once per factorisation, 56 MB at cfg 2)
__global__ __launch_bounds__(256) void k_gather_values(const double *__restrict__ nzval, const int *__restrict__ qsrc, double *__restrict__ out, long long cnt) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long long)gridDim.x * 256) out[i] = nzval[qsrc[i]];
}
void launch_gather_values(hipStream_t st, const double *nzval, const int *qsrc, double *out, long long cnt) {
    if (cnt <= 0) return;
    hipLaunchKernelGGL(k_gather_values, dim3((unsigned)std::min<long long>(8192, (cnt + 255) / 256)), dim3(256), 0, st, nzval, qsrc, out, cnt);
}
// Profiling aid (GMRFX_LEVEL_MARK=1, tools/sweep_levels.py): an empty kernel whose launch geometry names the phase and tree
// level that follows it in the stream, so that a kernel trace / counter pass can be cut into levels without guessing.
__global__ void k_level_mark() {}
void launch_level_mark(hipStream_t st, int phase, int level) {
    hipLaunchKernelGGL(k_level_mark, dim3(level + 2), dim3(64 * phase), 0, st);      // level -1 = the sweep tasks / subtrees
}
// nz[map[k]] = prior[map[k]] - h[k] on top of nz = prior: the Newton-loop update of the reference
// (_update_hessian!, src/workspace/gaussian_approximation.jl:103-129) with Q kept on the device.
__global__ __launch_bounds__(256) void k_copy_values(const double *__restrict__ src, double *__restrict__ dst, long long cnt) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long long)gridDim.x * 256) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void k_subtract_at(double *__restrict__ nz, const long long *__restrict__ map,
                                                     const double *__restrict__ h, long long cnt) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < cnt) nz[map[k]] -= h[k];     // the map is injective (one Q entry per Hessian entry)
}
void launch_newton_update(hipStream_t st, const double *prior, double *nz, long long nnz, const long long *map, const double *h,
                          long long cnt) {
    hipLaunchKernelGGL(k_copy_values, dim3((unsigned)std::min<long long>(4096, (nnz + 255) / 256)), dim3(256), 0, st, prior, nz, nnz);
    if (cnt > 0) hipLaunchKernelGGL(k_subtract_at, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, nz, map, h, cnt);
}
void launch_logdet(hipStream_t st, const double *L, const long long *diagoff, const unsigned char *own, int n, double *part,
                   int nparts, double *out) {
    hipLaunchKernelGGL(k_logdet_partial, dim3(nparts), dim3(256), 0, st, L, diagoff, own, n, part);
    hipLaunchKernelGGL(k_logdet_final, dim3(1), dim3(256), 0, st, part, nparts, out);
}
void launch_gather(hipStream_t st, const double *src, const long long *off, long long cnt, double *out) {
    if (cnt <= 0) return;
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, src, off, cnt, out);
}
void launch_seg_wsum(hipStream_t st, const double *src, const long long *segptr, long long nseg, const long long *off,
                     const double *w, double *out) {
    if (nseg <= 0) return;
    hipLaunchKernelGGL(k_seg_wsum, dim3((unsigned)nseg), dim3(64), 0, st, src, segptr, off, w, out);
}
void launch_seg_wsum_pairs(hipStream_t st, const double *src, const long long *segptr, long long nseg, const long long *off,
                           const int *pi, const int *qi, const double *vals, double *out) {
    if (nseg <= 0) return;
    hipLaunchKernelGGL(k_seg_wsum_pairs, dim3((unsigned)nseg), dim3(64), 0, st, src, segptr, off, pi, qi, vals, out);
}
void launch_gather_diag(hipStream_t st, const double *src, const long long *diagoff, const int *perm, int n, double *out) {
    hipLaunchKernelGGL(k_gather_diag, dim3(cdiv(n, 256)), dim3(256), 0, st, src, diagoff, perm, n, out);
}

}  // namespace gmrfx
