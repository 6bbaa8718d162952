// batch.hip -- the per-member kernels of a BATCHED handle (gmrfx_create_batched): B members with one pattern are factored as the
// block-diagonal matrix diag(Q_1 .. Q_B), whose elimination forest is B copies of the member's tree. The factorisation and the sweeps
// are the ordinary level-scheduled kernels on that forest; what has to see the members one by one lives here:
//   - log det and pivot status per member, in one pass over L's diagonal (member k owns the permuted columns [k n, (k+1) n));
//   - the right-hand-side permutation with a member stride (member k's n x nrhs block at A + k s, leading dimension ld);
//   - the quadratic forms (x_vk - mu_k)' Q_k (x_vk - mu_k) on the member pattern, values nzval + k nnz, all members in one launch.
// The hyper-parameter loop of docs/src/literate-tutorials/workspace_factorization_reuse.jl:94-102 evaluates logpdf for many values
// of the same pattern; WorkspacePool (src/workspace/workspace_pool.jl:5-22) runs such evaluations side by side.
#include <hip/hip_runtime.h>

#include <climits>

#include "kernel_common.h"

namespace gmrfx {

namespace {
constexpr int BD_COLS = 1024;    // diagonal entries per workgroup of k_batch_diag_partial (4 per thread)
constexpr int QF_COLS = 128;     // as k_quadform (quadform.hip): same sums in the same order
}

// ------------------------------------------------------------------------------------------
// Per-member log det + pivot status. Every factor kernel class flags a pivot p with !(p > 0) and stores L_jj = p rsqrt(p)
// (small.hip: x[0] = p[0] i00; potrf64_blocked.h: L = a rs, rs = rsqrt_nr2(p)); rsqrt of a negative or NaN pivot is NaN and the
// Newton steps turn rsqrt(0) = inf into NaN as well, so the stored diagonal is NaN exactly at the flagged columns and > 0
// elsewhere: !(L_jj > 0) <=> the column was flagged. The first such member-local column is what a plain handle of that member's
// values reports through its atomicMin -- without touching the factor kernels.
// Two stages with a fixed tree each: reproducible bits.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_diag_partial(const double *__restrict__ L, const long long *__restrict__ diagoff,
                                                            int nm, int parts, double *__restrict__ psum, int *__restrict__ pbad) {
    __shared__ double sh[256];
    __shared__ int sb[256];
    const int tid = threadIdx.x;
    const int k = blockIdx.x / parts, p = blockIdx.x - k * parts;
    const int c0 = p * BD_COLS, c1 = min(nm, c0 + BD_COLS);
    const long long base = (long long)k * nm;
    // all loads of the thread issued before the first use (the kernel is a chain of two dependent loads per column)
    long long off[BD_COLS / 256];
#pragma unroll
    for (int u = 0; u < BD_COLS / 256; u++) {
        const int c = c0 + tid + 256 * u;
        off[u] = c < c1 ? diagoff[base + c] : -1;
    }
    double d[BD_COLS / 256];
#pragma unroll
    for (int u = 0; u < BD_COLS / 256; u++) d[u] = off[u] >= 0 ? L[off[u]] : 1.0;
    double acc = 0.0;
    int bad = INT_MAX;
#pragma unroll
    for (int u = 0; u < BD_COLS / 256; u++) {
        acc += log(d[u]);
        if (!(d[u] > 0.0)) bad = min(bad, c0 + tid + 256 * u);
    }
    sh[tid] = acc;
    sb[tid] = bad;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) { sh[tid] += sh[tid + st]; sb[tid] = min(sb[tid], sb[tid + st]); }
        __syncthreads();
    }
    if (tid == 0) { psum[blockIdx.x] = sh[0]; pbad[blockIdx.x] = sb[0]; }
}

__global__ __launch_bounds__(256) void k_batch_diag_final(const double *__restrict__ psum, const int *__restrict__ pbad, int parts,
                                                          double *__restrict__ logdet, long long *__restrict__ info) {
    __shared__ double sh[256];
    __shared__ int sb[256];
    const int tid = threadIdx.x;
    const long long k = blockIdx.x;
    double acc = 0.0;
    int bad = INT_MAX;
    for (int i = tid; i < parts; i += 256) { acc += psum[k * parts + i]; bad = min(bad, pbad[k * parts + i]); }
    sh[tid] = acc;
    sb[tid] = bad;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) { sh[tid] += sh[tid + st]; sb[tid] = min(sb[tid], sb[tid + st]); }
        __syncthreads();
    }
    if (tid == 0) {
        logdet[k] = 2.0 * sh[0];
        info[k] = sb[0] == INT_MAX ? 0 : (long long)sb[0] + 1;
    }
}

int batch_diag_parts(int nm) { return (nm + BD_COLS - 1) / BD_COLS; }

void launch_batch_diag(hipStream_t st, const double *L, const long long *diagoff, int nm, int nbatch, double *psum, int *pbad,
                       double *logdet, long long *info) {
    const int parts = batch_diag_parts(nm);
    hipLaunchKernelGGL(k_batch_diag_partial, dim3((unsigned)((long long)parts * nbatch)), dim3(256), 0, st, L, diagoff, nm, parts, psum, pbad);
    hipLaunchKernelGGL(k_batch_diag_final, dim3((unsigned)nbatch), dim3(256), 0, st, psum, pbad, parts, logdet, info);
}

// ------------------------------------------------------------------------------------------
// Right-hand-side permutation with a member stride: forest row I = k nm + i (member k, member row i) of column j lives at
// A[k s + j ld + i] on the caller's side, at X[iperm[I] ldx + j] on the solver's side (row-major, elimination order; iperm == nullptr:
// identity -- the backward-only solve takes Z in elimination order, and the forest's elimination order is the members' one after
// the other). dir 0: gather A -> X, dir 1: scatter X -> A. The same two shapes as k_permute_narrow / k_permute (sweep_level.hip): a
// thread per forest row for passes of <= 8 columns (caller side coalesced along i, every element read once), a 64 x 64 LDS
// transpose for wider passes. Within a member consecutive rows are consecutive addresses; a run of 64 rows that crosses a member
// boundary splits into two coalesced pieces.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ long long member_addr(unsigned I, unsigned nm, long long s) {
    const unsigned k = I / nm;
    return (long long)k * s + (I - k * nm);
}

__global__ __launch_bounds__(256) void k_batch_permute_narrow(const int *__restrict__ iperm, int N, int nm, double *__restrict__ A,
                                                              long long ld, long long s, double *__restrict__ X, int nr, int ldx, int dir) {
    const int I = blockIdx.x * 256 + threadIdx.x;
    if (I >= N) return;
    const long long row = iperm ? iperm[I] : I;
    double *a = A + member_addr((unsigned)I, (unsigned)nm, s);
    double v[8];
    if (dir == 0) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = a[(long long)min(j, nr - 1) * ld];
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j < nr) X[row * ldx + j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = X[row * ldx + min(j, nr - 1)];
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j < nr) a[(long long)j * ld] = v[j];
    }
}

__global__ __launch_bounds__(256) void k_batch_permute(const int *__restrict__ iperm, int N, int nm, double *__restrict__ A,
                                                       long long ld, long long s, double *__restrict__ X, int nr, int ldx, int dir) {
    __shared__ double T[64 * 65];
    __shared__ int rowL[64];
    const int I0 = blockIdx.x * 64;
    const int tid = threadIdx.x;
    const int a = tid & 63, b = tid >> 6;
    if (tid < 64) rowL[tid] = (I0 + tid < N) ? (iperm ? iperm[I0 + tid] : I0 + tid) : 0;
    const int I = min(I0 + a, N - 1);
    double *ac = A + member_addr((unsigned)I, (unsigned)nm, s);
    double v[16];
    if (dir == 0) {
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = ac[(long long)min(b + 4 * u, nr - 1) * ld];
#pragma unroll
        for (int u = 0; u < 16; u++) T[a * 65 + b + 4 * u] = v[u];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int kk = b + 4 * u;
            if (I0 + kk < N && a < nr) X[(long long)rowL[kk] * ldx + a] = T[kk * 65 + a];
        }
    } else {
        __syncthreads();
        const int acol = min(a, nr - 1);
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = X[(long long)rowL[b + 4 * u] * ldx + acol];
#pragma unroll
        for (int u = 0; u < 16; u++) T[(b + 4 * u) * 65 + a] = v[u];
        __syncthreads();
        if (I0 + a < N) {
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (b + 4 * u < nr) ac[(long long)(b + 4 * u) * ld] = T[a * 65 + b + 4 * u];
        }
    }
}

void launch_batch_permute(hipStream_t st, const int *iperm, int N, int nm, double *A, long long ld, long long s, double *X, int nr, int ldx,
                          int dir) {
    if (nr <= 8) hipLaunchKernelGGL(k_batch_permute_narrow, dim3((N + 255) / 256), dim3(256), 0, st, iperm, N, nm, A, ld, s, X, nr, ldx, dir);
    else hipLaunchKernelGGL(k_batch_permute, dim3((N + 63) / 64), dim3(256), 0, st, iperm, N, nm, A, ld, s, X, nr, ldx, dir);
}

// ------------------------------------------------------------------------------------------
// Quadratic forms of all members in one launch: workgroup (x, y) = 128 member columns of pair y = k nvec + v (grid y is walked in
// strides of gridDim.y, which stays <= 65535). The body is k_quadform's (quadform.hip): for one member the same sums in the same
// order as gmrfx_quadform on that member's values.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_quadform(int nm, const long long *__restrict__ colptr, const int *__restrict__ row,
                                                        const double *__restrict__ val0, long long nnz, int use_lower,
                                                        const double *__restrict__ X0, long long ldx, long long sx, int nvec, int npairs,
                                                        const double *__restrict__ mu0, double *__restrict__ part) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const int g = tid >> 4, l = tid & 15;
    for (int y = blockIdx.y; y < npairs; y += gridDim.y) {
        const int k = y / nvec, v = y - k * nvec;
        const double *x = X0 + (long long)k * sx + (long long)v * ldx;
        const double *val = val0 + (long long)k * nnz;
        const double *mu = mu0 ? mu0 + (long long)k * nm : nullptr;
        double acc = 0.0;
#pragma unroll 2
        for (int t = 0; t < QF_COLS / 16; t++) {
            const int j = blockIdx.x * QF_COLS + t * 16 + g;
            if (j < nm) {
                const long long p0 = colptr[j], p1 = colptr[j + 1];
                const double dj = x[j] - (mu ? mu[j] : 0.0);
                double a = 0.0;
                for (long long p = p0 + l; p < p1; p += 16) {
                    const int i = row[p];
                    const bool in_tri = use_lower ? (i > j) : (i < j);
                    const double wgt = (i == j) ? 1.0 : (in_tri ? 2.0 : 0.0);
                    a += wgt * val[p] * (x[i] - (mu ? mu[i] : 0.0));
                }
                acc += a * dj;
            }
        }
        sh[tid] = acc;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) sh[tid] += sh[tid + st];
            __syncthreads();
        }
        if (tid == 0) part[(long long)y * gridDim.x + blockIdx.x] = sh[0];
        __syncthreads();      // sh is reused by the next pair
    }
}

__global__ __launch_bounds__(256) void k_batch_quadform_final(const double *__restrict__ part, int nblk, double *__restrict__ out) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const double *p = part + (long long)blockIdx.x * nblk;
    double acc = 0.0;
    for (int i = tid; i < nblk; i += 256) acc += p[i];
    sh[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) sh[tid] += sh[tid + st];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = sh[0];
}

int batch_quadform_blocks(int nm) { return (nm + QF_COLS - 1) / QF_COLS; }

void launch_batch_quadform(hipStream_t st, int nm, const long long *colptr, const int *row, const double *val, long long nnz, int use_lower,
                           const double *X, long long ldx, long long sx, int nvec, int nbatch, const double *mu, double *part, double *out) {
    const long long npairs = (long long)nvec * nbatch;
    if (npairs <= 0 || nm <= 0) return;
    const int nblk = batch_quadform_blocks(nm);
    const unsigned gy = (unsigned)(npairs < 65535 ? npairs : 65535);
    hipLaunchKernelGGL(k_batch_quadform, dim3(nblk, gy), dim3(256), 0, st, nm, colptr, row, val, nnz, use_lower, X, ldx, sx, nvec,
                       (int)npairs, mu, part);
    hipLaunchKernelGGL(k_batch_quadform_final, dim3((unsigned)npairs), dim3(256), 0, st, part, nblk, out);
}

}  // namespace gmrfx
