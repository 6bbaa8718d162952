// constraint.hip -- linear equality constraints A x = e on the device (gmrfx_constraints_*, gmrfx_sample): conditioning by
// kriging, Rue & Held 2005 section 2.3.3, as the reference's ConstraintInfo / WorkspaceGMRF do it on the host
// (src/workspace/workspace_gmrf.jl:22-56, 260-305). A has m <= 64 sparse rows (CSR, 32-bit columns); the n x m operands
// At = Q^-1 A' and B = At L_c^-T (L_c L_c' = W = A At) are column-major with leading dimension n.
//   k_con_scatter    the dense right-hand side A' of the one blocked solve, from the CSR rows (behind a memset)
//   k_con_ax_part    partial sums of (A X)[r, j] over fixed chunks of kConChunk entries of row r
//   k_con_ax_final   R[r, j] = sum of the chunk sums in chunk order (- e[r]) (+ add[r])
//   k_con_trsm       B = At L_c^-T, row by row, from the explicit m x m inverse L_c^-1
//   k_con_apply      X <- X (+ mu) - B (L_c^-1 R): FP64 MFMA tiles for m >= 4, a vector path for m < 4
//   k_con_var        out_i = max(sigma_i - sum_j B_ij^2, 0)
//   k_batch_con_chol L_c, L_c^-1, log det W and the pivot status of every member of a batched handle, one workgroup per member
//   k_batch_con_quad |L_c^-1 r|^2 per member
//   k_batch_con_maxabs max_r |r| per member (the residual A x - e the batched Gaussian approximation reports)
//   k_batch_con_void NaN into At_k and W_k of the members whose factorisation failed
// MEMBERS (batched handles, gmrfx_batch_constraints_*). Every kernel above takes a member index from its grid and member strides:
// member k's At / B at + k n m, L_c^-1 at + k m m, R at + k m cols, the chunk sums at + k totchunks cols, X at + k sx, mu at
// + k smu. A plain handle is one member; its arithmetic is what it was.
// ACTIVE (k_con_ax_part, k_con_ax_final, k_con_apply_*; the conventions of FisherEval::active): nbatch bytes on the device, null =
// every member. A workgroup of a member whose byte is 0 returns on its first statement (uniform, ahead of every barrier and load) and
// nothing of that member is written: not X, not R, not the chunk sums. The batched Gaussian approximation projects the steps of
// the members a step concerns this way (Device::bcon_project).
// DETERMINISM. Every sum has one fixed order that depends on the operands' INDICES only: a thread of k_con_ax_part takes
// the entry pairs t, t + 256, ... of its chunk in that order, the 256 thread sums meet in a fixed LDS tree, the chunk sums
// are added in chunk order by one thread; no floating-point atomics anywhere. Whether a pair of neighbouring entries is
// fetched by one 16-byte load or by two 8-byte loads (alignment of the caller's column, neighbouring column indices)
// changes the loads, not the arithmetic: same bits for any leading dimension or column offset.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernel_common.h"

namespace gmrfx {

typedef gmrfx_d4 d4;
typedef double d2a __attribute__((ext_vector_type(2)));      // 16-byte aligned pair

__global__ __launch_bounds__(256) void k_con_scatter(const long long *__restrict__ rowptr, const int *__restrict__ col,
                                                     const double *__restrict__ val, int n, double *__restrict__ out) {
    const int r = blockIdx.y;
    const long long p0 = rowptr[r], len = rowptr[r + 1] - p0;
    out += (long long)blockIdx.z * gridDim.y * n;        // member blockIdx.z: its n x m block
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < len; t += (long long)gridDim.x * 256)
        out[(long long)r * n + col[p0 + t]] = val[p0 + t];      // duplicates were summed on the host: one writer per element
}

// grid (chunks of the longest row x members, column tiles of kConColTile, m). Chunk c of row r -> part[(choff[r] + c) * k + j].
__global__ __launch_bounds__(256) void k_con_ax_part(const long long *__restrict__ rowptr, const int *__restrict__ col,
                                                     const double *__restrict__ val, const int *__restrict__ choff,
                                                     const double *__restrict__ X, long long ldx, int k, double *__restrict__ part,
                                                     int maxchunks, long long sx, const unsigned char *__restrict__ active) {
    if (active && !active[blockIdx.x / maxchunks]) return;
    constexpr int KT = kConColTile;
    __shared__ double red[KT][256];
    const int r = blockIdx.z, mb = blockIdx.x / maxchunks, c = blockIdx.x - mb * maxchunks, tid = threadIdx.x;
    if (c >= choff[r + 1] - choff[r]) return;          // (uniform over the workgroup)
    X += (long long)mb * sx;
    part += (long long)mb * choff[gridDim.z] * k;
    const long long p0 = rowptr[r] + (long long)c * kConChunk;
    const int len = (int)min((long long)kConChunk, rowptr[r + 1] - p0);
    const int j0 = blockIdx.y * KT;
    double acc[KT];
#pragma unroll
    for (int u = 0; u < KT; u++) acc[u] = 0.0;
    for (int t = tid; 2 * t < len; t += 256) {
        const long long p = p0 + 2 * t;
        const bool two = 2 * t + 1 < len;
        const int c0 = col[p], c1 = two ? col[p + 1] : c0;
        const double v0 = val[p], v1 = two ? val[p + 1] : 0.0;
        const bool adj = two && c1 == c0 + 1;
#pragma unroll
        for (int u = 0; u < KT; u++) {
            const int j = min(j0 + u, k - 1);           // columns past the edge re-read the last one; never stored
            const double *px = X + (long long)j * ldx + c0;
            double x0, x1;
            if (adj && ((uintptr_t)px & 15) == 0) {
                const d2a x = *(const d2a *)px;
                x0 = x.x; x1 = x.y;
            } else {
                x0 = px[0];
                x1 = two ? X[(long long)j * ldx + c1] : 0.0;
            }
            acc[u] = __builtin_fma(v0, x0, acc[u]);
            if (two) acc[u] = __builtin_fma(v1, x1, acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < KT; u++) red[u][tid] = acc[u];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int u = 0; u < KT; u++) red[u][tid] += red[u][tid + s];
        }
        __syncthreads();
    }
    if (tid < KT && j0 + tid < k) part[(long long)(choff[r] + c) * k + j0 + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void k_con_ax_final(const int *__restrict__ choff, const double *__restrict__ part, int m, int k,
                                                      const double *__restrict__ e, const double *__restrict__ add, double *__restrict__ R,
                                                      const unsigned char *__restrict__ active) {
    if (active && !active[blockIdx.y]) return;
    const int idx = blockIdx.x * 256 + threadIdx.x, mb = blockIdx.y;         // add: m values per member
    if (idx >= m * k) return;
    const int r = idx % m, j = idx / m;
    part += (long long)mb * choff[m] * k;
    double s = 0.0;
    for (int c = choff[r]; c < choff[r + 1]; c++) s += part[(long long)c * k + j];
    if (e) s -= e[r];
    if (add) s += add[(long long)mb * m + r];
    R[(long long)mb * m * k + idx] = s;
}

// B[i, l] = sum_{q <= l} Linv[l, q] At[i, q]  (Linv = L_c^-1, row-major m x m, lower triangular): one thread per row i
__global__ __launch_bounds__(256) void k_con_trsm(const double *__restrict__ At, const double *__restrict__ Linv, int n, int m,
                                                  double *__restrict__ B) {
    __shared__ double Ls[64 * 64];
    Linv += (long long)blockIdx.y * m * m;             // member blockIdx.y
    At += (long long)blockIdx.y * n * m;
    B += (long long)blockIdx.y * n * m;
    for (int t = threadIdx.x; t < m * m; t += 256) Ls[t] = Linv[t];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int l = 0; l < m; l++) {
        double s = 0.0;
        for (int q = 0; q <= l; q++) s = __builtin_fma(Ls[l * m + q], At[i + (long long)q * n], s);
        B[i + (long long)l * n] = s;
    }
}

__global__ __launch_bounds__(256) void k_con_var(const double *__restrict__ B, int n, int m, double *__restrict__ sig) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    B += (long long)blockIdx.y * n * m;                // member blockIdx.y
    sig += (long long)blockIdx.y * n;
    double s = 0.0;
    for (int l = 0; l < m; l++) { const double b = B[i + (long long)l * n]; s = __builtin_fma(b, b, s); }
    const double d = sig[i] - s;
    sig[i] = d != d ? d : fmax(d, 0.0);            // (a NaN stays one: fmax would return the zero)
}

// T = -(L_c^-1 R) for the 64 columns [jc0, jc0 + 64) of this workgroup, rows padded with zeros to MP: Ts[l * 65 + jj]
template <int MP>
__device__ __forceinline__ void con_form_t(double *Ts, const double *__restrict__ Linv, const double *__restrict__ R, int m, int k, int jc0) {
    for (int idx = threadIdx.x; idx < MP * 64; idx += 256) {
        const int l = idx >> 6, jj = idx & 63, j = jc0 + jj;
        double s = 0.0;
        if (l < m && j < k)
            for (int q = 0; q <= l; q++) s = __builtin_fma(Linv[l * m + q], R[q + (long long)j * m], s);
        Ts[l * 65 + jj] = -s;
    }
    __syncthreads();
}

// X[i, j] <- X[i, j] (+ mu[i]) - sum_l B[i, l] T[l, j] on v_mfma_f64_16x16x4_f64, computed transposed: the MFMA's "row" index
// is the column j of X (first operand -T' from LDS), its "column" index the row i (second operand B' straight from HBM, 16
// contiguous rows per k: 128-byte runs), so accumulator element rr of a lane is X[i0 + lm, j0 + lk + 4 rr]: 16 lanes on 16
// contiguous rows. A wave owns 16 rows, a workgroup 64; it keeps its B operands in registers over the 64 columns of its
// column block and walks row tiles blockIdx.x, + gridDim.x, ... so that T is formed a bounded number of times.
// Bytes: X once in and once out, B once per column block of 64.
template <int MQ>     // k-steps of 4: m <= 4 MQ
__global__ __launch_bounds__(256) void k_con_apply_mfma(const double *__restrict__ B, const double *__restrict__ Linv, const double *__restrict__ R,
                                                        const double *__restrict__ mu, double *__restrict__ X, long long ldx, int n, int m, int k,
                                                        long long sx, long long smu, const unsigned char *__restrict__ active) {
    if (active && !active[blockIdx.z]) return;
    __shared__ double Ts[4 * MQ * 65];
    const int jc0 = blockIdx.y * 64;
    {
        const long long mb = blockIdx.z;
        B += mb * n * m; Linv += mb * m * m; R += mb * m * k; X += mb * sx;
        if (mu) mu += mb * smu;
    }
    con_form_t<4 * MQ>(Ts, Linv, R, m, k, jc0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;
    const long long ntile = ((long long)n + 63) >> 6;
    for (long long rt = blockIdx.x; rt < ntile; rt += gridDim.x) {
        const long long i = rt * 64 + wave * 16 + lm;
        const long long ic = min(i, (long long)n - 1);
        double bv[MQ];
#pragma unroll
        for (int u = 0; u < MQ; u++) {
            const int l = 4 * u + lk;
            const double v = B[ic + (long long)min(l, m - 1) * n];
            bv[u] = (l < m && i < n) ? v : 0.0;
        }
        const double mi = mu ? mu[ic] : 0.0;
#pragma unroll
        for (int jt = 0; jt < 4; jt++) {
            const int j0 = jc0 + 16 * jt;
            if (j0 >= k) break;
            d4 acc;
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = min(j0 + lk + 4 * rr, k - 1);
                acc[rr] = X[ic + (long long)j * ldx];
            }
            if (mu) {
#pragma unroll
                for (int rr = 0; rr < 4; rr++) acc[rr] += mi;
            }
#pragma unroll
            for (int u = 0; u < MQ; u++) {
                const double av = Ts[(4 * u + lk) * 65 + 16 * jt + lm];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u], acc, 0, 0, 0);
            }
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = j0 + lk + 4 * rr;
                if (i < n && j < k) X[i + (long long)j * ldx] = acc[rr];
            }
        }
    }
}

// the same for m < 4 (and m = 0 with a mean: X += mu): one thread per row, the columns of the block one after the other
template <int M>
__global__ __launch_bounds__(256) void k_con_apply_vec(const double *__restrict__ B, const double *__restrict__ Linv, const double *__restrict__ R,
                                                       const double *__restrict__ mu, double *__restrict__ X, long long ldx, int n, int k,
                                                       long long sx, long long smu, const unsigned char *__restrict__ active) {
    if (active && !active[blockIdx.z]) return;
    __shared__ double Ts[(M > 0 ? M : 1) * 65];
    const int jc0 = blockIdx.y * 64;
    {
        const long long mb = blockIdx.z;
        if (M > 0) { B += mb * n * M; Linv += mb * M * M; R += mb * M * k; }
        X += mb * sx;
        if (mu) mu += mb * smu;
    }
    if (M > 0) con_form_t<M>(Ts, Linv, R, M, k, jc0);
    const int jn = min(64, k - jc0);
    const long long ntile = ((long long)n + 255) >> 8;
    for (long long rt = blockIdx.x; rt < ntile; rt += gridDim.x) {
        const long long i = rt * 256 + threadIdx.x;
        if (i >= n) continue;
        double b[M > 0 ? M : 1];
#pragma unroll
        for (int l = 0; l < M; l++) b[l] = B[i + (long long)l * n];
        const double mi = mu ? mu[i] : 0.0;
        for (int jj = 0; jj < jn; jj++) {
            double *px = X + i + (long long)(jc0 + jj) * ldx;
            double x = *px;
            if (mu) x += mi;
#pragma unroll
            for (int l = 0; l < M; l++) x = __builtin_fma(Ts[l * 65 + jj], b[l], x);
            *px = x;
        }
    }
}

// Member blockIdx.x of a batched handle: the Cholesky factor L_c of W_k (lower triangle of the column-major m x m block at
// W + k m m), its explicit inverse, log det W_k and the status word. ONE wave; S holds L_c in its lower triangle (row i at
// i * LD) and, once L_c is complete, L_c^-1 TRANSPOSED in the strict upper triangle (its diagonal is 1 / L_ii): 33 KB of LDS
// for m = 64. Column by column as the plain handle's host loop: lane i >= j forms W_ij - sum_{q < j} L_iq L_jq in ascending
// q, the pivot fails when it is not above 16 m eps |W_jj|; then lane j substitutes column j of L_c^-1 forwards.
// finfo (nullable): the members' factorisation status (batch_diag); a member whose factorisation failed gets cinfo = -1.
// A member that fails either way gets NaN for L_c^-1 and log det W: nothing derived from it looks like a result.
__global__ __launch_bounds__(64) void k_batch_con_chol(const double *__restrict__ W, int m, const long long *__restrict__ finfo,
                                                       double *__restrict__ Linv, double *__restrict__ logdet, long long *__restrict__ cinfo) {
    constexpr int LD = 65;
    __shared__ double S[64 * LD];
    __shared__ double dj_s;
    __shared__ int fail_s;
    const int mb = blockIdx.x, i = threadIdx.x;
    W += (long long)mb * m * m;
    Linv += (long long)mb * m * m;
    const double nan = __builtin_nan("");
    long long status = (finfo && finfo[mb] != 0) ? -1 : 0;
    if (status == 0) {
        if (i < m)
            for (int j = 0; j <= i; j++) S[i * LD + j] = W[i + j * m];
        if (i == 0) fail_s = 0;
        __syncthreads();
        double ld = 0.0;
        for (int j = 0; j < m; j++) {
            double s = 0.0;
            if (i >= j && i < m) {
                s = S[i * LD + j];
                for (int q = 0; q < j; q++) s = __builtin_fma(-S[i * LD + q], S[j * LD + q], s);
            }
            if (i == j) {
                const double wjj = S[j * LD + j];
                if (!(s > 16.0 * m * 2.220446049250313e-16 * fabs(wjj)) || !isfinite(s)) fail_s = 1 + j;
                dj_s = sqrt(s);
            }
            __syncthreads();
            if (fail_s) break;          // (uniform)
            const double dj = dj_s;
            ld += 2.0 * log(dj);        // every lane keeps the same sum, in column order
            if (i == j) S[j * LD + j] = dj;
            else if (i > j && i < m) S[i * LD + j] = s / dj;
            __syncthreads();
        }
        status = fail_s;
        if (status == 0) {
            if (i < m) {                 // column i of L_c^-1 into row i of the upper triangle
                const int j = i;
                const double ljj = 1.0 / S[j * LD + j];
                for (int r = j + 1; r < m; r++) {
                    double s = -S[r * LD + j] * ljj;
                    for (int q = j + 1; q < r; q++) s = __builtin_fma(-S[r * LD + q], S[j * LD + q], s);
                    S[j * LD + r] = s / S[r * LD + r];
                }
            }
            __syncthreads();
            for (int t = i; t < m * m; t += 64) {
                const int r = t / m, c = t - r * m;
                Linv[t] = r > c ? S[c * LD + r] : (r == c ? 1.0 / S[r * LD + r] : 0.0);
            }
            if (i == 0) logdet[mb] = ld;
        }
    }
    if (status != 0) {
        for (int t = i; t < m * m; t += 64) Linv[t] = nan;
        if (i == 0) logdet[mb] = nan;
    }
    if (i == 0) cinfo[mb] = status;
}

// quad[k] = |L_c^-1 r_k|^2, r_k = the m values at R + k sr: lane l forms row l of the product in ascending q, lane 0 adds the
// squares in ascending l
__global__ __launch_bounds__(64) void k_batch_con_quad(const double *__restrict__ Linv, const double *__restrict__ R, long long sr, int m,
                                                       double *__restrict__ quad) {
    __shared__ double t2[64];
    const int mb = blockIdx.x, l = threadIdx.x;
    Linv += (long long)mb * m * m;
    R += (long long)mb * sr;
    if (l < m) {
        double t = 0.0;
        for (int q = 0; q <= l; q++) t = __builtin_fma(Linv[l * m + q], R[q], t);
        t2[l] = t * t;
    }
    __syncthreads();
    if (l == 0) {
        double s = 0.0;
        for (int q = 0; q < m; q++) s += t2[q];
        quad[mb] = s;
    }
}

// out[k] = max_r |R[k m + r]| for the members whose byte in active is set (nullable = all); the others' entries are left
__global__ __launch_bounds__(64) void k_batch_con_maxabs(const double *__restrict__ R, int m, int nb, const unsigned char *__restrict__ active,
                                                         double *__restrict__ out) {
    const int mb = blockIdx.x * 64 + threadIdx.x;
    if (mb >= nb || (active && !active[mb])) return;
    double s = 0.0;
    for (int r = 0; r < m; r++) {
        const double v = fabs(R[(long long)mb * m + r]);
        s = (v != v || v > s) ? v : s;          // (a NaN stays one)
        if (v != v) break;
    }
    out[mb] = s;
}

// the members whose factorisation failed (cinfo = -1): At_k and W_k become NaN too, whatever the sweeps made of a broken factor
__global__ __launch_bounds__(256) void k_batch_con_void(const long long *__restrict__ cinfo, double *__restrict__ At, long long nat,
                                                        double *__restrict__ W, int nw) {
    const long long mb = blockIdx.y;
    if (cinfo[mb] != -1) return;
    const double nan = __builtin_nan("");
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < nat; t += (long long)gridDim.x * 256) At[mb * nat + t] = nan;
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < nw; t += 256) W[mb * nw + t] = nan;
}

void launch_batch_con_chol(hipStream_t st, const double *W, int m, int nb, const long long *finfo, double *Linv, double *logdet, long long *cinfo) {
    if (m <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_batch_con_chol, dim3((unsigned)nb), dim3(64), 0, st, W, m, finfo, Linv, logdet, cinfo);
}

void launch_batch_con_void(hipStream_t st, const long long *cinfo, double *At, long long nat, double *W, int nw, int nb) {
    if (nb <= 0 || nat <= 0) return;
    hipLaunchKernelGGL(k_batch_con_void, dim3((unsigned)std::min<long long>((nat + 255) / 256, 1024), (unsigned)nb), dim3(256), 0, st, cinfo, At, nat,
                       W, nw);
}

void launch_batch_con_quad(hipStream_t st, const double *Linv, const double *R, long long sr, int m, int nb, double *quad) {
    if (m <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_batch_con_quad, dim3((unsigned)nb), dim3(64), 0, st, Linv, R, sr, m, quad);
}

void launch_batch_con_maxabs(hipStream_t st, const double *R, int m, int nb, const unsigned char *active, double *out) {
    if (m <= 0 || nb <= 0) return;
    hipLaunchKernelGGL(k_batch_con_maxabs, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, R, m, nb, active, out);
}

void launch_con_scatter(hipStream_t st, const long long *rowptr, const int *col, const double *val, int n, int m, long long maxlen, double *out,
                        int nb) {
    if (m <= 0 || maxlen <= 0) return;
    const unsigned gx = (unsigned)std::min<long long>((maxlen + 255) / 256, 4096);
    hipLaunchKernelGGL(k_con_scatter, dim3(gx, (unsigned)m, (unsigned)nb), dim3(256), 0, st, rowptr, col, val, n, out);
}

void launch_con_ax(hipStream_t st, const long long *rowptr, const int *col, const double *val, const int *choff, int maxchunks, int m,
                   const double *X, long long ldx, int k, double *part, const double *e, const double *add, double *R, int nb, long long sx,
                   const unsigned char *active) {
    if (m <= 0 || k <= 0) return;
    hipLaunchKernelGGL(k_con_ax_part, dim3((unsigned)maxchunks * (unsigned)nb, (unsigned)((k + kConColTile - 1) / kConColTile), (unsigned)m),
                       dim3(256), 0, st, rowptr, col, val, choff, X, ldx, k, part, maxchunks, sx, active);
    hipLaunchKernelGGL(k_con_ax_final, dim3((unsigned)((m * k + 255) / 256), (unsigned)nb), dim3(256), 0, st, choff, part, m, k, e, add, R, active);
}

void launch_con_trsm(hipStream_t st, const double *At, const double *Linv, int n, int m, double *B, int nb) {
    if (n <= 0 || m <= 0) return;
    hipLaunchKernelGGL(k_con_trsm, dim3((unsigned)((n + 255) / 256), (unsigned)nb), dim3(256), 0, st, At, Linv, n, m, B);
}

void launch_con_var(hipStream_t st, const double *B, int n, int m, double *sig, int nb) {
    if (n <= 0 || m <= 0) return;
    hipLaunchKernelGGL(k_con_var, dim3((unsigned)((n + 255) / 256), (unsigned)nb), dim3(256), 0, st, B, n, m, sig);
}

void launch_con_apply(hipStream_t st, const double *B, const double *Linv, const double *R, const double *mu, double *X, long long ldx, int n,
                      int m, int k, int nb, long long sx, long long smu, const unsigned char *active) {
    if (n <= 0 || k <= 0 || (m <= 0 && !mu)) return;
    const unsigned gy = (unsigned)((k + 63) / 64);
#define GMRFX_CON_VEC(M)                                                                                                                  \
    hipLaunchKernelGGL(k_con_apply_vec<M>, dim3((unsigned)std::min<long long>(((long long)n + 255) / 256, kConApplyGroups), gy, (unsigned)nb), dim3(256), 0, st, B, \
                       Linv, R, mu, X, ldx, n, k, sx, smu, active)
#define GMRFX_CON_MFMA(MQ)                                                                                                                \
    hipLaunchKernelGGL(k_con_apply_mfma<MQ>, dim3((unsigned)std::min<long long>(((long long)n + 63) / 64, kConApplyGroups), gy, (unsigned)nb), dim3(256), 0, st, B, \
                       Linv, R, mu, X, ldx, n, m, k, sx, smu, active)
    if (m <= 0) GMRFX_CON_VEC(0);
    else if (m == 1) GMRFX_CON_VEC(1);
    else if (m == 2) GMRFX_CON_VEC(2);
    else if (m == 3) GMRFX_CON_VEC(3);
    else if (m <= 4) GMRFX_CON_MFMA(1);
    else if (m <= 8) GMRFX_CON_MFMA(2);
    else if (m <= 16) GMRFX_CON_MFMA(4);
    else if (m <= 32) GMRFX_CON_MFMA(8);
    else GMRFX_CON_MFMA(16);
#undef GMRFX_CON_VEC
#undef GMRFX_CON_MFMA
}

}  // namespace gmrfx
