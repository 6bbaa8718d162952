// kernel_common.h -- what the HIP kernels of more than one translation unit share (device code only: every .hip file includes it,
// no .cpp file does): vector typedefs, wave-level searches and products, split-K reductions, the geometry of a front.
//
// Layout in HBM
//   L      supernode panels, column-major r_s x c_s, leading dimension ld_s, 128-B aligned
//   CB     contribution blocks (r-c)x(r-c), column-major, lower triangle meaningful
//   X      right-hand sides in elimination order, ROW-major n x nrhs (a row = one DoF, so a
//          gather/scatter of a front's rows moves whole 8*nrhs-byte segments)
//   W      per-supernode update vectors (r-c) x nrhs, row-major (forward sweep hand-off)
// Dense contractions run on the FP64 matrix cores: v_mfma_f64_16x16x4_f64, whose C/D map is
// col = lane&15, row = (lane>>4) + 4*reg and A/B maps are A[lane&15][lane>>4],
// B[lane>>4][lane&15] (cdna_hip_programming.md section 3).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace gmrfx {

// a kernel with the grid, block and dynamic LDS that a choice function of device_plan.h returned
#define GMRFX_LAUNCH(kernel, c, st, ...) hipLaunchKernelGGL(kernel, dim3((c).gx, (c).gy, (c).gz), dim3((c).block), (c).lds, st, __VA_ARGS__)

// The time of a launch from the device's own wall clock instead of a pair of events on its stream (Device::syrk_ms): a slot of two
// 64-bit words, slot[0] = the earliest start and slot[1] = the latest end over the workgroups that stamp it (k_factor_reset sets the
// slot to all ones / 0; several launches may share one). One lane per workgroup, a plain device-scope atomic each way, nothing
// waits for either: for launches of few, long workgroups (k_syrk_big) and the reference form k_syrk_cb -- k_syrk_cb_rec, ~1000
// short tiles that start and end together, stores its times per tile instead (factor_kernels.hip). slot == nullptr: untimed.
__device__ __forceinline__ void stamp_begin(unsigned long long *slot, unsigned long long t0) {
    if (slot && threadIdx.x == 0) atomicMin(slot, t0);
}
__device__ __forceinline__ void stamp_end(unsigned long long *slot) {
    if (slot && threadIdx.x == 0) atomicMax(slot + 1, (unsigned long long)wall_clock64());
}

// two doubles that are only known to be 8-byte aligned (one 16-byte load; the hardware takes unaligned addresses)
typedef double gmrfx_d2u __attribute__((ext_vector_type(2), aligned(8)));
typedef double gmrfx_d4 __attribute__((ext_vector_type(4)));
// X[k][q] of the dense inverse X = L11^-1 of a big front (0 above the diagonal): strict lower part
// stored transposed in the strict upper triangle of the panel's diagonal block, diag = 1/L's.
// Unconditional clamped load + arithmetic mask (see inverse.hip).
// 1 / v by v_rcp_f64 + one Newton step (error <= 1 ulp for the normal, positive pivots it is used on): 3
// instructions where the IEEE division sequence takes ~15 -- and the accessors below sit in GEMM inner loops,
// evaluated for EVERY operand element (the diagonal select is computed unconditionally).
__device__ __forceinline__ double fast_rcp(double v) {
    const double y = __builtin_amdgcn_rcp(v);
    return __builtin_fma(__builtin_fma(-v, y, 1.0), y, y);
}
__device__ __forceinline__ double xinv_elem(const double *__restrict__ P, int ld, int c, int k, int q) {
    const int kk = min(max(k, 0), c - 1), qq = min(max(q, 0), c - 1);
    const double v = P[min(kk, qq) + (long long)max(kk, qq) * ld];
    const bool in = k >= 0 && q >= 0 && k < c && q < c;
    double x = v * ((in && q < k) ? 1.0 : 0.0);
    if (in && k == q) x = fast_rcp(v);
    return x;
}
// 32x32 (2x2 MFMA tiles) wave-level product  acc[a][b] += sum_{q in [qlo,qhi)} fa(m0+16a+lm, q) * fb(q, n0+16b+lm)
// with operand accessors that must be safe (clamped) for any index and return 0 outside.
template <class FA, class FB>
__device__ __forceinline__ void wave_gemm_32x32(gmrfx_d4 (&acc)[2][2], int m0, int n0, int qlo, int qhi, FA fa, FB fb,
                                                int lm, int lk) {
    constexpr int KU = 4;
    for (int q0 = qlo & ~3; q0 < qhi; q0 += 4 * KU) {
        double av[KU][2], bv[KU][2];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int q = q0 + 4 * u + lk;
            const double mk = (q >= qlo && q < qhi) ? 1.0 : 0.0;
#pragma unroll
            for (int a = 0; a < 2; a++) av[u][a] = fa(m0 + a * 16 + lm, q) * mk;
#pragma unroll
            for (int b = 0; b < 2; b++) bv[u][b] = fb(q, n0 + b * 16 + lm);
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a], bv[u][b], acc[a][b], 0, 0, 0);
    }
}

// ---- the same 32 x 32 wave product with the operand rows in PAIRS: MFMA row lm of tile 0 / 1 is row 2 lm / 2 lm + 1 of the
// wave's 32 (both dimensions), so a 16-byte load feeds two tiles. Output: acc[a][b][rr] = D[m0 + 2 (lk + 4 rr) + a][n0 + 2 lm + b].
// _pm: generic accessors (masked heads / tails); _rr: both operands with contiguous rows (base + q * stride); _rk: first
// operand with contiguous rows, second with contiguous k (one row pointer per tile): k in pairs, k-step 2 h + e of a batch
// holds k = batch + 8 h + 2 lk + e. The three share the row mapping, so pieces of one K range can use different forms.
template <class FA, class FB>
__device__ __forceinline__ void wave_gemm_32x32_pm(gmrfx_d4 (&acc)[2][2], int m0, int n0, int qlo, int qhi, FA fa, FB fb,
                                                   int lm, int lk) {
    constexpr int KU = 4;
    for (int q0 = qlo & ~3; q0 < qhi; q0 += 4 * KU) {
        double av[KU][2], bv[KU][2];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int q = q0 + 4 * u + lk;
            const double mk = (q >= qlo && q < qhi) ? 1.0 : 0.0;
#pragma unroll
            for (int a = 0; a < 2; a++) av[u][a] = fa(m0 + 2 * lm + a, q) * mk;
#pragma unroll
            for (int b = 0; b < 2; b++) bv[u][b] = fb(q, n0 + 2 * lm + b);
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a], bv[u][b], acc[a][b], 0, 0, 0);
    }
}
// qlo, qhi multiples of 4
// (Round 6, measured and dropped: the three-stage software pipeline of k_syrk_cb_rec<true> for ranges of >= 48 -- k_sel_dense 107 -> 123
//  VGPRs, still three waves per SIMD, bit-identical; selected inversion of cfg 3 12.59 / 12.65 -> 13.10 / 13.11 ms on the same box: that
//  kernel runs at the fabric's bandwidth limit already, requests further ahead only deepen the queues.)
__device__ __forceinline__ void wave_gemm_32x32_rr(gmrfx_d4 (&acc)[2][2], const double *pa2, long long sa, const double *pb2,
                                                   long long sb, int qlo, int qhi, int lk) {
    constexpr int KU = 4;
    int q0 = qlo;
    for (; q0 + 4 * KU <= qhi; q0 += 4 * KU) {
        gmrfx_d2u av[KU], bv[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const long long q = q0 + 4 * u + lk;
            av[u] = *(const gmrfx_d2u *)(pa2 + q * sa);
            bv[u] = *(const gmrfx_d2u *)(pb2 + q * sb);
        }
#pragma unroll
        for (int u = 0; u < KU; u++) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].x, bv[u].x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].x, bv[u].y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].y, bv[u].x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].y, bv[u].y, acc[1][1], 0, 0, 0);
        }
    }
    for (; q0 < qhi; q0 += 4) {
        const long long q = q0 + lk;
        const gmrfx_d2u av = *(const gmrfx_d2u *)(pa2 + q * sa), bv = *(const gmrfx_d2u *)(pb2 + q * sb);
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.y, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.x, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y, acc[1][1], 0, 0, 0);
    }
}
// batches of 8 k's from qlo while they fit below qhi; returns the first k it did NOT do (the caller finishes with _pm)
__device__ __forceinline__ int wave_gemm_32x32_rk(gmrfx_d4 (&acc)[2][2], const double *pa2, long long sa, const double *pb_t0,
                                                  const double *pb_t1, int qlo, int qhi, int lk) {
    int q0 = qlo;
    for (; q0 + 16 <= qhi; q0 += 16) {
        gmrfx_d2u av[4], b0[2], b1[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const long long q = q0 + 8 * h + 2 * lk;
            b0[h] = *(const gmrfx_d2u *)(pb_t0 + q);
            b1[h] = *(const gmrfx_d2u *)(pb_t1 + q);
            av[2 * h] = *(const gmrfx_d2u *)(pa2 + q * sa);
            av[2 * h + 1] = *(const gmrfx_d2u *)(pa2 + (q + 1) * sa);
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h].x, b0[h].x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h].x, b1[h].x, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h].y, b0[h].x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h].y, b1[h].x, acc[1][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h + 1].x, b0[h].y, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h + 1].x, b1[h].y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h + 1].y, b0[h].y, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2 * h + 1].y, b1[h].y, acc[1][1], 0, 0, 0);
        }
    }
    for (; q0 + 8 <= qhi; q0 += 8) {
        const long long q = q0 + 2 * lk;
        const gmrfx_d2u b0 = *(const gmrfx_d2u *)(pb_t0 + q), b1 = *(const gmrfx_d2u *)(pb_t1 + q);
        const gmrfx_d2u a0 = *(const gmrfx_d2u *)(pa2 + q * sa), a1 = *(const gmrfx_d2u *)(pa2 + (q + 1) * sa);
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b0.x, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b1.x, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b0.x, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b1.x, acc[1][1], 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b0.y, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b1.y, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b0.y, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b1.y, acc[1][1], 0, 0, 0);
    }
    return q0;
}

// the mirror image of _rk: FIRST operand with contiguous k (one row pointer per tile), second with contiguous rows
__device__ __forceinline__ int wave_gemm_32x32_kr(gmrfx_d4 (&acc)[2][2], const double *pa_t0, const double *pa_t1, const double *pb2,
                                                  long long sb, int qlo, int qhi, int lk) {
    int q0 = qlo;
    for (; q0 + 16 <= qhi; q0 += 16) {
        gmrfx_d2u bv[4], a0[2], a1[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const long long q = q0 + 8 * h + 2 * lk;
            a0[h] = *(const gmrfx_d2u *)(pa_t0 + q);
            a1[h] = *(const gmrfx_d2u *)(pa_t1 + q);
            bv[2 * h] = *(const gmrfx_d2u *)(pb2 + q * sb);
            bv[2 * h + 1] = *(const gmrfx_d2u *)(pb2 + (q + 1) * sb);
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h].x, bv[2 * h].x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h].x, bv[2 * h].y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[h].x, bv[2 * h].x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[h].x, bv[2 * h].y, acc[1][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h].y, bv[2 * h + 1].x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h].y, bv[2 * h + 1].y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[h].y, bv[2 * h + 1].x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[h].y, bv[2 * h + 1].y, acc[1][1], 0, 0, 0);
        }
    }
    for (; q0 + 8 <= qhi; q0 += 8) {
        const long long q = q0 + 2 * lk;
        const gmrfx_d2u a0 = *(const gmrfx_d2u *)(pa_t0 + q), a1 = *(const gmrfx_d2u *)(pa_t1 + q);
        const gmrfx_d2u b0 = *(const gmrfx_d2u *)(pb2 + q * sb), b1 = *(const gmrfx_d2u *)(pb2 + (q + 1) * sb);
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b0.x, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b0.y, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b0.x, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b0.y, acc[1][1], 0, 0, 0);
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b1.x, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b1.y, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b1.x, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b1.y, acc[1][1], 0, 0, 0);
    }
    return q0;
}

// Stage the inverse of the diagonal block into LDS as a full w x w lower-triangular matrix
// Ti[k*NB + q] = Linv[k][q] (zero above the diagonal, reciprocal on it).
__device__ __forceinline__ void stage_linv(const double *__restrict__ Dg, int ld, int w, double *Ti, int tid) {
    // 16 independent clamped loads per thread. Every use of the loaded value is unconditional
    // arithmetic (mask multiply / reciprocal), so the compiler cannot sink a load under a
    // branch and the 16 loads issue back to back.
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int idx = tid + 256 * u;
        const int q = idx % NB, k = idx / NB;   // element Linv[k][q], stored at (q, k) for q < k
        const int qq = min(q, w - 1), kk = min(k, w - 1);
        v[u] = Dg[min(qq, kk) + (long long)max(qq, kk) * ld];
    }
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int idx = tid + 256 * u;
        const int q = idx % NB, k = idx / NB;
        const double mk = (k < w && q < k) ? 1.0 : 0.0;
        double x = v[u] * mk;
        if (q == k && k < w) x = fast_rcp(v[u]);
        Ti[k * NB + q] = x;
    }
}

// Geometry of the front a workgroup works on: from the kernel arguments (one active front: the top-of-tree chains) or from
// ONE 32-byte record at the workgroup's position in the level list (Device::d_frec_*) -- not list -> five index arrays,
// which is a dependent round trip more on every launch of the panel chains.
__device__ __forceinline__ FrontView front_view(const FrontView *__restrict__ frec, const int z, const FrontArg &fa) {
    FrontView v;
    if (fa.on) {
        v.s = fa.s; v.c = fa.c; v.r = fa.r; v.ld = fa.ld; v.first = fa.first; v.pad = 0; v.pp = fa.pp;
    } else {
        // two 16-byte loads through a differently typed pointer: written as `v = frec[z]` the compiler merges the two
        // sources into ONE pointer (kernel arguments or record) and reads the fields with flat vector loads, one
        // dependent round trip for `c` and another for the rest
        const int4 *q = reinterpret_cast<const int4 *>(frec + z);
        const int4 a = q[0], b = q[1];
        v.s = a.x; v.c = a.y; v.r = a.z; v.ld = a.w; v.first = b.x; v.pad = 0;
        v.pp = ((long long)b.w << 32) | (unsigned)b.z;
    }
    return v;
}

// Split-K reduction for NW-wave workgroups with ONE 16-row tile (4 RHS tiles of 16 columns): every wave
// writes its four partial tiles, wave t < 4 then adds tile t over the waves in order 0..NW-1 (fixed,
// reproducible) and keeps the result in acc[t]. red: NW * 4 * 4 * 64 doubles.
// NW = 8 is for launches with about one workgroup per CU: a single wave per SIMD can only issue one FP64
// MFMA per ~138 cycles, two per SIMD reach the full 64-cycle rate (tools/micro/mix64.hip) -- and the K
// chain per wave halves as well.
template <int NW>
__device__ __forceinline__ void splitk_reduce_nw(gmrfx_d4 (&acc)[4], double *red, int wave, int lane) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) red[((wave * 4 + t) * 4 + rr) * 64 + lane] = acc[t][rr];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t == wave) {
            gmrfx_d4 sum;
#pragma unroll
            for (int rr = 0; rr < 4; rr++) sum[rr] = red[((0 * 4 + t) * 4 + rr) * 64 + lane];
#pragma unroll
            for (int w = 1; w < NW; w++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) sum[rr] += red[((w * 4 + t) * 4 + rr) * 64 + lane];
            acc[t] = sum;
        }
    }
}

// Split-K reduction across the 4 waves of a workgroup, DISTRIBUTED: every wave adds up ONE of the
// four 16-column tiles of each row tile (12 LDS reads in flight instead of 48 by a single wave,
// which cost ~100 VGPRs and one wave of occupancy). After the call wave w holds the complete tile
// acc[a][w] for every a; the partial sums are added in wave order 0..3 (fixed, reproducible).
// red: 4 * 3 * 4 * 64 doubles (24 KB).
template <int NA>
__device__ __forceinline__ void splitk_reduce4(gmrfx_d4 (&acc)[NA][4], double *red, int wave, int lane) {
#pragma unroll
    for (int a = 0; a < NA; a++) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t != wave) {
                const int slot = t < wave ? t : t - 1;
#pragma unroll
                for (int rr = 0; rr < 4; rr++) red[((wave * 3 + slot) * 4 + rr) * 64 + lane] = acc[a][t][rr];
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t == wave) {
                gmrfx_d4 part[4];
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    if (w == wave) part[w] = acc[a][t];
                    else {
                        const int slot = t < w ? t : t - 1;
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) part[w][rr] = red[((w * 3 + slot) * 4 + rr) * 64 + lane];
                    }
                }
#pragma unroll
                for (int rr = 0; rr < 4; rr++) acc[a][t][rr] = ((part[0][rr] + part[1][rr]) + part[2][rr]) + part[3][rr];
            }
        }
    }
}
// The same for two row tiles with PAIR ownership: after the call wave w holds the complete tiles acc[w >> 1][2 (w & 1)]
// and acc[w >> 1][2 (w & 1) + 1] -- two column tiles of ONE row tile, which the kernels that load right-hand sides in
// pairs (column tile t = right-hand sides 32 (t >> 1) + 2 lm + (t & 1)) then store 16 bytes per lane. Two passes (one
// per column-tile pair), partial sums added in wave order 0..3. red: 12 tiles = 24 KB, as above.
__device__ __forceinline__ void splitk_reduce4_pairs(gmrfx_d4 (&acc)[2][4], double *red, int wave, int lane) {
#pragma unroll
    for (int hc = 0; hc < 2; hc++) {
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int owner = 2 * a + hc;
            if (wave != owner) {
                const int rank = wave < owner ? wave : wave - 1;
#pragma unroll
                for (int e = 0; e < 2; e++)
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) red[(((a * 3 + rank) * 2 + e) * 4 + rr) * 64 + lane] = acc[a][2 * hc + e][rr];
            }
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int owner = 2 * a + hc;
            if (wave == owner) {
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    gmrfx_d4 part[4];
#pragma unroll
                    for (int w = 0; w < 4; w++) {
                        if (w == owner) part[w] = acc[a][2 * hc + e];
                        else {
                            const int rank = w < owner ? w : w - 1;
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) part[w][rr] = red[(((a * 3 + rank) * 2 + e) * 4 + rr) * 64 + lane];
                        }
                    }
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) acc[a][2 * hc + e][rr] = ((part[0][rr] + part[1][rr]) + part[2][rr]) + part[3][rr];
                }
            }
        }
    }
}

typedef gmrfx_d4 d4;
typedef gmrfx_d2u d2u;
typedef int i2u __attribute__((ext_vector_type(2), aligned(4)));   // two ints, 4-byte aligned: one 8-byte load

// Two lower bounds in the sorted array a[0..n) at once, by all 64 lanes of a wave together
// (64-ary search: 2 rounds of one load each for n <= 4096 instead of 12 dependent loads each).
// Must be called in wave-uniform control flow; the results are wave-uniform.
__device__ __forceinline__ void wave_lower_bound2(const int *__restrict__ a, const int n, const int k0, const int k1,
                                                  const int lane, int &r0, int &r1) {
    int lo0 = 0, hi0 = n, lo1 = 0, hi1 = n;
    while (lo0 < hi0 || lo1 < hi1) {
        const int st0 = max((hi0 - lo0 + 63) >> 6, 1), st1 = max((hi1 - lo1 + 63) >> 6, 1);
        const int x0 = lo0 + lane * st0, x1 = lo1 + lane * st1;
        const int v0 = a[min(x0, n - 1)], v1 = a[min(x1, n - 1)];
        const int c0 = __popcll(__ballot(x0 < hi0 && v0 < k0));
        const int c1 = __popcll(__ballot(x1 < hi1 && v1 < k1));
        if (lo0 < hi0) {
            if (c0 == 0) hi0 = lo0;
            else { const int nl = lo0 + (c0 - 1) * st0 + 1; hi0 = min(lo0 + c0 * st0, hi0); lo0 = nl; }
        }
        if (lo1 < hi1) {
            if (c1 == 0) hi1 = lo1;
            else { const int nl = lo1 + (c1 - 1) * st1 + 1; hi1 = min(lo1 + c1 * st1, hi1); lo1 = nl; }
        }
    }
    r0 = lo0;
    r1 = lo1;
}

}  // namespace gmrfx
