// sweep_level.hip -- HIP kernels (gfx950 / CDNA4) of the level schedule of the multi-RHS triangular sweeps -- the forward assembly and
// updates, the backward products -- and the permutation / transposition of right-hand sides; their launch wrappers (the variant
// and geometry of a launch: choose_*, device_plan.h). Memory layout and MFMA maps: kernel_common.h.
#include "kernel_common.h"

namespace gmrfx {

// ------------------------------------------------------------------------------------------
// Triangular sweeps, X row-major (ldx doubles per row), nr <= 64 right-hand sides per pass
// ------------------------------------------------------------------------------------------

// Forward: add the children's update vectors into this front's OWN rows of X (the trailing rows, W_s, are assembled
// inside k_fwd_update_longk and written once). A workgroup owns FWD_RB own rows x 64 right-hand sides; which row of a
// child lands in own row tc comes from the per-edge table DevSym::erow (no search), the rows of X are read once,
// receive the children one after the other (fixed order) in registers and are written once.
__global__ __launch_bounds__(256) void k_fwd_assemble(DevSym S, const int *__restrict__ list, double *__restrict__ X,
                                                      const double *__restrict__ W, int nr, int ldx) {
    const int s = list[blockIdx.y];
    const int c = S.sfirst[s + 1] - S.sfirst[s];
    const int i0 = blockIdx.x * FWD_RB;
    if (i0 >= c) return;
    const long long ch0 = S.childptr[s], ch1 = S.childptr[s + 1];
    if (ch0 == ch1) return;
    const int first = S.sfirst[s];
    const int j = threadIdx.x & 63, g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (j >= nr) return;
    constexpr int NU = FWD_RB / 4;                       // rows per thread: i0 + g + 4 u
    double x[NU];
#pragma unroll
    for (int u = 0; u < NU; u++) x[u] = X[(long long)(first + min(i0 + g + 4 * u, c - 1)) * ldx + j];
    for (long long ch = ch0; ch < ch1; ch++) {
        const EdgeRec er = S.edge[ch];
        const int *er_row = S.erow + er.eoff;
        const double *Wd = W + er.woff * ldx;
        int jr[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) jr[u] = er_row[min(i0 + g + 4 * u, c - 1)];      // wave-uniform
        double v[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) v[u] = jr[u] >= 0 ? Wd[(long long)jr[u] * ldx + j] : 0.0;
#pragma unroll
        for (int u = 0; u < NU; u++) x[u] += v[u];
    }
#pragma unroll
    for (int u = 0; u < NU; u++)
        if (i0 + g + 4 * u < c) X[(long long)(first + i0 + g + 4 * u) * ldx + j] = x[u];
}

// Forward update of a big front after y = L11^-1 b: W_s = (children) - L21 y with K = all c columns.
// A workgroup owns 32
// trailing rows x 64 right-hand sides, every wave sweeps a quarter of the K range for the WHOLE
// tile (16 MFMA tiles per k-step from 4 + 4 operand loads; 512-B contiguous panel segments per
// column), the partial tiles are summed through LDS and each wave writes one row tile.
template <int NA>   // 16-row tiles per workgroup: 2 normally, 1 for levels with a handful of fronts (twice the
                    // workgroups, half the MFMA chain of each: one CU only sustains ~0.14 TFLOP/s of FP64 MFMA)
__global__ __launch_bounds__(256) void k_fwd_update_longk(DevSym S, const int *__restrict__ list,
                                                         const double *__restrict__ L, double *__restrict__ X,
                                                         double *__restrict__ W, int nr, int ldx, int cmin) {
    __shared__ double red[3 * 16 * 64];
    constexpr int RT = 16 * NA;
    __shared__ double Tl[RT * 64];   // children's contributions to this tile of W_s
    const int s = list[blockIdx.y];
    const int c = S.sfirst[s + 1] - S.sfirst[s];
    if (c <= cmin) return;           // (narrow passes: k_fwd_update_wave has these fronts)
    const int r = (int)(S.rowptr[s + 1] - S.rowptr[s]);
    const int i0 = c + blockIdx.x * RT;
    if (i0 >= r) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const int ld = S.ld[s];
    const double *P = L + S.panelptr[s];
    const double *Yb = X + (long long)S.sfirst[s] * ldx;
    double *Ws = W + S.wptr[s] * ldx;
    // ---- gather the children's update vectors for these rows into LDS (fixed child order, no
    //      atomics): W_s is then written exactly once, with no zero-fill / read-modify-write passes
    {
        const int j = threadIdx.x & 63, g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int jcl = min(j, nr - 1);
        const double jm = j < nr ? 1.0 : 0.0;
        for (int i = g; i < RT; i += 4) Tl[i * 64 + j] = 0.0;
        __syncthreads();
        // children two at a time (see k_syrk_cb): records + tile ranges first, then at most 32
        // child rows per tile and child, all loads in flight at once; added in child order. The target rows of a
        // child come in ONE load (lane l: row a0 + l; each use reads its lane) and rows past the tile's range issue
        // nothing: a vector memory instruction costs the address unit ~16 cycles whatever its lanes do.
        const long long ch0 = S.childptr[s], ch1 = S.childptr[s + 1];
        const int T = (blockIdx.x * RT) >> 5;   // 32-row granularity of the tile table
        for (long long cb = ch0; cb < ch1; cb += 2) {
            EdgeRec er[2];
            int a0[2], a1[2];
#pragma unroll
            for (int q = 0; q < 2; q++) er[q] = S.edge[min(cb + q, ch1 - 1)];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                a0[q] = S.etile[er[q].tptr + T];
                a1[q] = S.etile[er[q].tptr + T + 1];
            }
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (cb + q < ch1) {
                    const int *reld = S.rel + er[q].reloff;
                    const double *Wd = W + er[q].woff * ldx;
                    const int rt = reld[min(a0[q] + j, er[q].md - 1)];
                    const int na = a1[q] - a0[q] - g;            // this wave's rows: a0 + g + 4 u < a1  <=>  4 u < na
                    double wv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (4 * u < na) wv[u] = Wd[(long long)(a0[q] + g + 4 * u) * ldx + jcl];
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (4 * u < na) {
                            const int tr = __builtin_amdgcn_readlane(rt, g + 4 * u);
                            if (tr >= i0 && tr < i0 + RT) Tl[(tr - i0) * 64 + j] += wv[u] * jm;
                        }
                    __syncthreads();
                }
            }
        }
    }
    d4 acc[NA][4];
#pragma unroll
    for (int a = 0; a < NA; a++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[a][t] = (d4){0.0, 0.0, 0.0, 0.0};
    // Operands in PAIRS (16-byte loads): NA = 2: MFMA row lm of row tile 0 / 1 is row 2 lm / 2 lm + 1 of the 32; column
    // tile t is right-hand side 32 (t >> 1) + 2 lm + (t & 1): one load feeds two tiles, three loads per k-step instead
    // of six. Lanes past the last row / right-hand side re-read the last one's pair (results never stored).
    const double *pa = P + (NA == 2 ? min(i0 + 2 * lm, r - 1) : min(i0 + lm, r - 1));
    const int jb[2] = {min(2 * lm, nr - 1), min(32 + 2 * lm, nr - 1)};
    constexpr int KU = 4;
    for (int k0 = wave * 4 * KU; k0 < c; k0 += 16 * KU) {
        double av[KU][NA], bv[KU][4];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int kk = k0 + 4 * u + lk;
            const int kc = min(kk, c - 1);
            const double mk = kk < c ? 1.0 : 0.0;
            if constexpr (NA == 2) {
                const d2u x = *(const d2u *)(pa + (long long)kc * ld);
                av[u][0] = x.x * mk; av[u][1] = x.y * mk;
            } else {
                av[u][0] = pa[(long long)kc * ld] * mk;
            }
#pragma unroll
            for (int t2 = 0; t2 < 2; t2++) {
                const d2u y = *(const d2u *)(Yb + (long long)kc * ldx + jb[t2]);
                bv[u][2 * t2] = y.x; bv[u][2 * t2 + 1] = y.y;
            }
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int a = 0; a < NA; a++)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    acc[a][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a], bv[u][t], acc[a][t], 0, 0, 0);
    }
    if constexpr (NA == 2) {
        // wave w owns row tile w >> 1 (rows i0 + 2 (lk + 4 rr) + (w >> 1)) x right-hand sides 32 (w & 1) + 2 lm, + 1:
        // W leaves 16 bytes per lane
        splitk_reduce4_pairs(acc, red, wave, lane);
        const int a = wave >> 1, hc = wave & 1;
        const int j = 32 * hc + 2 * lm;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int i = i0 + 2 * (lk + 4 * rr) + a;
            if (i < r && j < nr) {
                double *dst = Ws + (long long)(i - c) * ldx + j;
                const double *tl = Tl + (i - i0) * 64 + j;
                double x0 = 0.0, x1 = 0.0;
#pragma unroll
                for (int aa = 0; aa < 2; aa++)          // (a is wave-uniform; the accumulator index must be a constant)
#pragma unroll
                    for (int h = 0; h < 2; h++)
                        if (aa == a && h == hc) { x0 = tl[0] - acc[aa][2 * h][rr]; x1 = tl[1] - acc[aa][2 * h + 1][rr]; }
                if (j + 1 < nr) *(d2u *)dst = (d2u){x0, x1};
                else dst[0] = x0;
            }
        }
    } else {
        splitk_reduce4<NA>(acc, red, wave, lane);
        // wave w owns column tile w (right-hand sides 32 (w >> 1) + 2 lm + (w & 1))
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t == wave) {
                const int j = 32 * (t >> 1) + 2 * lm + (t & 1);
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const int i = i0 + lk + 4 * rr;
                    if (i < r && j < nr) Ws[(long long)(i - c) * ldx + j] = Tl[(i - i0) * 64 + j] - acc[0][t][rr];
                }
            }
        }
    }
}

// The same update driven by one 128-byte record per 32-row tile (FwdTile, device.h), handed out in one contiguous run per
// XCD like the contribution-block tiles: a tile of a mid-level front is a chain of round trips (front -> geometry ->
// edge records -> tile ranges -> entries -> k-batches), not arithmetic. Here the record arrives in one scalar load, the
// first k-batch and the first child's entries are requested right behind it. Same sums in the same order as
// k_fwd_update_longk<2>.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_fwd_update_rec(DevSym S, const FwdTile *__restrict__ recs, const SyrkSplit split,
                                                        const double *__restrict__ L, const double *__restrict__ X,
                                                        double *__restrict__ W, int nr, int ldx, int cmin) {
    __shared__ double red[3 * 16 * 64];
    __shared__ double Tl[32 * 64];   // children's contributions to this tile of W_s
    const int xcd = blockIdx.x & 7;
    const int tix = split.start[xcd] + (int)(blockIdx.x >> 3);
    if (tix >= split.start[xcd + 1]) return;
    const FwdTile T = recs[tix];
    if (T.c <= cmin) return;
    const int c = T.c, r = T.r, ld = T.ld, i0 = T.i0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const double *P = L + T.pp;
    const double *Yb = X + T.xoff * ldx;
    double *Ws = W + T.woff * ldx;
    // ---- first k-batch of this wave (rows / right-hand sides in pairs, see k_fwd_update_longk)
    const double *pa = P + min(i0 + 2 * lm, r - 1);
    const int jb[2] = {min(2 * lm, nr - 1), min(32 + 2 * lm, nr - 1)};
    constexpr int KU = 4;
    double av[KU][2], bv[KU][4];
    auto request = [&](int k0) {
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int kc = min(k0 + 4 * u + lk, c - 1);
            const d2u x = *(const d2u *)(pa + (long long)kc * ld);
            av[u][0] = x.x; av[u][1] = x.y;
#pragma unroll
            for (int t2 = 0; t2 < 2; t2++) {
                const d2u y = *(const d2u *)(Yb + (long long)kc * ldx + jb[t2]);
                bv[u][2 * t2] = y.x; bv[u][2 * t2 + 1] = y.y;
            }
        }
    };
    const int kfirst = wave * 4 * KU;
    if (kfirst < c) request(kfirst);
    // ---- the children's update vectors for these rows, gathered into LDS in child order
    const int j = lane, g = __builtin_amdgcn_readfirstlane(wave);
    const int jcl = min(j, nr - 1);
    const double jm = j < nr ? 1.0 : 0.0;
    int rt;
    double wv[8];
    auto fetch = [&](const int *reld, const double *Wd, int md, int a0, int a1) {
        rt = reld[min(a0 + j, md - 1)];
        const int na = a1 - a0 - g;                 // this wave's rows: a0 + g + 4 u < a1  <=>  4 u < na
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (4 * u < na) wv[u] = Wd[(long long)(a0 + g + 4 * u) * ldx + jcl];
    };
    auto add = [&](int a0, int a1) {
        const int na = a1 - a0 - g;
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (4 * u < na) {
                const int tr = __builtin_amdgcn_readlane(rt, g + 4 * u);
                if (tr >= i0 && tr < i0 + 32) Tl[(tr - i0) * 64 + j] += wv[u] * jm;
            }
    };
    if (T.nch > 0) fetch(S.rel + T.reloff[0], W + T.cwoff[0] * ldx, T.md[0], T.a0[0], T.a1[0]);
    for (int i = g; i < 32; i += 4) Tl[i * 64 + j] = 0.0;
    __syncthreads();
    if (T.nch > 0) {
        add(T.a0[0], T.a1[0]);
        __syncthreads();
    }
    if (T.nch > 1) {
        fetch(S.rel + T.reloff[1], W + T.cwoff[1] * ldx, T.md[1], T.a0[1], T.a1[1]);
        add(T.a0[1], T.a1[1]);
        __syncthreads();
    }
    for (long long cb = T.ch0 + 2; cb < T.ch0 + T.nch; cb++) {      // further children: the long way
        const EdgeRec er = S.edge[cb];
        const int a0 = S.etile[er.tptr + T.tile], a1 = S.etile[er.tptr + T.tile + 1];
        fetch(S.rel + er.reloff, W + er.woff * ldx, er.md, a0, a1);
        add(a0, a1);
        __syncthreads();
    }
    d4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[a][t] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = kfirst; k0 < c; k0 += 16 * KU) {
        if (k0 > kfirst) request(k0);
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const double mk = (k0 + 4 * u + lk) < c ? 1.0 : 0.0;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    acc[a][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a] * mk, bv[u][t], acc[a][t], 0, 0, 0);
        }
    }
    // wave w owns row tile w >> 1 (rows i0 + 2 (lk + 4 rr) + (w >> 1)) x right-hand sides 32 (w & 1) + 2 lm, + 1
    splitk_reduce4_pairs(acc, red, wave, lane);
    const int a = wave >> 1, hc = wave & 1;
    const int jj = 32 * hc + 2 * lm;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const int i = i0 + 2 * (lk + 4 * rr) + a;
        if (i < r && jj < nr) {
            double *dst = Ws + (long long)(i - c) * ldx + jj;
            const double *tl = Tl + (i - i0) * 64 + jj;
            double x0 = 0.0, x1 = 0.0;
#pragma unroll
            for (int aa = 0; aa < 2; aa++)
#pragma unroll
                for (int h = 0; h < 2; h++)
                    if (aa == a && h == hc) { x0 = tl[0] - acc[aa][2 * h][rr]; x1 = tl[1] - acc[aa][2 * h + 1][rr]; }
            if (jj + 1 < nr) *(d2u *)dst = (d2u){x0, x1};
            else dst[0] = x0;
        }
    }
}

// (Measured and dropped, round 5: the same update with ONE WAVE per record, no LDS and no barrier -- the children's rows entering
//  through the matrix pipe as k-steps against an indicator operand (-1 at the target row), sixteen independent chains per CU
//  instead of three. Forward sweep of cfg 2: 1.96 ms with this kernel, 1.89-1.91 with the wave form on the levels of >= 2 500-6 000
//  tiles: the mid levels already move their bytes -- panel rows, W written once and read once -- at ~4.5 TB/s; what is left is
//  the hand-off of W itself. And its sums round differently from k_fwd_update_longk's, which the sharded rehearsal compares bit for bit.)

// Passes of at most 16 right-hand sides (the single solve, the Newton step): the update of fronts up to `cmax` columns wide with
// ONE WAVE per record, no LDS and no barrier. The 64-column kernels above spend a 1-column pass on the same chain of round trips
// with a barrier between any two of them, three workgroups per CU: 0.71 of the 2.84 ms of a single-RHS solve of cfg 2 went there.
// Here a wave owns the 32 rows x 16 right-hand sides of a record for the whole K range, and the children's update vectors enter
// THROUGH THE MATRIX PIPE: a child row that lands on tile row i is one more k-step whose first operand is the indicator (-1 at
// row i, 0 elsewhere) and whose second operand is the child's row -- the accumulator ends as L21 y - (children), every child row
// added exactly once (a product with 0 adds an exact 0), children in edge order, rows in order: reproducible, and the same for a
// front whatever the level list it comes in (sharded or not). Eight independent chains per SIMD.
// Wider fronts (the top of the tree: K in the hundreds to thousands over a handful of tiles) keep the split-K kernels (cmin).
// NW = 4 (levels with fronts wider than kWaveSplitCols columns): the K range of such a front's tile is split over four waves -- a
// chain of up to 16 dependent batches otherwise --, their partial tiles summed in wave order through 8 KB of LDS; narrower fronts of
// the same launch are still done by wave 0 alone (the rule depends on the front's width only: its sums do not depend on the launch).
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_fwd_update_wave(DevSym S, const FwdTile *__restrict__ recs, const SyrkSplit split,
                                                        const double *__restrict__ L, const double *__restrict__ X,
                                                        double *__restrict__ W, int nr, int ldx, int cmax) {
    __shared__ double red[NW > 1 ? NW * 8 * 64 : 1];
    // (round 6) blockIdx.y = 16-column tile of the right-hand sides: a pass of 17 .. 32 columns runs these kernels on two tiles
    { const int jt = 16 * blockIdx.y; X += jt; W += jt; nr = min(nr - jt, 16); }
    const int xcd = blockIdx.x & 7;
    const int tix = split.start[xcd] + (int)(blockIdx.x >> 3);
    if (tix >= split.start[xcd + 1]) return;
    const FwdTile T = recs[tix];
    const int c = T.c, r = T.r, ld = T.ld, i0 = T.i0;
    if (c > cmax) return;
    const int wave = NW > 1 ? (int)(threadIdx.x >> 6) : 0;
    const int kw = (NW > 1 && c > kWaveSplitCols) ? NW : 1;       // waves that share this tile's K range
    if (wave >= kw) return;
    const int lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const double *P = L + T.pp;
    const double *Yb = X + T.xoff * ldx;
    double *Ws = W + T.woff * ldx;
    const double *pa = P + min(i0 + 2 * lm, r - 1);       // rows in pairs: MFMA row lm of row tile 0 / 1 = tile row 2 lm / 2 lm + 1
    const int jl = min(lm, nr - 1);
    constexpr int KU = 8;
    d4 acc[2] = {(d4){0.0, 0.0, 0.0, 0.0}, (d4){0.0, 0.0, 0.0, 0.0}};
    for (int k0 = wave * 4 * KU; k0 < c; k0 += kw * 4 * KU) {
        double av[KU][2], bv[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int kk = k0 + 4 * u + lk;
            const int kc = min(kk, c - 1);
            const double mk = kk < c ? 1.0 : 0.0;
            const d2u x = *(const d2u *)(pa + (long long)kc * ld);
            av[u][0] = x.x * mk; av[u][1] = x.y * mk;
            bv[u] = Yb[(long long)kc * ldx + jl];
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
            if (k0 + 4 * u < c) {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][0], bv[u], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][1], bv[u], acc[1], 0, 0, 0);
            }
    }
    const int myrow = i0 + 2 * lm;
    auto child = [&](const int *__restrict__ reld, const double *__restrict__ Wd, int a0, int a1) {
        for (int b0 = a0; b0 < a1; b0 += 4 * KU) {
            double sv[KU][2], wv[KU];
#pragma unroll
            for (int u = 0; u < KU; u++) {
                const int row = b0 + 4 * u + lk;
                const int rc = min(row, a1 - 1);
                const int d = reld[rc] - myrow;
                const bool ok = row < a1;
                sv[u][0] = (ok && d == 0) ? -1.0 : 0.0;
                sv[u][1] = (ok && d == 1) ? -1.0 : 0.0;
                wv[u] = Wd[(long long)rc * ldx + jl];
            }
#pragma unroll
            for (int u = 0; u < KU; u++)
                if (b0 + 4 * u < a1) {
                    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(sv[u][0], wv[u], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(sv[u][1], wv[u], acc[1], 0, 0, 0);
                }
        }
    };
    if (wave == 0) {
        if (T.nch > 0) child(S.rel + T.reloff[0], W + T.cwoff[0] * ldx, T.a0[0], T.a1[0]);
        if (T.nch > 1) child(S.rel + T.reloff[1], W + T.cwoff[1] * ldx, T.a0[1], T.a1[1]);
        for (long long cb = T.ch0 + 2; cb < T.ch0 + T.nch; cb++) {      // further children: the long way
            const EdgeRec er = S.edge[cb];
            const int a0 = S.etile[er.tptr + T.tile], a1 = S.etile[er.tptr + T.tile + 1];
            child(S.rel + er.reloff, W + er.woff * ldx, a0, a1);
        }
    }
    if constexpr (NW > 1) {
        if (kw > 1) {       // (all NW waves of the workgroup are here: none has left)
            if (wave > 0) {
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) red[(wave * 8 + a * 4 + rr) * 64 + lane] = acc[a][rr];
            }
            __syncthreads();
            if (wave > 0) return;
#pragma unroll
            for (int w = 1; w < NW; w++)
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) acc[a][rr] += red[(w * 8 + a * 4 + rr) * 64 + lane];
        }
    }
    // W = -(acc): lane (lm, lk), register rr of row tile a = row i0 + 2 (lk + 4 rr) + a, right-hand side lm
    if (lm < nr) {
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int i = i0 + 2 * (lk + 4 * rr) + a;
                if (i < r) Ws[(long long)(i - c) * ldx + lm] = -acc[a][rr];
            }
    }
}

// Blocked forward substitution inside a front wider than `cap` columns: after y_blk = X_blk b_blk, the own rows
// below the block get  b[i] -= sum_{q in block} L[i][q] y[q].  A workgroup owns 32 rows x 64 right-hand sides,
// its four waves split the K range (the block's columns); the partial tiles are summed through LDS.
__global__ __launch_bounds__(256) void k_fwd_own_update(DevSym S, const int *__restrict__ list,
                                                        const double *__restrict__ L, const double *__restrict__ Y,
                                                        double *__restrict__ X, int nr, int ldx, int blk, int cap) {
    __shared__ double red[3 * 16 * 64];
    const int s = list[blockIdx.y];
    const int c = S.sfirst[s + 1] - S.sfirst[s];
    const int q0 = blk * cap, q1 = min(c, (blk + 1) * cap);     // K range: the block's columns
    const int i0 = q1 + blockIdx.x * 32;                        // own rows below the block
    if (i0 >= c) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const int ld = S.ld[s];
    const int first = S.sfirst[s];
    const double *P = L + S.panelptr[s];
    const double *Yb = Y + (long long)first * ldx;
    double *Xb = X + (long long)first * ldx;
    const int nt = (nr + 15) >> 4;
    d4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[a][t] = (d4){0.0, 0.0, 0.0, 0.0};
    const double *pa[2] = {P + min(i0 + lm, c - 1), P + min(i0 + 16 + lm, c - 1)};
    const int jc[4] = {min(lm, nr - 1), min(16 + lm, nr - 1), min(32 + lm, nr - 1), min(48 + lm, nr - 1)};
    constexpr int KU = 4;
    for (int k0 = q0 + wave * 4 * KU; k0 < q1; k0 += 16 * KU) {
        double av[KU][2], bv[KU][4];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int kk = k0 + 4 * u + lk;
            const int kc = min(kk, q1 - 1);
            const double mk = kk < q1 ? 1.0 : 0.0;
#pragma unroll
            for (int a = 0; a < 2; a++) av[u][a] = pa[a][(long long)kc * ld] * mk;
#pragma unroll
            for (int t = 0; t < 4; t++) bv[u][t] = Yb[(long long)kc * ldx + jc[t]];
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    acc[a][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a], bv[u][t], acc[a][t], 0, 0, 0);
    }
    splitk_reduce4<2>(acc, red, wave, lane);
    // wave w owns the 16 right-hand sides 16 w .. of both row tiles: X -= acc (loads first, then stores)
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t == wave && t < nt) {
            const int j = t * 16 + lm, jcl = min(j, nr - 1);
            double xv[2][4];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) xv[a][rr] = Xb[(long long)min(i0 + a * 16 + lk + 4 * rr, c - 1) * ldx + jcl];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const int i = i0 + a * 16 + lk + 4 * rr;
                    if (i < c && j < nr) Xb[(long long)i * ldx + j] = xv[a][rr] - acc[a][t][rr];
                }
        }
    }
}

// Passes of at most 16 right-hand sides: t = y - L21' x[trailing rows] of a front with at most `mmax` trailing rows, ONE WAVE per
// 16 own columns for the whole K range -- no LDS, no barrier, a quarter of the registers of the 64-column kernels: eight chains
// per SIMD (k_fwd_update_wave is the forward twin). Operands in pairs along K as in k_bwd_gemm_longk: a lane loads rows q, q + 1
// of its column and of the row list, q = batch + 8 h + 2 lk, and feeds k-steps 2 h and 2 h + 1 with them. The row indices of
// batch k + 1 are requested with the operands of batch k. Fronts with more trailing rows keep the split-K kernels (mmin).
// NW = 4 (levels with fronts of more than kWaveSplitRows trailing rows): four waves share such a front's K range, partial tiles
// summed in wave order through LDS; fronts with fewer rows are still done by wave 0 alone (the rule depends on the front only).
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_bwd_wave(DevSym S, const int *__restrict__ list, const double *__restrict__ L, const double *X,
                                                 double *Xown, int nr, int ldx, int mmax) {
    __shared__ double red[NW > 1 ? NW * 4 * 64 : 1];
    { const int jt = 16 * blockIdx.z; X += jt; Xown += jt; nr = min(nr - jt, 16); }       // (round 6) blockIdx.z = 16-column tile of the right-hand sides
    const int s = list[blockIdx.y];
    const int c = S.sfirst[s + 1] - S.sfirst[s];
    const int r = (int)(S.rowptr[s + 1] - S.rowptr[s]);
    const int i0 = blockIdx.x * 16;
    if (i0 >= c || r <= c || r - c > mmax) return;
    const int wave = NW > 1 ? (int)(threadIdx.x >> 6) : 0;
    const int kw = (NW > 1 && r - c > kWaveSplitRows) ? NW : 1;
    if (wave >= kw) return;
    const int lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const int ld = S.ld[s];
    const int first = S.sfirst[s];
    const double *pa = L + S.panelptr[s] + (long long)min(i0 + lm, c - 1) * ld;
    const int *rows = S.rows + S.rowptr[s];
    const int jl = min(lm, nr - 1);
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
    constexpr int NH = 4;                   // pairs per lane and batch: 8 k-steps = 32 rows
    long long xr[2 * NH], xn[2 * NH];
    auto request_rows = [&](int kb) {
#pragma unroll
        for (int h = 0; h < NH; h++) {
            const int q = kb + 8 * h + 2 * lk;
            const i2u v = *(const i2u *)(rows + min(q, r - 1));
            xn[2 * h] = v.x;
            xn[2 * h + 1] = q + 1 < r ? v.y : v.x;          // past the list: any valid row (its product is masked)
        }
    };
    request_rows(c + wave * 8 * NH);
    for (int k0 = c + wave * 8 * NH; k0 < r; k0 += kw * 8 * NH) {
        double av[2 * NH], bv[2 * NH];
#pragma unroll
        for (int u = 0; u < 2 * NH; u++) xr[u] = xn[u];
        request_rows(k0 + kw * 8 * NH);
#pragma unroll
        for (int h = 0; h < NH; h++) {
            const int q = k0 + 8 * h + 2 * lk;
            const d2u v = *(const d2u *)(pa + min(q, r - 1));
            av[2 * h] = v.x * (q < r ? 1.0 : 0.0); av[2 * h + 1] = v.y * (q + 1 < r ? 1.0 : 0.0);
        }
#pragma unroll
        for (int u = 0; u < 2 * NH; u++) bv[u] = X[xr[u] * ldx + jl];
#pragma unroll
        for (int u = 0; u < 2 * NH; u++)
            if (k0 + 8 * (u >> 1) < r) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
    if constexpr (NW > 1) {
        if (kw > 1) {
            if (wave > 0) {
#pragma unroll
                for (int rr = 0; rr < 4; rr++) red[(wave * 4 + rr) * 64 + lane] = acc[rr];
            }
            __syncthreads();
            if (wave > 0) return;
#pragma unroll
            for (int w = 1; w < NW; w++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) acc[rr] += red[(w * 4 + rr) * 64 + lane];
        }
    }
    // t[col][rhs]: register rr of lane (lm, lk) = own column i0 + lk + 4 rr, right-hand side lm (all loads, then all stores)
    double xv[4];
#pragma unroll
    for (int rr = 0; rr < 4; rr++) xv[rr] = Xown[(long long)(first + min(i0 + lk + 4 * rr, c - 1)) * ldx + jl];
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const int col = i0 + lk + 4 * rr;
        if (col < c && lm < nr) Xown[(long long)(first + col) * ldx + lm] = xv[rr] - acc[rr];
    }
}

// Backward update of a big front: own columns -= L21' * x_R over ALL trailing rows: a
// workgroup owns 64 own columns x 64 right-hand sides, its waves split the trailing rows.
template <int NA, int NW>   // NA: 16-column tiles of own columns per workgroup; NW: waves per workgroup splitting K
__global__ __launch_bounds__(64 * NW) void k_bwd_gemm_longk(DevSym S, const int *__restrict__ list,
                                                          const double *__restrict__ L, const double *X, double *Xown, int nr,
                                                          int ldx, int blk, int cap, int mmin) {
    // blk < 0: all own columns, K = the trailing rows [c, r). blk >= 0 (blocked substitution inside a front wider
    // than `cap` columns): own columns of block blk only, K = the OWN rows below the block, [(blk + 1) cap, c)
    // -- the same product with other bounds (rows[] lists the own columns first, so x of own rows is found the
    // same way as x of trailing rows).
    __shared__ double red[NW == 4 ? 3 * 16 * 64 : NW * 16 * 64];
    const int s = list[blockIdx.y];
    const int cfull = S.sfirst[s + 1] - S.sfirst[s];
    const int rfull = (int)(S.rowptr[s + 1] - S.rowptr[s]);
    const int col0 = blk < 0 ? 0 : blk * cap;
    const int c = blk < 0 ? cfull : min(cfull, (blk + 1) * cap);      // own columns [col0, c); K starts at row c
    const int r = blk < 0 ? rfull : cfull;                             // K ends at row r
    const int i0 = col0 + blockIdx.x * 16 * NA;
    if (i0 >= c || r <= c) return;
    if (blk < 0 && r - c <= mmin) return;       // (narrow passes: k_bwd_wave has the fronts with at most mmin trailing rows)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const int ld = S.ld[s];
    const int first = S.sfirst[s];
    const double *P = L + S.panelptr[s];
    const int *rows = S.rows + S.rowptr[s];
    d4 acc[NA][4];
#pragma unroll
    for (int a = 0; a < NA; a++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[a][t] = (d4){0.0, 0.0, 0.0, 0.0};
    const double *pa[NA];
#pragma unroll
    for (int a = 0; a < NA; a++) pa[a] = P + (long long)min(i0 + a * 16 + lm, c - 1) * ld;
    // Everything in PAIRS (16-byte / 8-byte loads; the CU's address unit is what this kernel keeps busiest):
    //  * the panel along k: a lane loads rows q, q + 1 of its column, q = batch + 8 h + 2 lk, and feeds k-steps 2 h and
    //    2 h + 1 with them (k-step 2 h + e covers rows batch + 8 h + 2 lk + e, lk = 0..3);
    //  * the row indices of those rows the same way;
    //  * x along the right-hand sides: column tile t is right-hand side 32 (t >> 1) + 2 lm + (t & 1).
    // Per batch of 16 rows: 2 NA + 8 + 2 loads instead of 4 NA + 16 + 4.
    // (Round 6, measured and dropped: this loop as a three-stage software pipeline of half-batches -- operands requested two stages
    //  ahead, their row indices three, unconditional requests and scheduling barriers as in k_syrk_cb_rec<true>; 126 / 166 VGPRs for
    //  the <1, 8> / <2, 8> forms, same occupancy, bit-identical. Backward sweep of cfg 2: 1.434-1.441 ms without, 1.434-1.440 with it on
    //  either or both forms. The top-level launches are not a chain of exposed round trips: a level of 126 workgroups puts 2000 MFMAs
    //  on each of 126 compute units -- 13.8 us at the pipe's peak -- while the other half of the chip idles; only spreading a front's
    //  work over more compute units would shorten them.)
    const int jb[2] = {min(2 * lm, nr - 1), min(32 + 2 * lm, nr - 1)};
    constexpr int KU = 4;
    // The row indices of batch k+1 are requested together with the operands of batch k: one round
    // trip per batch instead of two (index -> X row). Long trailing parts (K = r - c up to 2000 at
    // the top of the tree) make this loop a pure latency chain.
    long long xr[KU], xn[KU];
    auto request_rows = [&](int kb) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int q = kb + 8 * h + 2 * lk;
            const i2u v = *(const i2u *)(rows + min(q, r - 1));
            xn[2 * h] = v.x;
            xn[2 * h + 1] = q + 1 < r ? v.y : v.x;          // past the list: any valid row (its product is masked)
        }
    };
    request_rows(c + wave * 4 * KU);
    for (int k0 = c + wave * 4 * KU; k0 < r; k0 += NW * 4 * KU) {
        double av[KU][NA], bv[KU][4];
#pragma unroll
        for (int u = 0; u < KU; u++) xr[u] = xn[u];
        request_rows(k0 + NW * 4 * KU);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int q = k0 + 8 * h + 2 * lk;
            const double m0 = q < r ? 1.0 : 0.0, m1 = q + 1 < r ? 1.0 : 0.0;
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const d2u v = *(const d2u *)(pa[a] + min(q, r - 1));
                av[2 * h][a] = v.x * m0; av[2 * h + 1][a] = v.y * m1;
            }
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int t2 = 0; t2 < 2; t2++) {
                const d2u y = *(const d2u *)(X + xr[u] * ldx + jb[t2]);
                bv[u][2 * t2] = y.x; bv[u][2 * t2 + 1] = y.y;
            }
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int a = 0; a < NA; a++)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    acc[a][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a], bv[u][t], acc[a][t], 0, 0, 0);
    }
    if constexpr (NA == 2 && NW == 4) {
        // wave w owns row tile w >> 1 (own columns i0 + 16 (w >> 1) + lk + 4 rr) x right-hand sides 32 (w & 1) + 2 lm, + 1:
        // x is read and written 16 bytes per lane (all loads, then all stores)
        splitk_reduce4_pairs(acc, red, wave, lane);
        const int a = wave >> 1, hc = wave & 1;
        const int j = 32 * hc + 2 * lm;
        d2u xv[4];
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
            xv[rr] = *(const d2u *)(Xown + (long long)(first + min(i0 + a * 16 + lk + 4 * rr, c - 1)) * ldx + min(j, nr - 1));
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int col = i0 + a * 16 + lk + 4 * rr;
            if (col < c && j < nr) {
                double x0 = 0.0, x1 = 0.0;
#pragma unroll
                for (int aa = 0; aa < 2; aa++)
#pragma unroll
                    for (int h = 0; h < 2; h++)
                        if (aa == a && h == hc) { x0 = xv[rr].x - acc[aa][2 * h][rr]; x1 = xv[rr].y - acc[aa][2 * h + 1][rr]; }
                double *dst = Xown + (long long)(first + col) * ldx + j;
                if (j + 1 < nr) *(d2u *)dst = (d2u){x0, x1};
                else dst[0] = x0;
            }
        }
    } else {
        if (NW == 4) splitk_reduce4<NA>(acc, red, wave, lane);
        else {
#pragma unroll
            for (int a = 0; a < NA; a++) {
                if (a > 0) __syncthreads();         // (the buffer of the partial tiles is reused)
                splitk_reduce_nw<NW>(acc[a], red, wave, lane);
            }
        }
        // X -= acc in two passes (all loads, then all stores: one round trip instead of a chain of 8)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t == wave) {
                const int j = 32 * (t >> 1) + 2 * lm + (t & 1);
                const int jcl = min(j, nr - 1);
                double xv[NA][4];
#pragma unroll
                for (int a = 0; a < NA; a++)
#pragma unroll
                    for (int rr = 0; rr < 4; rr++)
                        xv[a][rr] = Xown[(long long)(first + min(i0 + a * 16 + lk + 4 * rr, c - 1)) * ldx + jcl];
#pragma unroll
                for (int a = 0; a < NA; a++)
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) {
                        const int col = i0 + a * 16 + lk + 4 * rr;
                        if (col < c && j < nr) Xown[(long long)(first + col) * ldx + j] = xv[a][rr] - acc[a][t][rr];
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Right-hand-side permutation + transposition (column-major caller layout <-> row-major X)
// ------------------------------------------------------------------------------------------
// dir 0: X[k, j] = B[perm[k] + j*ldb]   (perm == nullptr: identity)
// dir 1: B[perm[k] + j*ldb] = X[k, j]
__global__ __launch_bounds__(256) void k_permute(const int *__restrict__ iperm, int n, double *__restrict__ Bc,
                                                 long long ldb, double *__restrict__ X, int nr, int ldx, int dir) {
    // Caller side: column-major n x nr (a DoF is strided by ldb); solver side: row-major, one DoF =
    // one contiguous 8 nr-byte row, in elimination order. A workgroup owns 64 consecutive ORIGINAL
    // rows i: the caller side is then read / written in 512-byte runs per column and the solver side
    // one whole row (iperm[i]) at a time -- both sides coalesced, the 64 x 64 transpose goes through
    // LDS. (Walking the elimination order instead and gathering caller rows perm[k] costs 2.7x the
    // bytes in partially used 64-byte sectors.) iperm == nullptr: identity.
    __shared__ double T[64 * 65];
    __shared__ int rowL[64];
    const int i0 = blockIdx.x * 64;
    const int tid = threadIdx.x;
    const int a = tid & 63, b = tid >> 6;
    if (tid < 64) rowL[tid] = (i0 + tid < n) ? (iperm ? iperm[i0 + tid] : i0 + tid) : 0;
    // all 16 loads of a thread are issued before the first use (clamped addresses, predicated stores): the kernel only
    // moves bytes, and a load -> LDS store -> load chain leaves 15 of every 16 round trips idle
    double v[16];
    if (dir == 0) {
        const int i = i0 + a, ic = min(i, n - 1);
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = Bc[ic + (long long)min(b + 4 * u, nr - 1) * ldb];
#pragma unroll
        for (int u = 0; u < 16; u++) T[a * 65 + b + 4 * u] = v[u];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int kk = b + 4 * u;
            if (i0 + kk < n && a < nr) X[(long long)rowL[kk] * ldx + a] = T[kk * 65 + a];
        }
    } else {
        __syncthreads();
        const int ac = min(a, nr - 1);
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = X[(long long)rowL[b + 4 * u] * ldx + ac];
#pragma unroll
        for (int u = 0; u < 16; u++) T[(b + 4 * u) * 65 + a] = v[u];
        __syncthreads();
        const int i = i0 + a;
        if (i < n) {
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (b + 4 * u < nr) Bc[i + (long long)(b + 4 * u) * ldb] = T[a * 65 + b + 4 * u];
        }
    }
}
// The same for passes of at most 8 right-hand sides (the single solve): a thread per ORIGINAL row -- the caller side coalesced, the
// solver side 8 nr-byte pieces. The 64 x 64 transpose above spends 60 + 41 us on a 1-column pass of 10^6 rows (15 625 workgroups
// of which one column in 64 carries data); this one 8 + 8.
__global__ __launch_bounds__(256) void k_permute_narrow(const int *__restrict__ iperm, int n, double *__restrict__ Bc,
                                                        long long ldb, double *__restrict__ X, int nr, int ldx, int dir) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long row = iperm ? iperm[i] : i;
    double v[8];
    if (dir == 0) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = Bc[i + (long long)min(j, nr - 1) * ldb];
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j < nr) X[row * ldx + j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = X[row * ldx + min(j, nr - 1)];
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j < nr) Bc[i + (long long)j * ldb] = v[j];
    }
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
void launch_fwd_assemble(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, double *X,
                         const double *W, int nr, int ldx) {
    if (nfronts <= 0 || max_cols <= 0) return;
    hipLaunchKernelGGL(k_fwd_assemble, dim3(odd(cdiv(max_cols, FWD_RB)), nfronts), dim3(256), 0, st, S, list, X, W, nr, ldx);
}
void launch_fwd_update(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_trail, const double *L,
                       double *X, double *W, int nr, int ldx, int cmin) {
    const Launch c = choose_fwd_update(nfronts, max_trail);
    if (c.variant == kFwdUpdate16) GMRFX_LAUNCH(k_fwd_update_longk<1>, c, st, S, list, L, X, W, nr, ldx, cmin);
    else if (c.variant == kFwdUpdate32) GMRFX_LAUNCH(k_fwd_update_longk<2>, c, st, S, list, L, X, W, nr, ldx, cmin);
}
void launch_fwd_update_recs(hipStream_t st, const DevSym &S, const FwdTile *recs, const SyrkSplit &split, int per_xcd, const double *L,
                            double *X, double *W, int nr, int ldx, int cmin) {
    if (per_xcd <= 0) return;
    hipLaunchKernelGGL(k_fwd_update_rec, dim3(8 * (unsigned)per_xcd), dim3(256), 0, st, S, recs, split, L, X, W, nr, ldx, cmin);
}
void launch_fwd_update_wave(hipStream_t st, const DevSym &S, const FwdTile *recs, const SyrkSplit &split, int per_xcd, const double *L,
                            double *X, double *W, int nr, int ldx, int cmax, bool split_k) {
    const Launch c = choose_fwd_update_wave(per_xcd, nr, split_k);
    if (c.variant == kWaveSplitK) GMRFX_LAUNCH(k_fwd_update_wave<4>, c, st, S, recs, split, L, X, W, nr, ldx, cmax);
    else if (c.variant == kWaveWhole) GMRFX_LAUNCH(k_fwd_update_wave<1>, c, st, S, recs, split, L, X, W, nr, ldx, cmax);
}
void launch_bwd_gemm(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, const double *L,
                     const double *X, double *Xown, int nr, int ldx, int blk, int cap, int mmin) {
    const Launch c = choose_bwd_gemm(nfronts, max_cols, blk, cap);
    switch (c.variant) {
    case kBwdGemm32x8: GMRFX_LAUNCH((k_bwd_gemm_longk<2, 8>), c, st, S, list, L, X, Xown, nr, ldx, blk, cap, mmin); break;
    case kBwdGemm16x8: GMRFX_LAUNCH((k_bwd_gemm_longk<1, 8>), c, st, S, list, L, X, Xown, nr, ldx, blk, cap, mmin); break;
    case kBwdGemm32x4: GMRFX_LAUNCH((k_bwd_gemm_longk<2, 4>), c, st, S, list, L, X, Xown, nr, ldx, blk, cap, mmin); break;
    default: break;
    }
}
void launch_bwd_wave(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, const double *L, const double *X, double *Xown,
                     int nr, int ldx, int mmax, bool split_k) {
    const Launch c = choose_bwd_wave(nfronts, max_cols, nr, split_k);
    if (c.variant == kWaveSplitK) GMRFX_LAUNCH(k_bwd_wave<4>, c, st, S, list, L, X, Xown, nr, ldx, mmax);
    else if (c.variant == kWaveWhole) GMRFX_LAUNCH(k_bwd_wave<1>, c, st, S, list, L, X, Xown, nr, ldx, mmax);
}
void launch_fwd_own_update(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, const double *L,
                           const double *Y, double *X, int nr, int ldx, int blk, int cap) {
    const Launch c = choose_fwd_own_update(nfronts, max_cols, blk, cap);
    if (c.variant == kFwdOwnUpdate) GMRFX_LAUNCH(k_fwd_own_update, c, st, S, list, L, Y, X, nr, ldx, blk, cap);
}
void launch_permute(hipStream_t st, const int *perm, int n, double *Bc, long long ldb, double *X, int nr, int ldx, int dir) {
    const Launch c = choose_permute(n, nr);
    if (c.variant == kPermuteNarrow) GMRFX_LAUNCH(k_permute_narrow, c, st, perm, n, Bc, ldb, X, nr, ldx, dir);
    else if (c.variant == kPermuteTiles) GMRFX_LAUNCH(k_permute, c, st, perm, n, Bc, ldb, X, nr, ldx, dir);
}

}  // namespace gmrfx
