// factor_kernels.hip -- HIP kernels (gfx950 / CDNA4) of the numeric factorisation of the multifrontal supernodal Cholesky: assembly,
// the panel chain below the diagonal block (TRSM, GEMM), the contribution-block SYRKs, the 128 x 128 tile of huge fronts; their
// launch wrappers (the variant and geometry of a launch: choose_*, device_plan.h). Memory layout and MFMA maps: kernel_common.h.
#include <climits>

#include "kernel_common.h"

namespace gmrfx {

// ------------------------------------------------------------------------------------------
// Factorisation
// ------------------------------------------------------------------------------------------

// Zero the panel, scatter Q's values, extend-add the children's contribution blocks.
// ONE WAVE owns one front-local column (workgroup (bx, f) = columns 4 bx .. 4 bx + 3 of front f):
// every target entry has exactly one owner, which applies the children one after the other, so
// the sum order is fixed (bit-reproducible, no atomics) and no barrier is needed at all; the
// kernel is a chain of dependent HBM round trips, kept short by the wave-wide searches.
template <int WIDE>   // 0: one WAVE per column; 1: one WORKGROUP per column (levels with a few tall fronts)
__global__ __launch_bounds__(256) void k_assemble(DevSym S, const int *__restrict__ list,
                                                  const double *__restrict__ nzval, double *__restrict__ L,
                                                  double *__restrict__ CB, int cyc_w, int cyc_r, int cyc_compact) {
    // PANEL part of the front only (front-local columns < c). The contribution-block part is
    // assembled inside k_syrk_cb (children gathered into an LDS tile, CB written exactly once).
    // WIDE: a column of a top-of-tree front has thousands of rows and the level only has a handful
    // of fronts -- the whole workgroup shares one column (a quarter of the dependent round trips
    // per wave); the phases are then separated by barriers (different waves touch the same rows).
    constexpr int NL = WIDE ? 256 : 64;          // lanes cooperating on one column
    const int s = list[blockIdx.y];
    const int c = S.sfirst[s + 1] - S.sfirst[s];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tl = WIDE ? (int)threadIdx.x : lane;
    const int tc = WIDE ? (int)blockIdx.x : blockIdx.x * ASM_CW + __builtin_amdgcn_readfirstlane(wave);
    if (tc >= c) return;
    // distributed root (cyc_w > 0): this rank assembles the 256-column blocks it owns, block b on rank b mod cyc_w
    if (cyc_w > 0 && (tc >> 8) % cyc_w != cyc_r) return;
    const int ld = S.ld[s];
    // block-cyclic STORAGE (cyc_compact; round 6): this rank keeps only its own 256-column blocks of the front, one behind the
    // other -- block b at local position b / cyc_w: column tc sits 256 (b - b / cyc_w) columns further down than in the full panel
    const int tcs = cyc_compact ? tc - 256 * ((tc >> 8) - (tc >> 8) / cyc_w) : tc;
    double *Pc = L + S.panelptr[s] + (long long)tcs * ld;
    for (int i = 2 * tl; i < ld; i += 2 * NL) *(d2u *)(Pc + i) = (d2u){0.0, 0.0};      // ld is even
    if (WIDE) __syncthreads();
    {   // Q's entries of this column: [qcolptr[k], qcolptr[k + 1]) for column k of L (no search)
        const int gk = S.sfirst[s] + tc;
        const int lo = S.qcolptr[gk], hi = S.qcolptr[gk + 1];
        for (int q = lo + tl; q < hi; q += NL) Pc[S.qdst[q]] = nzval[S.qsrc[q]];
    }
    if (WIDE) __syncthreads();
    for (long long ch = S.childptr[s]; ch < S.childptr[s + 1]; ch++) {
        const EdgeRec er = S.edge[ch];
        const int md = er.md;
        const int *reld = S.rel + er.reloff;
        const int j = S.erow[er.eoff + tc];       // the child's row that maps to column tc (table, no search)
        if (j < 0) continue;                      // none (workgroup-uniform)
        const double *Uc = CB + er.cboff + (long long)j * md;
        // four independent row chunks in flight per lane (rel -> P read-modify-write chain; row pairs per lane as in
        // k_assemble_lds were measured slower here: the scattered read-modify-write of P is the long pole, not the loads)
        for (int i0 = j + tl; i0 < md; i0 += 4 * NL) {
            int ri[4];
            double u[4], pv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) ri[q] = reld[min(i0 + NL * q, md - 1)];
#pragma unroll
            for (int q = 0; q < 4; q++) u[q] = Uc[min(i0 + NL * q, md - 1)];
#pragma unroll
            for (int q = 0; q < 4; q++) pv[q] = Pc[ri[q]];
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (i0 + NL * q < md) Pc[ri[q]] = pv[q] + u[q];
        }
        if (WIDE) __syncthreads();
    }
}

// Write-once assembly for fronts whose columns fit in LDS (all but the top levels): one wave builds
// its column in LDS -- zero, Q's values, the children's contributions in fixed order -- and stores it
// to HBM ONCE. The HBM version above zero-fills the panel and then read-modify-writes it per child
// (measured: k_assemble moved 6.5 GB per step and ran at ~4.6 TB/s, i.e. HBM bound on bytes it need
// not move). Same summation order, bit-identical panels. Dynamic LDS: 4 * ldmax doubles.
template <int WIDE>   // 0: one WAVE per column (four columns per workgroup); 1: one WORKGROUP per column (tall columns: top of the tree)
__global__ __launch_bounds__(256) void k_assemble_lds(DevSym S, const AsmRec *__restrict__ arec,
                                                      const double *__restrict__ nzp, double *__restrict__ L,
                                                      const double *__restrict__ CB, int ldmax) {
    extern __shared__ double col_lds[];
    constexpr int NL = WIDE ? 256 : 64, PW = 2 * NL;       // lanes on one column; rows one pair-load of all of them covers
    const AsmRec R = arec[blockIdx.y];                     // the front and its first two children: one scalar load
    const int c = R.c;
    const int wave = threadIdx.x >> 6;
    const int lane = WIDE ? (int)threadIdx.x : (int)(threadIdx.x & 63);         // position among the column's lanes
    const int tc = WIDE ? (int)blockIdx.x : blockIdx.x * ASM_CW + __builtin_amdgcn_readfirstlane(wave);
    if (tc >= c) return;
    const int ld = R.ld;
    double *Cw = WIDE ? col_lds : col_lds + wave * ldmax;
    double *Pc = L + R.pp + (long long)tc * ld;
    // A column is a chain of dependent round trips (front -> Q's range / child records -> the child's row -> entries): everything
    // the FIRST TWO children and Q's first 64 entries need is requested before any of it is used -- records and rows of both
    // children side by side, then all entry loads -- and only then does the column build up in LDS, in the old order (zero, Q,
    // child by child): same bits, three round trips (record | Q's range, the children's rows | entries and Q's values) instead of nine.
    const int nch = R.nch;
    const long long ch0 = R.ch0, ch1 = ch0 + nch;
    const int gk = R.first + tc;
    const int qlo = S.qcolptr[gk], qhi = S.qcolptr[gk + 1];
    struct { int md; long long reloff, cboff; } er[2] = {{R.md[0], R.reloff[0], R.cboff[0]}, {R.md[1], R.reloff[1], R.cboff[1]}};
    int jj[2] = {-1, -1};
#pragma unroll
    for (int q = 0; q < 2; q++)
        if (q < nch) jj[q] = S.erow[R.eoff[q] + tc];        // the child's row that maps to column tc (table, no search); < 0: none
    int qd0 = 0;
    double qv0 = 0.0;
    if (qlo + lane < qhi) { qd0 = S.qdst[qlo + lane]; qv0 = nzp[qlo + lane]; }        // (values in assembly order: no index in between)
    // (WIDE: the waves of the workgroup touch the same rows: a barrier between the phases; rows are distinct within a phase)
    // Rows in PAIRS per lane (one 16-byte value load + one 8-byte index load cover 128 rows of the column), four
    // chunks in flight, and chunks past the end of the child's column issue nothing: the kernel is bound by the
    // CU's address unit (a vector memory instruction costs it ~16 cycles whatever its lanes do), not by HBM.
    // The pair that starts at the last row reads one element past the column: the next column, or the 16 bytes of
    // slack every device array ends in (Device::dalloc); never used.
    i2u ri[2][4];
    d2u u[2][4];
#pragma unroll
    for (int q = 0; q < 2; q++)
        if (jj[q] >= 0) {
            const int md = er[q].md;
            const int *reld = S.rel + er[q].reloff;
            const double *Uc = CB + er[q].cboff + (long long)jj[q] * md;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (jj[q] + PW * k < md) {
                    const int ic = min(jj[q] + PW * k + 2 * lane, md - 1);
                    ri[q][k] = *(const i2u *)(reld + ic);
                    u[q][k] = *(const d2u *)(Uc + ic);
                }
        }
    for (int i = lane; i < ld; i += NL) Cw[i] = 0.0;
    if (WIDE) __syncthreads();
    // Q's entries of this column: [qcolptr[k], qcolptr[k + 1]) for column k of L (no search)
    if (qlo + lane < qhi) Cw[qd0] = qv0;
    for (int q = qlo + NL + lane; q < qhi; q += NL) Cw[S.qdst[q]] = nzp[q];
    if (WIDE) __syncthreads();
    auto chunk = [&](const int *reld, const double *Uc, int md, int base) {
        i2u r2[4];
        d2u u2[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (base + PW * k < md) {
                const int ic = min(base + PW * k + 2 * lane, md - 1);
                r2[k] = *(const i2u *)(reld + ic);
                u2[k] = *(const d2u *)(Uc + ic);
            }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (base + PW * k < md) {
                const int i = base + PW * k + 2 * lane;
                if (i < md) Cw[r2[k].x] += u2[k].x;          // distinct rows within a child: no conflicts
                if (i + 1 < md) Cw[r2[k].y] += u2[k].y;
            }
    };
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (jj[q] >= 0) {
            const int md = er[q].md;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (jj[q] + PW * k < md) {
                    const int i = jj[q] + PW * k + 2 * lane;
                    if (i < md) Cw[ri[q][k].x] += u[q][k].x;
                    if (i + 1 < md) Cw[ri[q][k].y] += u[q][k].y;
                }
            const int *reld = S.rel + er[q].reloff;
            const double *Uc = CB + er[q].cboff + (long long)jj[q] * md;
            for (int base = jj[q] + 4 * PW; base < md; base += 4 * PW) chunk(reld, Uc, md, base);
        }
        if (WIDE && q < nch) __syncthreads();
    }
    for (long long ch = ch0 + 2; ch < ch1; ch++) {          // further children: one at a time
        const EdgeRec e3 = S.edge[ch];
        const int md = e3.md;
        const int *reld = S.rel + e3.reloff;
        const int j = S.erow[e3.eoff + tc];
        if (j >= 0) {
            const double *Uc = CB + e3.cboff + (long long)j * md;
            for (int base = j; base < md; base += 4 * PW) chunk(reld, Uc, md, base);
        }
        if (WIDE) __syncthreads();
    }
    for (int i = 2 * lane; i < ld; i += PW) *(d2u *)(Pc + i) = (d2u){Cw[i], Cw[i + 1]};      // ld is even
}

// Panel rows below the diagonal block as a GEMM with the inverted block (FP64 MFMA):
//   mode 0 (factorisation):      A[i, blk] <- A[i, blk] * Linv'      (in place, = L21 rows)
//   mode 1 (selected inversion): Yh[i, :]  <- L[i, blk] * Linv
// One wave owns 16 rows (reads all of them before it writes), a workgroup 64 rows.
template <int MODE, int SPLIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_trsm(DevSym S, const FrontView *__restrict__ frec, int kb,
                                              double *__restrict__ L, double *__restrict__ Yh,
                                              const long long *__restrict__ yoff, FrontArg fa) {
    // SPLIT = 0: a workgroup owns 128 rows, each wave 32 of them (all four 16-column tiles) as 16 row PAIRS: MFMA
    // row lm of tile 0 / 1 is row 2 lm / 2 lm + 1 of the wave's 32, so one 16-byte load per lane and k-step feeds both
    // tiles and the results leave 16 bytes at a time (half the vector memory instructions, half the LDS reads and half
    // the stagings of the inverse block per row; the kernel streams the block column once in, once out);
    // SPLIT = 1 (latency variant for levels with a handful of fronts): a workgroup owns 16 rows
    // and each wave ONE column tile of them -- many more workgroups, a quarter of the MFMA
    // chain per wave (a single CU sustains only ~0.14 TFLOP/s of FP64 MFMA).
    __shared__ double Ti[NB * NB];
    const FrontView fv = front_view(frec, blockIdx.y, fa);
    const int s = fv.s, c = fv.c, r = fv.r;
    if (kb >= c) return;
    const int w = min(NB, c - kb);
    const int row0 = kb + w + blockIdx.x * (SPLIT ? 16 : 128);
    if (row0 >= r) return;
    const int ld = fv.ld;
    double *Pp = L + fv.pp;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const double *A = Pp + (long long)kb * ld;
    double *out = MODE == 0 ? Pp + (long long)kb * ld : Yh + yoff[s];
    const int ldo = MODE == 0 ? ld : r;
    // Linv is lower triangular: MODE 0 (A Linv') needs q <= k, MODE 1 (L Linv) needs q >= k
    if (SPLIT) {
        const int i0 = row0;
        const int i = i0 + lm;
        const double *pa = A + min(i, r - 1);
        // this wave's rows of the block column are requested BEFORE the inverse block is staged: the two global
        // round trips of this latency-bound kernel overlap instead of following each other
        double bv[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int q = 4 * u + lk;
            bv[u] = pa[(long long)min(q, w - 1) * ld];   // B[kk=q][n=i]; Ti is zero for q >= w, rows >= r never stored
        }
        stage_linv(Pp + kb + (long long)kb * ld, ld, w, Ti, threadIdx.x);
        __syncthreads();
        const int t = wave;
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
        const int k = t * 16 + lm;
        const int ulo = MODE == 0 ? 0 : 4 * t, uhi = MODE == 0 ? 4 * t + 4 : 16;
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int q = 4 * u + lk;                                             // A[m=k][kk=q]
            const double av = MODE == 0 ? Ti[k * NB + q] : Ti[q * NB + k];
            if (u >= ulo && u < uhi && 4 * u < w) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u], acc, 0, 0, 0);
        }
        __syncthreads();   // in place: the other waves read the columns this wave overwrites
        if (i >= r) return;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int kk = t * 16 + lk + 4 * rr;
            if (kk < w) out[i + (long long)kk * ldo] = acc[rr];
        }
    } else {
        const int i0 = row0 + wave * 32;
        const int i = i0 + 2 * lm;                     // this lane's row pair: i, i + 1
        // (lanes past the last row re-read the last row's pair; its second half is padding, the next column's first
        //  entry or the slack behind the array -- never stored)
        const double *pa = A + min(i, r - 1);
        d2u bv[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int q = 4 * u + lk;
            bv[u] = *(const d2u *)(pa + (long long)min(q, w - 1) * ld);
        }
        stage_linv(Pp + kb + (long long)kb * ld, ld, w, Ti, threadIdx.x);
        __syncthreads();
        if (i0 >= r) return;
        d4 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int t = 0; t < 4; t++) acc[a][t] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int q = 4 * u + lk;
            if (4 * u < w) {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (MODE == 0 ? (u <= 4 * t + 3) : (u >= 4 * t)) {
                        const int k = t * 16 + lm;                                    // A[m=k][kk=q]
                        const double av = MODE == 0 ? Ti[k * NB + q] : Ti[q * NB + k];
                        acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u].x, acc[0][t], 0, 0, 0);
                        acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u].y, acc[1][t], 0, 0, 0);
                    }
                }
            }
        }
        if (i >= r) return;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int k = t * 16 + lk + 4 * rr;
                if (k < w) {
                    double *dst = out + i + (long long)k * ldo;
                    if (i + 1 < r) *(d2u *)dst = (d2u){acc[0][t][rr], acc[1][t][rr]};
                    else dst[0] = acc[0][t][rr];
                }
            }
    }
}

// The same product for blocks at most 32 columns wide (the panels of the wide levels of the tree: thousands of narrow fronts per
// launch). The general kernel holds 16 k-steps of operands and 8 accumulator tiles per wave and lives on three waves per SIMD;
// half of that is never used here. 8 k-steps, 4 tiles, an 8 KB inverse block: five to six waves per SIMD. The k-steps that exist
// are issued in the same order with the same operands: the same bits.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_trsm_narrow(const FrontView *__restrict__ frec, int kb, double *__restrict__ L) {
    constexpr int W = 32;
    __shared__ double Ti[W * W];
    const FrontView fv = front_view(frec, blockIdx.y, FrontArg{0, 0, 0, 0, 0, 0, 0});
    const int c = fv.c, r = fv.r;
    if (kb >= c) return;
    const int w = min(NB, c - kb);          // <= 32 by the launch's contract
    const int row0 = kb + w + blockIdx.x * 128;
    if (row0 >= r) return;
    const int ld = fv.ld;
    double *Pp = L + fv.pp;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lm = lane & 15, lk = lane >> 4;
    double *A = Pp + (long long)kb * ld;
    const int i0 = row0 + wave * 32;
    const int i = i0 + 2 * lm;                     // this lane's row pair: i, i + 1
    const double *pa = A + min(i, r - 1);
    d2u bv[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int q = 4 * u + lk;
        bv[u] = *(const d2u *)(pa + (long long)min(q, w - 1) * ld);
    }
    {   // the inverse block: Ti[k * W + q] = Linv[k][q] (stored transposed in the strict upper triangle; diag = 1 / L[k][k])
        const double *Dg = Pp + kb + (long long)kb * ld;
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = threadIdx.x + 256 * u;
            const int q = idx % W, k = idx / W;
            const int qq = min(q, w - 1), kk = min(k, w - 1);
            v[u] = Dg[min(qq, kk) + (long long)max(qq, kk) * ld];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = threadIdx.x + 256 * u;
            const int q = idx % W, k = idx / W;
            const double mk = (k < w && q < k) ? 1.0 : 0.0;
            double x = v[u] * mk;
            if (q == k && k < w) x = fast_rcp(v[u]);
            Ti[k * W + q] = x;
        }
    }
    __syncthreads();
    if (i0 >= r) return;
    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int t = 0; t < 2; t++) acc[a][t] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int q = 4 * u + lk;
        if (4 * u < w) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if (u <= 4 * t + 3) {
                    const int k = t * 16 + lm;                                    // A[m=k][kk=q]
                    const double av = Ti[k * W + q];
                    acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u].x, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u].y, acc[1][t], 0, 0, 0);
                }
            }
        }
    }
    if (i >= r) return;
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int k = t * 16 + lk + 4 * rr;
            if (k < w) {
                double *dst = A + i + (long long)k * ld;
                if (i + 1 < r) *(d2u *)dst = (d2u){acc[0][t][rr], acc[1][t][rr]};
                else dst[0] = acc[0][t][rr];
            }
        }
}

// C[i,j] -= sum_k A[i,k] * B[j,k]  on 64x64 tiles (4 waves x 32x32), FP64 MFMA, operands read
// straight from HBM/L2. The MFMA is issued "transposed" (first operand = rows of B) so that
// the 16 lanes sharing a register index walk down a COLUMN of the column-major C.
// Trailing update inside the panel (see the comment in the kernel); the contribution block is k_syrk_cb.
// CB -= L21 L21' (K = all c columns).
template <int TW>   // MFMA tiles per wave and dimension: wave tile 16*TW squared, workgroup tile twice that
__global__ __launch_bounds__(256) void k_gemm_nt(DevSym S, const FrontView *__restrict__ frec, int k0, int K, int c0, int c1,
                                                 double *__restrict__ L, FrontArg fa) {
    // panel columns [c0, min(c1, c)) of the front, rows c0 .. r-1:  C -= A A'  with A = the K
    // (finished) panel columns k0 .. k0+K-1 of those rows. Two-level blocking: K = 64 updates stay
    // inside the current 256-column block, the rest of the panel is updated once per 256 columns
    // with K = 256 (a quarter of the read-modify-write traffic of a flat right-looking sweep).
    const FrontView fv = front_view(frec, blockIdx.z, fa);
    const int c = fv.c;
    if (c0 >= c) return;
    const int r = fv.r;
    const int ld = fv.ld;
    double *P = L + fv.pp;
    const int M = r - c0, N = min(c1, c) - c0, ldc = ld;
    const double *A = (fa.on && fa.ppa != kNoPpa ? L + fa.ppa : P) + c0 + (long long)k0 * ld;
    double *C = P + c0 + (long long)c0 * ld;
    const int bi = blockIdx.x, bj = blockIdx.y;
    constexpr int WT = 16 * TW, GT = 2 * WT;
    if (bj > bi || bi * GT >= M || bj * GT >= N) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i0 = bi * GT + (wave & 1) * WT, j0 = bj * GT + (wave >> 1) * WT;
    if (i0 >= M || j0 >= N || j0 > i0 + WT - 1) return;
    const int lm = lane & 15, lk = lane >> 4;
    d4 acc[TW][TW];
#pragma unroll
    for (int a = 0; a < TW; a++)
#pragma unroll
        for (int b = 0; b < TW; b++) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
    // Operand rows are clamped (always-valid addresses, values masked afterwards) so that the
    // loads of a whole batch of KU k-steps issue back to back; the next batch is fetched into
    // a second register set before the current batch's MFMAs (software double buffering).
    constexpr int KU = TW == 2 ? 4 : 16;      // TW = 1 (latency variant): a K = 64 update is ONE batch -- one round trip for all operands
    // TW = 2: operand rows in PAIRS -- MFMA row lm of tile 0 / 1 is row 2 lm / 2 lm + 1 of the wave's 32 -- so one 16-byte
    // load per lane feeds both tiles, and C is read and written 16 bytes at a time as well: half the vector memory
    // instructions (the CU's address unit, not the MFMA pipe, is the busiest unit of this kernel). Lanes past the last
    // row re-read the last pair; the odd row after an odd count is padding or the next column's first entry.
    const int Mlast = (M - 1) & ~1, Nlast = (N - 1) & ~1;
    const double *pa[TW], *pb[TW];
#pragma unroll
    for (int a = 0; a < TW; a++) pa[a] = A + (TW == 2 ? min(i0 + 2 * lm, Mlast) : min(i0 + a * 16 + lm, M - 1));
#pragma unroll
    for (int b = 0; b < TW; b++) pb[b] = A + (TW == 2 ? min(j0 + 2 * lm, Nlast) : min(j0 + b * 16 + lm, N - 1));
    double ca[KU][TW], cb[KU][TW];
    auto load_step = [&](long long off, double (&xa)[TW], double (&xb)[TW]) {
        if constexpr (TW == 2) {
            const d2u va = *(const d2u *)(pa[0] + off), vb = *(const d2u *)(pb[0] + off);
            xa[0] = va.x; xa[1] = va.y; xb[0] = vb.x; xb[1] = vb.y;
        } else {
#pragma unroll
            for (int a = 0; a < TW; a++) xa[a] = pa[a][off];
#pragma unroll
            for (int b = 0; b < TW; b++) xb[b] = pb[b][off];
        }
    };
    // full batches: no masking at all, so the prefetch of batch k+1 really overlaps the MFMAs of
    // batch k (nothing consumes the loaded registers before the MFMAs that need them)
    auto fetch = [&](int k0, double (&xa)[KU][TW], double (&xb)[KU][TW]) {
#pragma unroll
        for (int u = 0; u < KU; u++) load_step((long long)(k0 + 4 * u + lk) * ld, xa[u], xb[u]);
    };
    auto mma = [&](double (&xa)[KU][TW], double (&xb)[KU][TW]) {
#pragma unroll
        for (int u = 0; u < KU; u++)
#pragma unroll
            for (int a = 0; a < TW; a++)
#pragma unroll
                for (int b = 0; b < TW; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[u][b], xa[u][a], acc[a][b], 0, 0, 0);
    };
    // TW = 1: the tile's own values are requested BEFORE the operands (they only meet in the epilogue): one round trip less
    // on the latency-bound levels this variant serves
    double cv[TW][TW][4];
    if constexpr (TW != 2) {
#pragma unroll
        for (int a = 0; a < TW; a++)
#pragma unroll
            for (int b = 0; b < TW; b++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const int i = min(i0 + a * 16 + lm, M - 1);
                    const int j = min(j0 + b * 16 + lk + 4 * rr, N - 1);
                    cv[a][b][rr] = C[i + (long long)j * ldc];
                }
    }
    const int kfull = K / (4 * KU) * (4 * KU);
    // single-buffered batches: latency is hidden by the other resident waves (4-5 per SIMD at
    // this register budget); hipcc turns a register double-buffer into vmcnt(0) at the loop head
    // anyway, which defeats the overlap. (Round 6: the three-stage loop of k_syrk_cb_rec<true> -- unconditional refills, scheduling
    // barriers -- does overlap; built here for K >= 48, bit-identical, and dropped: factor 8.44 / 8.44 -> 8.34 / 8.46 ms on one box, inside
    // the noise -- these launches sit on the panel chain and are bounded by their own latency, not by the product loop.)
    for (int k0 = 0; k0 < kfull; k0 += 4 * KU) {
        fetch(k0, ca, cb);
        mma(ca, cb);
    }
    if (kfull < K) {   // masked tail (k beyond K contributes 0 via an arithmetic mask on one operand;
                       // a select would let the compiler sink the load under a branch)
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int kk = kfull + 4 * u + lk;
            const double mk = kk < K ? 1.0 : 0.0;
            load_step((long long)min(kk, K - 1) * ld, ca[u], cb[u]);
#pragma unroll
            for (int a = 0; a < TW; a++) ca[u][a] *= mk;
        }
        mma(ca, cb);
    }
    // D[m][n]: m (rows of the first operand = C's column) = lk + 4*reg, n = lm = C's row
    // read-modify-write of C in two passes (all loads, then all stores): one round trip instead of
    // a chain of 4 TW^2 (the compiler cannot reorder a load of C past the previous store to C)
    if constexpr (TW == 2) {
        // tile a of the rows = row i0 + 2 lm + a, tile b of the columns = column j0 + 2 (lk + 4 rr) + b
        d2u cv[2][4];
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = min(j0 + 2 * (lk + 4 * rr) + b, N - 1);
                cv[b][rr] = *(const d2u *)(C + min(i0 + 2 * lm, Mlast) + (long long)j * ldc);
            }
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int i = i0 + 2 * lm, j = j0 + 2 * (lk + 4 * rr) + b;
                const bool v0 = i < M && j < N && i >= j, v1 = i + 1 < M && j < N && i + 1 >= j;
                double *dst = C + i + (long long)j * ldc;
                const double x0 = cv[b][rr].x - acc[0][b][rr], x1 = cv[b][rr].y - acc[1][b][rr];
                if (v0 && v1) *(d2u *)dst = (d2u){x0, x1};
                else {
                    if (v0) dst[0] = x0;
                    if (v1) dst[1] = x1;
                }
            }
    } else {
#pragma unroll
        for (int a = 0; a < TW; a++)
#pragma unroll
            for (int b = 0; b < TW; b++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const int i = i0 + a * 16 + lm;
                    const int j = j0 + b * 16 + lk + 4 * rr;
                    if (i < M && j < N && i >= j) C[i + (long long)j * ldc] = cv[a][b][rr] - acc[a][b][rr];
                }
    }
}

// Contribution block of a big front, written ONCE:  CB = (extend-add of the children's CBs) - L21 L21'.
// One workgroup per 64x64 lower tile: the children's entries that fall into the tile are gathered
// into an LDS tile (fixed child order, no atomics), the product runs on the FP64 MFMA, the
// epilogue stores LDS tile minus accumulators. No zero-fill, no read-modify-write of CB in HBM.
// (Reference form on a plain 3-D grid, front x tile row x tile column: GMRFX_SYRK_XCD=0. The product path is
// k_syrk_cb_rec below -- same arithmetic, tiles handed out per XCD from self-contained records.)
// STAMP: the level's launch, timed (stamp_begin / stamp_end, kernel_common.h); the distributed fronts' launches are not, and keep
// the code they had (with the stamps the compiler takes 102 registers instead of 76: 3 waves per SIMD instead of 4).
template <bool STAMP>
__global__ __launch_bounds__(256) void k_syrk_cb(DevSym S, const int *__restrict__ list, const double *__restrict__ L,
                                                 double *__restrict__ CB, int cyc_w, int cyc_r, int cyc_b0, unsigned long long *stamp) {
    __shared__ double Tl[64 * 65];
    const int s = list[blockIdx.z], bi = blockIdx.x, bj = blockIdx.y;
    const int c = S.sfirst[s + 1] - S.sfirst[s];
    const int r = (int)(S.rowptr[s + 1] - S.rowptr[s]);
    const int m = r - c;
    if (bj > bi || bi * 64 >= m) return;
    // distributed front (cyc_w > 0): this rank computes the 256-column blocks of the contribution block it owns -- block q on
    // position (cyc_b0 + q) mod cyc_w of the group, cyc_b0 = the panel's blocks (the dealing continues behind the panel)
    if (cyc_w > 0 && (cyc_b0 + (bj >> 2)) % cyc_w != cyc_r) return;
    // every workgroup with a tile stamps (the grid is a plain one: no workgroup is known to be the first or the last to run)
    if (STAMP) stamp_begin(stamp, (unsigned long long)wall_clock64());
    const int ld = S.ld[s];
    const double *A = L + S.panelptr[s] + c;
    double *C = CB + S.cbptr[s];
    const int tid = threadIdx.x;
    const int ti0 = bi * 64, tj0 = bj * 64;      // tile origin inside CB
    for (int idx = tid; idx < 64 * 65; idx += 256) Tl[idx] = 0.0;
    __syncthreads();
    {
        // Children two at a time: edge records and tile ranges of both first (two round trips for
        // the pair), then 16 entries per thread and child with all loads in flight at once. The
        // children are still ADDED one after the other (fixed order, bit-reproducible).
        const long long ch0 = S.childptr[s], ch1 = S.childptr[s + 1];
        const int nT = (m + 31) >> 5;
        const int la = tid & 63, lb = tid >> 6;
        for (long long cb = ch0; cb < ch1; cb += 2) {
            EdgeRec er[2];
            int a0[2], a1[2], b0[2], b1[2];
#pragma unroll
            for (int q = 0; q < 2; q++) er[q] = S.edge[min(cb + q, ch1 - 1)];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int *et = S.etile + er[q].tptr;
                a0[q] = et[2 * bi]; a1[q] = et[min(2 * bi + 2, nT)];
                b0[q] = et[2 * bj]; b1[q] = et[min(2 * bj + 2, nT)];
            }
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (cb + q < ch1) {
                    const int md = er[q].md;
                    const int *reld = S.rel + er[q].reloff;
                    const double *Ud = CB + er[q].cboff;
                    const int a = a0[q] + la, ac = min(a, md - 1);
                    const int ti = reld[ac] - c - ti0;
                    int tb[16];
                    double uv[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        const int b = min(b0[q] + lb + 4 * u, md - 1);
                        tb[u] = reld[b];
                        uv[u] = Ud[ac + (long long)b * md];
                    }
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        const int b = b0[q] + lb + 4 * u;
                        if (a < a1[q] && b < b1[q] && a >= b) Tl[ti + (tb[u] - c - tj0) * 65] += uv[u];
                    }
                    __syncthreads();
                }
            }
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = ti0 + (wave & 1) * 32, j0 = tj0 + (wave >> 1) * 32;
    if (i0 >= m || j0 >= m || j0 > i0 + 31) return;       // (never wave 0, whose first lane stamps the end)
    const int lm = lane & 15, lk = lane >> 4;
    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
    auto fa = [&](int j, int q) { return A[min(j, m - 1) + (long long)min(max(q, 0), c - 1) * ld]; };
    auto fb = [&](int q, int i) { return A[min(i, m - 1) + (long long)min(max(q, 0), c - 1) * ld]; };
    // D[m_ = j][n = i] = sum_q L21[j][q] L21[i][q]: rows i on the lanes (contiguous in column-major CB)
    wave_gemm_32x32(acc, j0, i0, 0, c, fa, fb, lm, lk);
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = j0 + a * 16 + lk + 4 * rr, i = i0 + b * 16 + lm;
                if (i < m && j < m && i >= j) C[i + (long long)j * m] = Tl[(i - ti0) + (j - tj0) * 65] - acc[a][b][rr];
            }
    if (STAMP) stamp_end(stamp);
}

// The product form of the same tile, driven by one 128-byte record per tile (SyrkTile, device.h) and handed out per
// XCD: workgroups go to the 8 XCDs round-robin by linear id, so id & 7 is the XCD and id >> 3 the position in that
// XCD's run of the level's tile list. A run holds whole fronts or compact 8 x 8-tile squares of one front, so the L21
// row blocks its tiles share are fetched into ONE L2 instead of all eight (L2-miss traffic of the launches of one
// factorisation: 17.2 GB on the 3-D grid, 6.95 GB here, 5.77 GB algorithmic -- tools/syrk_levels.py traffic).
// A tile of a narrow front is a chain of round trips, not arithmetic: the record arrives in one scalar load (instead of
// tile -> front geometry -> edge records -> tile ranges), the first k-batch of the product and the first child's entries
// are requested right behind it, and only then does anything wait. Children are still added one after the other, the k
// order is unchanged: bit-identical to k_syrk_cb.
struct SyrkOps { d2u a[2], b[2]; };       // the operands of two k-steps (rows in pairs): one stage of the pipelined product loop
template <bool PIPED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_syrk_cb_rec(DevSym S, const SyrkTile *__restrict__ recs, const SyrkSplit split,
                                                     const double *__restrict__ L, double *__restrict__ CB, int noprod,
                                                     unsigned long long *__restrict__ times) {
    // noprod: the children's extend-add only -- the product follows as its own launch on 128 x 128 staged tiles (k_syrk_big: the
    // huge fronts of 3-D problems)
    __shared__ double Tl[64 * 65];
    const int x = blockIdx.x & 7;
    const int t = split.start[x] + (int)(blockIdx.x >> 3);
    if (t >= split.start[x + 1]) return;
    // the launch's time (Device::syrk_ms): every tile leaves the device wall clock of its start and of its end in its own two words
    // of `times`, by one plain store behind its last one; k_syrk_reduce turns a level's tiles into the launch's slot behind the
    // last level. (No atomics here: a launch has ~1000 tiles that start and end together, and atomics execute at the memory side,
    // one address after the other -- measured, one atomic minimum and one maximum per tile into the launch's slot: k_syrk_cb_rec
    // 3.35 -> 4.05 ms per step.)
    const unsigned long long t_begin = (unsigned long long)wall_clock64();
    const SyrkTile T = recs[t];
    const int c = T.c, m = T.m, ld = T.ld, bi = T.bi, bj = T.bj;
    const double *A = L + T.pa;
    double *C = CB + T.cb;
    const int tid = threadIdx.x;
    const int ti0 = bi * 64, tj0 = bj * 64;
    const int wave = tid >> 6, lane = tid & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const int i0 = ti0 + (wave & 1) * 32, j0 = tj0 + (wave >> 1) * 32;
    const bool live = !(i0 >= m || j0 >= m || j0 > i0 + 31);       // this wave's 32 x 32 part reaches the lower triangle
    constexpr int KU = 4;
    // Operand rows in PAIRS: MFMA row lm of tile 0 / tile 1 is row 2 lm / 2 lm + 1 of the wave's 32 (not lm / 16 + lm),
    // so one 16-byte load per lane feeds both tiles -- half the vector memory instructions of the k-loop, which is
    // what these kernels are bound by (see above). Lanes past the last row re-read the last pair (never stored); the
    // odd row after an odd m is padding or the next column's first entry (never stored either).
    const int mlast = (m - 1) & ~1;
    const double *pa2 = A + min(j0 + 2 * lm, mlast);
    const double *pb2 = A + min(i0 + 2 * lm, mlast);
    double av[KU][2], bv[KU][2];
    auto request = [&](int q0) {
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const long long ko = (long long)min(q0 + 4 * u + lk, c - 1) * ld;
            const d2u xa = *(const d2u *)(pa2 + ko), xb = *(const d2u *)(pb2 + ko);
            av[u][0] = xa.x; av[u][1] = xa.y;
            bv[u][0] = xb.x; bv[u][1] = xb.y;
        }
    };
    // Tiles of WIDE fronts (c >= pipe_min): the product loop in three stages of two k-steps, each stage requested two stages ahead
    // (see the loop below)
    constexpr bool piped = PIPED;
    SyrkOps oA, oB, oC;
    // Addresses without vector arithmetic: a SCALAR base per k-step (the record is the same for every lane) + a 32-bit lane offset
    // (the lane's row pair + its column lk of the k-step). Requests behind the last k-step are clamped to the last four columns of
    // the PADDED panel (symbolic.cpp, panel_span: zero columns up to a multiple of 4): in vain, or masked in the tail.
    const unsigned voa = (unsigned)(min(j0 + 2 * lm, mlast) + lk * ld) * 8u, vob = (unsigned)(min(i0 + 2 * lm, mlast) + lk * ld) * 8u;
    const int cp4 = ((c + 3) & ~3) - 4;
    auto req2 = [&](SyrkOps &x, int q0) {
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const char *sb = (const char *)(A + (long long)min(q0 + 4 * u, cp4) * ld);
            x.a[u] = *(const d2u *)(sb + voa); x.b[u] = *(const d2u *)(sb + vob);
        }
    };
    if (live && !noprod) {
        if (piped) { req2(oA, 0); req2(oB, 8); req2(oC, 16); }
        else request(0);
    }
    // the first two children's entries: (row la, column lb + 4 u) of the child's rows / columns inside this tile.
    // Round trips: record -> [k-batch 0 + child 0] -> child 1 -> k-batch 1 ...
    // Every vector memory instruction costs the CU's address unit ~16 cycles whatever its lanes do, and these levels
    // are bound by exactly that (TA busy 87 %): so the child's column indices come in ONE load (lane l holds the
    // index of column b0 + l; each use reads its lane), columns beyond the tile's range issue nothing at all, and
    // neither do lanes beyond its row range.
    const int la = lane;
    const int lb = __builtin_amdgcn_readfirstlane(wave);
    // BOTH of the first two children are requested up front (two register sets): the second child's round trip used to start
    // only after the first child had been added -- on the narrow fronts of the mid levels a tile is little else than these
    // round trips
    int ti[2], rb[2];
    double uv[2][16];
    auto fetch = [&](int q) {
        const int md = T.md[q];
        const int *reld = S.rel + T.reloff[q];
        const double *Ud = CB + T.cboff[q];
        const int a = T.a0[q] + la;
        const int ac = min(a, md - 1);
        ti[q] = reld[ac];
        rb[q] = reld[min(T.b0[q] + la, md - 1)];
        const int nb = T.b1[q] - T.b0[q] - lb;          // this wave's columns: b0 + lb + 4 u < b1  <=>  4 u < nb
        if (a < T.a1[q]) {
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (4 * u < nb) uv[q][u] = Ud[ac + (long long)(T.b0[q] + lb + 4 * u) * md];
        }
    };
    auto add = [&](int q) {
        const int a = T.a0[q] + la;
        const int nb = T.b1[q] - T.b0[q] - lb;
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if (4 * u < nb) {
                const int tc = __builtin_amdgcn_readlane(rb[q], lb + 4 * u) - c - tj0;
                if (a < T.a1[q] && a >= T.b0[q] + lb + 4 * u) Tl[(ti[q] - c - ti0) + tc * 65] += uv[q][u];
            }
        }
    };
    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
    auto mfma_batch = [&](int q0) {
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const double mk = (q0 + 4 * u + lk) < c ? 1.0 : 0.0;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a] * mk, bv[u][b], acc[a][b], 0, 0, 0);
        }
    };
    if (T.nch > 0 && !piped) fetch(0);        // (piped: behind the product -- its three operand stages take the registers of a child's entries)
    for (int idx = tid; idx < 64 * 65; idx += 256) Tl[idx] = 0.0;
    // The product needs nothing from the children: it runs HERE, between the children's requests and their use, so that its
    // MFMAs cover the children's round trips (the accumulators meet the gathered tile only in the epilogue). Measured by
    // compiling parts out (profiles/r04_syrk_parts.txt): gather, product and store used to follow each other, a third of a
    // mid-level tile's time each.
    // D[m_ = j][n = i] = sum_q L21[j][q] L21[i][q]: rows i on the lanes (contiguous in column-major CB)
    auto mma2 = [&](const SyrkOps &x, int q0, bool masked) {
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const double mk = (!masked || (q0 + 4 * u + lk) < c) ? 1.0 : 0.0;
            const double a0 = masked ? x.a[u].x * mk : x.a[u].x, a1 = masked ? x.a[u].y * mk : x.a[u].y;
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, x.b[u].x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, x.b[u].y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, x.b[u].x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, x.b[u].y, acc[1][1], 0, 0, 0);
        }
    };
    if (live && !noprod) {
        if (piped) {
            // same k-steps in the same order as the plain loop (bit-identical sums); a stage's registers are refilled as soon as
            // its MFMAs have read them, two stages (16 MFMAs) before they are used again. The refills are UNCONDITIONAL (clamped
            // rows: the last ones of a tile are requested in vain): a conditional request makes the compiler count zero loads behind
            // every stage, i.e. wait for everything in flight.
            int q0 = 0;
            for (; q0 + 24 <= c; q0 += 24) {
                // (the scheduler would sink all refills to the end of the iteration: one exposed round trip per iteration again)
                mma2(oA, q0, false); __builtin_amdgcn_sched_barrier(0); req2(oA, q0 + 24); __builtin_amdgcn_sched_barrier(0);
                mma2(oB, q0 + 8, false); __builtin_amdgcn_sched_barrier(0); req2(oB, q0 + 32); __builtin_amdgcn_sched_barrier(0);
                mma2(oC, q0 + 16, false); __builtin_amdgcn_sched_barrier(0); req2(oC, q0 + 40); __builtin_amdgcn_sched_barrier(0);
            }
            if (q0 < c) {
                mma2(oA, q0, true);
                if (q0 + 8 < c) {
                    mma2(oB, q0 + 8, true);
                    if (q0 + 16 < c) mma2(oC, q0 + 16, true);
                }
            }
        } else
            for (int q0 = 0; q0 < c; q0 += 4 * KU) {
                if (q0 > 0) request(q0);
                mfma_batch(q0);
            }
    }
    if (T.nch > 0 && piped) fetch(0);
    if (T.nch > 1) fetch(1);        // (the second child's registers would not fit beside the product's: behind it, before the first is added)
    __syncthreads();
    if (T.nch > 0) {
        add(0);
        __syncthreads();
    }
    if (T.nch > 1) {
        add(1);
        __syncthreads();
    }
    if (T.nch > 2) {       // further children: edge record -> tile ranges -> entries, one child at a time
        const int nT = (m + 31) >> 5;
        for (long long cb = T.ch0 + 2; cb < T.ch0 + T.nch; cb++) {
            const EdgeRec er = S.edge[cb];
            const int *et = S.etile + er.tptr;
            const int a0 = et[2 * bi], a1 = et[min(2 * bi + 2, nT)], b0 = et[2 * bj], b1 = et[min(2 * bj + 2, nT)];
            const int md = er.md;
            const int *reld = S.rel + er.reloff;
            const double *Ud = CB + er.cboff;
            const int a = a0 + la, ac = min(a, md - 1);
            const int tr = reld[ac] - c - ti0;
            int tc[16];
            double w[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int b = min(b0 + lb + 4 * u, md - 1);
                tc[u] = reld[b];
                w[u] = Ud[ac + (long long)b * md];
            }
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int b = b0 + lb + 4 * u;
                if (a < a1 && b < b1 && a >= b) Tl[tr + (tc[u] - c - tj0) * 65] += w[u];
            }
            __syncthreads();
        }
    }
    if (!live) return;       // (never wave 0 -- a tile's first 32 x 32 part reaches the lower triangle --, whose first lane stamps the end)
    // rows i, i + 1 of column j leave together (16 bytes) wherever both lie inside the lower triangle
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int j = j0 + 2 * (lk + 4 * rr) + a, i = i0 + 2 * lm;
            if (j < m) {
                const double *tl = Tl + (i - ti0) + (j - tj0) * 65;
                double *dst = C + i + (long long)j * m;
                const bool v0 = i < m && i >= j, v1 = i + 1 < m && i + 1 >= j;
                if (v0 && v1) *(d2u *)dst = (d2u){tl[0] - acc[a][0][rr], tl[1] - acc[a][1][rr]};
                else {
                    if (v0) dst[0] = tl[0] - acc[a][0][rr];
                    if (v1) dst[1] = tl[1] - acc[a][1][rr];
                }
            }
        }
    if (tid == 0) *(ulonglong2 *)(times + 2 * (long long)(t)) = make_ulonglong2(t_begin, (unsigned long long)wall_clock64());
}

// The same update for the HUGE fronts of 3-D problems (round 5): 128 x 128 workgroup tiles, operands staged through LDS -- 16 k
// at a time, double-buffered through registers -- and shared by eight waves of 32 x 64 (tools/micro/dgemm_mfma.hip: 54 TFLOP/s on
// an ideal shape against 47-49 for the direct-operand 64 x 64 tile above, which is what the three top levels of the 126^3 mesh
// ran at). The transplant lost twice at cfg 2 (a quarter of the tiles, one wave per SIMD on half the chip);
// it is only used where a launch has thousands of such tiles: K a multiple of 16, at least 4096 rows below the block.
// Same arithmetic per entry (the k order inside an entry's sum is the same); the strict upper triangle of the diagonal tiles
// is computed and not stored.
// C (M x N, leading dimension ldc; lower part, i >= j) -= A[0 .. M) A[0 .. N)' over K columns of A (leading dimension lda); K any
// (a k beyond K is staged as zero)
__device__ __forceinline__ void gemm_nt_big_tile(const double *__restrict__ A, int lda, double *__restrict__ C, long long ldc, int M, int N, int K) {
    constexpr int TM = 128, KB = 16;
    __shared__ double As[2][KB][TM + 8], Bs[2][KB][TM + 8];      // +8: consecutive k rows start in different banks
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi || bi * TM >= M || bj * TM >= N) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lm = lane & 15, lk = lane >> 4;
    const int m0 = bi * TM, n0 = bj * TM;
    const int wi = (wave & 3) * 32, wj = (wave >> 2) * 64;       // wave sub-tile: 32 rows x 64 columns
    d4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
    // staging: 512 threads, a 128 x 16 slab = 4 doubles per thread (row tid % 128 -- clamped: rows past the edge are never
    // stored --, k = 4 (tid / 128) ..)
    const int lr = tid & 127, l4 = (tid >> 7) * 4;
    const double *pa = A + min(m0 + lr, M - 1);
    const double *pb = A + min(n0 + lr, M - 1);
    double ra[4], rb[4];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = kb * KB + l4 + q;
            const long long ko = (long long)min(k, K - 1) * lda;
            const double mk = k < K ? 1.0 : 0.0;
            ra[q] = pa[ko] * mk; rb[q] = pb[ko];
        }
    };
    fetch(0);
#pragma unroll
    for (int q = 0; q < 4; q++) { As[0][l4 + q][lr] = ra[q]; Bs[0][l4 + q][lr] = rb[q]; }
    __syncthreads();
    const int nk = (K + KB - 1) / KB;
    for (int kb = 0; kb < nk; kb++) {
        const int cur = kb & 1;
        if (kb + 1 < nk) fetch(kb + 1);
#pragma unroll
        for (int sidx = 0; sidx < KB / 4; sidx++) {
            double av[2], bv[4];
#pragma unroll
            for (int a = 0; a < 2; a++) av[a] = As[cur][4 * sidx + lk][wi + 16 * a + lm];
#pragma unroll
            for (int b = 0; b < 4; b++) bv[b] = Bs[cur][4 * sidx + lk][wj + 16 * b + lm];
            // D[m = column j][n = row i]: first operand = rows of B (columns of C), second = rows of A (the lanes walk i)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[b], av[a], acc[a][b], 0, 0, 0);
        }
        if (kb + 1 < nk) {
#pragma unroll
            for (int q = 0; q < 4; q++) { As[cur ^ 1][l4 + q][lr] = ra[q]; Bs[cur ^ 1][l4 + q][lr] = rb[q]; }
        }
        __syncthreads();
    }
    // C -= acc, lower part only (i >= j), all loads before all stores
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = m0 + wi + 16 * a + lm;
            double cv[4];
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = n0 + wj + 16 * b + lk + 4 * rr;
                cv[rr] = C[min(i, M - 1) + (long long)min(j, N - 1) * ldc];
            }
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = n0 + wj + 16 * b + lk + 4 * rr;
                if (i < M && j < N && i >= j) C[i + (long long)j * ldc] = cv[rr] - acc[a][b][rr];
            }
        }
}
__global__ __launch_bounds__(512) void k_gemm_nt_big(const FrontView *__restrict__ frec, int k0, int K, int c0, int c1,
                                                     double *__restrict__ L, FrontArg fa) {
    const FrontView fv = front_view(frec, blockIdx.z, fa);
    const int c = fv.c;
    if (c0 >= c) return;
    double *P = L + fv.pp;
    const double *PA = fa.on && fa.ppa != kNoPpa ? L + fa.ppa : P;
    gemm_nt_big_tile(PA + c0 + (long long)k0 * fv.ld, fv.ld, P + c0 + (long long)c0 * fv.ld, fv.ld, fv.r - c0, min(c1, c) - c0, K);
}
// The contribution block's product on the same tiles: CB -= L21 L21' behind a gather-only pass of k_syrk_cb_rec (noprod). At
// cfg 4 the one-pass kernel's 64 x 64 tiles stream K = 8 000-16 000 columns of both operands per tile (8 flop per byte: it ran at
// ~34 TFLOP/s, 3.5 of the 5.1 s); a 128 x 128 tile halves the operand bytes per flop. The extra read-modify-write of the block
// (m^2 doubles twice) is milliseconds against seconds there.
__global__ __launch_bounds__(512) void k_syrk_big(DevSym S, const int *__restrict__ list, const double *__restrict__ L, double *__restrict__ CB,
                                                  unsigned long long *stamp) {
    const int s = list[blockIdx.z];
    const int c = S.sfirst[s + 1] - S.sfirst[s];
    const int r = (int)(S.rowptr[s + 1] - S.rowptr[s]);
    const int m = r - c;
    if (m <= 0) return;
    // every workgroup of the lower triangle stamps (those without a tile leave gemm_nt_big_tile at once: all of it inside the launch)
    const bool stamps = stamp && blockIdx.y <= blockIdx.x;
    if (stamps) stamp_begin(stamp, (unsigned long long)wall_clock64());
    gemm_nt_big_tile(L + S.panelptr[s] + c, S.ld[s], CB + S.cbptr[s], m, m, m, c);
    if (stamps) stamp_end(stamp);
}

// Behind the last level of a factorisation (or of a phase of one): the tile times of k_syrk_cb_rec, level by level, into the
// levels' slots -- earliest start, latest end. One workgroup per level; the atomics (two per level) meet what k_syrk_big stamped
// into the same slot.
__global__ __launch_bounds__(256) void k_syrk_reduce(const SyrkLevelTimes *__restrict__ lev, const unsigned long long *__restrict__ times,
                                                     unsigned long long *__restrict__ stamps) {
    __shared__ unsigned long long lo[256], hi[256];
    const SyrkLevelTimes r = lev[blockIdx.x];
    if (r.slot < 0 || r.cnt <= 0) return;
    unsigned long long a = ~0ull, b = 0ull;
    for (int k = threadIdx.x; k < r.cnt; k += 256) {
        const ulonglong2 v = *(const ulonglong2 *)(times + 2 * (r.off + k));
        a = min(a, v.x); b = max(b, v.y);
    }
    lo[threadIdx.x] = a; hi[threadIdx.x] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            lo[threadIdx.x] = min(lo[threadIdx.x], lo[threadIdx.x + w]);
            hi[threadIdx.x] = max(hi[threadIdx.x], hi[threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMin(stamps + 2 * r.slot, lo[0]);
        atomicMax(stamps + 2 * r.slot + 1, hi[0]);
    }
}

// The words a factorisation reports through, before its first launch: the pivot word = INT_MAX ("no pivot failed"), the SYRK
// slots = (all ones, 0) for the atomic minimum / maximum of the stamps.
__global__ __launch_bounds__(256) void k_factor_reset(int *__restrict__ info, unsigned long long *__restrict__ stamps, int nslots) {
    if (threadIdx.x == 0) *info = INT_MAX;
    for (int k = threadIdx.x; k < nslots; k += 256) {
        stamps[2 * k] = ~0ull;
        stamps[2 * k + 1] = 0ull;
    }
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
void launch_assemble(hipStream_t st, const DevSym &S, const int *list, const AsmRec *arec, const double *nzp, int nfronts, int max_cols, int max_rows,
                     const double *nzval, double *L, double *CB) {
    Launch c = choose_assemble(nfronts, max_cols, max_rows);
    if (c.raised_lds) {
        static const bool once = [] { return hipFuncSetAttribute((const void *)k_assemble_lds<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072) == hipSuccess; }();
        if (!once) c = choose_assemble_hbm(nfronts, max_cols);
    }
    const int ldmax = asm_ldmax(max_rows);
    switch (c.variant) {
    case kAssembleLdsWave: GMRFX_LAUNCH(k_assemble_lds<0>, c, st, S, arec, nzp, L, CB, ldmax); break;
    case kAssembleLdsWg: GMRFX_LAUNCH(k_assemble_lds<1>, c, st, S, arec, nzp, L, CB, ldmax); break;
    case kAssembleHbmWg: GMRFX_LAUNCH(k_assemble<1>, c, st, S, list, nzval, L, CB, 0, 0, 0); break;
    case kAssembleHbmWave: GMRFX_LAUNCH(k_assemble<0>, c, st, S, list, nzval, L, CB, 0, 0, 0); break;
    default: break;
    }
}
// the distributed root: one front, only the 256-column blocks b with b mod cyc_w == cyc_r (one workgroup per column)
void launch_assemble_cyclic(hipStream_t st, const DevSym &S, const int *list, int ncols, const double *nzval, double *L, double *CB,
                            int cyc_w, int cyc_r, bool compact) {
    hipLaunchKernelGGL(k_assemble<1>, dim3(odd(ncols), 1), dim3(256), 0, st, S, list, nzval, L, CB, cyc_w, cyc_r, compact ? 1 : 0);
}
void launch_factor_reset(hipStream_t st, int *info, unsigned long long *stamps, int nslots) {
    hipLaunchKernelGGL(k_factor_reset, dim3(1), dim3(256), 0, st, info, stamps, nslots);
}
void launch_syrk_cb(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_trail, const double *L, double *CB, unsigned long long *stamp) {
    if (nfronts <= 0 || max_trail <= 0) return;
    hipLaunchKernelGGL(k_syrk_cb<true>, dim3(odd(cdiv(max_trail, 64)), odd(cdiv(max_trail, 64)), nfronts), dim3(256), 0, st, S, list, L, CB, 0, 0, 0, stamp);
}
void launch_syrk_cb_cyclic(hipStream_t st, const DevSym &S, const int *list, int trail, const double *L, double *CB, int cyc_w, int cyc_r, int cyc_b0) {
    if (trail <= 0) return;
    hipLaunchKernelGGL(k_syrk_cb<false>, dim3(odd(cdiv(trail, 64)), odd(cdiv(trail, 64)), 1), dim3(256), 0, st, S, list, L, CB, cyc_w, cyc_r, cyc_b0,
                       (unsigned long long *)nullptr);
}
void launch_syrk_cb_recs(hipStream_t st, const DevSym &S, const SyrkTile *recs, const SyrkSplit &split, int per_xcd, const double *L, double *CB,
                         unsigned long long *times, int noprod, bool piped) {
    if (per_xcd <= 0) return;
    if (piped) hipLaunchKernelGGL(k_syrk_cb_rec<true>, dim3(8 * (unsigned)per_xcd), dim3(256), 0, st, S, recs, split, L, CB, noprod, times);
    else hipLaunchKernelGGL(k_syrk_cb_rec<false>, dim3(8 * (unsigned)per_xcd), dim3(256), 0, st, S, recs, split, L, CB, noprod, times);
}
void launch_syrk_reduce(hipStream_t st, const SyrkLevelTimes *lev, int nlev, const unsigned long long *times, unsigned long long *stamps) {
    if (nlev <= 0) return;
    hipLaunchKernelGGL(k_syrk_reduce, dim3((unsigned)nlev), dim3(256), 0, st, lev, times, stamps);
}
void launch_syrk_big(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_trail, const double *L, double *CB, unsigned long long *stamp) {
    if (nfronts <= 0 || max_trail <= 0) return;
    const int nt = cdiv(max_trail, 128);
    hipLaunchKernelGGL(k_syrk_big, dim3(odd(nt), odd(nt), nfronts), dim3(512), 0, st, S, list, L, CB, stamp);
}
void launch_trsm(hipStream_t st, const DevSym &S, const FrontView *frec, int nactive, int kb, int mode, int max_rows_below,
                 double *L, double *Yh, const long long *yoff, const FrontArg &fa) {
    const Launch c = choose_trsm(nactive, max_rows_below);
    if (c.variant == kNoLaunch) return;
    const bool split = c.variant == kTrsmSplit;
    if (mode == 0) {
        if (split) GMRFX_LAUNCH((k_trsm<0, 1>), c, st, S, frec, kb, L, Yh, yoff, fa);
        else GMRFX_LAUNCH((k_trsm<0, 0>), c, st, S, frec, kb, L, Yh, yoff, fa);
    } else {
        if (split) GMRFX_LAUNCH((k_trsm<1, 1>), c, st, S, frec, kb, L, Yh, yoff, fa);
        else GMRFX_LAUNCH((k_trsm<1, 0>), c, st, S, frec, kb, L, Yh, yoff, fa);
    }
}
void launch_trsm_narrow(hipStream_t st, const FrontView *frec, int nactive, int kb, int max_rows_below, double *L) {
    if (nactive <= 0 || max_rows_below <= 0) return;
    hipLaunchKernelGGL(k_trsm_narrow, dim3(odd(cdiv(max_rows_below, 128)), nactive), dim3(256), 0, st, frec, kb, L);
}
void launch_gemm_nt(hipStream_t st, const DevSym &S, const FrontView *frec, int nactive, int k0, int K, int c0, int c1,
                    int maxM, int maxN, double *L, const FrontArg &fa) {
    // 64x64 workgroup tiles, operands straight from L2 at 3-4 waves per SIMD. Measured on MI355X: the
    // sustained v_mfma_f64_16x16x4_f64 rate is 36.3 TFLOP/s (tools/micro/mfma64.hip), this kernel reaches
    // ~27 TFLOP/s on the top-of-tree SYRKs; 128x128 tiles (register- or LDS-staged) were tried and lost
    // to it because they drop to one wave per SIMD.
    const Launch c = choose_gemm_nt(nactive, K, maxM, maxN);
    switch (c.variant) {
    case kGemmNtBig: GMRFX_LAUNCH(k_gemm_nt_big, c, st, frec, k0, K, c0, c1, L, fa); break;
    case kGemmNt32: GMRFX_LAUNCH(k_gemm_nt<1>, c, st, S, frec, k0, K, c0, c1, L, fa); break;
    case kGemmNt64: GMRFX_LAUNCH(k_gemm_nt<2>, c, st, S, frec, k0, K, c0, c1, L, fa); break;
    default: break;
    }
}

}  // namespace gmrfx
