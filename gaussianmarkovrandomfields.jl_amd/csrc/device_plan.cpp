// device_plan.cpp -- the tables of Device::upload and the level schedule, from the symbolic analysis alone (host code, no HIP).
#include "device_plan.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace gmrfx {

// one 32-byte geometry record per position of a level list (kernel_common.h, front_view)
static std::vector<FrontView> front_views(const Symbolic &S, const std::vector<i32> &lst) {
    std::vector<FrontView> v(lst.size());
    for (size_t k = 0; k < lst.size(); k++) {
        const i32 s = lst[k];
        v[k] = FrontView{(int)s, S.ncols(s), S.nrows(s), (int)S.ld[s], (int)S.sfirst[s], 0, (long long)S.panelptr[s]};
    }
    return v;
}

// the level lists with every level's big fronts split into their even / odd positions (two panel chains per level)
static std::vector<int> even_odd_levellist(const Symbolic &S) {
    std::vector<int> l2(S.levellist.begin(), S.levellist.end());
    for (i32 l = 0; l < S.nlevels; l++) {
        const i64 f = S.levelptr[l] + S.level_nsmall[l], e = S.levelptr[l + 1];
        i64 w = f;
        for (i64 k = f; k < e; k += 2) l2[w++] = S.levellist[k];
        for (i64 k = f + 1; k < e; k += 2) l2[w++] = S.levellist[k];
    }
    return l2;
}

static std::vector<LevelInfo> level_infos(const Symbolic &S, const std::vector<i64> &lptr, const std::vector<i32> &llist,
                                          const std::vector<i32> &lnsmall, const std::vector<i32> &lncls, double *syrk_flops) {
    std::vector<LevelInfo> LV(S.nlevels);
    for (i32 l = 0; l < S.nlevels; l++) {
        LevelInfo &L = LV[l];
        L.first = (int)lptr[l];
        L.count = (int)(lptr[l + 1] - lptr[l]);
        L.nsmall = lnsmall[l];
        for (int k = 0; k < 4; k++) L.ncls[k] = lncls[(size_t)l * 4 + k];
        L.max_rows = L.max_cols = 0;
        int max_trail = 0, min_trail = INT_MAX;
        for (int k = L.nsmall; k < L.count; k++) {
            i32 s = llist[L.first + k];
            L.max_rows = std::max(L.max_rows, S.nrows(s));
            L.max_cols = std::max(L.max_cols, S.ncols(s));
            max_trail = std::max(max_trail, S.nrows(s) - S.ncols(s));
            if (S.nrows(s) > S.ncols(s)) min_trail = std::min(min_trail, S.nrows(s) - S.ncols(s));
            const double cc = S.ncols(s), mm = S.nrows(s) - S.ncols(s);
            if (syrk_flops) *syrk_flops += cc * mm * (mm + 1);   // lower triangle of the contribution block: 2 c flops per entry
        }
        auto wider_than = [&](int w) {      // big fronts with more than w columns (sorted by decreasing columns)
            int cnt = 0;
            for (int k = L.nsmall; k < L.count && S.ncols(llist[L.first + k]) > w; k++) cnt++;
            return cnt;
        };
        std::vector<int> blk((size_t)L.nblk());
        for (int b = 0; b < L.nblk(); b++) blk[b] = wider_than(b * NB);
        L.set_block_counts(std::move(blk));
        for (int q = 0; q < 3; q++) L.wider[q] = wider_than(48 - 16 * q);
        L.max_trail = max_trail;
        L.min_trail = min_trail == INT_MAX ? 0 : min_trail;
    }
    return LV;
}

EnvKnobs read_env_knobs() {
    EnvKnobs k;
    if (const char *e = std::getenv("GMRFX_INV_CAP")) {
        const int v = std::atoi(e);
        k.inv_cap = NB;
        while (k.inv_cap < v) k.inv_cap *= 2;
    }
    if (const char *e = std::getenv("GMRFX_TASK_MODE")) {       // A/B knob: "wg" / "wave" force one form for every width
        const std::string m(e);
        k.wave_max_nr = m == "wg" ? 0 : m == "wave" ? 64 : k.wave_max_nr;
    }
    if (const char *e = std::getenv("GMRFX_LEVEL_MARK")) k.level_mark = std::atoi(e) != 0;
    if (const char *e = std::getenv("GMRFX_BWD_FRONT")) k.bwd_front_min = std::atoi(e);
    if (const char *e = std::getenv("GMRFX_FWD_FRONT")) k.fwd_front_min = std::atoi(e);
    if (const char *e = std::getenv("GMRFX_SYRK_XCD")) k.syrk_xcd = std::atoi(e) != 0;
    if (const char *e = std::getenv("GMRFX_SYRK_PIPED")) k.syrk_piped_min = std::atoi(e);
    return k;
}

// The fronts of at most min(front_max_cols, inv_cap) columns (a front needs its WHOLE inverse for the one-workgroup step) are the
// tail of the list; the front kernel takes them on levels with at least front_min of them (enough to fill the chip), when allowed.
static LevelBlocks split_level(const LevelInfo &L, bool front_kernel, int front_min, const SweepKnobs &k) {
    LevelBlocks b{&L, k.inv_cap, 0, L.nbig(), std::max(1, (L.max_cols + k.inv_cap - 1) / k.inv_cap)};
    const int nwide = L.wider_than(std::min(k.front_max_cols, k.inv_cap) / NB * NB);
    if (front_kernel && front_min > 0 && b.nf - nwide >= front_min) { b.ntail = b.nf - nwide; b.nf = nwide; }
    return b;
}

FwdLevelPlan plan_forward_level(const LevelInfo &L, int nr, const SweepKnobs &k) {
    const bool narrow = nr <= k.narrow_pass_max;      // (the front kernel is for passes wider than the narrow kernels take)
    FwdLevelPlan p{split_level(L, !narrow, k.fwd_front_min, k), 0, false, false, FwdLevelPlan::kNone};
    // the record-driven update skips the fronts the front kernel took by their width (its records cover the level)
    p.cmin = narrow ? (k.tile_records ? kFwdWaveCols : 0) : p.ntail > 0 ? std::min(k.front_max_cols, k.inv_cap) / NB * NB : 0;
    p.wave = narrow && k.tile_records && L.wider_than(kFwdWaveCols) < p.nf;
    p.wave_split_k = L.max_cols > k.wave_split_cols;
    // levels with many tiles: record-driven, per-XCD runs; the handful-of-fronts levels keep the 16-row latency variant
    if (p.nf > 0 && L.max_cols > p.cmin)
        p.update = k.tile_records && (long long)cdiv(L.max_trail, 32) * p.nf > kFwdUpdate16MaxTiles ? FwdLevelPlan::kRecords : FwdLevelPlan::kGrid;
    return p;
}

BwdLevelPlan plan_backward_level(const LevelInfo &L, int nr, const SweepKnobs &k) {
    const bool narrow = nr <= k.narrow_pass_max_bwd;
    BwdLevelPlan p{split_level(L, !narrow, k.bwd_front_min, k), 0, false, false, false};
    p.mmin = narrow ? kBwdWaveRows : 0;
    p.wave = narrow && L.max_trail > 0 && L.min_trail <= kBwdWaveRows;
    p.wave_split_k = L.max_trail > k.wave_split_rows;
    p.gemm = L.max_trail > p.mmin;
    return p;
}

// ---- launch choices (device_plan.h) ---------------------------------------------------------------------------------------------------
Launch choose_assemble_hbm(int nfronts, int max_cols) {
    if (nfronts <= 0) return {};
    if ((long long)cdiv(max_cols, ASM_CW) * nfronts <= kAsmHbmWgMaxGroups) return {kAssembleHbmWg, odd(max_cols), (unsigned)nfronts, 1, 256};
    return {kAssembleHbmWave, odd(cdiv(max_cols, ASM_CW)), (unsigned)nfronts, 1, 256};
}
Launch choose_assemble(int nfronts, int max_cols, int max_rows) {
    if (nfronts <= 0) return {};
    const int ldmax = asm_ldmax(max_rows);
    const size_t col = (size_t)ldmax * sizeof(double);
    if (ldmax <= kAsmLdsWaveMaxRows) return {kAssembleLdsWave, odd(cdiv(max_cols, ASM_CW)), (unsigned)nfronts, 1, 256, 4 * col};
    if (ldmax <= kAsmLdsWgMaxRows) return {kAssembleLdsWg, odd(max_cols), (unsigned)nfronts, 1, 256, col, col > 65536};
    return choose_assemble_hbm(nfronts, max_cols);
}
Launch choose_trsm(int nactive, int max_rows_below) {
    if (nactive <= 0 || max_rows_below <= 0) return {};
    const bool split = (long long)cdiv(max_rows_below, 64) * nactive <= kTrsmSplitMaxTiles;
    return {split ? kTrsmSplit : kTrsmWhole, odd(cdiv(max_rows_below, split ? 16 : 128)), (unsigned)nactive, 1, 256};
}
Launch choose_gemm_nt(int nactive, int K, int maxM, int maxN) {
    if (nactive <= 0 || maxM <= 0 || maxN <= 0) return {};
    if (K % kGemmBigKStep == 0 && K >= kGemmBigMinK && maxM >= kGemmBigMinM && maxN >= kGemmBigMinN)
        return {kGemmNtBig, odd(cdiv(maxM, 128)), odd(cdiv(maxN, 128)), (unsigned)nactive, 512};
    if ((long long)cdiv(maxM, 64) * cdiv(maxN, 64) * nactive <= kGemmSmallTileMax)
        return {kGemmNt32, odd(cdiv(maxM, 32)), odd(cdiv(maxN, 32)), (unsigned)nactive, 256};
    return {kGemmNt64, odd(cdiv(maxM, 64)), odd(cdiv(maxN, 64)), (unsigned)nactive, 256};
}
Launch choose_fwd_update(int nfronts, int max_trail) {
    if (nfronts <= 0 || max_trail <= 0) return {};
    if ((long long)cdiv(max_trail, 32) * nfronts <= kFwdUpdate16MaxTiles) return {kFwdUpdate16, odd(cdiv(max_trail, 16)), (unsigned)nfronts, 1, 256};
    return {kFwdUpdate32, odd(cdiv(max_trail, 32)), (unsigned)nfronts, 1, 256};
}
Launch choose_fwd_update_wave(int per_xcd, int nr, bool split_k) {
    if (per_xcd <= 0) return {};
    return {split_k ? kWaveSplitK : kWaveWhole, 8 * (unsigned)per_xcd, (unsigned)cdiv(nr, 16), 1, split_k ? 256u : 64u};
}
Launch choose_fwd_own_update(int nfronts, int max_cols, int blk, int cap) {
    const int rows_below = max_cols - (blk + 1) * cap;      // own rows below the block in the widest front
    if (nfronts <= 0 || rows_below <= 0) return {};
    return {kFwdOwnUpdate, odd(cdiv(rows_below, 32)), (unsigned)nfronts, 1, 256};
}
Launch choose_bwd_gemm(int nfronts, int max_cols, int blk, int cap) {
    if (nfronts <= 0 || max_cols <= 0) return {};
    if (blk >= 0) max_cols = std::min(max_cols - blk * cap, cap);
    if (max_cols <= 0) return {};
    const long long wg32 = (long long)cdiv(max_cols, 32) * nfronts;
    if (wg32 > kBwdGemm8Max) return {kBwdGemm32x4, odd(cdiv(max_cols, 32)), (unsigned)nfronts, 1, 256};
    if (wg32 >= kBwdGemmWide8Min) return {kBwdGemm32x8, odd(cdiv(max_cols, 32)), (unsigned)nfronts, 1, 512};
    return {kBwdGemm16x8, odd(cdiv(max_cols, 16)), (unsigned)nfronts, 1, 512};
}
Launch choose_bwd_wave(int nfronts, int max_cols, int nr, bool split_k) {
    if (nfronts <= 0 || max_cols <= 0) return {};
    return {split_k ? kWaveSplitK : kWaveWhole, odd(cdiv(max_cols, 16)), (unsigned)nfronts, (unsigned)cdiv(nr, 16), split_k ? 256u : 64u};
}
Launch choose_permute(int n, int nr) {
    if (n <= 0) return {};
    if (nr <= kPermuteNarrowMaxNr) return {kPermuteNarrow, (unsigned)cdiv(n, 256), 1, 1, 256};
    return {kPermuteTiles, (unsigned)cdiv(n, 64), 1, 1, 256};
}

Launch choose_grad_pattern(int n, int nbatch) {
    if (n <= 0 || nbatch <= 0) return {};
    return {kGradPattern, (unsigned)cdiv(n, kGradCols), (unsigned)nbatch, 1, 256};
}
Launch choose_grad_mubar(int n, int nbatch) {
    if (n <= 0 || nbatch <= 0) return {};
    return {kGradMubar, (unsigned)cdiv(n, kGradRows), (unsigned)nbatch, 1, 256};
}
Launch choose_grad_dot(long long nnz, int p, int nbatch) {
    if (nnz <= 0 || p <= 0 || nbatch <= 0) return {};
    return {kGradDot, (unsigned)((nnz + kGradDotChunk - 1) / kGradDotChunk), (unsigned)p, (unsigned)nbatch, 256};
}

// Dense-inverse stage B: T-buffer offsets of the fronts wider than B, a list sorted by decreasing width; *total = doubles.
static std::vector<long long> stage_offsets(const Symbolic &S, const std::vector<int> &fronts, int B, long long *total) {
    std::vector<long long> off;
    long long acc = 0;
    for (int s : fronts) {
        if (S.ncols(s) <= B) break;
        off.push_back(acc);
        acc += (long long)((S.ncols(s) + 2 * B - 1) / (2 * B)) * B * B;
    }
    *total = acc;
    return off;
}

// Cuts a level's tiles (in hand-out order) into 8 runs of equal estimated cost, one per XCD; *per = the longest run.
static void cut_xcd_runs(const std::vector<double> &cost, SyrkSplit &split, int *per, const char *what) {
    const size_t nt = cost.size();
    if (nt >= (size_t)INT_MAX / 8) throw std::runtime_error(std::string("too many ") + what + " tiles in one level");
    double tot = 0, acc = 0;
    for (size_t t = 0; t < nt; t++) tot += cost[t];
    int x = 0;
    split.start[0] = 0;
    for (size_t t = 0; t < nt; t++) {
        while (x < 7 && acc >= tot * (x + 1) / 8) split.start[++x] = (int)t;
        acc += cost[t];
    }
    while (x < 8) split.start[++x] = (int)nt;
    *per = 0;
    for (int q = 0; q < 8; q++) *per = std::max(*per, split.start[q + 1] - split.start[q]);
}

DevicePlan build_device_plan(const Symbolic &S, const PlanOptions &o) {
    const int ns = S.nsuper;
    if (S.nnz_in >= (i64)INT_MAX) throw std::runtime_error("nnz(Q) >= 2^31 not supported by the device scatter map yet");
    DevicePlan P;
    {   // selected inversion: one gather record per supernode
        P.selrec.resize((size_t)ns);
        for (i32 s = 0; s < ns; s++) {
            SelRec t{};
            const i32 p = S.sparent[s];
            t.p = (int)p;
            t.rel = (long long)S.rowptr[s] + S.ncols(s);
            t.m = S.nrows(s) - S.ncols(s);
            t.out = (long long)S.zbptr[s];
            if (p >= 0) {
                t.zp = (long long)S.panelptr[p]; t.zbp = (long long)S.zbptr[p];
                t.cp = S.ncols(p); t.mp = S.nrows(p) - S.ncols(p); t.ldp = (int)S.ld[p];
            }
            t.foreign = (S.shard_plan && p >= 0 && S.owner[p] != S.shard_rank) ? 1 : 0;   // (= DevSym::foreign_parent)
            P.selrec[(size_t)s] = t;
        }
    }
    {
        std::vector<int> &qs = P.qsrc, &qd = P.qdst, &qc = P.qcol;
        qs.resize(S.qsrc.size()); qd.resize(S.qdst.size()); qc.resize(S.qdst.size());
        for (i32 s = 0; s < ns; s++)
            for (i64 q = S.qptr[s]; q < S.qptr[s + 1]; q++) {
                qs[q] = (int)S.qsrc[q];
                const i64 rel = S.qdst[q] - S.panelptr[s];      // column-major offset inside the panel (may exceed 2^31)
                qc[q] = (int)(rel / S.ld[s]);
                qd[q] = (int)(rel % S.ld[s]);
            }
        P.nq = (long long)qs.size();
        // entries are sorted by column inside a front: one pointer per column of L replaces a search per panel column
        std::vector<int> &qcp = P.qcolptr;
        qcp.resize((size_t)S.n + 1);
        for (i32 s = 0; s < ns; s++) {
            i64 q = S.qptr[s];
            for (i32 tc = 0; tc < S.ncols(s); tc++) {
                qcp[(size_t)S.sfirst[s] + tc] = (int)q;
                while (q < S.qptr[s + 1] && qc[q] == tc) q++;
            }
            if (q != S.qptr[s + 1]) throw std::runtime_error("scatter map of a front is not sorted by column");
        }
        qcp[(size_t)S.n] = (int)S.qptr[ns];
    }
    P.sum_trail = S.wptr[ns];     // (Symbolic::wptr: per-rank layout on sharded handles)
    {
        std::vector<int> &etile = P.etile, &erow = P.erow;
        P.edge.resize(S.children.size());
        for (i32 p = 0; p < ns; p++) {
            const int cp = S.ncols(p), mp = S.nrows(p) - cp, nT = (mp + 31) / 32;
            for (i64 ch = S.childptr[p]; ch < S.childptr[p + 1]; ch++) {
                const i32 d = S.children[ch];
                const int cd = S.ncols(d), md = S.nrows(d) - cd;
                const i64 reloff = S.rowptr[d] + cd;
                if (etile.size() + (size_t)nT + 1 >= (size_t)INT_MAX) throw std::runtime_error("edge tile table too large");
                EdgeRec e{d, md, (int)etile.size(), 0, (long long)reloff, S.wptr[d], (long long)S.cbptr[d], (long long)erow.size()};
                int a = 0;
                for (int T = 0; T <= nT; T++) {
                    const int key = cp + 32 * T;
                    while (a < md && S.rel[reloff + a] < key) a++;
                    etile.push_back(a);
                }
                e.nown = etile[e.tptr];
                erow.resize(erow.size() + (size_t)cp, -1);      // which child row lands in own column tc of the parent
                for (int a2 = 0; a2 < e.nown; a2++) erow[(size_t)e.eoff + (size_t)S.rel[reloff + a2]] = a2;
                P.edge[ch] = e;
            }
        }
        if (etile.empty()) etile.push_back(0);
        if (erow.empty()) erow.push_back(-1);
    }
    if (S.shard_plan) {
        P.owncol.assign(S.n, 0);
        for (i32 s = 0; s < ns; s++) {
            const bool mine = S.owner[s] == S.shard_rank;
            if (mine) for (i32 j = S.sfirst[s]; j < S.sfirst[s + 1]; j++) P.owncol[j] = 1;
        }
        // selected inversion across ranks: which of my fronts get their trailing inverse block from another rank, and
        // which fronts of other ranks get theirs from me (gathered here, level by level, then sent)
        P.foreign_parent.assign(ns, 0);
        std::vector<std::vector<int>> fc(S.nlevels);
        for (i32 s = 0; s < ns; s++) {
            const i32 pr = S.sparent[s];
            if (pr < 0) continue;
            if (S.owner[pr] != S.shard_rank) P.foreign_parent[s] = 1;
            if (S.owner[pr] == S.shard_rank && S.owner[s] != S.shard_rank) fc[S.level[s]].push_back(s);
        }
        P.fc_levelptr.assign(S.nlevels + 1, 0);
        P.fc_maxtrail.assign(S.nlevels, 0);
        for (i32 l = 0; l < S.nlevels; l++) {
            for (int s : fc[l]) { P.fchild.push_back(s); P.fc_maxtrail[l] = std::max(P.fc_maxtrail[l], S.nrows(s) - S.ncols(s)); }
            P.fc_levelptr[l + 1] = (int)P.fchild.size();
        }
    }
    {
        P.nswt = (int)S.swt_first.size();
        std::vector<SweepTask> &tk = P.swt;
        tk.resize((size_t)P.nswt);
        for (int t = 0; t < P.nswt; t++) {
            const i32 f = S.swt_first[t], r = S.swt_last[t];
            SweepTask &T = tk[t];
            T.s0 = f; T.s1 = r; T.col0 = S.sfirst[f]; T.nt = S.sfirst[r + 1] - S.sfirst[f];
            T.mroot = S.nrows(r) - S.ncols(r); T.pad = 0;
            T.p0 = S.panelptr[f]; T.p1 = S.panelptr[r + 1];
            T.rp0 = S.rowptr[f]; T.rp1 = S.rowptr[r + 1];
            T.rroot = S.rowptr[r] + S.ncols(r);
            T.woff = S.wptr[r];
            T.c0 = S.swc_ptr[t]; T.nch = S.swc_ptr[t + 1] - S.swc_ptr[t];
            T.b0 = S.swc_bptr[t]; T.nbw = S.swc_bptr[t + 1] - S.swc_bptr[t];
            for (int q = 0; q < 4; q++) { T.scnt[q] = S.swc_slot[(size_t)8 * t + q]; T.sbar[q] = S.swc_slot[(size_t)8 * t + 4 + q]; }
        }
        // chunk records and their target-row lists. The kernels take a target row as the BYTE offset of its column 0 in the
        // local vector (row-major, NC columns, odd rows with their 16-column tiles swapped: sweep_chunk.hip, vbyte) and add
        // the lane's column with one XOR; padding rows go to the spare row. Forward order per 32-row pair: [lk][tile][rr] =
        // pair row 2 (lk + 4 rr) + tile; backward order per 16-row k-tile: [lk][h][e] = row 8 h + 2 lk + e.
        P.nswc = S.swc_nchunks;
        if (P.nswc > 0) {
            const int nc = o.chunk_nc, spare = o.chunk_spare_row;
            auto enc = [&](i32 row) { const int r = row < 0 ? spare : row; return (r * nc + (nc >= 32 ? (r & 1) << 4 : 0)) * 8; };
            // (64 entries of slack: the backward kernel requests a fixed number of k-tiles per chunk, the last chunk's past its list)
            std::vector<int> &lf = P.swc_listf, &lb = P.swc_listb;
            lf.assign(S.swc_rows.size() + 64, 0); lb.assign(S.swc_rows.size() + 64, 0);
            for (size_t b0 = 0; b0 < S.swc_rows.size(); b0 += 32) {
                const i32 *src = S.swc_rows.data() + b0;
                for (int lk = 0; lk < 4; lk++)
                    for (int tl = 0; tl < 2; tl++)
                        for (int rr = 0; rr < 4; rr++) lf[b0 + lk * 8 + tl * 4 + rr] = enc(src[2 * (lk + 4 * rr) + tl]);
                for (int kt = 0; kt < 2; kt++)
                    for (int lk = 0; lk < 4; lk++)
                        for (int h = 0; h < 2; h++)
                            for (int e = 0; e < 2; e++) lb[b0 + 16 * kt + lk * 4 + h * 2 + e] = enc(src[16 * kt + 8 * h + 2 * lk + e]);
            }
        }
        // wave tasks (sweep_wave.hip): the tasks by LDS class -- rows of the local vector <= kWaveRows[k] -- heaviest first inside
        // a class (the list is already sorted by work); the big class is launched first
        std::vector<int> &ord = P.wave_order;
        for (int k = 0; k < kWaveClasses; k++) {
            P.wave_first[k] = (int)ord.size();
            for (int t = 0; t < P.nswt; t++) {
                const int rows = tk[t].nt + tk[t].mroot;
                if (rows <= kWaveRows[k] && (k == 0 || rows > kWaveRows[k - 1])) ord.push_back(t);
            }
            P.wave_count[k] = (int)ord.size() - P.wave_first[k];
        }
        if ((int)ord.size() != P.nswt) throw std::runtime_error("internal: a sweep task exceeds the largest wave-task class");
        for (int t = 0; t < P.nswt; t++) ord.push_back(t);       // ... and all of them, heaviest first (passes of at most 4 columns: one launch)
    }
    P.levellist2 = even_odd_levellist(S);
    for (int k = 0; k < 3; k++) P.nsub_cls[k] = S.nsub_cls[k];
    P.frec = front_views(S, S.levellist);
    P.sel_frec = front_views(S, S.sel_levellist);
    P.frec2 = front_views(S, P.levellist2);

    P.sel_max_cols.assign(S.nlevels, 0);
    P.sel_max_trail.assign(S.nlevels, 0);
    for (i32 l = 0; l < S.nlevels; l++)
        for (i64 k = S.sel_levelptr[l] + S.sel_level_nsmall[l]; k < S.sel_levelptr[l + 1]; k++) {
            const i32 s = S.sel_levellist[k];
            P.sel_max_cols[l] = std::max(P.sel_max_cols[l], (int)S.ncols(s));
            P.sel_max_trail[l] = std::max(P.sel_max_trail[l], (int)(S.nrows(s) - S.ncols(s)));
        }
    P.levels = level_infos(S, S.levelptr, S.levellist, S.level_nsmall, S.level_ncls, &P.syrk_flops);
    P.swlevels = level_infos(S, S.sw_levelptr, S.sw_levellist, S.sw_level_nsmall, S.sw_level_ncls, nullptr);

    // fronts with more than one 64-column block, by decreasing width: dense-inverse stages
    {
        std::vector<int> &il = P.invlist;
        for (i32 s = 0; s < ns; s++) {
            const bool mine = !S.shard_plan || S.owner[s] == S.shard_rank;
            if (S.ncols(s) > NB && mine) il.push_back(s);     // sharded handles only hold the panels they factored
        }
        std::sort(il.begin(), il.end(), [&](int a, int b) { return S.ncols(a) != S.ncols(b) ? S.ncols(a) > S.ncols(b) : a < b; });
        P.inv_maxc = il.empty() ? 0 : S.ncols(il[0]);
        for (int B = NB; B < P.inv_maxc; B *= 2) {
            long long acc = 0;
            P.inv_toff.push_back(stage_offsets(S, il, B, &acc));
            P.inv_nact.push_back((int)P.inv_toff.back().size());
            P.inv_tsize = std::max(P.inv_tsize, acc);
        }
        // the same stages level by level (pipelined factor + solve: the inverses of a level are built right behind its
        // factorisation; the levels follow each other on one stream, so they share the workspace)
        std::vector<int> &cat = P.inv_lvl_list;
        P.inv_lvl_first.assign(S.nlevels + 1, 0); P.inv_lvl_maxc.assign(S.nlevels, 0); P.inv_lvl_nact.assign(S.nlevels, {});
        std::vector<std::vector<int>> per(S.nlevels);
        for (int s : il) per[S.level[s]].push_back(s);      // (il is sorted by decreasing width: so is every level's list)
        for (i32 l = 0; l < S.nlevels; l++) {
            P.inv_lvl_first[l] = (int)cat.size();
            P.inv_lvl_maxc[l] = per[l].empty() ? 0 : S.ncols(per[l][0]);
            cat.insert(cat.end(), per[l].begin(), per[l].end());
        }
        P.inv_lvl_first[S.nlevels] = (int)cat.size();
        for (int B = NB; !cat.empty() && B < P.inv_maxc; B *= 2) {
            std::vector<long long> off(cat.size(), 0);
            for (i32 l = 0; l < S.nlevels; l++) {
                long long acc = 0;
                const std::vector<long long> lo = stage_offsets(S, per[l], B, &acc);
                std::copy(lo.begin(), lo.end(), off.begin() + P.inv_lvl_first[l]);
                P.inv_lvl_nact[l].push_back((int)lo.size());
            }
            P.inv_lvl_toff.push_back(off);
        }
    }
    {   // the highest level a sweep task or a one-workgroup subtree reaches: the bottom of the forward sweep starts behind it
        int &btl = P.bottom_top_level;
        for (size_t t = 0; t < S.swt_last.size(); t++) btl = std::max<int>(btl, S.level[S.swt_last[t]]);
        for (i32 s = 0; s < ns; s++) if (S.in_subtree[s]) btl = std::max<int>(btl, S.level[s]);
        btl = std::min<int>(btl, std::max<int>(S.nlevels - 1, 0));
        // The bottom of the forward sweep is throughput work whose workgroups hold a CU's LDS for their whole life; started
        // while the factorisation still is throughput work itself (the wide middle of the tree) it only takes the chip away
        // from it. It is held back until the factorisation reaches its latency-bound top: the first level from which on every
        // level has at most 32 fronts (re-swept in round 4: 4 .. 10 levels below the root are within 0.2 ms of it).
        int gate = S.nlevels - 1;
        while (gate > 0 && P.levels[gate - 1].count <= 32) gate--;
        P.fused_gate_level = std::min<int>(std::max(gate, btl), std::max<int>(S.nlevels - 1, 0));
    }

    // Contribution-block tiles of every level in hand-out order: front by front (the level list's order), inside a
    // front by 8 x 8-tile squares of the lower triangle (row-major inside a square), then cut into 8 runs of equal
    // estimated cost -- one per XCD. One self-contained record per tile (factor_kernels.hip, k_syrk_cb_rec).
    std::vector<double> cost;
    constexpr int SQ = 8;
    for (i32 l = 0; l < S.nlevels; l++) {
        LevelInfo &L = P.levels[l];
        cost.clear();
        L.syrk_off = (long long)P.syrk_recs.size();
        for (int k = L.nsmall; o.syrk_xcd && k < L.count; k++) {
            const i32 s = S.levellist[L.first + k];
            const int c = S.ncols(s), m = S.nrows(s) - c;
            const int T = (m + 63) / 64, nT = (m + 31) / 32;
            const i64 ch0 = S.childptr[s];
            const int nch = (int)(S.childptr[s + 1] - ch0);
            for (int I = 0; I < T; I += SQ)
                for (int J = 0; J <= I; J += SQ)
                    for (int bi = I; bi < std::min(I + SQ, T); bi++)
                        for (int bj = J; bj < std::min(J + SQ, bi + 1); bj++) {
                            // k-loop of 3 (diagonal tile) or 4 waves + the gather / epilogue of a tile, in columns of K
                            cost.push_back((double)(c + 48) * (bi == bj ? 3 : 4));
                            SyrkTile t{};
                            t.pa = (long long)S.panelptr[s] + c;
                            t.cb = (long long)S.cbptr[s];
                            t.ch0 = (long long)ch0;
                            t.c = c; t.m = m; t.ld = (int)S.ld[s]; t.nch = nch;
                            t.bi = bi; t.bj = bj;
                            for (int q = 0; q < std::min(nch, 2); q++) {
                                const EdgeRec &e = P.edge[ch0 + q];
                                const int *et = P.etile.data() + e.tptr;
                                t.reloff[q] = e.reloff; t.cboff[q] = e.cboff; t.md[q] = e.md;
                                t.a0[q] = et[2 * bi]; t.a1[q] = et[std::min(2 * bi + 2, nT)];
                                t.b0[q] = et[2 * bj]; t.b1[q] = et[std::min(2 * bj + 2, nT)];
                            }
                            P.syrk_recs.push_back(t);
                        }
        }
        cut_xcd_runs(cost, L.syrk_split, &L.syrk_per, "contribution-block");
    }
    if (P.syrk_recs.empty()) P.syrk_recs.push_back(SyrkTile{});
    // forward update: one record per 32-row tile of the trailing rows of every big front of the SWEEP levels, front
    // by front, cut into 8 runs of equal cost (a front's tiles share its y and its children's update vectors)
    for (i32 l = 0; l < S.nlevels; l++) {
        LevelInfo &L = P.swlevels[l];
        cost.clear();
        L.fwd_off = (long long)P.fwd_recs.size();
        for (int k = L.nsmall; o.syrk_xcd && k < L.count; k++) {
            const i32 s = S.sw_levellist[L.first + k];
            const int c = S.ncols(s), r = S.nrows(s), m = r - c;
            const i64 ch0 = S.childptr[s];
            const int nch = (int)(S.childptr[s + 1] - ch0);
            for (int T = 0; T * 32 < m; T++) {
                FwdTile t{};
                t.pp = (long long)S.panelptr[s]; t.xoff = S.sfirst[s]; t.woff = S.wptr[s]; t.ch0 = (long long)ch0;
                t.c = c; t.r = r; t.ld = (int)S.ld[s]; t.i0 = c + 32 * T; t.nch = nch; t.tile = T;
                for (int q = 0; q < std::min(nch, 2); q++) {
                    const EdgeRec &e = P.edge[ch0 + q];
                    t.md[q] = e.md; t.reloff[q] = e.reloff; t.cwoff[q] = e.woff;
                    t.a0[q] = P.etile[(size_t)e.tptr + T]; t.a1[q] = P.etile[(size_t)e.tptr + T + 1];
                }
                P.fwd_recs.push_back(t);
                cost.push_back((double)(c + 64));
            }
        }
        cut_xcd_runs(cost, L.fwd_split, &L.fwd_per, "update-vector");
    }
    if (P.fwd_recs.empty()) P.fwd_recs.push_back(FwdTile{});
    // panel-assembly records, one per level-list position
    P.arec.resize(S.levellist.size());
    for (size_t k = 0; k < S.levellist.size(); k++) {
        const i32 s = S.levellist[k];
        AsmRec a{};
        a.pp = (long long)S.panelptr[s];
        a.ch0 = (long long)S.childptr[s];
        a.c = S.ncols(s); a.ld = (int)S.ld[s]; a.first = (int)S.sfirst[s];
        a.nch = (int)(S.childptr[s + 1] - S.childptr[s]);
        for (int q = 0; q < std::min(a.nch, 2); q++) {
            const EdgeRec &e = P.edge[a.ch0 + q];
            a.reloff[q] = e.reloff; a.cboff[q] = e.cboff; a.eoff[q] = e.eoff; a.md[q] = e.md;
        }
        P.arec[k] = a;
    }
    if (P.arec.empty()) P.arec.push_back(AsmRec{});

    P.first_multiblock_level = S.nlevels;
    // (over the SWEEP lists: the forward sweep waits there for the dense inverses, and a sharded handle's factor lists leave
    //  out the distributed root, which its owner still sweeps)
    for (i32 l = 0; l < S.nlevels; l++) if (P.swlevels[l].max_cols > NB) { P.first_multiblock_level = l; break; }
    P.l_size = S.panelptr[ns];
    return P;
}

}  // namespace gmrfx
