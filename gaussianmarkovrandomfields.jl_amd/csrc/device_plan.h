// device_plan.h -- the host images of the tables the kernels read and the level schedule the drivers keep, built from the
// symbolic analysis on the host (device_plan.cpp, no HIP); Device::upload copies the tables to the device as they are.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "symbolic.h"

namespace gmrfx {

constexpr int NB = 64;       // block-column width of the dense partial factorisation / sweeps
// chunk form of the sweep tasks (sweep_chunk.hip): right-hand-side columns of a workgroup's local vector, and its spare row
// (row 288 of 289: target rows of padding land there)
constexpr int kChunkNc = 16;
constexpr int kChunkSpareRow = 288;
// wave tasks (sweep_wave.hip): the LDS classes of the tasks, by rows of the local vector
constexpr int kWaveClasses = 2;
constexpr int kWaveRows[kWaveClasses] = {160, 288};

// One record per (child -> parent) edge of the assembly tree, in childptr order: everything a
// parent's workgroup needs to gather from that child, in ONE load instead of a chain of dependent
// index loads (children[ch] -> sfirst/rowptr/cbptr/wptr[d] -> ...).
struct EdgeRec {
    int d, md;         // child supernode and its number of trailing rows
    int tptr;          // offset of this edge's tile table in DevSym::etile
    int nown;          // child rows that map into the parent's OWN columns (= etile[tptr])
    long long reloff;  // offset of the child's trailing rows in DevSym::rel
    long long woff;    // DevSym::wptr[d]
    long long cboff;   // DevSym::cbptr[d]
    long long eoff;    // offset of this edge's column table in DevSym::erow
};

// One sweep task (Symbolic::swt_*): everything its workgroup needs in ONE load.
struct SweepTask {
    int s0, s1;            // first / last (= root) supernode
    int col0, nt;          // first own column of the subtree, number of own columns (= local rows 0 .. nt-1)
    int mroot, pad;        // trailing rows of the root (= local rows nt .. nt+mroot-1)
    long long p0, p1;      // the subtree's panels in the factor storage (contiguous: postorder)
    long long rp0, rp1;    // its range in the row / local-row lists
    long long rroot;       // offset of the root's trailing rows in DevSym::rows
    long long woff;        // DevSym::wptr[root]
    // chunk form (sweep_chunk.hip; Symbolic::swc_*): first chunk record / number of chunks, the backward programs of the four
    // row-tile slots (chunks per slot, barriers behind a slot's last chunk)
    int c0, nch;           // forward records
    int b0, nbw;           // backward records (every chunk once)
    int scnt[4], sbar[4];
};

// geometry of one front for the panel kernels, one record per level-list position (the panel chain gets it in the kernel
// arguments instead: FrontArg, device.h)
struct FrontView { int s, c, r, ld, first, pad; long long pp; };   // 32 bytes

// Everything a column of the panel assembly (k_assemble_lds) needs to know about its front and the front's first two children,
// in ONE 96-byte record per level-list position (one scalar load) instead of front -> geometry arrays -> edge records.
struct AsmRec {
    long long pp;            // panel offset in the factor storage
    long long ch0;           // first child edge (children beyond the second go the long way)
    int c, ld, first, nch;   // columns, leading dimension, first global column, number of children
    long long reloff[2], cboff[2], eoff[2];     // per child: rel[] offset of its trailing rows, arena offset of its contribution block, erow offset
    int md[2];               // per child: trailing rows
    int pad[2];
};

struct SyrkSplit { int start[9]; };   // tile runs of the 8 XCDs inside a level's tile list

// Everything a workgroup of k_syrk_cb_rec needs for one 64 x 64 contribution-block tile, in ONE 128-byte record (one
// scalar load) instead of four rounds of dependent index loads (tile -> front geometry -> edge records -> tile ranges):
// the levels with narrow fronts spend their time in exactly that chain.
struct SyrkTile {
    long long pa;            // offset of L21 (panel + c rows down) in the factor storage
    long long cb;            // offset of the front's contribution block in the arena
    long long ch0;           // first child edge of the front (children beyond the second go the long way)
    int c, m, ld, nch;       // columns, trailing rows, leading dimension, number of children
    int bi, bj, pad0, pad1;  // tile row / column
    long long reloff[2], cboff[2];   // first two children: relative-row list, contribution block
    int md[2];                       //   trailing rows of the child
    int a0[2], a1[2], b0[2], b1[2];  //   the child's rows that fall into the tile's rows [a0, a1) / columns [b0, b1)
};
static_assert(sizeof(SyrkTile) == 128, "SyrkTile is one 128-byte record");

// The same idea for the forward update of a big front (k_fwd_update_rec): one record per 32-row tile of the trailing rows.
struct FwdTile {
    long long pp;            // offset of the front's panel in the factor storage
    long long xoff;          // first own row of the front in X (= sfirst)
    long long woff;          // first row of the front's update vector in W (= wptr)
    long long ch0;           // first child edge (children beyond the second go the long way)
    int c, r, ld, i0;        // columns, rows, leading dimension, first front row of the tile (>= c)
    int nch, tile;           // number of children, 32-row tile index (for the long way)
    int md[2], a0[2], a1[2]; // first two children: trailing rows, and the rows [a0, a1) that fall into this tile
    int pad[4];
    long long reloff[2], cwoff[2];   // their relative-row lists and update vectors
};
static_assert(sizeof(FwdTile) == 128, "FwdTile is one 128-byte record");

// What k_sel_gather needs about a front and its parent, in one 64-byte record per supernode (selected inversion).
struct SelRec {
    long long rel;           // offset of the front's trailing rows in DevSym::rel
    long long zp;            // parent's panel in Z
    long long zbp;           // parent's trailing inverse block in the arena (selected-inversion layout)
    long long out;           // this front's trailing inverse block
    int m, cp, mp, ldp;      // trailing rows; parent's columns, trailing rows, leading dimension
    int p, foreign, pad[2];  // parent (-1: root), 1 = the block arrives over the wire (sharded)
};
static_assert(sizeof(SelRec) == 64, "SelRec is 64 bytes");

struct LevelInfo {
    int first;        // offset into levellist
    int count;        // fronts in level
    int nsmall;       // prefix handled by the fused small-front kernels
    int ncls[4];      // of which r <= 48 / 64 / 96 / 128 (in this order)
    int max_rows;     // over big fronts
    int max_cols;     // over big fronts (they are sorted by decreasing column count)
    int max_trail = 0; // most trailing rows of a big front
    int min_trail = 0; // fewest trailing rows of a big front with any (0: none has)
    int wider[3] = {0, 0, 0}; // big fronts with more than 48 / 32 / 16 columns (first 64-column block: the diagonal-block kernel's shapes)
    // contribution-block SYRK: the level's 64 x 64 tiles in the order they are handed out, cut into one run per XCD
    long long syrk_off = 0;   // offset of the level's tiles in Device::d_syrk_recs_
    SyrkSplit syrk_split{};   // run of XCD x = [start[x], start[x + 1])
    int syrk_per = 0;         // longest run: the grid is 8 * syrk_per workgroups
    // forward update (sweep levels only): 32-row tiles of the trailing rows, same per-XCD hand-out
    long long fwd_off = 0;
    SyrkSplit fwd_split{};
    int fwd_per = 0;

    int nbig() const { return count - nsmall; }             // big fronts: positions nsmall .. count - 1 of the level's list
    int nblk() const { return (max_cols + NB - 1) / NB; }   // 64-column blocks of the widest big front
    // Big fronts with more than `cols` columns, cols a multiple of NB: they are the first wider_than(cols) of the width-sorted
    // list of big fronts. 0 from max_cols on, however large cols is.
    int wider_than(int cols) const { const size_t k = (size_t)cols / NB; return k < wider_blk_.size() ? wider_blk_[k] : 0; }
    void set_block_counts(std::vector<int> counts) { wider_blk_ = std::move(counts); }   // (level_infos: one per block of nblk())
private:
    std::vector<int> wider_blk_;   // [k] = big fronts with more than k NB columns, k < nblk()
};

constexpr int kSyrkPipedMinCols = 128;     // see EnvKnobs::syrk_piped_min (kernels.h: the measurement)
// The environment's testing / A/B / profiling knobs, read once per handle (Device::init; a clone reads them again).
struct EnvKnobs {
    int inv_cap = 2048;          // GMRFX_INV_CAP: testing knob, rounded up to a power of two >= 64 (the default: Device::inv_cap_)
    int wave_max_nr = 16;        // GMRFX_TASK_MODE = wg / wave: 0 / 64. Passes of up to this many right-hand sides use the wave tasks (0: never)
    bool level_mark = false;     // GMRFX_LEVEL_MARK=1: an empty marker kernel in front of every level (profiling aid, tools/sweep_levels.py)
    int fwd_front_min = 384;     // GMRFX_FWD_FRONT. The forward twin (k_fwd_front): levels with at least this many such fronts (measured at cfg 2, round 6, one workgroup per
                                 // front against the three launches, us: level 5 (1472 fronts) 103 / 128, 6 (2271) 167 / 211, 7 (1034) 159 / 207, 8 (513) 103 / 131,
                                 // 9 (256, 236 of them eligible) 103 + 58 / 113: a level needs about two workgroups per compute unit)
    int bwd_front_min = 192;     // GMRFX_BWD_FRONT. Backward step of fronts <= 128 columns wide as one workgroup (sweep_front.hip) on levels with at least this many of them (0: never)
    bool syrk_xcd = true;        // GMRFX_SYRK_XCD=0: k_syrk_cb on a plain 3-D grid (front, tile row, tile column) instead, and no tile records at all
    int syrk_piped_min = kSyrkPipedMinCols;    // GMRFX_SYRK_PIPED=N: levels whose widest front has >= N columns take the software-pipelined
                                 // product loop of k_syrk_cb_rec (0: every level; a huge N: none) -- same bits either way
};
EnvKnobs read_env_knobs();

// ---- the sweeps' per-level decisions: which fronts of a level's width-sorted list of big fronts go to which launch -----------------
// Plain functions of values (no device, no HIP): Device::forward / backward read the plan and launch; tools/sanitize_host.cpp
// walks every level of its plans through them.
// Passes of at most kNarrowPassMax right-hand sides, forward: the fronts up to kFwdWaveCols columns wide go one WAVE per 32-row tile
// (no LDS, no barrier: k_fwd_update_wave), chosen per FRONT so that a front's sums do not depend on the list it comes in
constexpr int kFwdWaveCols = 1024;      // (measured at cfg 2, 1 RHS, forward ms, with four waves sharing the K range of a front wider than 128
                                        //  columns: 256: 0.933, 512: 0.841, 1024: 0.832, 2048: 0.836)
// Passes of at most kNarrowPassMaxBwd right-hand sides, backward: t = y - L21' x one WAVE per 16 own columns for the fronts with at
// most kBwdWaveRows trailing rows (k_bwd_wave), the split-K kernels for the others, x = L11^-T t as everywhere
constexpr int kBwdWaveRows = 4096;      // (every front of a 2-D problem; measured at cfg 2, 1 RHS, backward ms, with four waves sharing the K range of a front of more than 256
                                        //  rows: 768: 0.848, 1100: 0.824, 1600: 0.814, every front: 0.792; one wave per tile only: 768 was the optimum, 1.177)

// What the decisions read besides the level: the handle's knobs and the limits of the launch side (the constants below; Device::sweep_knobs)
struct SweepKnobs {
    int inv_cap;                     // Device::inv_cap_: wider fronts substitute block by block
    int fwd_front_min, bwd_front_min;   // EnvKnobs
    bool tile_records;               // EnvKnobs::syrk_xcd: the forward update's tile records exist
    int narrow_pass_max, narrow_pass_max_bwd;   // kNarrowPassMax / kNarrowPassMaxBwd: widest pass of the narrow level kernels
    int front_max_cols;              // kFrontMaxCols: widest front of the one-workgroup front kernels
    int wave_split_cols, wave_split_rows;       // kWaveSplitCols / kWaveSplitRows
};

// How a level's big fronts are split between the one-workgroup front kernel and the blocked substitution. The list is sorted by
// decreasing width: [0, nf) is the head, [nf, nf + ntail) the tail.
struct LevelBlocks {
    const LevelInfo *L;
    int inv_cap;
    int ntail;    // the narrow tail, every front at most min(front_max_cols, inv_cap) columns wide: its WHOLE step is k_fwd_front's / k_bwd_front's (0: not used)
    int nf;       // the head: everything below runs on these fronts only
    int nbk;      // blocks of inv_cap columns of the widest front (1: every front multiplies by its whole inverse)
    // launch_xmul of block j: the head fronts wider than j inv_cap (block 0: the whole head -- never the tail, which is finished)
    int xmul_fronts(int j) const { return std::min(nf, L->wider_than(j * inv_cap)); }
    // own-rows update of block j (launch_fwd_own_update / launch_bwd_gemm, j + 1 < nbk): the head fronts that have a block j + 1
    int own_fronts(int j) const { return std::min(nf, L->wider_than((j + 1) * inv_cap)); }
};
struct FwdLevelPlan : LevelBlocks {
    int cmin;             // head fronts up to this width are not the split-K update's: kFwdWaveCols with the wave kernel, the tail's width bound with k_fwd_front
    bool wave;            // launch_fwd_update_wave runs (cmax = cmin): some head front is at most kFwdWaveCols wide
    bool wave_split_k;
    enum Update { kNone, kRecords, kGrid } update;   // W -= L21 y of the head fronts wider than cmin: none left / record-driven / plain grid
};
struct BwdLevelPlan : LevelBlocks {
    int mmin;             // head fronts with at most this many trailing rows are not the split-K product's (kBwdWaveRows with the wave kernel)
    bool wave;            // launch_bwd_wave runs (mmax = mmin)
    bool wave_split_k;
    bool gemm;            // launch_bwd_gemm over all blocks runs: some head front has more than mmin trailing rows
};
FwdLevelPlan plan_forward_level(const LevelInfo &L, int nr, const SweepKnobs &k);
BwdLevelPlan plan_backward_level(const LevelInfo &L, int nr, const SweepKnobs &k);

// ---- the launch wrappers' choices: which variant of a kernel a launch gets, and its geometry -----------------------------------------
// Plain functions of values as well: a wrapper (kernels.h) returns on kNoLaunch, switches on the variant and launches with this grid,
// block and dynamic LDS; tools/sanitize_host.cpp pins every threshold and walks every level of its plans through them.
constexpr int ASM_CW = 4;    // front columns owned by one assembly workgroup
constexpr int FWD_RB = 32;    // front rows owned by one forward-assembly workgroup
// Columns through LDS, written once: a wave per column while four columns of a workgroup fit in 40 KB, a workgroup per column
// for the tall columns of the top of the tree (up to 128 KB). Measured at cfg 2 (factorisation): HBM assembly above 1280 rows
// 9.33 ms; wave-per-column up to 2048 rows 9.10; + workgroup-per-column above: 9.03; wave-per-column up to 1280, workgroup-per-column
// above: 8.96.
constexpr int kAsmLdsWaveMaxRows = 1280, kAsmLdsWgMaxRows = 16384;
constexpr int kAsmHbmWgMaxGroups = 2200;     // HBM form: one WORKGROUP per column up to this many four-column groups (levels with a few tall fronts)
constexpr int kTrsmSplitMaxTiles = 128;      // k_trsm<MODE, 1> (16 rows per workgroup instead of 128) up to this many 64-row tiles
// k_gemm_nt_big is only used where a launch has thousands of such tiles: K a multiple of 16, at least 4096 rows below the block
constexpr int kGemmBigKStep = 16, kGemmBigMinK = 256, kGemmBigMinM = 4096, kGemmBigMinN = 512;
// Levels with a handful of fronts are latency bound: 32x32 workgroup tiles there (four times
// the workgroups, a quarter of the MFMA chain per wave).
constexpr int kGemmSmallTileMax = 256;       // ... up to this many 64x64 tiles
constexpr int kFwdUpdate16MaxTiles = 128;    // k_fwd_update_longk<1> (16-row tiles) up to this many 32-row tiles: the handful-of-fronts levels
// the 8-wave variants up to ~3 workgroups per CU (measured: 512-1024 beats 128 and 2048). Every workgroup of a front gathers ALL
// of the front's trailing rows of x: 32 own columns per workgroup instead of 16 halves those re-reads (levels 10-13 of cfg 2
// moved 2.5-3 x their algorithmic bytes) on levels that still fill the chip with them (measured at cfg 2, 32 / 16 columns per
// workgroup: level 10 (768 workgroups of 32) 72 / 83 us, 11 (576) 79 / 88; 12 (352) 79 / 73, 13: 85 / 75, 14: 66 / 55, 15: 62 / 47)
constexpr int kBwdGemmWide8Min = 384, kBwdGemm8Max = 768;      // workgroups of 32 own columns: <1, 8> below, <2, 8> inside, <2, 4> above
constexpr int kPermuteNarrowMaxNr = 8;       // k_permute_narrow: passes of at most 8 right-hand sides
// Passes of up to 32 right-hand sides take the narrow FORWARD kernels (k_fwd_update_wave, k_xmul_narrow) on two right-hand-side tiles
// (round 6; measured at cfg 2, tools/nrhs_sweep.py: 17 / 24 / 32 columns 3.22 / 3.29 / 3.35 -> 2.98 / 3.05 / 3.09 ms; the same on three
// or four tiles loses: 48 columns 3.54 -> 3.85 ms). The BACKWARD kernels of such passes stay the 64-column ones -- k_bwd_front /
// k_bwd_gemm_longk beat k_bwd_wave on two tiles (backward 1.39 vs 1.42-1.47 ms) --, and so do the bottom tasks (chunk form on two column
// slices: 2.98 ms at 17 columns against 3.37 with one wave per task and tile).
// widest pass (right-hand sides) that takes the narrow level kernels -- one wave / one right-hand-side tile per workgroup, grid z (y
// for k_fwd_update_wave) = ceil(nr / 16) tiles: k_fwd_update_wave, k_bwd_wave, k_xmul_narrow
constexpr int kNarrowPassMax = 32, kNarrowPassMaxBwd = 16;
// k_fwd_update_wave<4> / k_bwd_wave<4>: four waves share the K range of a front wider than this / with more trailing rows than this
constexpr int kWaveSplitCols = 128, kWaveSplitRows = 256;
constexpr int kFrontMaxCols = 128;           // columns of a front the one-workgroup front kernels take (sweep_front.hip)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// Workgroups are handed to the 8 XCDs round-robin by linear id (x fastest). Rectangular grids whose
// x extent (or x*y extent) is a multiple of 8 put tile (bi, bj) of EVERY front on the same XCD --
// with triangular / ragged tile sets that leaves some XCDs idle and others with twice the work
// (measured: the 4x4-tile level of k_syrk_cb ran 1.9x longer than the 3x3 and 6x6 levels around
// it). Odd extents make consecutive fronts rotate through all XCDs; the extra workgroups exit at
// once through the kernels' own range checks.
inline unsigned odd(int v) { return (unsigned)(v | 1); }
inline int asm_ldmax(int max_rows) { return (max_rows + 1) & ~1; }       // Symbolic rounds ld up to even

enum KernelVariant {
    kNoLaunch,                                                            // an empty launch: the wrapper returns
    kAssembleLdsWave, kAssembleLdsWg, kAssembleHbmWg, kAssembleHbmWave,   // k_assemble_lds<0> / <1>, k_assemble<1> / <0>
    kTrsmSplit, kTrsmWhole,                                               // k_trsm<MODE, 1> / <MODE, 0>
    kGemmNtBig, kGemmNt32, kGemmNt64,                                     // k_gemm_nt_big, k_gemm_nt<1> / <2>
    kFwdUpdate16, kFwdUpdate32,                                           // k_fwd_update_longk<1> / <2>
    kBwdGemm16x8, kBwdGemm32x8, kBwdGemm32x4,                             // k_bwd_gemm_longk<1, 8> / <2, 8> / <2, 4>
    kPermuteNarrow, kPermuteTiles,                                        // k_permute_narrow, k_permute
    kWaveWhole, kWaveSplitK,                                              // k_fwd_update_wave / k_bwd_wave <1> / <4>
    kFwdOwnUpdate,
    kGradPattern, kGradMubar, kGradDot,                                   // k_grad_pattern, k_grad_mubar, k_grad_dot_part (grad.hip)
    kVariantCount
};
struct Launch {
    KernelVariant variant = kNoLaunch;
    unsigned gx = 0, gy = 1, gz = 1, block = 0;
    size_t lds = 0;             // dynamic LDS bytes
    bool raised_lds = false;    // lds is more than the 64 KB a kernel may ask for as it is: the wrapper raises the kernel's limit first
};
// (launch_assemble falls back to the HBM choice when the limit cannot be raised)
Launch choose_assemble(int nfronts, int max_cols, int max_rows);
Launch choose_assemble_hbm(int nfronts, int max_cols);
Launch choose_trsm(int nactive, int max_rows_below);
Launch choose_gemm_nt(int nactive, int K, int maxM, int maxN);
Launch choose_fwd_update(int nfronts, int max_trail);
Launch choose_fwd_update_wave(int per_xcd, int nr, bool split_k);
Launch choose_fwd_own_update(int nfronts, int max_cols, int blk, int cap);    // own rows below block blk of `cap` columns
Launch choose_bwd_gemm(int nfronts, int max_cols, int blk, int cap);          // blk >= 0: the own columns of that block only
Launch choose_bwd_wave(int nfronts, int max_cols, int nr, bool split_k);
Launch choose_permute(int n, int nr);
// grad.hip -- log-density gradients on Q's pattern. A lane group of kGradLanes lanes walks one column (pattern kernel) or one row of
// symmetric Q (mean kernel) in passes of kGradLanes entries; a workgroup of 256 threads is 16 such groups. The pattern kernel gives a
// group kGradColsPerGroup columns, so a workgroup owns kGradCols consecutive columns. The contraction sums fixed chunks of
// kGradDotChunk stored entries per workgroup (the sums' order depends on it). Members of a batch ride in grid y (z: the contraction).
constexpr int kGradLanes = 16, kGradColsPerGroup = 4, kGradCols = 16 * kGradColsPerGroup, kGradRows = 16;
constexpr int kGradDotChunk = 4096;
Launch choose_grad_pattern(int n, int nbatch);
Launch choose_grad_mubar(int n, int nbatch);
Launch choose_grad_dot(long long nnz, int p, int nbatch);

// What changes the tables besides the analysis.
struct PlanOptions {
    bool syrk_xcd = true;       // GMRFX_SYRK_XCD: tile records of the contribution-block SYRK and the forward update (false: none)
    int chunk_nc = kChunkNc, chunk_spare_row = kChunkSpareRow;   // layout of the local vector the chunk target rows address
};

struct DevicePlan {
    // tables: every array Device::upload builds, in its device form (arrays of the analysis that already have it go up directly)
    std::vector<SelRec> selrec;                   // one per supernode
    std::vector<int> qsrc, qdst, qcol, qcolptr;   // the scatter map split into row and column (DevSym)
    std::vector<EdgeRec> edge;
    std::vector<int> etile, erow;
    std::vector<unsigned char> owncol, foreign_parent;   // sharded handles only
    std::vector<int> fchild;                             //   (grouped by level: fc_levelptr)
    std::vector<SweepTask> swt;
    std::vector<int> swc_listf, swc_listb;        // chunk target rows as LDS byte offsets (only with chunks)
    std::vector<int> wave_order;
    std::vector<int> levellist2;                  // the level lists with every level's big fronts split into even / odd positions
    std::vector<FrontView> frec, frec2, sel_frec; // parallel to levellist, levellist2, sel_levellist
    std::vector<int> invlist;                     // dense-inverse stages: fronts by decreasing width ...
    std::vector<std::vector<long long>> inv_toff; // ... the T-buffer offsets of each stage
    std::vector<int> inv_lvl_list;                // the same level by level (empty: no multi-block front)
    std::vector<std::vector<long long>> inv_lvl_toff;
    std::vector<SyrkTile> syrk_recs;
    std::vector<FwdTile> fwd_recs;
    std::vector<AsmRec> arec;
    // schedule: what the drivers read on the host (Device keeps each in its member of that name: levels -> levels_)
    std::vector<LevelInfo> levels, swlevels;
    std::vector<int> sel_max_cols, sel_max_trail;
    int inv_maxc = 0;
    long long inv_tsize = 0;                      // doubles of the dense-inverse workspace
    std::vector<int> inv_nact, inv_lvl_first, inv_lvl_maxc;
    std::vector<std::vector<int>> inv_lvl_nact;
    std::vector<int> fc_levelptr, fc_maxtrail;
    int wave_first[kWaveClasses] = {}, wave_count[kWaveClasses] = {};
    int nsub_cls[3] = {};
    int bottom_top_level = 0, fused_gate_level = 0, first_multiblock_level = 0;
    double syrk_flops = 0;
    long long sum_trail = 0, l_size = 0, nq = 0;
    int nswt = 0, nswc = 0;
};

// Throws std::runtime_error when a table outgrows its index type.
DevicePlan build_device_plan(const Symbolic &S, const PlanOptions &o);

}  // namespace gmrfx
