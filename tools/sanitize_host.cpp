// sanitize_host.cpp -- CPU-only sanitizer job for the host C++ of libgmrfx: the symbolic phase
// (ordering.cpp, symbolic.cpp) spawns threads, the C ABI (api_*.cpp) parses caller arrays, device_plan.cpp builds the device
// tables with index arithmetic over the analysis (called directly: it needs no device). Built twice by
// `make -C gaussianmarkovrandomfields.jl_amd sanitize` (AddressSanitizer + UBSan, ThreadSanitizer) from the SAME
// sources as the product, driven through the C ABI with symbolic_only handles (no GPU is touched; the HIP kernel
// launch wrappers stay unresolved and are never called). Exit code 0 = clean. Run by tests/test_sanitizers.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../gaussianmarkovrandomfields.jl_amd/csrc/device_plan.h"
#include "../gaussianmarkovrandomfields.jl_amd/csrc/ga_rules.h"
#include "../include/gmrfx.h"

// 19-point pattern of (5-point Laplacian)^2 on an nx x ny grid, both triangles, 0-based
static void grid_pattern(int nx, int ny, std::vector<int64_t> &cp, std::vector<int64_t> &ri, std::vector<double> &xy) {
    const int64_t n = (int64_t)nx * ny;
    cp.assign(n + 1, 0);
    ri.clear();
    xy.resize(2 * n);
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const int64_t v = (int64_t)j * nx + i;
            xy[2 * v] = i; xy[2 * v + 1] = j;
            for (int dj = -2; dj <= 2; dj++)
                for (int di = -2; di <= 2; di++) {
                    if (std::abs(di) + std::abs(dj) > 2) continue;
                    const int a = i + di, b = j + dj;
                    if (a < 0 || b < 0 || a >= nx || b >= ny) continue;
                    ri.push_back((int64_t)b * nx + a);
                }
            cp[v + 1] = (int64_t)ri.size();
        }
}

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "FAILED: %s (line %d)\n", #c, __LINE__); fails++; } } while (0)

static void one_handle(const std::vector<int64_t> &cp, const std::vector<int64_t> &ri, const double *coords, int64_t n, int ordering) {
    gmrfx_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (int32_t)sizeof(o);
    o.device = -1; o.symbolic_only = 1; o.ordering = ordering;
    if (coords) { o.coord_dim = 2; o.coords = coords; }
    gmrfx_handle *h = nullptr;
    EXPECT(gmrfx_create(n, cp.data(), ri.data(), 0, nullptr, &o, &h) == GMRFX_OK);
    if (!h) return;
    std::vector<int64_t> perm(n);
    EXPECT(gmrfx_get_perm(h, 0, perm.data()) == GMRFX_OK);
    std::vector<char> seen(n, 0);
    for (int64_t k = 0; k < n; k++) { EXPECT(perm[k] >= 0 && perm[k] < n && !seen[perm[k]]); if (perm[k] >= 0 && perm[k] < n) seen[perm[k]] = 1; }
    gmrfx_stats st;
    EXPECT(gmrfx_get_stats(h, &st, (int32_t)sizeof(st)) == GMRFX_OK);
    EXPECT(st.nnz_l >= st.nnz_q_tri && st.nsuper > 0);
    double x = 0;
    EXPECT(gmrfx_logdet(h, &x) == GMRFX_ERR_NO_DEVICE);          // numeric entry points fail loudly without a device
    // a second handle with the first one's permutation (user-permutation path), cloned and destroyed
    gmrfx_handle *h2 = nullptr, *h3 = nullptr;
    EXPECT(gmrfx_create(n, cp.data(), ri.data(), 0, perm.data(), &o, &h2) == GMRFX_OK);
    if (h2) {
        // linear equality constraints on a symbolic handle: the host side of gmrfx_constraints_set (sorting, summed duplicates,
        // log det(A A')), each refused form, and the copy a clone carries
        std::vector<int64_t> rp = {0, n, n + 3}, ci((size_t)n + 3);
        std::vector<double> va((size_t)n + 3, 1.0), e = {0.0, 1.0};
        for (int64_t j = 0; j < n; j++) ci[(size_t)j] = n - 1 - j;
        ci[(size_t)n] = 2; ci[(size_t)n + 1] = 0; ci[(size_t)n + 2] = 2;
        int64_t m = -1;
        double lda = 0, ldw = 0;
        EXPECT(gmrfx_constraints_set(h2, 2, rp.data(), ci.data(), va.data(), 0, e.data()) == GMRFX_OK);
        EXPECT(gmrfx_constraints_info(h2, &m, nullptr, &lda, nullptr) == GMRFX_OK && m == 2 && lda > 0);
        EXPECT(gmrfx_constraints_info(h2, &m, &ldw, nullptr, nullptr) == GMRFX_ERR_NO_DEVICE);
        EXPECT(gmrfx_constraints_var(h2, va.data()) == GMRFX_ERR_NO_DEVICE);
        ci[1] = n;
        EXPECT(gmrfx_constraints_set(h2, 2, rp.data(), ci.data(), va.data(), 0, e.data()) == GMRFX_ERR_INVALID_ARG);
        std::vector<int64_t> rp2 = {0, 2, 2}, rp3 = {0, 2, 1};
        EXPECT(gmrfx_constraints_set(h2, 2, rp2.data(), ci.data() + n, va.data(), 0, e.data()) == GMRFX_ERR_INVALID_ARG);
        EXPECT(gmrfx_constraints_set(h2, 2, rp3.data(), ci.data() + n, va.data(), 0, e.data()) == GMRFX_ERR_INVALID_ARG);
        EXPECT(gmrfx_constraints_set(h2, 65, rp.data(), ci.data(), va.data(), 0, e.data()) == GMRFX_ERR_INVALID_ARG);
        EXPECT(gmrfx_constraints_info(h2, &m, nullptr, nullptr, nullptr) == GMRFX_OK && m == 2);
        EXPECT(gmrfx_clone(h2, &h3) == GMRFX_OK);
        if (h3) EXPECT(gmrfx_constraints_info(h3, &m, nullptr, nullptr, nullptr) == GMRFX_OK && m == 2);
        EXPECT(gmrfx_constraints_set(h2, 0, nullptr, nullptr, nullptr, 0, nullptr) == GMRFX_OK);
        EXPECT(gmrfx_constraints_info(h2, &m, nullptr, nullptr, nullptr) == GMRFX_OK && m == 0);
        gmrfx_destroy(h3); gmrfx_destroy(h2);
    }
    gmrfx_destroy(h);
}

// a sharded plan (symbolic only): per-rank layouts, groups of the distributed top fronts, the column-range transfer list.
// Every range must lie inside its child's block, start at whole columns, and join two different ranks.
static void sharded_handles(const std::vector<int64_t> &cp, const std::vector<int64_t> &ri, const double *coords, int64_t n, int world) {
    setenv("GMRFX_DIST_MIN", "128", 1);       // small enough for the test grid's top separators
    for (int rank = 0; rank < world; rank++) {
        gmrfx_opts o;
        std::memset(&o, 0, sizeof(o));
        o.struct_size = (int32_t)sizeof(o);
        o.device = -1; o.symbolic_only = 1; o.ordering = 0; o.shard_rank = rank; o.shard_world = world;
        if (coords) { o.coord_dim = 2; o.coords = coords; }
        gmrfx_handle *h = nullptr;
        EXPECT(gmrfx_create(n, cp.data(), ri.data(), 0, nullptr, &o, &h) == GMRFX_OK);
        if (!h) continue;
        int64_t cnt[4] = {0, 0, 0, 0};
        EXPECT(gmrfx_shard_dist_fronts(h, cnt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GMRFX_OK);
        EXPECT(cnt[3] == world && cnt[0] >= 1);
        std::vector<int64_t> front(cnt[0]), cols(cnt[0]), rows(cnt[0]), po(cnt[0]), pl(cnt[0]), lv(cnt[0]), gp(cnt[0] + 1), gr(cnt[1]);
        EXPECT(gmrfx_shard_dist_fronts(h, cnt, front.data(), cols.data(), rows.data(), po.data(), pl.data(), lv.data(), gp.data(), gr.data()) == GMRFX_OK);
        for (int64_t k = 0; k < cnt[0]; k++) {
            EXPECT(gp[k + 1] - gp[k] >= 2 && cols[k] >= 128 && rows[k] >= cols[k] && pl[k] >= rows[k]);
            for (int64_t q = gp[k]; q < gp[k + 1]; q++) EXPECT(gr[q] >= 0 && gr[q] < world && (q == gp[k] || gr[q] > gr[q - 1]));
        }
        std::vector<int64_t> ch(cnt[2]), src(cnt[2]), dst(cnt[2]), lev(cnt[2]), off(cnt[2]), num(cnt[2]), c0(cnt[2]);
        EXPECT(gmrfx_shard_transfers(h, ch.data(), src.data(), dst.data(), lev.data(), off.data(), num.data(), c0.data()) == GMRFX_OK);
        gmrfx_stats st;
        EXPECT(gmrfx_get_stats(h, &st, (int32_t)sizeof(st)) == GMRFX_OK);
        for (int64_t k = 0; k < cnt[2]; k++) {
            EXPECT(src[k] != dst[k] && src[k] >= 0 && src[k] < world && dst[k] >= 0 && dst[k] < world);
            // offsets are per rank: inside this rank's arena when it is an end of the transfer, -1 otherwise
            if (src[k] == rank || dst[k] == rank) EXPECT(off[k] >= 0 && (off[k] + num[k]) * 8.0 <= st.bytes_cb_arena + 1.0);
            else EXPECT(off[k] == -1);
            EXPECT(num[k] > 0 && c0[k] >= 0);
            EXPECT(k == 0 || lev[k] >= lev[k - 1]);
        }
        gmrfx_destroy(h);
    }
    unsetenv("GMRFX_DIST_MIN");
}

// The per-XCD runs of the tile records (contribution-block SYRK, forward update), as the kernels take them: every level's
// split starts at 0 and is monotone, its longest run is `per`, and the levels' records follow each other up to the end of the
// table (a table without records holds one empty record).
static void check_runs(const std::vector<gmrfx::LevelInfo> &LV, bool fwd, size_t nrec, bool any) {
    long long end = 0;
    for (const gmrfx::LevelInfo &L : LV) {
        const gmrfx::SyrkSplit &sp = fwd ? L.fwd_split : L.syrk_split;
        const long long off = fwd ? L.fwd_off : L.syrk_off;
        int per = 0;
        EXPECT(sp.start[0] == 0 && off == end);
        for (int x = 0; x < 8; x++) { EXPECT(sp.start[x] <= sp.start[x + 1]); per = std::max(per, sp.start[x + 1] - sp.start[x]); }
        EXPECT(per == (fwd ? L.fwd_per : L.syrk_per));
        end = off + sp.start[8];
    }
    EXPECT(end == (long long)nrec || (end == 0 && nrec == 1));
    EXPECT(any || end == 0);
}

// The launch choices (device_plan.h, choose_*): what every launch must satisfy, and how many launches reached each variant.
static long long variant_hits[gmrfx::kVariantCount];
static const char *const variant_names[gmrfx::kVariantCount] = {
    "no launch", "k_assemble_lds<0>", "k_assemble_lds<1>", "k_assemble<1>", "k_assemble<0>", "k_trsm<.,1>", "k_trsm<.,0>", "k_gemm_nt_big",
    "k_gemm_nt<1>", "k_gemm_nt<2>", "k_fwd_update_longk<1>", "k_fwd_update_longk<2>", "k_bwd_gemm_longk<1,8>", "k_bwd_gemm_longk<2,8>",
    "k_bwd_gemm_longk<2,4>", "k_permute_narrow", "k_permute", "wave kernel <1>", "wave kernel <4>", "k_fwd_own_update",
    "k_grad_pattern", "k_grad_mubar", "k_grad_dot_part"};
// rows / columns a workgroup of the variant owns along grid x (gemm_nt: and y)
static int variant_tile(gmrfx::KernelVariant v) {
    using namespace gmrfx;
    switch (v) {
    case kAssembleLdsWave: case kAssembleHbmWave: return ASM_CW;
    case kAssembleLdsWg: case kAssembleHbmWg: case kWaveSplitK: case kWaveWhole: return 1;     // (wave kernels: per call site)
    case kTrsmSplit: case kFwdUpdate16: case kBwdGemm16x8: return 16;
    case kGemmNt32: case kFwdUpdate32: case kBwdGemm32x8: case kBwdGemm32x4: case kFwdOwnUpdate: return 32;
    case kGemmNt64: case kPermuteTiles: return 64;
    case kTrsmWhole: case kGemmNtBig: return 128;
    case kPermuteNarrow: return 256;
    default: return 0;
    }
}
// empty: the launch has nothing to do (no variant may be chosen, and one must be otherwise); ox / oy: the odd() rule governs grid x / y;
// ex / ey / ez: the extents the grid has to cover with tx / ty / tz rows, columns or right-hand sides per workgroup (0: the variant's own tile)
static void check_launch(const gmrfx::Launch &c, bool empty, bool ox, bool oy, long long ex, int tx = 0, long long ey = 1, int ty = 1,
                         long long ez = 1, int tz = 1) {
    variant_hits[c.variant]++;
    EXPECT((c.variant == gmrfx::kNoLaunch) == empty);
    if (c.variant == gmrfx::kNoLaunch) return;
    if (!tx) tx = variant_tile(c.variant);
    if (!ty) ty = variant_tile(c.variant);
    EXPECT(c.gx >= 1 && c.gy >= 1 && c.gz >= 1 && c.gy <= 65535 && c.gz <= 65535 && (c.block == 64 || c.block == 256 || c.block == 512));
    EXPECT((long long)c.gx * tx >= ex && (long long)c.gy * ty >= ey && (long long)c.gz * tz >= ez);
    EXPECT((!ox || c.gx % 2 == 1) && (!oy || c.gy % 2 == 1));
    EXPECT(c.lds <= (c.raised_lds ? 131072u : 65536u) && (!c.raised_lds || c.lds > 65536u));
}

// Both sides of every threshold of the choice functions, against the variant and geometry the wrappers used to pick inline.
static void check_launch_edges() {
    using namespace gmrfx;
    auto is = [](const Launch &c, KernelVariant v, unsigned gx, unsigned gy, unsigned gz, unsigned block, size_t lds = 0, bool raised = false) {
        return c.variant == v && c.gx == gx && c.gy == gy && c.gz == gz && c.block == block && c.lds == lds && c.raised_lds == raised;
    };
    // gemm_nt: the 128 x 128 tile needs K % 16 == 0, K >= 256, M >= 4096, N >= 512; then 32 x 32 tiles up to 256 tiles of 64 x 64
    EXPECT(is(choose_gemm_nt(3, 256, 4096, 512), kGemmNtBig, 33, 5, 3, 512));
    EXPECT(choose_gemm_nt(3, 240, 4096, 512).variant == kGemmNt64 && choose_gemm_nt(3, 264, 4096, 512).variant == kGemmNt64);
    EXPECT(choose_gemm_nt(3, 256, 4095, 512).variant == kGemmNt64 && choose_gemm_nt(3, 256, 4096, 511).variant == kGemmNt64);
    EXPECT(is(choose_gemm_nt(1, 64, 1024, 1024), kGemmNt32, 33, 33, 1, 256));           // 16 x 16 tiles = 256
    EXPECT(is(choose_gemm_nt(1, 64, 64 * 257, 64), kGemmNt64, 257, 1, 1, 256));         // 257
    EXPECT(is(choose_gemm_nt(4, 64, 512, 512), kGemmNt32, 17, 17, 4, 256) && choose_gemm_nt(4, 64, 513, 512).variant == kGemmNt64);
    EXPECT(choose_gemm_nt(0, 64, 64, 64).variant == kNoLaunch && choose_gemm_nt(1, 64, 0, 64).variant == kNoLaunch &&
           choose_gemm_nt(1, 64, 64, 0).variant == kNoLaunch);
    // trsm: 64-row tiles x fronts
    EXPECT(is(choose_trsm(1, 64 * 128), kTrsmSplit, 513, 1, 1, 256) && is(choose_trsm(1, 64 * 128 + 1), kTrsmWhole, 65, 1, 1, 256));
    EXPECT(is(choose_trsm(64, 128), kTrsmSplit, 9, 64, 1, 256) && is(choose_trsm(64, 129), kTrsmWhole, 3, 64, 1, 256));
    EXPECT(choose_trsm(0, 5).variant == kNoLaunch && choose_trsm(5, 0).variant == kNoLaunch);
    // fwd_update: 32-row tiles x fronts
    EXPECT(is(choose_fwd_update(1, 32 * 128), kFwdUpdate16, 257, 1, 1, 256) && is(choose_fwd_update(1, 32 * 128 + 1), kFwdUpdate32, 129, 1, 1, 256));
    EXPECT(is(choose_fwd_update(128, 32), kFwdUpdate16, 3, 128, 1, 256) && is(choose_fwd_update(129, 32), kFwdUpdate32, 1, 129, 1, 256));
    EXPECT(choose_fwd_update(0, 5).variant == kNoLaunch && choose_fwd_update(5, 0).variant == kNoLaunch);
    // bwd_gemm: workgroups of 32 own columns
    EXPECT(is(choose_bwd_gemm(1, 32 * 383, -1, 1 << 30), kBwdGemm16x8, 767, 1, 1, 512));
    EXPECT(is(choose_bwd_gemm(1, 32 * 384, -1, 1 << 30), kBwdGemm32x8, 385, 1, 1, 512));
    EXPECT(is(choose_bwd_gemm(768, 32, -1, 1 << 30), kBwdGemm32x8, 1, 768, 1, 512));
    EXPECT(is(choose_bwd_gemm(769, 32, -1, 1 << 30), kBwdGemm32x4, 1, 769, 1, 256));
    // ... of the block alone: block 1 of 64 columns is whole, block 2 of a 129-column front has one column, of a 128-column front none
    EXPECT(is(choose_bwd_gemm(4, 129, 1, 64), kBwdGemm16x8, 5, 4, 1, 512) && is(choose_bwd_gemm(4, 129, 2, 64), kBwdGemm16x8, 1, 4, 1, 512));
    EXPECT(choose_bwd_gemm(4, 128, 2, 64).variant == kNoLaunch && choose_bwd_gemm(4, 128, 3, 64).variant == kNoLaunch);
    EXPECT(choose_bwd_gemm(0, 128, -1, 1 << 30).variant == kNoLaunch && choose_bwd_gemm(4, 0, -1, 1 << 30).variant == kNoLaunch);
    // fwd_own_update: the own rows below block blk
    EXPECT(is(choose_fwd_own_update(4, 129, 1, 64), kFwdOwnUpdate, 1, 4, 1, 256) && choose_fwd_own_update(4, 128, 1, 64).variant == kNoLaunch);
    EXPECT(is(choose_fwd_own_update(4, 4096, 0, 2048), kFwdOwnUpdate, 65, 4, 1, 256) && choose_fwd_own_update(0, 4096, 0, 2048).variant == kNoLaunch);
    // assemble: by the rows of the tallest column, rounded up to even first
    EXPECT(is(choose_assemble(7, 100, 1280), kAssembleLdsWave, 25, 7, 1, 256, 4 * 1280 * 8));
    EXPECT(is(choose_assemble(7, 100, 1279), kAssembleLdsWave, 25, 7, 1, 256, 4 * 1280 * 8));
    EXPECT(is(choose_assemble(7, 100, 1281), kAssembleLdsWg, 101, 7, 1, 256, 1282 * 8) && is(choose_assemble(7, 100, 1282), kAssembleLdsWg, 101, 7, 1, 256, 1282 * 8));
    EXPECT(is(choose_assemble(7, 100, 8192), kAssembleLdsWg, 101, 7, 1, 256, 65536));
    EXPECT(is(choose_assemble(7, 100, 8193), kAssembleLdsWg, 101, 7, 1, 256, 8194 * 8, true) && is(choose_assemble(7, 100, 8194), kAssembleLdsWg, 101, 7, 1, 256, 8194 * 8, true));
    EXPECT(is(choose_assemble(7, 100, 16384), kAssembleLdsWg, 101, 7, 1, 256, 131072, true));
    EXPECT(is(choose_assemble(7, 100, 16385), kAssembleHbmWg, 101, 7, 1, 256) && is(choose_assemble(7, 100, 16386), kAssembleHbmWg, 101, 7, 1, 256));
    EXPECT(is(choose_assemble_hbm(1, 8800), kAssembleHbmWg, 8801, 1, 1, 256) && is(choose_assemble_hbm(1, 8801), kAssembleHbmWave, 2201, 1, 1, 256));
    EXPECT(is(choose_assemble_hbm(2200, 4), kAssembleHbmWg, 5, 2200, 1, 256) && is(choose_assemble_hbm(2201, 4), kAssembleHbmWave, 1, 2201, 1, 256));
    EXPECT(choose_assemble(0, 100, 100).variant == kNoLaunch && choose_assemble_hbm(0, 100).variant == kNoLaunch);
    // permute and the wave kernels
    EXPECT(is(choose_permute(1000, 8), kPermuteNarrow, 4, 1, 1, 256) && is(choose_permute(1000, 9), kPermuteTiles, 16, 1, 1, 256));
    // gradients on Q's pattern: 64 columns / 16 rows per workgroup, chunks of 4096 entries; members in grid y (z: the contraction)
    EXPECT(is(choose_grad_pattern(64, 3), kGradPattern, 1, 3, 1, 256) && is(choose_grad_pattern(65, 1), kGradPattern, 2, 1, 1, 256) && choose_grad_pattern(0, 1).variant == kNoLaunch);
    EXPECT(is(choose_grad_mubar(16, 2), kGradMubar, 1, 2, 1, 256) && is(choose_grad_mubar(17, 1), kGradMubar, 2, 1, 1, 256) && choose_grad_mubar(5, 0).variant == kNoLaunch);
    EXPECT(is(choose_grad_dot(4096, 5, 2), kGradDot, 1, 5, 2, 256) && is(choose_grad_dot(4097, 1, 1), kGradDot, 2, 1, 1, 256) && choose_grad_dot(0, 1, 1).variant == kNoLaunch);
    EXPECT(is(choose_fwd_update_wave(5, 17, false), kWaveWhole, 40, 2, 1, 64) && is(choose_fwd_update_wave(5, 16, true), kWaveSplitK, 40, 1, 1, 256));
    EXPECT(is(choose_bwd_wave(3, 100, 16, false), kWaveWhole, 7, 3, 1, 64) && is(choose_bwd_wave(3, 100, 1, true), kWaveSplitK, 7, 3, 1, 256));
    EXPECT(choose_fwd_update_wave(0, 1, true).variant == kNoLaunch && choose_bwd_wave(0, 100, 1, true).variant == kNoLaunch &&
           choose_bwd_wave(3, 0, 1, true).variant == kNoLaunch);
    EXPECT(cdiv(0, 4) == 0 && cdiv(1, 4) == 1 && cdiv(4, 4) == 1 && cdiv(5, 4) == 2 && odd(0) == 1 && odd(7) == 7 && odd(8) == 9);
}

// The launches of a factorisation level as Device::factor_levels / panel_block issue them (the panel chain whole, and as the even / odd
// halves of two chains on levels that run two), through the choice functions.
static void check_factor_launches(const std::vector<gmrfx::LevelInfo> &LV) {
    using namespace gmrfx;
    constexpr int OBK = 4, narrow_min = 256;     // (device.cpp: 64-column blocks per outer block; fronts for the narrow-block trsm)
    for (const LevelInfo &L : LV) {
        const int nf = L.nbig();
        check_launch(choose_assemble(nf, L.max_cols, L.max_rows), nf <= 0, true, false, L.max_cols);
        check_launch(choose_assemble_hbm(nf, L.max_cols), nf <= 0, true, false, L.max_cols);        // (the fallback)
        const bool two = nf >= 2 && L.nblk() >= 4;
        for (int half = two ? 0 : -1; half < (two ? 2 : 0); half++) {
            auto of = [&](int a) { return half < 0 ? a : half == 0 ? (a + 1) / 2 : a / 2; };
            for (int b = 0; b < L.nblk(); b++) {
                const int n = of(L.wider_than(b * NB)), kb = b * NB, below = L.max_rows - kb - 1;
                if (n <= 0) continue;
                const int cut32 = b == 0 ? of(L.wider[1]) : n;
                const int ntrsm = b == 0 && n - cut32 >= narrow_min ? cut32 : n;
                check_launch(choose_trsm(ntrsm, below), ntrsm <= 0 || below <= 0, true, false, below);
                const int J1 = (b / OBK + 1) * OBK, nnext = of(L.wider_than((b + 1) * NB)), nouter = of(L.wider_than(J1 * NB));
                if (b + 1 < J1 && nnext > 0) {
                    const int M = L.max_rows - kb - NB, N = std::min(J1 * NB, L.max_cols) - kb - NB;
                    check_launch(choose_gemm_nt(nnext, NB, M, N), M <= 0 || N <= 0, true, true, M, 0, N, 0);
                }
                if (b + 1 == J1 && nouter > 0) {
                    const int M = L.max_rows - J1 * NB, N = L.max_cols - J1 * NB;
                    check_launch(choose_gemm_nt(nouter, OBK * NB, M, N), M <= 0 || N <= 0, true, true, M, 0, N, 0);
                }
            }
        }
    }
}

// The level schedule the drivers read (device_plan.h): LevelInfo's counts against a brute-force walk over the level's list of big
// fronts, and the sweeps' step plans (plan_forward_level / plan_backward_level) for every pass width, inverse cap, front-kernel
// minimum and both values of the records flag: every big front is finished exactly once -- by the one-workgroup front kernel or
// by the blocks of the substitution, never both (the list arithmetic that once ran the blocked loop over the finished tail). sweep: these are the levels the sweeps walk --
// the launches Device::forward / backward issue from a plan go through the choice functions.
static int levels_with_wide_head_and_tail = 0;
static void check_level_plans(const gmrfx::Symbolic &S, const std::vector<gmrfx::LevelInfo> &LV, const std::vector<gmrfx::i32> &llist, bool sweep) {
    using namespace gmrfx;
    const EnvKnobs env;
    for (const LevelInfo &L : LV) {
        std::vector<int> cols, trail;
        for (int k = L.nsmall; k < L.count; k++) {
            const i32 s = llist[(size_t)L.first + k];
            cols.push_back(S.ncols(s)); trail.push_back(S.nrows(s) - S.ncols(s));
        }
        const int nbig = (int)cols.size();
        EXPECT(nbig == L.nbig());
        auto wider = [&](int c, int upto) { int cnt = 0; for (int i = 0; i < upto; i++) cnt += cols[i] > c; return cnt; };
        int max_cols = 0, max_trail = 0, min_trail = 0;
        for (int i = 0; i < nbig; i++) {
            EXPECT(i == 0 || cols[i] <= cols[i - 1]);          // sorted by decreasing width
            max_cols = std::max(max_cols, cols[i]); max_trail = std::max(max_trail, trail[i]);
            if (trail[i] > 0) min_trail = min_trail ? std::min(min_trail, trail[i]) : trail[i];
        }
        EXPECT(L.max_cols == max_cols && L.max_trail == max_trail && L.min_trail == min_trail && L.nblk() == (max_cols + NB - 1) / NB);
        for (int c = 0; c <= max_cols + 2 * NB; c += NB) { EXPECT(L.wider_than(c) == wider(c, nbig)); EXPECT(c < max_cols || L.wider_than(c) == 0); }
        EXPECT(L.wider_than(INT32_MAX / NB * NB) == 0);
        bool counted = false;
        for (int nr : {1, 16, 17, 32, 33, 64})
            for (int cap : {64, 128, 2048})
                for (int fm = 0; fm < 3; fm++)
                    for (bool rec : {true, false}) {
                        // (the limits as the launch side has them today; the properties hold for any)
                        const SweepKnobs kn{cap, fm < 2 ? fm : env.fwd_front_min, fm < 2 ? fm : env.bwd_front_min, rec, kNarrowPassMax, kNarrowPassMaxBwd,
                                            kFrontMaxCols, kWaveSplitCols, kWaveSplitRows};
                        const FwdLevelPlan f = plan_forward_level(L, nr, kn);
                        const BwdLevelPlan b = plan_backward_level(L, nr, kn);
                        for (const LevelBlocks *p : {(const LevelBlocks *)&f, (const LevelBlocks *)&b}) {
                            EXPECT(p->nf >= 0 && p->ntail >= 0 && p->nf + p->ntail == nbig);
                            EXPECT(p->nbk == std::max(1, (max_cols + cap - 1) / cap));
                            for (int j = 0; j < p->nbk; j++) {
                                EXPECT(p->xmul_fronts(j) == wider(j * cap, p->nf));                 // block j: the head fronts wider than j cap
                                if (j + 1 < p->nbk) EXPECT(p->own_fronts(j) == wider((j + 1) * cap, p->nf));
                            }
                            for (int i = 0; i < nbig; i++) {
                                int blocks = 0;
                                for (int j = 0; j < p->nbk; j++) blocks += i < p->xmul_fronts(j);
                                // the tail is the front kernel's alone, a head front gets each of its blocks once
                                if (i >= p->nf) EXPECT(blocks == 0 && cols[i] <= std::min(128, cap));
                                else EXPECT(blocks == (cols[i] + cap - 1) / cap);
                            }
                            if (p->ntail > 0 && wider(cap, p->nf) > 0 && !counted) { levels_with_wide_head_and_tail++; counted = true; }
                        }
                        EXPECT(nr > 32 || f.ntail == 0);      // narrow passes never take the front kernels
                        EXPECT(nr > 16 || b.ntail == 0);
                        for (int i = 0; i < f.nf; i++)      // a front's update W -= L21 y: exactly one form, by its width
                            EXPECT((f.wave && cols[i] <= f.cmin) + (f.update != FwdLevelPlan::kNone && cols[i] > f.cmin) == 1);
                        EXPECT(f.update != FwdLevelPlan::kRecords || rec);
                        EXPECT(!f.wave || (rec && f.cmin == kFwdWaveCols));
                        for (int i = 0; i < b.nf; i++)      // ... and t = y - L21' x, by its trailing rows
                            if (trail[i] > 0) EXPECT((b.wave && trail[i] <= b.mmin) + (b.gemm && trail[i] > b.mmin) == 1);
                        if (!sweep) continue;
                        if (f.ntail == 0 || f.nf > 0) {
                            for (int j = 0; j + 1 < f.nbk; j++) {
                                const int below = L.max_cols - (j + 1) * cap;
                                check_launch(choose_fwd_own_update(f.own_fronts(j), L.max_cols, j, cap), f.own_fronts(j) <= 0 || below <= 0, true, false, below);
                            }
                            if (f.wave) check_launch(choose_fwd_update_wave(L.fwd_per, nr, f.wave_split_k), L.fwd_per <= 0, false, false, L.fwd_split.start[8], 1, nr, 16);
                            if (f.update == FwdLevelPlan::kGrid) check_launch(choose_fwd_update(f.nf, L.max_trail), f.nf <= 0 || L.max_trail <= 0, true, false, L.max_trail);
                        }
                        if (b.ntail == 0 || b.nf > 0) {
                            if (b.wave) check_launch(choose_bwd_wave(b.nf, L.max_cols, nr, b.wave_split_k), b.nf <= 0 || L.max_cols <= 0, true, false, L.max_cols, 16, b.nf, 1, nr, 16);
                            if (b.gemm) check_launch(choose_bwd_gemm(b.nf, L.max_cols, -1, 1 << 30), b.nf <= 0 || L.max_cols <= 0, true, false, L.max_cols);
                            for (int j = 0; j + 1 < b.nbk; j++) {
                                const int own = std::min(L.max_cols - j * cap, cap);
                                check_launch(choose_bwd_gemm(b.own_fronts(j), L.max_cols, j, cap), b.own_fronts(j) <= 0 || own <= 0, true, false, own);
                            }
                        }
                    }
    }
}

// The decisions of the Fisher-scoring loop (ga_rules.h), driven alone with scripted numbers: both loops of the device take them from here.
static void check_ga_rules() {
    using namespace gmrfx;
    const double eps = 2.220446049250313e-16, inf = INFINITY;
    const GaOpts o{10, 5, 1e-4, 1e-3, 1 | 2 | 4}, plain{10, 5, 1e-4, 1e-3, 0}, refactors{1, 1, 0, 0, 8};
    EXPECT(o.adaptive() && o.retry_full() && o.predictive() && !o.refactor_final() && !plain.adaptive() && refactors.refactor_final());
    // acceptance: the bound is the merit plus 64 eps max(|energy| + |loglik|, 1); a merit at the bound accepts, one ulp above rejects
    const double e[2] = {3.0, 1.0}, small[2] = {0.25, -0.125};
    const double bound = ga_line_search_bound(e);
    EXPECT(ga_merit(e) == 2.0 && bound == 2.0 + 256 * eps && ga_line_search_bound(small) == 0.375 + 64 * eps && merit_atol(0.0) == 64 * eps);
    GaMember m;
    EXPECT(m.alpha == 1.0 && m.alpha_prev == 1.0 && m.dec_prev == 0.0 && std::isnan(m.dec) && m.status == kGaRun && !m.frozen && m.iters == 0);
    EXPECT(ga_line_search_probe(m, bound, bound) && m.alpha == 1.0);                                   // (sqrt(1) = 1)
    // the step lengths 1 -> 0.1 -> 0.01 -> accept -> 0.1
    EXPECT(!ga_line_search_probe(m, std::nextafter(bound, inf), bound) && m.alpha == 0.1);
    EXPECT(!ga_line_search_probe(m, std::nan(""), bound) && m.alpha == 0.1 * 0.1);                      // (a NaN merit backtracks)
    EXPECT(ga_line_search_probe(m, 2.0, bound) && m.alpha == std::sqrt(0.1 * 0.1) && std::fabs(m.alpha - 0.1) < 1e-16);
    // the full-step retry: only under its flag and only below the full step; accepted, it sets the full step
    EXPECT(ga_line_search_retries_full(o, m) && !ga_line_search_retries_full(plain, m));
    EXPECT(!ga_line_search_full_step(m, std::nextafter(bound, inf), bound) && m.alpha < 1.0 && !ga_line_search_full_step(m, std::nan(""), bound));
    EXPECT(ga_line_search_full_step(m, bound, bound) && m.alpha == 1.0 && !ga_line_search_retries_full(o, m));
    // the tiny-step exit: alpha |step|_inf against dec_tol / 1000, both sides
    const double tiny = o.dec_tol / 1000;
    EXPECT(!ga_line_search_tiny_step(o, m, tiny) && ga_line_search_tiny_step(o, m, std::nextafter(tiny, 0.0)));
    m.alpha = 0.5;
    EXPECT(!ga_line_search_tiny_step(o, m, 2 * tiny) && ga_line_search_tiny_step(o, m, std::nextafter(2 * tiny, 0.0)) && !ga_line_search_tiny_step(o, m, std::nan("")));
    // convergence, each condition alone: the decrement, the mean change, the mean change relative to |x| (floored at 1e-10: x = 0 is
    // no division by zero)
    auto verdict = [&](const GaOpts &op, GaMember &mm, long long iter, double dec, double diff2, double x2) {
        const double st[4] = {dec, diff2, x2, 7.0};
        const GaVerdict v = ga_iterate_verdict(op, mm, iter, st);
        EXPECT(mm.dec == dec || (std::isnan(dec) && std::isnan(mm.dec)));       // the verdict records dec, and dec_prev is the caller's
        return v;
    };
    GaMember c;
    EXPECT(verdict(plain, c, 1, std::nextafter(1e-3, 0.0), 1.0, 1.0) == kGaConverges && verdict(plain, c, 1, 1e-3, 1.0, 1.0) == kGaContinue);
    EXPECT(verdict(plain, c, 1, 1.0, 25e-10, 0.0) == kGaConverges && verdict(plain, c, 1, 1.0, 4e-8, 0.0) == kGaContinue);      // (sqrt: 5e-5, 2e-4)
    EXPECT(verdict(plain, c, 1, 1.0, 1.0, 1e10) == kGaConverges && verdict(plain, c, 1, 1.0, 1.0, 1e6) == kGaContinue);        // (1e-5, 1e-3)
    const GaOpts floor_only{10, 5, 0.0, 0.0, 0};       // nothing is below a tolerance of 0: 0 / max(0, 1e-10) = 0, not NaN
    EXPECT(verdict(floor_only, c, 1, 1.0, 0.0, 0.0) == kGaContinue && verdict(plain, c, 1, std::nan(""), 1.0, 1.0) == kGaContinue && c.dec_prev == 0.0);
    // the look-ahead: dec (dec / dec_prev)^2 < dec_tol, under its flag, after the first iterate, and both step lengths exactly 1
    auto ahead = [&](const GaOpts &op, long long iter, double alpha, double alpha_prev, double dec_prev) {
        GaMember p;
        p.alpha = alpha; p.alpha_prev = alpha_prev; p.dec_prev = dec_prev;
        return verdict(op, p, iter, 1e-2, 1.0, 1.0);
    };
    EXPECT(ahead(o, 2, 1.0, 1.0, 0.1) == kGaLooksAhead);                    // 1e-2 (1e-1)^2 = 1e-4
    EXPECT(ahead(o, 1, 1.0, 1.0, 0.1) == kGaContinue && ahead(plain, 2, 1.0, 1.0, 0.1) == kGaContinue);
    EXPECT(ahead(o, 2, std::nextafter(1.0, 0.0), 1.0, 0.1) == kGaContinue && ahead(o, 2, 1.0, std::nextafter(1.0, 0.0), 0.1) == kGaContinue);
    EXPECT(ahead(o, 2, 1.0, 1.0, 0.02) == kGaContinue);                     // 1e-2 (0.5)^2 = 2.5e-3
    // the chord step of the frozen finish decides by !(dec < tol): a NaN does not converge it, and only a deciding step is recorded
    GaMember f;
    f.dec = 0.5;
    EXPECT(!frozen_finish_decides(o, f, std::nan("")) && f.dec == 0.5 && !frozen_finish_decides(o, f, 1e-3) && f.dec == 0.5);
    EXPECT(frozen_finish_decides(o, f, 5e-4) && f.dec == 5e-4 && kFrozenFinishSteps == 3);
    // the counters and the eight-number row
    GaMember r;
    r.alpha = 0.25;
    ga_iterate_begun(r);
    ga_iterate_begun(r);
    r.alpha = 0.5; r.dec = 1e-5; r.nmerit = 7;
    EXPECT(r.alpha_prev == 0.25 && r.nfact == 2 && r.nsolve == 2);
    ga_stop(r, kGaConverged, 3, true);
    double row[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
    ga_result_row(r, row);
    const double want[9] = {3, 1, 0.5, 1e-5, 2, 2, 7, 1, -1};
    EXPECT(std::equal(row, row + 9, want));
    ga_stop(r, kGaMaxIter, 10, false);
    ga_result_row(r, row);
    EXPECT(row[0] == 10 && row[1] == 0 && row[7] == 0);
    ga_stop(r, kGaFailed, 2, false);
    ga_result_row(r, row);
    EXPECT(row[0] == 2 && row[1] == 0 && row[7] == 0);
}

// the device tables of every rank of a (sharded, world > 1) analysis, with and without the tile records (GMRFX_SYRK_XCD=0)
static void device_plans(const std::vector<int64_t> &cp, const std::vector<int64_t> &ri, const double *coords, int64_t n, int world) {
    for (int rank = 0; rank < world; rank++) {
        gmrfx::SymOptions so;
        if (coords) { so.coord_dim = 2; so.coords = coords; }
        if (world > 1) { so.shard_rank = rank; so.shard_world = world; so.subtree_max = 0; so.dist_min_cols = 128; }   // (as gmrfx_create)
        gmrfx::Symbolic S;
        gmrfx::analyze(n, cp.data(), ri.data(), 0, nullptr, so, S);
        for (bool xcd : {true, false}) {
            const gmrfx::DevicePlan P = gmrfx::build_device_plan(S, gmrfx::PlanOptions{xcd});
            check_runs(P.levels, false, P.syrk_recs.size(), xcd);
            check_runs(P.swlevels, true, P.fwd_recs.size(), xcd);
            EXPECT(P.edge.size() == S.children.size() && (int)P.levels.size() == S.nlevels);
            check_level_plans(S, P.levels, S.levellist, false);
            check_level_plans(S, P.swlevels, S.sw_levellist, true);
            check_factor_launches(P.levels);
            for (int nr : {1, 8, 9, 64}) check_launch(gmrfx::choose_permute((int)n, nr), false, false, false, n);
            EXPECT(S.shard_plan ? P.owncol.size() == (size_t)n && P.fc_levelptr.back() == (int)P.fchild.size() : P.owncol.empty());
        }
    }
}

int main() {
    std::vector<int64_t> cp, ri;
    std::vector<double> xy;
    // large enough for the threaded nested dissection (> 20 000 vertices per half) and the threaded scatter map (> 2e6 entries)
    grid_pattern(420, 400, cp, ri, xy);
    const int64_t n = 420 * 400;
    one_handle(cp, ri, xy.data(), n, 0);      // geometric nested dissection
    one_handle(cp, ri, nullptr, n, 0);        // graph nested dissection
    one_handle(cp, ri, nullptr, n, 1);        // natural ordering
    sharded_handles(cp, ri, xy.data(), n, 2);
    sharded_handles(cp, ri, xy.data(), n, 4);
    sharded_handles(cp, ri, xy.data(), n, 8);      // the width the driver scales to
    check_launch_edges();
    check_ga_rules();
    device_plans(cp, ri, xy.data(), n, 1);
    device_plans(cp, ri, xy.data(), n, 2);         // owner columns, foreign parents, other ranks' children
    // distinct handles are used concurrently from different host threads (WorkspacePool contract)
    {
        std::vector<int64_t> cp2, ri2; std::vector<double> xy2;
        grid_pattern(90, 70, cp2, ri2, xy2);
        std::vector<std::thread> th;
        th.reserve(4);
        for (int t = 0; t < 4; t++) th.emplace_back([&, t] { one_handle(cp2, ri2, t % 2 ? xy2.data() : nullptr, 90 * 70, 0); });
        for (auto &x : th) x.join();
        device_plans(cp2, ri2, xy2.data(), 90 * 70, 1);
    }
    // the RBMC block plan (csrc/rbmc_plan.cpp: the symmetric row structure, the subset walk, the threaded enclosures) on a symbolic-only
    // handle, two-call protocol; every node is written by exactly one block
    {
        gmrfx_opts o; std::memset(&o, 0, sizeof(o)); o.struct_size = (int32_t)sizeof(o); o.symbolic_only = 1; o.device = -1;
        gmrfx_handle *h = nullptr;
        EXPECT(gmrfx_create(n, cp.data(), ri.data(), 0, nullptr, &o, &h) == GMRFX_OK && h != nullptr);
        int64_t counts[3] = {0, 0, 0};
        EXPECT(gmrfx_rbmc_plan(h, 2, 1, counts, nullptr, nullptr, nullptr, nullptr) == GMRFX_OK);
        std::vector<int64_t> bp(counts[0] + 1), rows(counts[1]), ni(counts[0]), own(counts[1]), hits(n, 0);
        EXPECT(gmrfx_rbmc_plan(h, 2, 1, counts, bp.data(), rows.data(), ni.data(), own.data()) == GMRFX_OK);
        EXPECT(bp[counts[0]] == counts[1] && counts[2] <= 512);
        for (int64_t r = 0; r < counts[1]; r++) { EXPECT(rows[r] >= 1 && rows[r] <= n); if (own[r]) hits[rows[r] - 1]++; }
        for (int64_t i = 0; i < n; i++) EXPECT(hits[i] == 1);
        EXPECT(gmrfx_rbmc_plan(h, -1, 0, counts, nullptr, nullptr, nullptr, nullptr) == GMRFX_ERR_INVALID_ARG);
        gmrfx_destroy(h);
    }
    // malformed input is rejected, not read out of bounds
    {
        gmrfx_opts o; std::memset(&o, 0, sizeof(o)); o.struct_size = (int32_t)sizeof(o); o.symbolic_only = 1; o.device = -1;
        gmrfx_handle *h = nullptr;
        std::vector<int64_t> bad = cp; bad[5] = bad[4] - 3;
        EXPECT(gmrfx_create(n, bad.data(), ri.data(), 0, nullptr, &o, &h) != GMRFX_OK && h == nullptr);
        std::vector<int64_t> badr = ri; badr[10] = n + 7;
        EXPECT(gmrfx_create(n, cp.data(), badr.data(), 0, nullptr, &o, &h) != GMRFX_OK && h == nullptr);
        std::vector<int64_t> p(n, 0);
        EXPECT(gmrfx_create(n, cp.data(), ri.data(), 0, p.data(), &o, &h) != GMRFX_OK && h == nullptr);
    }
    // (levels with a front wider than the inverse cap in the head AND a tail for the front kernel: what the check above is for)
    std::printf("levels with a wide head and a front-kernel tail: %d\n", levels_with_wide_head_and_tail);
    // (a report: the plans here are small, no variant's count is a condition)
    for (int v = 0; v < gmrfx::kVariantCount; v++) std::printf("launches of the plans' levels choosing %s: %lld\n", variant_names[v], variant_hits[v]);
    EXPECT(levels_with_wide_head_and_tail > 0);
    std::printf("sanitize_host: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
