"""The numeric factorisation on fronts of PRESCRIBED shape: the cases selinv_shapes.py / sweep_shapes.py do not have, the
factorisation's level driver and launch choices restated in plain Python, the extended-precision reference factor and the
per-front error measure (test_factor_shapes_host.py on symbolic-only handles, test_gpu_factor_shapes.py on the device).

Cases are selinv_shapes specs (ss.build / ss.make under ss.KW, ss.check_shapes). Reused as they are: ss.chain_cases,
ss.small_path_cases, ws.children_cases, ws.record_level_cases, ws.backward_class_cases, ws.wide_cases. New here (the *_cases
functions below): the four width classes of the diagonal-block kernel on one level, levels of narrow siblings on both sides
of narrow_min, levels on both sides of the trsm and gemm tile thresholds, the dense front that reaches k_gemm_nt<2> by the
outer update and k_assemble_lds<1> with its twin under both thresholds, the two-level blocking's edges, levels with two
panel chains, contribution blocks at the SYRK tile edges and over 0 .. 5 tall children, the small-front classes at their row
edges and over 0 .. 5 children (subtrees under SUBTREE), two amalgamated fronts that hold padding.

The restated plan: ws.fronts(be) -> factor_levels() (subtrees() / ws.small_class mirror csrc/symbolic.cpp; FLevel mirrors
LevelInfo) -> reached(), which walks Device::factor_levels / factor_small_fronts / factor_panel_chains / panel_block /
factor_contribution_blocks of csrc/device.cpp with choose_assemble / choose_trsm / choose_gemm_nt of csrc/device_plan.cpp and
launch_potrf64's shapes, and lists every (variant, c, m, children, block, alone in its launch). The variant carries what the
launch was chosen by: "k_potrf64_b<8,4>:cut" (a piece of block 0's width-sorted list), ":list" (the record list), ":arg"
(the last active front, geometry from FrontArg); "k_gemm_nt<1>:K64" / ":K256"; "k_trsm_narrow:head" / ":nohead" (with /
without fronts wider than 32 columns in front of it); "two_chains:equal" / ":unequal" (the halves of a level with two
chains). block = -1 for the launches that are not per 64-column block. WANT is the coverage table the host test holds runs()
to; a WANT row is (variant, {condition: value}) with the conditions of features().

m = 0 fronts exist in the 48- and 64-row classes only (a small front has at most 64 columns: m = 0 means at most 64 rows).
Subtree tasks are off by default: the SUBTREE setting (GMRFX_SUBTREE_MAX=8, GMRFX_SMALL_ROWS=128) turns them on.

Reference: ws.cholesky_longdouble of Q[perm][:, perm], kept as a float64 pair (hi, lo). It checks itself: residual() is
max |A - L L'| / max |A| with every sum in np.longdouble. Error of a stored entry: |Lg - Lref|[i, j] / max_i |Lref[i, j]|."""
import os
import re

import numpy as np

import selinv_shapes as ss
import sweep_shapes as ws

cdiv = ws.cdiv
SACRIFICE = ss.SACRIFICE
NARROW_SACRIFICE = (30, 3, "first")     # a sacrificial child of at most 32 columns: it counts among the narrow fronts
assert not ss.absorbed(30, 3, 150, 0)


# ---- cases -------------------------------------------------------------------------------------------------------------
WIDTHS_C = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
WIDTHS_WIDE = ((100, 21), (110, 60))         # at block 1 the launch's widest block has 46 columns: <4,3> at a later block


def width_cases():
    """widths: siblings of WIDTHS_C columns and two above 64 under one root (with the 40-column sacrificial child every piece
    of block 0's list is non-empty), under the 110-column one a second level of 64-, 60-, 10- and 5-column fronts (pieces <8,4>
    and <1,1> only: the two in between are empty). widths_two: the same level with a 193-column sibling: four blocks, so two
    chains, and every piece non-empty in both halves (checked by the host test)."""
    rng = np.random.default_rng(7)
    sib = [(c, int(rng.integers(1, 41)), "cols") for c in WIDTHS_C]
    grand = [(64, 30, "both"), (60, 41, "both"), (10, 35, "both"), (5, 64, "both")]
    assert not any(ss.absorbed(g[0], g[1], 110, 60) for g in grand)
    wide = [(100, 21, "cols"), (110, 60, "cols", grand)]
    sib2 = [(c, int(rng.integers(1, 41)), "cols") for c in WIDTHS_C for _ in (0, 1)]
    return [{"name": "widths", "root": 150, "children": sib + wide + [SACRIFICE], "seed": 601},
            {"name": "widths_two", "root": 150, "children": sib2 + [(100, 21, "cols"), (110, 60, "cols"), (193, 20, "cols"), (41, 9, "cols"), SACRIFICE], "seed": 602}]


def narrow_cases():
    """Levels of N narrow siblings (at most 32 columns, 1 .. 40 trailing rows), the sacrificial child one of them: N = 255 and
    256 without a front wider than 32 columns (cut32 == 0), and the same with three 40-column fronts in front (cut32 == 3)."""
    out = []
    for name, cnt, head in (("narrow255", 255, 0), ("narrow256", 256, 0), ("narrow255_head", 255, 3), ("narrow256_head", 256, 3)):
        rng = np.random.default_rng(cnt + head)
        kids = [(int(rng.integers(1, 9)), int(rng.integers(1, 41)), "cols") for _ in range(cnt - 3)] + [(32, 40, "cols"), (17, 1, "cols")]
        kids += [(40, int(rng.integers(1, 41)), "cols") for _ in range(head)]
        out.append({"name": name, "root": 150, "children": kids + [NARROW_SACRIFICE], "seed": 610 + cnt + head, "nnarrow": cnt, "head": head})
    return out


def trsm_cases():
    """64 / 65 siblings whose tallest has 129 rows (128 below the first diagonal entry: two 64-row tiles per front): 128 tiles
    take k_trsm<0,1>, 130 take k_trsm<0,0>. The sacrificial child counts."""
    out = []
    for name, cnt in (("trsm128", 64), ("trsm130", 65)):
        rng = np.random.default_rng(cnt)
        kids = [(10, 119, "cols")] + [(int(rng.integers(3, 15)), int(rng.integers(1, 100)), "cols") for _ in range(cnt - 2)]
        out.append({"name": name, "root": 150, "children": kids + [SACRIFICE], "seed": 620 + cnt, "tiles": 2 * cnt})
    return out


def gemm_cases():
    """The K = 64 update at block 0 of a level whose widest front is (192, 400): 9 x 2 tiles per front with a second block;
    14 such fronts are 252 tiles (k_gemm_nt<1>), 15 are 270 (k_gemm_nt<2>). Three blocks: one chain."""
    out = []
    for name, cnt in (("gemm252", 14), ("gemm270", 15)):
        kids = [(192, 400, "cols")] + [(65 + k % 3, 5 + k, "cols") for k in range(cnt - 1)]
        out.append({"name": name, "root": 400, "children": kids + [SACRIFICE], "seed": 630 + cnt, "tiles": 18 * cnt})
    return out


DENSE_OVER, DENSE_UNDER = 1281, 1280


def dense_cases():
    """One dense front of 1281 columns: the smallest that has more than 16 x 16 tiles behind its first outer block (17 x 17 =
    289 > 256: k_gemm_nt<2> at K = 256), an even-rounded leading dimension above 1280 (k_assemble_lds<1>) and 21 blocks through
    FrontArg. Its twin of 1280 columns has 256 tiles (k_gemm_nt<1> at K = 256) and ld = 1280 (k_assemble_lds<0>)."""
    return [{"name": f"dense{c}", "root": c, "children": [], "seed": 640 + c, "alone": True} for c in (DENSE_OVER, DENSE_UNDER)]


BLOCKING_C = (192, 193, 256, 257, 320, 513, 577)


def blocking_cases():
    """c in BLOCKING_C as lone fronts (m = 0) and as chain fronts with 33 trailing rows, one front per level: the first block
    of an outer block, the last one before J1, J1 itself, a ragged last block, a ragged outer update."""
    out = [{"name": f"block{c}_m0", "root": c, "children": [], "seed": 650 + c, "alone": True} for c in BLOCKING_C]
    for k, cs in enumerate(((192, 193, 256, 320), (257, 513, 577))):
        spec = None
        for c in cs:
            spec = (c, 33, "both", [spec] if spec else [])
        out.append({"name": f"block_chain{k}", "root": ss.HELPER_ROOT, "children": [(ss.HELPER[0], ss.HELPER[1], "cols", [spec])],
                    "seed": 660 + k, "alone": True})
    return out


def chain_pair_cases():
    """Levels of big fronts with four or more blocks (two chains from two fronts on): two fronts (equal halves), three
    (unequal), two whose chains end four blocks apart (449 and 193 columns), one front (one chain), and three fronts of three
    blocks (one chain). The sacrificial child is a small front at the defaults."""
    lv = {"pair2": [(257, 20), (200, 30)], "pair3": [(257, 20), (200, 30), (193, 25)], "pair_apart": [(449, 20), (193, 30)],
          "pair1": [(257, 20)], "pair_nblk3": [(192, 20), (190, 30), (180, 25)]}
    return [{"name": name, "root": 150, "children": [(c, m, "cols") for c, m in kids] + [SACRIFICE], "seed": 670 + k, "big": kids}
            for k, (name, kids) in enumerate(lv.items())]


SYRK_M = (1, 63, 64, 65, 127, 128, 129, 193)
_TALL = [(20, 100, "trail"), (33, 90, "trail"), (9, 120, "trail"), (17, 80, "trail"), (25, 140, "both")]   # > 64 rows in the parent's trailing rows


def syrk_cases():
    """syrk_w127 / syrk_w128: siblings of 70 columns with SYRK_M trailing rows beside a widest front of 127 / 128 columns
    (kSyrkPipedMinCols). syrk_kids<k>: a (70, 150) parent over k = 0, 1, 2, 3, 5 children each of which has more than 64 rows
    in the parent's trailing rows (scattered over 150: they cross a tile edge as rows and as columns of the block);
    syrk_kids_cols: two children, the second with all its rows in the parent's own columns."""
    out = [{"name": f"syrk_w{w}", "root": 200, "children": [(70, m, "cols") for m in SYRK_M] + [(w, 5, "cols"), SACRIFICE], "seed": 680 + w, "widest": w}
           for w in (127, 128)]
    assert not any(ss.absorbed(kc, km, 70, 150) for kc, km, _ in _TALL + [(12, 40, "cols")])
    for k in ws.KID_COUNTS:
        out.append({"name": f"syrk_kids{k}", "root": 200, "children": [(70, 150, "cols", _TALL[:k]), SACRIFICE], "seed": 690 + k, "parent": (70, 150, k)})
    out.append({"name": "syrk_kids_cols", "root": 200, "children": [(70, 150, "cols", [_TALL[0], (12, 40, "cols")]), SACRIFICE], "seed": 699, "parent": (70, 150, 2)})
    return out


SMALL_EDGES = [(1, 47), (1, 48), (1, 63), (1, 64), (1, 95), (1, 96), (1, 127), (48, 1), (64, 1), (64, 32), (64, 33), (64, 64)]
SMALL_PARENTS = [(10, 38), (20, 44), (30, 66), (40, 88)]        # 48, 64, 96 and 128 rows
_LITTLE = [(3, 10, "both"), (4, 12, "both"), (2, 9, "both"), (5, 11, "both"), (3, 7, "both"), (2, 8, "both"), (4, 6, "both"), (3, 9, "both")]


def small_cases():
    """small_edges: r = c + m in {48, 49, 64, 65, 96, 97, 128} at c = 1 and at c = 64 (48 where 64 columns do not fit).
    small_kids<k>: one parent per row class (48, 64, 96, 128 rows) over k = 0, 1, 2, 3, 5 children; under SUBTREE the first
    three are subtree tasks of the three classes, the fourth (128 rows) is not. small_kids8: 9 fronts, one more than
    GMRFX_SUBTREE_MAX=8 takes; subtree_rows97: a (30, 67) root over one child, one row too many for a subtree."""
    out = [{"name": "small_edges", "root": 150, "children": [(c, m, "cols") for c, m in SMALL_EDGES] + [SACRIFICE], "seed": 700}]
    assert not any(ss.absorbed(kc, km, c, m) for kc, km, _ in _LITTLE for c, m in SMALL_PARENTS + [(30, 67)])
    for k in ws.KID_COUNTS:
        out.append({"name": f"small_kids{k}", "root": 150, "children": [(c, m, "cols", _LITTLE[:k]) for c, m in SMALL_PARENTS] + [SACRIFICE], "seed": 710 + k, "kids": k})
    out.append({"name": "small_kids8", "root": 150, "children": [(10, 38, "cols", _LITTLE[:8]), SACRIFICE], "seed": 720})
    out.append({"name": "subtree_rows97", "root": 150, "children": [(30, 67, "cols", _LITTLE[:1]), SACRIFICE], "seed": 721})
    return out


def amalgamated_cases():
    """A child that ss.absorbed() says its parent takes (under ss.KW, the settings of every case here): merged by the
    four-column rule (2 + 2 columns, the child reaches 4 of the parent's 30 trailing rows) and by the 2 % rule (a 30-column
    child that reaches all 50 columns and 38 of the 40 trailing rows of its parent). The merged front stores the rows the
    child does not reach as padding: exact zeros of the true factor."""
    assert ss.absorbed(2, 6, 2, 30) and ss.absorbed(30, 88, 50, 40)
    return [{"name": "merged_cols4", "root": 150, "children": [(2, 30, "cols", [(2, 6, "first")]), SACRIFICE], "seed": 730, "merged": (4, 30)},
            {"name": "merged_2pct", "root": 150, "children": [(50, 40, "cols", [(30, 88, "first")]), SACRIFICE], "seed": 731, "merged": (80, 40)}]


def new_cases():
    return (width_cases() + narrow_cases() + trsm_cases() + gemm_cases() + dense_cases() + blocking_cases() + chain_pair_cases() + syrk_cases()
            + small_cases() + amalgamated_cases())


# ---- settings and the list of runs ----------------------------------------------------------------------------------------
DEFAULTS, LEVEL, LEVEL0, LEVEL128, XCD0 = ws.DEFAULTS, ws.LEVEL, ws.LEVEL0, ws.LEVEL128, ws.XCD0
PIPED0, PIPED_NEVER = {"GMRFX_SYRK_PIPED": "0"}, {"GMRFX_SYRK_PIPED": "1000000"}
SUBTREE = {"GMRFX_SUBTREE_MAX": "8", "GMRFX_SMALL_ROWS": "128"}
LEVEL0_XCD0 = dict(LEVEL0, **XCD0)
SYRK_SETTINGS = [DEFAULTS, PIPED0, PIPED_NEVER, XCD0]


def runs():
    """[(group, cases, [setting])]: what test_gpu_factor_shapes.py runs and test_factor_shapes_host.py holds to WANT."""
    return [
        ("chains", ss.chain_cases(), [DEFAULTS, LEVEL0, XCD0]),
        ("children", ws.children_cases(), SYRK_SETTINGS + [LEVEL, LEVEL0]),
        ("records", ws.record_level_cases(), [DEFAULTS, XCD0, LEVEL0]),
        ("bwd_classes", ws.backward_class_cases(), [DEFAULTS, LEVEL0]),
        ("wide", ws.wide_cases(), [DEFAULTS, LEVEL, PIPED0, XCD0]),
        ("widths", width_cases(), [LEVEL0, LEVEL0_XCD0, DEFAULTS]),
        ("narrow", narrow_cases(), [LEVEL0, DEFAULTS]),
        ("trsm", trsm_cases(), [LEVEL0]),
        ("gemm", gemm_cases(), [DEFAULTS, LEVEL0]),
        ("dense", dense_cases(), [DEFAULTS]),
        ("blocking", blocking_cases(), [DEFAULTS, PIPED_NEVER, XCD0]),
        ("two_chains", chain_pair_cases(), [DEFAULTS, LEVEL128, XCD0]),
        ("syrk", syrk_cases(), SYRK_SETTINGS + [LEVEL0]),
        ("small", small_cases(), [DEFAULTS, LEVEL, LEVEL0, LEVEL128, SUBTREE]),
        ("small_path", ss.small_path_cases(), [DEFAULTS, LEVEL128, SUBTREE]),
        ("amalgamated", amalgamated_cases(), [DEFAULTS, LEVEL0, LEVEL128]),
    ]


label, apply_setting = ws.label, ws.apply_setting


# ---- the restated decisions -----------------------------------------------------------------------------------------------
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianmarkovrandomfields.jl_amd", "csrc")


def lib_const(fname, name):
    """An integer constant of the library's source: the restated choices below follow the thresholds the library is built
    with, so that a threshold that moves takes the cases built around it off their side of it (the host test then fails)."""
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(r"\b" + name + r" = (\d+)\b", f.read())
    assert m, f"{fname}: no constant {name}"
    return int(m.group(1))


def _width_cuts():
    """level_infos: L.wider[q] = wider_than(48 - 16 * q)"""
    with open(os.path.join(_CSRC, "device_plan.cpp")) as f:
        m = re.search(r"L\.wider\[q\] = wider_than\((\d+) - (\d+) \* q\)", f.read())
    assert m, "device_plan.cpp: the cuts of block 0"
    return tuple(int(m.group(1)) - int(m.group(2)) * q for q in range(3))


NB = 64
OBK = lib_const("device.cpp", "OBK")
NARROW_MIN = lib_const("device.cpp", "narrow_min")
WIDTH_CUTS = _width_cuts()
CLS_ROWS = ws.CLS_ROWS
K_TRSM_SPLIT_MAX_TILES = lib_const("device_plan.h", "kTrsmSplitMaxTiles")
K_GEMM_SMALL_TILE_MAX = lib_const("device_plan.h", "kGemmSmallTileMax")
K_GEMM_BIG = tuple(lib_const("device_plan.h", k) for k in ("kGemmBigKStep", "kGemmBigMinK", "kGemmBigMinM", "kGemmBigMinN"))
K_ASM_LDS_WAVE_MAX_ROWS, K_ASM_LDS_WG_MAX_ROWS = lib_const("device_plan.h", "kAsmLdsWaveMaxRows"), lib_const("device_plan.h", "kAsmLdsWgMaxRows")
K_SYRK_PIPED_MIN_COLS = lib_const("device_plan.h", "kSyrkPipedMinCols")
POTRF_SHAPE = {16: "k_potrf64_b<1,1>", 32: "k_potrf64_b<2,2>", 48: "k_potrf64_b<4,3>", 64: "k_potrf64_b<8,4>"}


def knobs(setting):
    """SymbolicOptions / EnvKnobs of a handle created under `setting`, as far as the factorisation reads them."""
    k = {"small_rows": 64, "subtree_max": 0, "syrk_xcd": True, "piped_min": K_SYRK_PIPED_MIN_COLS}
    for var, key in (("GMRFX_SMALL_ROWS", "small_rows"), ("GMRFX_SUBTREE_MAX", "subtree_max"), ("GMRFX_SYRK_PIPED", "piped_min")):
        if var in setting:
            k[key] = int(setting[var])
    if "GMRFX_SYRK_XCD" in setting:
        k["syrk_xcd"] = int(setting["GMRFX_SYRK_XCD"]) != 0
    return k


def subtrees(fr, k):
    """symbolic.cpp's subtree tasks -> {root: (first front, class 0 .. 2)}: maximal subtrees (postorder id ranges) of at most
    subtree_max fronts, every one of the three smallest row classes; the class is the tallest front's."""
    ns, submax = len(fr), k["subtree_max"]
    cnt, maxr, ok, allok = [1] * ns, [0] * ns, [False] * ns, [True] * ns
    for s, c, m, _, _, p in fr:
        maxr[s] = max(maxr[s], c + m)
        ok[s] = submax > 0 and ws.small_class(c, m, k["small_rows"]) <= 2 and allok[s] and cnt[s] <= submax
        if p >= 0:
            cnt[p] += cnt[s]
            maxr[p] = max(maxr[p], maxr[s])
            allok[p] = allok[p] and ok[s]
    return {s: (s - cnt[s] + 1, 0 if maxr[s] <= 48 else 1 if maxr[s] <= 64 else 2) for s, _, _, _, _, p in fr if ok[s] and not (p >= 0 and ok[p])}


class FLevel:
    """LevelInfo of one factorisation level: the small fronts by class, the big ones sorted by decreasing width."""

    def __init__(self, fr, small_rows):
        self.small = [[f for f in fr if ws.small_class(f[1], f[2], small_rows) == q] for q in range(4)]
        self.big = sorted((f for f in fr if ws.small_class(f[1], f[2], small_rows) == 4), key=lambda f: (-f[1], f[0]))
        self.max_cols = max((f[1] for f in self.big), default=0)
        self.max_rows = max((f[1] + f[2] for f in self.big), default=0)
        self.max_trail = max((f[2] for f in self.big), default=0)
        self.wider = [sum(f[1] > w for f in self.big) for w in WIDTH_CUTS]

    def nblk(self):
        return cdiv(self.max_cols, NB)

    def wider_than(self, cols):
        return sum(f[1] > cols for f in self.big)


def factor_levels(fr, k):
    """-> ({level: FLevel}, {subtree root: (first, class)}): the level lists leave out the fronts of the subtree tasks."""
    subs = subtrees(fr, k)
    inside = {s for r, (f, _) in subs.items() for s in range(f, r + 1)}
    by = {}
    for f in fr:
        if f[0] not in inside:
            by.setdefault(f[3], []).append(f)
    return {l: FLevel(v, k["small_rows"]) for l, v in by.items()}, subs


def choose_assemble(nfronts, max_cols, max_rows):
    if nfronts <= 0:
        return None
    ldmax = (max_rows + 1) & ~1
    if ldmax <= K_ASM_LDS_WAVE_MAX_ROWS:
        return "k_assemble_lds<0>"
    if ldmax <= K_ASM_LDS_WG_MAX_ROWS:
        return "k_assemble_lds<1>" + (":raised_lds" if ldmax * 8 > 65536 else "")
    return "k_assemble"


def trsm_tiles(nactive, max_rows_below):
    return cdiv(max_rows_below, 64) * nactive


def choose_trsm(nactive, max_rows_below):
    if nactive <= 0 or max_rows_below <= 0:
        return None
    return "k_trsm<0,1>" if trsm_tiles(nactive, max_rows_below) <= K_TRSM_SPLIT_MAX_TILES else "k_trsm<0,0>"


def gemm_tiles(nactive, maxM, maxN):
    return cdiv(maxM, 64) * cdiv(maxN, 64) * nactive


def choose_gemm_nt(nactive, K, maxM, maxN):
    if nactive <= 0 or maxM <= 0 or maxN <= 0:
        return None
    step, mink, minm, minn = K_GEMM_BIG
    if K % step == 0 and K >= mink and maxM >= minm and maxN >= minn:
        return "k_gemm_nt_big"
    return "k_gemm_nt<1>" if gemm_tiles(nactive, maxM, maxN) <= K_GEMM_SMALL_TILE_MAX else "k_gemm_nt<2>"


def potrf_shape(wmax):
    return POTRF_SHAPE[next(w for w in (16, 32, 48, 64) if wmax <= w or w == 64)]


def two_chains(L):
    return len(L.big) >= 2 and L.nblk() >= 4


def choose_syrk(L, k):
    """-> [variant]: Device::factor_contribution_blocks."""
    if not L.big or L.max_trail <= 0:
        return []
    huge = k["syrk_xcd"] and L.max_trail >= 4096 and L.max_cols >= 1024
    v = [("k_syrk_cb_rec<true>" if L.max_cols >= k["piped_min"] else "k_syrk_cb_rec<false>") if k["syrk_xcd"] else "k_syrk_cb"]
    return v + ["k_syrk_big"] if huge else v


def panel_launches(L):
    """Device::factor_panel_chains / panel_block -> [(variant, [fronts of the launch], block)] in launch order."""
    out = []
    nf, nblk = len(L.big), L.nblk()
    two = two_chains(L)
    chains = [(L.big[0::2], lambda a: (a + 1) // 2), (L.big[1::2], lambda a: a // 2)] if two else [(L.big, lambda a: a)]
    for b in range(nblk):
        for lst, of in chains:
            n, kb = of(L.wider_than(b * NB)), b * NB
            if n <= 0:
                continue
            if b == 0 and n > 1:
                cut = [0, of(L.wider[0]), of(L.wider[1]), of(L.wider[2]), n]
                for q, w in enumerate((64, 48, 32, 16)):
                    if cut[q + 1] > cut[q]:
                        out.append((potrf_shape(min(w, L.max_cols)) + ":cut", lst[cut[q]:cut[q + 1]], b))
            else:
                out.append((potrf_shape(min(NB, L.max_cols - kb)) + (":arg" if n == 1 else ":list"), lst[:n], b))
            cut32 = of(L.wider[1]) if b == 0 else n
            nnarrow = n - cut32
            below = L.max_rows - kb - 1
            if b == 0 and nnarrow >= NARROW_MIN:
                if cut32 > 0 and choose_trsm(cut32, below):
                    out.append((choose_trsm(cut32, below), lst[:cut32], b))
                if below > 0:
                    out.append(("k_trsm_narrow:" + ("head" if cut32 > 0 else "nohead"), lst[cut32:n], b))
            elif choose_trsm(n, below):
                out.append((choose_trsm(n, below), lst[:n], b))
            J1 = (b // OBK + 1) * OBK
            nnext, nouter = of(L.wider_than((b + 1) * NB)), of(L.wider_than(J1 * NB))
            if b + 1 < J1 and nnext > 0:
                v = choose_gemm_nt(nnext, NB, L.max_rows - kb - NB, min(J1 * NB, L.max_cols) - kb - NB)
                if v:
                    out.append((v + ":K64", lst[:nnext], b))
            if b + 1 == J1 and nouter > 0:
                v = choose_gemm_nt(nouter, OBK * NB, L.max_rows - J1 * NB, L.max_cols - J1 * NB)
                if v:
                    out.append((v + ":K256", lst[:nouter], b))
    return out


def reached(fr, k):
    """{(variant, c, m, children, block, alone)} of one factorisation of a handle with knobs k: every launch of
    Device::factor_levels and the fronts it works on."""
    levels, subs = factor_levels(fr, k)
    out = set()

    def add(variant, flist, b=-1, alone=None):
        for f in flist:
            out.add((variant, f[1], f[2], f[4], b, len(flist) == 1 if alone is None else alone))

    for q in range(3):
        roots = [r for r, (_, cl) in subs.items() if cl == q]
        for r in roots:
            add(f"k_factor_subtree<{CLS_ROWS[q]}>", [fr[s] for s in range(subs[r][0], r + 1)], alone=len(roots) == 1)
    for L in levels.values():
        for q in range(4):
            add(f"k_factor_small<{CLS_ROWS[q]}>", L.small[q])
        if not L.big:
            continue
        add(choose_assemble(len(L.big), L.max_cols, L.max_rows), L.big)
        if two_chains(L):
            add("two_chains:" + ("equal" if len(L.big) % 2 == 0 else "unequal"), L.big)
        for v, flist, b in panel_launches(L):
            add(v, flist, b)
        for v in choose_syrk(L, k):
            add(v, [f for f in L.big if f[2] > 0], alone=len(L.big) == 1)
    return out


# ---- the coverage table ---------------------------------------------------------------------------------------------------
def features(t):
    """The conditions a WANT row may ask of a reached() tuple (variant, c, m, children, block, alone)."""
    _, c, m, nch, b, alone = t
    return {"ch": nch, "m": m, "alone": alone, "later": b > 0, "partial": b > 0 and c - b * NB < NB, "b0": b == 0}


def _want():
    w = []
    for r in (48, 64, 96):
        w.append((f"k_factor_subtree<{r}>", {}))
    for r in CLS_ROWS:
        w.extend((f"k_factor_small<{r}>", {"ch": ch}) for ch in (0, 1, 2, "3+"))
    w.extend(("k_assemble_lds<0>", {"ch": ch}) for ch in ws.KID_COUNTS)
    w.append(("k_assemble_lds<1>", {}))
    for shape in POTRF_SHAPE.values():
        w.append((shape + ":cut", {"b0": True}))
        w.append((shape + ":*", {"later": True}))
        w.append((shape + ":*", {"partial": True}))
    w.append(("k_potrf64_b<8,4>:arg", {}))
    w.extend((v, {}) for v in ("k_trsm<0,1>", "k_trsm<0,0>", "k_trsm_narrow:head", "k_trsm_narrow:nohead"))
    w.extend((f"k_gemm_nt<{t}>:K{kk}", {}) for t in (1, 2) for kk in (64, 256))
    w.extend((v, {}) for v in ("two_chains:equal", "two_chains:unequal"))
    for v in ("k_syrk_cb_rec<false>", "k_syrk_cb_rec<true>", "k_syrk_cb"):
        w.extend((v, {"ch": ch}) for ch in ws.KID_COUNTS)
        w.extend((v, {"m": m}) for m in SYRK_M)
    return w


WANT = _want()
# what n <= ws.N_MAX cannot reach, and where it is exercised today
LEFT_OUT = {
    "k_gemm_nt_big": "test_gpu_parity.py, the dense front of 4700 unknowns",
    "k_syrk_big": "test_gpu_parity.py, the 4700-unknown tests of the huge-front kernels",
    "k_assemble": "the HBM assembly forms need a column above 16384 rows",
    "k_assemble_lds<1>:raised_lds": "the raised-LDS form needs ld above 8192",
    "cyclic root": "the cyclic / distributed root: test_shard_gloo.py and the shard tests of test_gpu_parity.py",
}


def _matches(w, t):
    name, cond = w
    if not (t[0] == name or (name.endswith(":*") and t[0].startswith(name[:-1]))):
        return False
    f = features(t)
    return all((f["ch"] >= 3) if (key == "ch" and val == "3+") else f[key] == val for key, val in cond.items())


def missing(got):
    """WANT rows that no reached() tuple of `got` matches."""
    by = {}
    for t in got:
        by.setdefault(t[0].split(":")[0], []).append(t)
    return [w for w in WANT if not any(_matches(w, t) for t in by.get(w[0].split(":")[0], ()))]


# ---- reference ---------------------------------------------------------------------------------------------------------------
def reference_factor(Q, perm):
    """-> (hi, lo, cols): L = hi + lo of Q[perm][:, perm] = L L' (float64 pair of the np.longdouble factor), cols[j] = rows of
    column j."""
    assert Q.shape[0] <= ws.N_MAX
    A = Q.toarray()[np.ix_(perm, perm)]
    L, cols = ws.cholesky_longdouble(A)
    hi = np.asarray(L, dtype=np.float64)
    lo = np.asarray(L - hi.astype(np.longdouble), dtype=np.float64)
    return hi, lo, cols


def residual(Q, perm, hi, lo, blk=96):
    """max |A - L L'| / max |A|, every product and sum in np.longdouble, A = Q[perm][:, perm], L = hi + lo; by blocks of
    columns, over the columns of L that the block's rows hold at all (the others contribute exact zeros)."""
    A = Q.toarray()[np.ix_(perm, perm)]
    n = A.shape[0]
    nz = hi != 0.0
    worst = np.longdouble(0)
    for j0 in range(0, n, blk):
        j1 = min(n, j0 + blk)
        K = np.nonzero(nz[j0:j1].any(axis=0))[0]
        rows = j0 + np.nonzero(nz[j0:, K].any(axis=1))[0]
        Lr = hi[np.ix_(rows, K)].astype(np.longdouble) + lo[np.ix_(rows, K)]
        Lj = hi[j0:j1][:, K].astype(np.longdouble) + lo[j0:j1][:, K]
        R = A[np.ix_(rows, np.arange(j0, j1))].astype(np.longdouble) - Lr @ Lj.T
        worst = max(worst, np.abs(R).max())
        other = np.setdiff1d(np.arange(j0, n), rows)
        if len(other):
            worst = max(worst, np.abs(A[np.ix_(other, np.arange(j0, j1))]).max())
    return float(worst / np.abs(A).max())


def logdet_ref(hi, lo):
    d = np.diag(hi).astype(np.longdouble) + np.diag(lo)
    return float(2 * np.log(d).sum())


def panels(sym, vals, n):
    """-> (L, stored): the dense n x n factor of the panels' lower trapezoids (elimination order) and the mask of stored
    entries, padding included."""
    L = np.zeros((n, n))
    stored = np.zeros((n, n), dtype=bool)
    for s in range(len(sym.super_parent)):
        f, c = int(sym.super_first[s]), int(sym.super_first[s + 1] - sym.super_first[s])
        rows = sym.rows[sym.row_ptr[s]:sym.row_ptr[s + 1]]
        ld, pp = int(sym.panel_ld[s]), int(sym.panel_ptr[s])
        P = vals[pp:pp + c * ld].reshape(c, ld)[:, :len(rows)].T            # rows x columns of the front
        keep = np.tril(np.ones((len(rows), c), dtype=bool))
        L[rows[:, None], f + np.arange(c)[None, :]] = np.where(keep, P, 0.0)
        stored[rows[:, None], f + np.arange(c)[None, :]] = keep
    return L, stored


def errors(Lg, stored, hi, lo):
    """err[i, j] = |Lg - Lref|[i, j] / max_i |Lref[i, j]| at every stored entry (0 elsewhere). A nonzero of the reference
    outside the stored pattern is an error of the analysis: asserted."""
    assert not ((hi != 0.0) & ~stored).any(), "the reference factor has an entry the panels do not store"
    return np.where(stored, np.abs((Lg - hi) - lo) / np.abs(hi).max(axis=0), 0.0)


def per_front(be, err):
    """[(err, s, c, m, level, children, row in the front, column in the front)]: the worst stored entry of every front."""
    sym = be.symbolic()
    out = []
    for s, c, m, lev, nch, _ in ws.fronts(be):
        rows = sym.rows[sym.row_ptr[s]:sym.row_ptr[s + 1]]
        f = int(sym.super_first[s])
        blk = err[rows][:, f:f + c]
        i, j = np.unravel_index(int(np.argmax(blk)), blk.shape)
        out.append((float(blk[i, j]), s, c, m, lev, nch, int(i), int(j)))
    return out


describe = ws.describe


def padding(stored, hi):
    """Stored entries outside the pattern of the true factor."""
    return stored & (hi == 0.0)


def plant_pivot(Q, perm, hi, lo, ks):
    """Q with the diagonal entry of every elimination column k of ks lowered to L[k, :k] . L[k, :k] - 0.5: pivot k becomes
    -0.5, the columns before k keep their values."""
    Qb = Q.copy().tolil()
    for k in ks:
        row = hi[k, :k].astype(np.longdouble) + lo[k, :k]
        Qb[perm[k], perm[k]] = float(row @ row) - 0.5
    Qb = Qb.tocsc()
    Qb.sort_indices()
    assert np.array_equal(Qb.indptr, Q.indptr) and np.array_equal(Qb.indices, Q.indices)
    return Qb
