"""The triangular sweeps on fronts of PRESCRIBED shape: the cases selinv_shapes.py does not have, the sweeps' per-level
decisions restated in plain Python, an independent extended-precision reference of both solves and the per-front error
measure (test_sweep_shapes_host.py on symbolic-only handles, test_gpu_sweep_shapes.py on the device).

Cases are selinv_shapes specs (build / make under ss.KW, check_shapes); chain_cases, lone_cases, small_path_cases,
mixed_cases and gather_cases are reused as they are. New here (the *_cases functions below): a level whose forward update
is record-driven and its twin just under the threshold, parents with 0 / 1 / 2 / 3 / 5 children, levels in the three
classes of choose_bwd_gemm, wide fronts for the blocked substitution, the split-K edges of the narrow kernels and bottom
subtrees at the sweep tasks' local-vector classes. All three classes of k_bwd_gemm_longk are reached within n = 2000
(400 siblings of at most 8 columns and two of 40: cdiv(40, 32) * 402 = 804 workgroups), with GMRFX_BWD_FRONT=0 -- at the
default a level of >= 192 such fronts is k_bwd_front's -- and GMRFX_SMALL_ROWS=0; nothing is left to the mesh tests.

The restated plan: fronts(be) -> sweep_levels() -> plan_forward / plan_backward / choose_* mirror csrc/device_plan.cpp and
the launch wrappers (launch_xmul's variant choice included), small_class / task_roots mirror the `cls` lambda and the
sweep-task rule of csrc/symbolic.cpp. reached() lists, for one handle and one number of right-hand sides, every
(kernel variant, c, m, children, pass width, alone in its launch) the solves run; WANT is the coverage table the host test
holds the RUNS list to. A WANT row is (variant, c class, m class, children class, nr class, alone), None = any. Variants
whose threshold IS a count of fronts (the record-driven update, k_fwd_update_longk<2>, k_bwd_gemm_longk<2, 8> / <2, 4>, the
four-wave k_xmul forms) cannot be alone in their launch and are asked for with alone = False.

Reference. Full solve: LAPACK's cho_solve plus one correction step, the residual B - Q X evaluated exactly (float64 BLAS
products of Q - diag(Q), entries multiples of 2^-10, with 24-bit slices of X, summed in np.longdouble: the scheme of
selinv_shapes._exact_residual for a right-hand side). Backward-only solve x = P' L^-T z: a Cholesky factorisation of
P Q P' in np.longdouble on the pattern of LAPACK's float64 factor (exact zeros there are zeros of L), column by column,
and a back substitution in np.longdouble; the factor is checked by solving Q x = b with it and comparing with the first
reference. Largest n it is used for: 2134 (wide_level), N_MAX = 2400 is asserted; both references of a case take at most
about 4 s on CPUs (the chains of 250-column fronts)."""
import numpy as np
import scipy.linalg as sl

import selinv_shapes as ss

SACRIFICE = ss.SACRIFICE


def cdiv(a, b):
    return (a + b - 1) // b


# ---- cases -------------------------------------------------------------------------------------------------------------
def _siblings(n_big, seed, extra=()):
    """n_big big leaves (more than 64 rows, or more than 64 columns) with c <= 70, m <= 131, m = 131 and an m < 32 among
    them, plus `extra`."""
    rng = np.random.default_rng(seed)
    kids = [(70, 131, "cols"), (66, 7, "cols"), (50, 20, "cols"), (1, 131, "cols"), (33, 32, "cols")]
    while len(kids) < n_big:
        c = int(rng.integers(1, 71))
        m = int(rng.integers(max(1, 65 - c), 132))
        kids.append((c, m, "cols"))
    assert all(c > 64 or c + m > 64 for c, m, _ in kids)
    return kids[:n_big] + list(extra)


def record_level_cases():
    """rec_over: 38 big siblings (two of them with 3 and 5 children, the third and later taking the long way of FwdTile)
    under one root, cdiv(131, 32) * 38 = 190 > 128 tiles: k_fwd_update_rec (k_fwd_update_longk<2> without tile records);
    rec_under: 25 of them, 125 tiles: k_fwd_update_longk<1>. Each with small fronts beside them."""
    small = [(10, 20, "cols"), (31, 33, "cols"), (60, 4, "cols")]
    par3 = (68, 90, "cols", [(9, 30, "both"), (12, 41, "both"), (7, 35, "both")])
    par5 = (69, 100, "cols", [(9, 30, "both"), (12, 41, "both"), (7, 35, "both"), (5, 64, "both"), (11, 33, "both")])
    return [{"name": "rec_over", "root": 220, "children": _siblings(36, 81) + [par3, par5] + small + [SACRIFICE], "seed": 81},
            {"name": "rec_under", "root": 220, "children": _siblings(23, 82) + [par3, par5] + small + [SACRIFICE], "seed": 82}]


KID_COUNTS = (0, 1, 2, 3, 5)
_KIDS = [(20, 50, "both"), (33, 40, "both"), (9, 70, "both"), (17, 31, "both"), (25, 64, "both")]


def children_cases():
    """A parent with 60 trailing rows ALONE on its level over 0, 1, 2, 3 and 5 children whose trailing rows land in its own
    columns and in its trailing rows; 70 columns (never a task) and 40 columns (with its children a sweep task at the
    defaults, a level front under GMRFX_SWEEP_TASK_ROWS=0)."""
    assert not any(ss.absorbed(c, 60, 150, 0) or ss.absorbed(kc, km, c, 60) for c in (70, 40) for kc, km, _ in _KIDS)
    return [{"name": f"kids{k}_c{c}", "root": 150, "children": [(c, 60, "cols", _KIDS[:k])], "seed": 90 + 10 * k + c,
             "parent": (c, 60, k)} for k in KID_COUNTS for c in (70, 40)]


def backward_class_cases():
    """Levels of many narrow siblings (big under GMRFX_SMALL_ROWS=0) in the classes of choose_bwd_gemm by
    cdiv(max_cols, 32) * nfronts (the sacrificial child counts): 2 * 122 = 244 < 384, 2 * 202 = 404 in 384..768,
    2 * 402 = 804 > 768."""
    out = []
    for name, cnt in (("bwd_below", 120), ("bwd_inside", 200), ("bwd_above", 400)):
        rng = np.random.default_rng(cnt)
        kids = [(40, 37, "cols")] + [(int(rng.integers(1, 9)), int(rng.integers(1, 41)), "cols") for _ in range(cnt)]
        out.append({"name": name, "root": 150, "children": kids + [SACRIFICE], "seed": cnt, "nsib": cnt + 1})
    return out


WIDE_C, WIDE_M = (65, 127, 128, 129, 191, 257), (0, 33, 257)


def wide_cases():
    """c in WIDE_C at m = 0 (lone fronts), m = 33 and m = 257 (chains, one front per level), and all of them on ONE level
    (wide_level: the blocks' launches shrink from front to front), for GMRFX_INV_CAP=64 / 128: 2 .. 5 blocks, ragged last."""
    out = [{"name": f"wide{c}_m0", "root": c, "children": [], "seed": 500 + c, "alone": True} for c in WIDE_C]
    for m in WIDE_M[1:]:
        spec = None
        for c in WIDE_C:
            spec = (c, m, "both", [spec] if spec else [])
        out.append({"name": f"wide_m{m}", "root": ss.HELPER_ROOT, "children": [(ss.HELPER[0], ss.HELPER[1], "cols", [spec])],
                    "seed": 520 + m, "alone": True})
    out.append({"name": "wide_level", "root": 300, "children": [(c, m, "cols") for c in WIDE_C for m in WIDE_M[1:]] + [SACRIFICE], "seed": 560})
    return out


def splitk_cases():
    """c in {128, 129} x m in {256, 257}, one front per level: kWaveSplitCols, kWaveSplitRows; below them one 16-column tile
    with 257 trailing rows."""
    spec = None
    for c, m in ((16, 257), (128, 256), (129, 257), (129, 256), (128, 257)):
        spec = (c, m, "both", [spec] if spec else [])
    return [{"name": "splitk", "root": ss.HELPER_ROOT, "children": [(ss.HELPER[0], ss.HELPER[1], "cols", [spec])], "seed": 570, "alone": True}]


TASK_ROWS = (159, 160, 161, 287, 288)       # own columns of the subtree + trailing rows of its root
TASK_COLS = (15, 16, 17, 32, 33, 64)        # chunk width edges


def task_cases():
    """Five bottom subtrees under one root whose local vectors have TASK_ROWS rows, with fronts of TASK_COLS columns."""
    low = [(64, 30), (16, 10), (26, 9)]
    low2 = [(64, 30), (17, 10), (26, 9)]
    low3 = [(64, 30), (33, 10), (27, 9)]
    tall = [(64, 40, "both", [(32, 20), (16, 11)]), (63, 21), (17, 12)]
    subs = [(33, 20, "cols", low), (32, 21, "cols", low2), (15, 22, "cols", low3), (64, 31, "cols", tall), (64, 32, "cols", tall)]
    for sub, rows in zip(subs, TASK_ROWS):
        assert ss._size(sub) + sub[1] == rows
    return [{"name": "tasks", "root": 200, "children": subs + [SACRIFICE], "seed": 580}]


def new_cases():
    return record_level_cases() + children_cases() + backward_class_cases() + wide_cases() + splitk_cases() + task_cases()


# ---- settings, widths and the list of runs ------------------------------------------------------------------------------------
WIDTHS = (1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 37, 63, 64, 65)
KNOB_VARS = ("GMRFX_FWD_FRONT", "GMRFX_BWD_FRONT", "GMRFX_SWEEP_TASK_ROWS", "GMRFX_SUBTREE_MAX", "GMRFX_SMALL_ROWS", "GMRFX_SYRK_XCD",
             "GMRFX_INV_CAP", "GMRFX_TASK_MODE", "GMRFX_LEVEL_MARK", "GMRFX_SYRK_PIPED")
DEFAULTS = {}
FRONT = {"GMRFX_FWD_FRONT": "1", "GMRFX_BWD_FRONT": "1"}
LEVEL = {"GMRFX_SWEEP_TASK_ROWS": "0", "GMRFX_SUBTREE_MAX": "0"}
LEVEL0 = dict(LEVEL, GMRFX_SMALL_ROWS="0")
LEVEL128 = dict(LEVEL, GMRFX_SMALL_ROWS="128")
XCD0 = {"GMRFX_SYRK_XCD": "0"}
CAP64, CAP128 = {"GMRFX_INV_CAP": "64"}, {"GMRFX_INV_CAP": "128"}
TASK_WG, TASK_WAVE = {"GMRFX_TASK_MODE": "wg"}, {"GMRFX_TASK_MODE": "wave"}
BWD_GEMM = {"GMRFX_BWD_FRONT": "0", "GMRFX_SMALL_ROWS": "0"}
W_WIDE = (17, 31, 32, 33, 37, 63, 64, 65)                 # passes the front kernels take
W_EDGE = (1, 8, 9, 16, 17, 32, 33, 64, 65)
W_FEW = (1, 16, 17, 33, 64)


def runs():
    """[(group, cases, [(setting, widths)])]: what test_gpu_sweep_shapes.py runs and test_sweep_shapes_host.py holds to WANT."""
    return [
        ("chains", ss.chain_cases(), [(DEFAULTS, WIDTHS), (FRONT, W_WIDE), (LEVEL, WIDTHS), (LEVEL0, W_EDGE), (LEVEL128, W_FEW), (XCD0, W_EDGE)]),
        ("lone", ss.lone_cases(), [(DEFAULTS, W_EDGE), (FRONT, W_WIDE)]),
        ("small", ss.small_path_cases(), [(DEFAULTS, W_FEW), (LEVEL, W_EDGE), (LEVEL0, W_FEW), (LEVEL128, W_EDGE)]),
        ("mixed", ss.mixed_cases() + ss.gather_cases(), [(DEFAULTS, WIDTHS), (FRONT, W_WIDE), (LEVEL, WIDTHS), (XCD0, W_EDGE)]),
        ("records", record_level_cases(), [(DEFAULTS, WIDTHS), (FRONT, W_WIDE), (LEVEL, W_EDGE), (XCD0, WIDTHS)]),
        ("children", children_cases(), [(DEFAULTS, WIDTHS), (FRONT, W_WIDE), (LEVEL, WIDTHS), (XCD0, W_EDGE), (dict(LEVEL, **XCD0), W_EDGE)]),
        ("bwd_classes", backward_class_cases(), [(DEFAULTS, W_FEW), (BWD_GEMM, W_EDGE)]),
        ("wide", wide_cases(), [(DEFAULTS, W_EDGE), (CAP64, WIDTHS), (CAP128, WIDTHS), (dict(CAP64, **FRONT), W_WIDE), (dict(CAP128, **FRONT), W_WIDE)]),
        ("splitk", splitk_cases(), [(DEFAULTS, WIDTHS), (LEVEL, WIDTHS), (XCD0, W_EDGE)]),
        ("tasks", task_cases(), [(DEFAULTS, WIDTHS), (TASK_WG, WIDTHS), (TASK_WAVE, WIDTHS)]),
    ]


def label(setting):
    return ",".join(f"{k[6:]}={v}" for k, v in setting.items()) or "defaults"


def apply_setting(monkeypatch, setting):
    """Knobs are read when a handle is created: set them before constructing it."""
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in setting.items():
        monkeypatch.setenv(k, v)


# ---- the restated decisions -----------------------------------------------------------------------------------------------------
NB = 64
CLS_ROWS = (48, 64, 96, 128)
K_NARROW_FWD, K_NARROW_BWD = 32, 16                  # kNarrowPassMax, kNarrowPassMaxBwd
K_FRONT_MAX_COLS = 128
K_FWD_WAVE_COLS, K_BWD_WAVE_ROWS = 1024, 4096
K_SPLIT_COLS, K_SPLIT_ROWS = 128, 256
K_FWD16_MAX_TILES = 128
K_BWD_WIDE8_MIN, K_BWD_8_MAX = 384, 768
K_PERMUTE_NARROW = 8
K_WAVE_ROWS = (160, 288)


def knobs(setting):
    """EnvKnobs / SymbolicOptions of a handle created under `setting`."""
    k = {"inv_cap": 2048, "fwd_front_min": 384, "bwd_front_min": 192, "tile_records": True, "wave_max_nr": 16, "small_rows": 64, "task_rows": 288}
    if "GMRFX_INV_CAP" in setting:
        k["inv_cap"] = NB
        while k["inv_cap"] < int(setting["GMRFX_INV_CAP"]):
            k["inv_cap"] *= 2
    if "GMRFX_TASK_MODE" in setting:
        k["wave_max_nr"] = {"wg": 0, "wave": 64}[setting["GMRFX_TASK_MODE"]]
    for var, key in (("GMRFX_FWD_FRONT", "fwd_front_min"), ("GMRFX_BWD_FRONT", "bwd_front_min"), ("GMRFX_SMALL_ROWS", "small_rows")):
        if var in setting:
            k[key] = int(setting[var])
    if "GMRFX_SWEEP_TASK_ROWS" in setting:
        k["task_rows"] = min(288, int(setting["GMRFX_SWEEP_TASK_ROWS"]))
    if "GMRFX_SYRK_XCD" in setting:
        k["tile_records"] = int(setting["GMRFX_SYRK_XCD"]) != 0
    return k


def small_class(c, m, small_rows):
    """symbolic.cpp's `cls`: 0 .. 3 = the fused small-front kernel of <= 48 / 64 / 96 / 128 rows, 4 = a big front."""
    if c > 64:
        return 4
    for k, rows in enumerate(CLS_ROWS):
        if c + m <= min(rows, small_rows):
            return k
    return 4


def fronts(be):
    """[(s, c, m, level, children, parent)] of every front."""
    sym = be.symbolic()
    c = np.diff(sym.super_first)
    m = np.diff(sym.row_ptr) - c
    nch = np.bincount(sym.super_parent[sym.super_parent >= 0], minlength=len(c))
    return [(s, int(c[s]), int(m[s]), int(sym.level[s]), int(nch[s]), int(sym.super_parent[s])) for s in range(len(c))]


def task_roots(fr, rcap):
    """symbolic.cpp's sweep-task rule -> {root: first front}: maximal subtrees (postorder id ranges) of >= 2 fronts of <= 64
    columns whose own columns plus max(root's trailing rows, 15) fit rcap rows, <= 64 fronts, <= 96 forward chunk records."""
    ns = len(fr)
    cnt, ncol, maxc, nchk, ok = [1] * ns, [0] * ns, [0] * ns, [0] * ns, [False] * ns
    allok = [True] * ns
    for s, c, m, _, _, p in fr:
        ncol[s] += c
        maxc[s] = max(maxc[s], c)
        nchk[s] += sum(max(1, (c + m - min(c, j0 + 16) + 127) // 128) for j0 in range(0, c, 16))
        ok[s] = rcap > 0 and allok[s] and maxc[s] <= 64 and ncol[s] + max(m, 15) <= rcap and cnt[s] <= 64 and nchk[s] <= 96
        if p >= 0:
            cnt[p] += cnt[s]; ncol[p] += ncol[s]; maxc[p] = max(maxc[p], maxc[s]); nchk[p] += nchk[s]
            allok[p] = allok[p] and ok[s]
    return {s: s - cnt[s] + 1 for s, _, _, _, _, p in fr if ok[s] and cnt[s] >= 2 and not (p >= 0 and ok[p])}


class Level:
    """LevelInfo of one sweep level: the small fronts by class, the big ones sorted by decreasing width."""

    def __init__(self, fr, small_rows):
        self.small = [[f for f in fr if small_class(f[1], f[2], small_rows) == k] for k in range(4)]
        self.big = sorted((f for f in fr if small_class(f[1], f[2], small_rows) == 4), key=lambda f: (-f[1], f[0]))
        self.max_cols = max((f[1] for f in self.big), default=0)
        self.max_trail = max((f[2] for f in self.big), default=0)
        self.min_trail = min((f[2] for f in self.big if f[2] > 0), default=0)

    def wider_than(self, cols):
        return sum(f[1] > cols // NB * NB for f in self.big)


def sweep_levels(fr, k):
    """-> ({level: Level}, {root: first}): the sweep lists leave out the fronts of the tasks."""
    tasks = task_roots(fr, k["task_rows"])
    in_task = {s for r, f in tasks.items() for s in range(f, r + 1)}
    by = {}
    for f in fr:
        if f[0] not in in_task:
            by.setdefault(f[3], []).append(f)
    return {l: Level(v, k["small_rows"]) for l, v in by.items()}, tasks


def _split_level(L, front_kernel, front_min, k):
    nf, ntail = len(L.big), 0
    nbk = max(1, cdiv(L.max_cols, k["inv_cap"]))
    nwide = L.wider_than(min(K_FRONT_MAX_COLS, k["inv_cap"]) // NB * NB)
    if front_kernel and front_min > 0 and nf - nwide >= front_min:
        ntail, nf = nf - nwide, nwide
    return {"nf": nf, "ntail": ntail, "nbk": nbk,
            "xmul_fronts": lambda j: min(nf, L.wider_than(j * k["inv_cap"])),
            "own_fronts": lambda j: min(nf, L.wider_than((j + 1) * k["inv_cap"]))}


def plan_forward(L, nr, k):
    narrow = nr <= K_NARROW_FWD
    p = _split_level(L, not narrow, k["fwd_front_min"], k)
    if narrow:
        p["cmin"] = K_FWD_WAVE_COLS if k["tile_records"] else 0
    else:
        p["cmin"] = min(K_FRONT_MAX_COLS, k["inv_cap"]) // NB * NB if p["ntail"] > 0 else 0
    p["wave"] = narrow and k["tile_records"] and L.wider_than(K_FWD_WAVE_COLS) < p["nf"]
    p["wave_split_k"] = L.max_cols > K_SPLIT_COLS
    p["update"] = None
    if p["nf"] > 0 and L.max_cols > p["cmin"]:
        p["update"] = "records" if k["tile_records"] and cdiv(L.max_trail, 32) * p["nf"] > K_FWD16_MAX_TILES else "grid"
    return p


def plan_backward(L, nr, k):
    narrow = nr <= K_NARROW_BWD
    p = _split_level(L, not narrow, k["bwd_front_min"], k)
    p["mmin"] = K_BWD_WAVE_ROWS if narrow else 0
    p["wave"] = narrow and L.max_trail > 0 and L.min_trail <= K_BWD_WAVE_ROWS
    p["wave_split_k"] = L.max_trail > K_SPLIT_ROWS
    p["gemm"] = L.max_trail > p["mmin"]
    return p


def choose_fwd_update(nfronts, max_trail):
    if nfronts <= 0 or max_trail <= 0:
        return None
    return "k_fwd_update_longk<1>" if cdiv(max_trail, 32) * nfronts <= K_FWD16_MAX_TILES else "k_fwd_update_longk<2>"


def choose_bwd_gemm(nfronts, max_cols, blk=-1, cap=1 << 30):
    if nfronts <= 0 or max_cols <= 0:
        return None
    if blk >= 0:
        max_cols = min(max_cols - blk * cap, cap)
    if max_cols <= 0:
        return None
    wg32 = cdiv(max_cols, 32) * nfronts
    if wg32 > K_BWD_8_MAX:
        return "k_bwd_gemm_longk<2,4>"
    return "k_bwd_gemm_longk<2,8>" if wg32 >= K_BWD_WIDE8_MIN else "k_bwd_gemm_longk<1,8>"


def choose_permute(n, nr):
    return None if n <= 0 else "k_permute_narrow" if nr <= K_PERMUTE_NARROW else "k_permute"


def choose_xmul(nfronts, max_c, trans, nr, blk, cap):
    """launch_xmul (inverse.hip)."""
    max_c = min(max_c - blk * cap, cap)
    if nfronts <= 0 or max_c <= 0:
        return None
    name = "k_xmul_narrow" if nr <= (K_NARROW_BWD if trans else K_NARROW_FWD) else "k_xmul"
    return f"{name}<{8 if cdiv(max_c, 16) * nfronts <= 256 else 4}>"


def passes(nrhs):
    """Device::solve: passes of 64 columns and the rest."""
    return [64] * (nrhs // 64) + ([nrhs % 64] if nrhs % 64 else [])


def reached(fr, n, k, nrhs):
    """{(variant, c, m, children, nr, alone)} of a full solve plus a backward-only solve of nrhs right-hand sides on a handle
    with knobs k: every launch of Device::forward / backward / sweep_tasks and the fronts it works on. c = m = children = -1
    for the launches that are not per front (k_permute*)."""
    levels, tasks = sweep_levels(fr, k)
    out = set()
    cap = k["inv_cap"]

    def add(variant, flist, nr):
        for f in flist:
            out.add((variant, f[1], f[2], f[4], nr, len(flist) == 1))

    for nr in passes(nrhs):
        out.add((choose_permute(n, nr), -1, -1, -1, nr, True))
        for root, first in tasks.items():
            rows = sum(fr[s][1] for s in range(first, root + 1)) + fr[root][2]
            form = "task_chunk" if nr > k["wave_max_nr"] else "task_wave"
            cls = "" if form == "task_chunk" or nr <= 4 else "<=160" if rows <= K_WAVE_ROWS[0] else "<=288"
            for s in range(first, root + 1):
                out.add((f"{form}{cls}[rows={rows}]", fr[s][1], fr[s][2], fr[s][4], nr, len(tasks) == 1))
        for L in levels.values():
            for q in range(4):
                add(f"k_fwd_small<{CLS_ROWS[q]}>", L.small[q], nr)
                add(f"k_bwd_small<{CLS_ROWS[q]}>", L.small[q], nr)
            # forward
            p = plan_forward(L, nr, k)
            add("k_fwd_front", L.big[p["nf"]:p["nf"] + p["ntail"]], nr)
            head = L.big[:p["nf"]]
            if head:
                add("k_fwd_assemble", head, nr)
                for j in range(p["nbk"]):
                    fl = head[:p["xmul_fronts"](j)]
                    v = choose_xmul(len(fl), L.max_cols, 0, nr, j, cap)
                    if v:
                        add(v + ":fwd" + (f"[blocks={cdiv(L.max_cols, cap)}]" if p["nbk"] > 1 else ""), fl, nr)
                    fo = head[:p["own_fronts"](j)]
                    if j + 1 < p["nbk"] and fo and L.max_cols - (j + 1) * cap > 0:
                        add("k_fwd_own_update", fo, nr)
                if p["wave"]:
                    add("k_fwd_update_wave<4>" if p["wave_split_k"] else "k_fwd_update_wave<1>", [f for f in head if f[1] <= p["cmin"] and f[2] > 0], nr)
                if p["update"] == "records":
                    add("k_fwd_update_rec", [f for f in head if f[1] > p["cmin"] and f[2] > 0], nr)
                elif p["update"] == "grid":
                    v = choose_fwd_update(len(head), L.max_trail)
                    if v:
                        fl = [f for f in head if f[1] > p["cmin"] and f[2] > 0]
                        out.update((v, f[1], f[2], f[4], nr, len(head) == 1) for f in fl)
            # backward (both forms: y left in X2, and in place with k_copy_own)
            p = plan_backward(L, nr, k)
            add("k_bwd_front", L.big[p["nf"]:p["nf"] + p["ntail"]], nr)
            head = L.big[:p["nf"]]
            if head:
                if p["wave"]:
                    add("k_bwd_wave<4>" if p["wave_split_k"] else "k_bwd_wave<1>", [f for f in head if 0 < f[2] <= p["mmin"]], nr)
                if p["gemm"]:
                    v = choose_bwd_gemm(len(head), L.max_cols)
                    out.update((v, f[1], f[2], f[4], nr, len(head) == 1) for f in head if f[2] > p["mmin"])
                for j in range(p["nbk"] - 1, -1, -1):
                    fo = head[:p["own_fronts"](j)]
                    if j + 1 < p["nbk"] and fo:
                        v = choose_bwd_gemm(len(fo), L.max_cols, j, cap)
                        if v:
                            add(v + ":block", fo, nr)
                    fl = head[:p["xmul_fronts"](j)]
                    v = choose_xmul(len(fl), L.max_cols, 1, nr, j, cap)
                    if v:
                        add(v + ":bwd" + (f"[blocks={cdiv(L.max_cols, cap)}]" if p["nbk"] > 1 else ""), fl, nr)
                        add("k_copy_own" + ("[blocked]" if p["nbk"] > 1 else ""), fl, nr)
    return out


# ---- classes and the coverage table ---------------------------------------------------------------------------------------------
def c_class(c):
    return next((f"c<={b}" for b in (16, 32, 64, 128, 256) if c <= b), "c>256")


def m_class(m):
    return "m=0" if m == 0 else "m<16" if m < 16 else "m<32" if m < 32 else "m<=256" if m <= 256 else "m>256"


def ch_class(nch):
    return min(nch, 3)


def nr_class(nr):
    return next(name for hi, name in ((1, "1"), (8, "2-8"), (15, "9-15"), (16, "16"), (31, "17-31"), (32, "32"), (63, "33-63"), (64, "64")) if nr <= hi)


def classes(t):
    """(variant, c class, m class, children class, nr class, alone) of a reached() tuple."""
    return (t[0], c_class(t[1]), m_class(t[2]), ch_class(t[3]), nr_class(t[4]), t[5])


NR_NARROW_BWD = ("1", "2-8", "9-15", "16")
NR_NARROW_FWD = NR_NARROW_BWD + ("17-31", "32")
NR_WIDE_FWD = ("33-63", "64")
NR_WIDE_BWD = ("17-31", "32") + NR_WIDE_FWD
NR_ALL = NR_NARROW_FWD + NR_WIDE_FWD
M_FRONT = ("m=0", "m<16", "m<32", "m<=256")


def _want():
    w = []

    def rows(variant, cs=(None,), ms=(None,), chs=(None,), nrs=(None,), alone=True):
        w.extend((variant, c, m, ch, nr, alone) for c in cs for m in ms for ch in chs for nr in nrs)

    rows("k_permute_narrow", nrs=("1", "2-8"))
    rows("k_permute", nrs=NR_ALL[2:])
    # the one-workgroup front kernels: column-tile classes x every wide pass class, trailing-row classes, children
    rows("k_fwd_front", cs=("c<=16", "c<=32", "c<=64", "c<=128"), nrs=NR_WIDE_FWD)
    rows("k_fwd_front", ms=M_FRONT, nrs=NR_WIDE_FWD)
    rows("k_fwd_front", chs=(0, 1, 2, 3))
    rows("k_bwd_front", cs=("c<=16", "c<=32", "c<=64", "c<=128"), nrs=NR_WIDE_BWD)
    rows("k_bwd_front", ms=M_FRONT, nrs=NR_WIDE_BWD)
    # the fused small-front kernels, four row classes
    for r in CLS_ROWS:
        rows(f"k_fwd_small<{r}>", nrs=("1", "16", "17-31", "33-63", "64"))
        rows(f"k_bwd_small<{r}>", nrs=("1", "16", "17-31", "33-63", "64"))
    # head fronts: assembly with 0 .. 3+ children, whole inverse
    rows("k_fwd_assemble", chs=(0, 1, 2, 3), nrs=("1", "17-31", "64"))
    rows("k_xmul_narrow<8>:fwd", cs=("c<=16", "c<=64", "c<=128", "c<=256", "c>256"), nrs=NR_NARROW_FWD)
    rows("k_xmul<8>:fwd", cs=("c<=16", "c<=64", "c<=128", "c<=256", "c>256"), nrs=NR_WIDE_FWD)
    rows("k_xmul_narrow<8>:bwd", cs=("c<=16", "c<=64", "c<=128", "c<=256", "c>256"), nrs=NR_NARROW_BWD)
    rows("k_xmul<8>:bwd", cs=("c<=16", "c<=64", "c<=128", "c<=256", "c>256"), nrs=NR_WIDE_BWD)
    for v in ("k_xmul_narrow<4>:fwd", "k_xmul<4>:fwd", "k_xmul_narrow<4>:bwd", "k_xmul<4>:bwd"):
        rows(v, alone=False)
    rows("k_copy_own", nrs=("1", "16", "17-31", "64"))
    # blocked substitution: 2, 3 and 5 blocks, alone on the level
    for nb in (2, 3, 5):
        for d, nrs in (("fwd", NR_NARROW_FWD + NR_WIDE_FWD), ("bwd", NR_NARROW_BWD + NR_WIDE_BWD)):
            for nrc in nrs:
                name = "k_xmul_narrow" if nrc in (NR_NARROW_FWD if d == "fwd" else NR_NARROW_BWD) else "k_xmul"
                rows(f"{name}<8>:{d}[blocks={nb}]", nrs=(nrc,))
    rows("k_fwd_own_update", ms=("m=0", "m<=256", "m>256"), nrs=NR_ALL)
    rows("k_bwd_gemm_longk<1,8>:block", ms=("m=0", "m<=256", "m>256"), nrs=NR_ALL)
    rows("k_copy_own[blocked]", nrs=("1", "16", "17-31", "64"))
    # forward update
    rows("k_fwd_update_wave<1>", chs=(0, 1, 2, 3), nrs=NR_NARROW_FWD)
    rows("k_fwd_update_wave<1>", ms=("m<16", "m<32", "m<=256", "m>256"), nrs=NR_NARROW_FWD)
    rows("k_fwd_update_wave<4>", ms=("m<32", "m<=256", "m>256"), nrs=NR_NARROW_FWD)
    rows("k_fwd_update_longk<1>", chs=(0, 1, 2, 3), nrs=NR_WIDE_FWD)
    rows("k_fwd_update_longk<1>", ms=("m<16", "m<32", "m<=256", "m>256"), nrs=NR_ALL)
    rows("k_fwd_update_rec", ms=("m<16", "m<32", "m<=256"), nrs=NR_WIDE_FWD, alone=False)
    rows("k_fwd_update_rec", chs=(0, 3), nrs=NR_WIDE_FWD, alone=False)
    rows("k_fwd_update_longk<2>", chs=(0, 3), nrs=NR_ALL, alone=False)
    # backward product
    rows("k_bwd_wave<1>", ms=("m<16", "m<32", "m<=256"), cs=("c<=16", "c<=64", "c<=128", "c>256"), nrs=NR_NARROW_BWD)
    rows("k_bwd_wave<4>", cs=("c<=16", "c<=128", "c<=256", "c>256"), nrs=NR_NARROW_BWD)
    rows("k_bwd_gemm_longk<1,8>", ms=("m<16", "m<32", "m<=256", "m>256"), nrs=NR_WIDE_BWD)
    rows("k_bwd_gemm_longk<1,8>", cs=("c<=16", "c<=32", "c<=64", "c<=128", "c<=256", "c>256"), nrs=NR_WIDE_BWD)
    rows("k_bwd_gemm_longk<2,8>", nrs=NR_WIDE_BWD, alone=False)
    rows("k_bwd_gemm_longk<2,4>", nrs=NR_WIDE_BWD, alone=False)
    return w


WANT = _want()
LEFT_TO_MESH_TESTS = ()          # at most the k_bwd_gemm_longk<2,4> class may stand here; it is reached (bwd_above)


def task_variants(rows, mode):
    """The task variants a subtree of `rows` local rows must reach under GMRFX_TASK_MODE = None / "wg" / "wave": {(variant, nr class)}."""
    wave_max = {None: 16, "wg": 0, "wave": 64}[mode]
    out = set()
    for nr in (1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 37, 63, 64):
        form = "task_chunk" if nr > wave_max else "task_wave"
        cls = "" if form == "task_chunk" or nr <= 4 else "<=160" if rows <= K_WAVE_ROWS[0] else "<=288"
        out.add((f"{form}{cls}[rows={rows}]", nr_class(nr)))
    return out


def missing(got):
    """WANT rows no reached class matches. got: set of classes() tuples."""
    idx = {}
    for g in got:
        idx.setdefault(g[0], []).append(g)
    out = []
    for w in WANT:
        if not any(all(a is None or a == b for a, b in zip(w[1:5], g[1:5])) and (g[5] or not w[5]) for g in idx.get(w[0], ())):
            out.append(w)
    return out


# ---- reference -------------------------------------------------------------------------------------------------------------------
N_MAX = 2400


def rhs(n, seed):
    """65 right-hand sides; a solve of width w takes the first w."""
    return np.random.default_rng(1000 + seed).standard_normal((n, 65))


def exact_product(Qd, X, dX=None):
    """Q (X + dX) in np.longdouble, the products with X exact (selinv_shapes: Q = D + A, A on the 2^-10 grid)."""
    n = Qd.shape[0]
    d = np.diag(Qd).copy()
    A = Qd - np.diag(d)
    assert np.array_equal(A * 1024.0, np.round(A * 1024.0)) and np.abs(A).max() <= 1.0 and n <= 8192
    P = d.astype(np.longdouble)[:, None] * X.astype(np.longdouble)
    unit = 2.0 ** np.ceil(np.log2(np.abs(X).max(axis=0)))
    rem = X.copy()
    for p in (1, 2, 3):
        g = unit * 2.0 ** (-24 * p)
        piece = np.round(rem / g) * g
        rem -= piece
        P += A @ piece
    assert np.abs(rem / unit).max() <= 2.0 ** -72
    if dX is not None:
        P += d.astype(np.longdouble)[:, None] * dX.astype(np.longdouble) + (A @ dX)
    return P


def reference_solve(Q, B):
    """-> (X, dX, res): Q^-1 B = X + dX, res[j] = max_i |B - Q (X + dX)|[i, j] / max_i |X[i, j]|. Q is strictly diagonally
    dominant by 1, so |Q^-1|_inf <= 1 and res bounds the reference's own err."""
    Qd = Q.toarray()
    cf = sl.cho_factor(Qd, lower=True)
    X = sl.cho_solve(cf, B)
    R = B.astype(np.longdouble) - exact_product(Qd, X)
    dX = sl.cho_solve(cf, np.asarray(R, dtype=np.float64))
    R2 = B.astype(np.longdouble) - exact_product(Qd, X, dX)
    return X, dX, np.asarray(np.abs(R2).max(axis=0), dtype=np.float64) / np.abs(X).max(axis=0)


def cholesky_longdouble(A):
    """L of A = L L' in np.longdouble, column by column on the pattern of LAPACK's float64 factor. -> (L dense, [rows of column j])"""
    n = A.shape[0]
    L0 = np.linalg.cholesky(A)
    L = np.zeros((n, n), dtype=np.longdouble)
    Al = A.astype(np.longdouble)
    pat = L0 != 0.0
    cols = [np.nonzero(pat[j:, j])[0] + j for j in range(n)]
    for j in range(n):
        r = cols[j]
        K = np.nonzero(pat[j, :j])[0]
        v = Al[r, j]
        if len(K):
            v = v - L[np.ix_(r, K)] @ L[j, K]
        v[0] = np.sqrt(v[0])
        v[1:] /= v[0]
        L[r, j] = v
    return L, cols


def _back_substitute(L, cols, Z):
    X = Z.astype(np.longdouble)
    for j in range(L.shape[0] - 1, -1, -1):
        r = cols[j][1:]
        if len(r):
            X[j] -= L[r, j] @ X[r]
        X[j] /= L[j, j]
    return X


def _forward_substitute(L, cols, B):
    Y = B.astype(np.longdouble)
    for j in range(L.shape[0]):
        Y[j] /= L[j, j]
        r = cols[j][1:]
        if len(r):
            Y[r] -= np.outer(L[r, j], Y[j])
    return Y


def reference_backward(Q, perm, Z, B=None, X=None, dX=None):
    """-> (Xb, dXb, res): P' L^-T Z = Xb + dXb (float64 pair) with L the np.longdouble factor of Q[perm][:, perm]; res =
    the larger of max |L' x - z| / max |x| per column and, with (B, X, dX) of reference_solve, the distance of the solve
    through L from that reference (the check of L itself)."""
    assert Q.shape[0] <= N_MAX
    A = Q.toarray()[np.ix_(perm, perm)]
    L, cols = cholesky_longdouble(A)
    xl = _back_substitute(L, cols, Z)
    scale = np.abs(xl).max(axis=0)
    Ltx = np.stack([L[cols[j], j] @ xl[cols[j]] for j in range(len(cols))])
    res = np.asarray(np.abs(Ltx - Z.astype(np.longdouble)).max(axis=0) / scale, dtype=np.float64)
    if B is not None:
        w = min(B.shape[1], 4)
        xs = _back_substitute(L, cols, _forward_substitute(L, cols, B[perm, :w]))
        d = (xs - X[perm, :w].astype(np.longdouble)) - dX[perm, :w].astype(np.longdouble)
        res = np.maximum(res, float((np.abs(d).max(axis=0) / np.abs(X[:, :w]).max(axis=0)).max()))
    Xb = np.empty(Z.shape)
    dXb = np.empty(Z.shape)
    hi = np.asarray(xl, dtype=np.float64)
    Xb[perm] = hi
    dXb[perm] = np.asarray(xl - hi.astype(np.longdouble), dtype=np.float64)
    return Xb, dXb, res


def errors(G, X, dX):
    """err[i, j] = |G[i, j] - ref[i, j]| / max_i |ref[i, j]|, ref = X + dX."""
    return np.abs((G - X) - dX) / np.abs(X).max(axis=0)


def per_front(be, err):
    """[(err, s, c, m, level, children, row in the front, column)]: the worst entry of every front's own rows."""
    perm = be.ordering_permutation()
    first = be.symbolic().super_first
    e = err[perm]                                  # rows in elimination order
    out = []
    for s, c, m, lev, nch, _ in fronts(be):
        blk = e[int(first[s]):int(first[s]) + c]
        i, j = np.unravel_index(int(np.argmax(blk)), blk.shape)
        out.append((float(blk[i, j]), s, c, m, lev, nch, int(i), int(j)))
    return out


def describe(pf):
    e = max(pf)
    return e[0], f"front {e[1]} (c={e[2]}, m={e[3]}, level {e[4]}, {e[5]} children): row {e[6]} of the front, column {e[7]}, err {e[0]:.3e}"
