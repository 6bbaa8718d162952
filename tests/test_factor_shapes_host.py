"""The case list of test_gpu_factor_shapes.py, verified WITHOUT a device: on symbolic-only handles every new matrix of
tests/factor_shapes.py must come out with exactly the fronts it was built for, the restated small / subtree / big
classification must agree with the analysis under every setting the GPU test uses, the threshold cases must sit on the side
of their threshold they claim, and the restated level driver, walked over every (case, setting) of runs(), must reach every
row of factor_shapes.WANT. A change of the analysis or of a threshold that silently stops a shape from occurring fails here."""
import numpy as np
import pytest

import gmrfx
import orc
import selinv_shapes as ss
import sweep_shapes as ws
import factor_shapes as fs


def _handle(case, monkeypatch, setting):
    fs.apply_setting(monkeypatch, setting)
    Q, blocks = ss.make(case)
    be = gmrfx.MI355XBackend(Q, symbolic_only=True, **ss.KW)
    return be, Q, blocks


def _level_of(got, names):
    lv = {got[n][2] for n in names}
    assert len(lv) == 1
    return lv.pop()


def _children_level(be, got, setting):
    """FLevel of the level right under the root."""
    fr = ws.fronts(be)
    levels, _ = fs.factor_levels(fr, fs.knobs(setting))
    return levels[got["root"][2] - 1], fr


def test_new_cases_have_their_fronts(monkeypatch):
    for case in fs.new_cases():
        be, Q, blocks = _handle(case, monkeypatch, fs.DEFAULTS)
        name = case["name"]
        assert Q.shape[0] <= ws.N_MAX, name
        if "merged" in case:
            # the child is absorbed: one front fewer, the parent's front has the child's columns and its own trailing rows
            got = ss.fronts_of(be, blocks)
            assert len(be.symbolic().level) == len(blocks) - 1 and got["0"] is None and got["0.0"] is None, name
            assert sum((f[1], f[2], f[4]) == (*case["merged"], 0) for f in ws.fronts(be)) == 1, name
            be.close()
            continue
        got = ss.check_shapes(be, blocks)
        kids = [n for n in got if n != "root" and "." not in n]
        if case.get("alone"):
            lv = [g[2] for g in got.values()]
            assert len(set(lv)) == len(lv), name
        if len(kids):
            _level_of(got, kids)                     # the root's children share one level
        be.close()


def test_width_classes_fill_every_piece_of_block_0(monkeypatch):
    case, two = fs.width_cases()
    be, Q, blocks = _handle(case, monkeypatch, fs.LEVEL0)
    got = ss.check_shapes(be, blocks)
    L, fr = _children_level(be, got, fs.LEVEL0)
    assert be.stats()["n_small_fronts"] == 0 and not fs.two_chains(L) and fs.WIDTH_CUTS == (48, 32, 16) and fs.OBK == 4
    assert [f[1] for f in L.big] == sorted(fs.WIDTHS_C + (100, 110, 40), reverse=True)
    cuts = [(v, sorted(f[1] for f in fl)) for v, fl, b in fs.panel_launches(L) if v.endswith(":cut")]
    assert cuts == [("k_potrf64_b<8,4>:cut", [49, 63, 64, 100, 110]), ("k_potrf64_b<4,3>:cut", [33, 40, 47, 48]),
                    ("k_potrf64_b<2,2>:cut", [17, 31, 32]), ("k_potrf64_b<1,1>:cut", [1, 15, 16])]
    # the level under the 110-column front: the first and the last piece only
    levels, _ = fs.factor_levels(fr, fs.knobs(fs.LEVEL0))
    low = levels[got["root"][2] - 2]
    cuts = [(v, sorted(f[1] for f in fl)) for v, fl, b in fs.panel_launches(low) if v.endswith(":cut")]
    assert cuts == [("k_potrf64_b<8,4>:cut", [60, 64]), ("k_potrf64_b<1,1>:cut", [5, 10])]
    # block 1: the 100- and the 110-column front, 46 columns at most
    assert [(v, b) for v, fl, b in fs.panel_launches(L) if b == 1 and "potrf" in v] == [("k_potrf64_b<4,3>:list", 1)]
    # the pivot test's two-level pair: leaves of the upper level numbered before and after the lower front
    lowf = next(f for f in fr if (f[1], f[2]) == (5, 64))
    leaves = [f[0] for f in fr if f[3] == lowf[3] + 1 and f[4] == 0]
    assert min(leaves) < lowf[0] < max(leaves)
    be.close()
    # with a 193-column sibling: two chains, every piece non-empty in both halves
    be, Q, blocks = _handle(two, monkeypatch, fs.LEVEL0)
    got = ss.check_shapes(be, blocks)
    L, fr = _children_level(be, got, fs.LEVEL0)
    assert fs.two_chains(L) and L.nblk() == 4
    cuts = [v for v, fl, b in fs.panel_launches(L) if v.endswith(":cut")]
    assert sorted(cuts) == sorted(2 * [s + ":cut" for s in fs.POTRF_SHAPE.values()])
    be.close()


def test_threshold_cases_sit_where_they_claim(monkeypatch):
    # narrow_min: the narrow siblings, the sacrificial child among them
    for case in fs.narrow_cases():
        be, Q, blocks = _handle(case, monkeypatch, fs.LEVEL0)
        L, _ = _children_level(be, ss.check_shapes(be, blocks), fs.LEVEL0)
        nnarrow = len(L.big) - L.wider[1]
        assert (nnarrow, L.wider[1]) == (case["nnarrow"], case["head"]) and nnarrow in (255, 256) and fs.NARROW_MIN == 256
        v = {x for x, _, _ in fs.panel_launches(L) if "trsm" in x}
        want = {255: {"k_trsm<0,0>"}, 256: {"k_trsm_narrow:head", "k_trsm<0,1>"} if case["head"] else {"k_trsm_narrow:nohead"}}[nnarrow]
        assert v == want, (case["name"], v)
        assert all(1 <= f[2] <= 40 and f[1] <= 32 for f in L.big[L.wider[1]:])
        be.close()
    # choose_trsm: 128 and 130 tiles
    for case, tiles, v in zip(fs.trsm_cases(), (128, 130), ("k_trsm<0,1>", "k_trsm<0,0>")):
        be, Q, blocks = _handle(case, monkeypatch, fs.LEVEL0)
        L, _ = _children_level(be, ss.check_shapes(be, blocks), fs.LEVEL0)
        assert fs.trsm_tiles(len(L.big), L.max_rows - 1) == tiles == case["tiles"] and fs.K_TRSM_SPLIT_MAX_TILES == 128
        assert [x for x, _, b in fs.panel_launches(L) if "trsm" in x and b == 0] == [v]
        be.close()
    # choose_gemm_nt at K = 64: 252 and 270 tiles
    for case, tiles, v in zip(fs.gemm_cases(), (252, 270), ("k_gemm_nt<1>:K64", "k_gemm_nt<2>:K64")):
        for setting in (fs.DEFAULTS, fs.LEVEL0):
            be, Q, blocks = _handle(case, monkeypatch, setting)
            L, _ = _children_level(be, ss.check_shapes(be, blocks), setting)
            assert not fs.two_chains(L) and L.max_cols == 192
            assert fs.gemm_tiles(L.wider_than(64), L.max_rows - 64, min(256, L.max_cols) - 64) == tiles == case["tiles"] and fs.K_GEMM_SMALL_TILE_MAX == 256
            assert [x for x, _, b in fs.panel_launches(L) if "gemm" in x and b == 0] == [v]
            be.close()
    # the dense front and its twin: tiles of the K = 256 update, ld of the assembly, FrontArg blocks
    for case, tiles, ld, nblk, gemm, asm in zip(fs.dense_cases(), (289, 256), (1282, 1280), (21, 20), ("k_gemm_nt<2>:K256", "k_gemm_nt<1>:K256"),
                                                ("k_assemble_lds<1>", "k_assemble_lds<0>")):
        be, Q, blocks = _handle(case, monkeypatch, fs.DEFAULTS)
        fr = ws.fronts(be)
        levels, _ = fs.factor_levels(fr, fs.knobs(fs.DEFAULTS))
        (L,) = levels.values()
        c = L.max_cols
        assert int(be.symbolic().panel_ld[0]) == ld and (ld > fs.K_ASM_LDS_WAVE_MAX_ROWS) == (asm == "k_assemble_lds<1>")
        assert fs.gemm_tiles(1, c - 256, c - 256) == tiles and fs.choose_assemble(1, c, c) == asm
        la = fs.panel_launches(L)
        assert [x for x, _, b in la if "gemm" in x and b == 3] == [gemm]
        assert sum("potrf" in x and x.endswith(":arg") for x, _, _ in la) == nblk and len(fr) == 1
        be.close()
    # kSyrkPipedMinCols: widest front of 127 and of 128 columns
    for case, v in zip(fs.syrk_cases()[:2], ("k_syrk_cb_rec<false>", "k_syrk_cb_rec<true>")):
        be, Q, blocks = _handle(case, monkeypatch, fs.DEFAULTS)
        L, _ = _children_level(be, ss.check_shapes(be, blocks), fs.DEFAULTS)
        assert L.max_cols == case["widest"] and fs.choose_syrk(L, fs.knobs(fs.DEFAULTS)) == [v] and fs.K_SYRK_PIPED_MIN_COLS == 128
        assert sorted(f[2] for f in L.big if f[1] == 70) == list(fs.SYRK_M)
        assert fs.choose_syrk(L, fs.knobs(fs.PIPED0)) == ["k_syrk_cb_rec<true>"] and fs.choose_syrk(L, fs.knobs(fs.PIPED_NEVER)) == ["k_syrk_cb_rec<false>"]
        assert fs.choose_syrk(L, fs.knobs(fs.XCD0)) == ["k_syrk_cb"]
        be.close()


def test_chain_and_children_cases(monkeypatch):
    # two chains: from two fronts and four blocks on
    want = {"pair2": (True, 2), "pair3": (True, 3), "pair_apart": (True, 2), "pair1": (False, 1), "pair_nblk3": (False, 3)}
    for case in fs.chain_pair_cases():
        be, Q, blocks = _handle(case, monkeypatch, fs.DEFAULTS)
        L, _ = _children_level(be, ss.check_shapes(be, blocks), fs.DEFAULTS)
        assert (fs.two_chains(L), len(L.big)) == want[case["name"]] and [(f[1], f[2]) for f in L.big] == case["big"]
        assert (L.nblk() >= 4) == (case["name"] != "pair_nblk3") and len(L.small[0]) == 1
        if case["name"] == "pair_apart":       # blocks 4 .. 7 run on the first chain alone, through FrontArg
            assert [(v, b) for v, fl, b in fs.panel_launches(L) if "potrf" in v and b >= 4] == [("k_potrf64_b<8,4>:arg", b) for b in (4, 5, 6)] + [("k_potrf64_b<1,1>:arg", 7)]
        be.close()
    # SYRK children: more than 64 of each child's rows land in the parent's trailing rows and span more than one 64-row tile
    for case in fs.syrk_cases()[2:]:
        be, Q, blocks = _handle(case, monkeypatch, fs.DEFAULTS)
        ss.check_shapes(be, blocks)
        fr = ws.fronts(be)
        c, m, k = case["parent"]
        (par,) = [f for f in fr if (f[1], f[2]) == (c, m)]
        assert par[4] == k and sum(f[3] == par[3] and ws.small_class(f[1], f[2], 64) == 4 for f in fr) == 1
        sym = be.symbolic()
        in_cols = 0
        for d in np.nonzero(sym.super_parent == par[0])[0]:
            rel = sym.rel[sym.row_ptr[d] + (sym.super_first[d + 1] - sym.super_first[d]):sym.row_ptr[d + 1]]
            if rel.max() < c:
                in_cols += 1
                continue
            t = rel[rel >= c] - c
            assert len(t) > 64 and t.min() // 64 < t.max() // 64, (case["name"], d)
        assert in_cols == (case["name"] == "syrk_kids_cols")
        be.close()
    # small fronts: the classes at their row edges, the parents per class, the subtrees
    be, Q, blocks = _handle(fs.small_cases()[0], monkeypatch, fs.LEVEL128)
    L, _ = _children_level(be, ss.check_shapes(be, blocks), fs.LEVEL128)
    assert [sorted((f[1], f[2]) for f in q) for q in L.small] == [[(1, 47), (40, 3)], [(1, 48), (1, 63), (48, 1)], [(1, 64), (1, 95), (64, 1), (64, 32)],
                                                                 [(1, 96), (1, 127), (64, 33), (64, 64)]]
    be.close()
    for case in fs.small_cases()[1:6]:
        be, Q, blocks = _handle(case, monkeypatch, fs.SUBTREE)
        got = ss.check_shapes(be, blocks)
        fr = ws.fronts(be)
        levels, subs = fs.factor_levels(fr, fs.knobs(fs.SUBTREE))
        k = case["kids"]
        cls = sorted((q, r - f + 1) for r, (f, q) in subs.items())
        # the 48-, 64- and 96-row parents with their children, the sacrificial child, the children of the 128-row parent
        assert cls == sorted([(0, k + 1), (1, k + 1), (2, k + 1), (0, 1)] + k * [(0, 1)]), (case["name"], cls)
        assert [(f[1], f[2], f[4]) for f in levels[got["root"][2] - 1].small[3]] == [(40, 88, k)]
        be.close()
    for case, big in zip(fs.small_cases()[6:], ((10, 38, 8), (30, 67, 1))):
        be, Q, blocks = _handle(case, monkeypatch, fs.SUBTREE)
        ss.check_shapes(be, blocks)
        fr = ws.fronts(be)
        levels, subs = fs.factor_levels(fr, fs.knobs(fs.SUBTREE))
        (par,) = [f for f in fr if (f[1], f[2], f[4]) == big]
        assert par[0] not in subs and all(r - f == 0 for r, (f, _) in subs.items()) and len(subs) == big[2] + 1
        be.close()


def test_every_row_of_the_coverage_table_is_reached(monkeypatch):
    got = set()
    for group, cases, settings in fs.runs():
        for case in cases:
            for setting in settings:
                be, Q, blocks = _handle(case, monkeypatch, setting)
                k = fs.knobs(setting)
                fr = ws.fronts(be)
                levels, subs = fs.factor_levels(fr, k)
                # the restated classification against the analysis
                sym, st = be.symbolic(), be.stats()
                in_sub = sum(r - f + 1 for r, (f, _) in subs.items())
                nsmall = sum(len(q) for L in levels.values() for q in L.small)
                assert st["n_small_fronts"] == nsmall + in_sub and st["n_big_fronts"] == sum(len(L.big) for L in levels.values()), (case["name"], setting)
                assert nsmall == sum(ws.small_class(f[1], f[2], k["small_rows"]) < 4 for L in levels.values() for q in L.small for f in q)
                assert sorted(levels) == sorted({int(l) for s, l in enumerate(sym.level) if not any(f <= s <= r for r, (f, _) in subs.items())})
                if k["subtree_max"] > 0:
                    assert be.sweep_tasks()[0] == 0          # the sweep tasks give way to the subtree tasks
                else:
                    assert not subs
                got |= fs.reached(fr, k)
                be.close()
    miss = fs.missing(got)
    assert not miss, f"{len(miss)} rows of the coverage table are not reached, the first: {miss[:8]}"
    # what this size cannot reach is exactly LEFT_OUT, and none of it is reached
    assert set(fs.LEFT_OUT) == {"k_gemm_nt_big", "k_syrk_big", "k_assemble", "k_assemble_lds<1>:raised_lds", "cyclic root"}
    assert not {t[0].split(":K")[0] for t in got} & set(fs.LEFT_OUT)


def test_wanted_variants_name_every_launch_of_the_factorisation():
    names = {w[0] for w in fs.WANT}
    for v in ("k_factor_subtree<48>", "k_factor_subtree<64>", "k_factor_subtree<96>", "k_factor_small<48>", "k_factor_small<64>", "k_factor_small<96>",
              "k_factor_small<128>", "k_assemble_lds<0>", "k_assemble_lds<1>", "k_potrf64_b<1,1>:cut", "k_potrf64_b<2,2>:cut", "k_potrf64_b<4,3>:cut",
              "k_potrf64_b<8,4>:cut", "k_potrf64_b<8,4>:arg", "k_trsm<0,1>", "k_trsm<0,0>", "k_trsm_narrow:head", "k_trsm_narrow:nohead", "k_gemm_nt<1>:K64",
              "k_gemm_nt<1>:K256", "k_gemm_nt<2>:K64", "k_gemm_nt<2>:K256", "two_chains:equal", "two_chains:unequal", "k_syrk_cb_rec<false>",
              "k_syrk_cb_rec<true>", "k_syrk_cb"):
        assert v in names, v
    for shape in fs.POTRF_SHAPE.values():
        assert (shape + ":*", {"later": True}) in fs.WANT and (shape + ":*", {"partial": True}) in fs.WANT
    for v in ("k_syrk_cb_rec<false>", "k_syrk_cb_rec<true>", "k_syrk_cb"):
        assert all((v, {"m": m}) in fs.WANT for m in (1, 63, 64, 65, 127, 128, 129, 193)) and all((v, {"ch": c}) in fs.WANT for c in (0, 1, 2, 3, 5))


def test_reference_checks_itself_and_a_perturbed_entry_names_its_front(monkeypatch):
    """The reference on the 3-children SYRK case: its own residual, both float64 witnesses against it (what the device bound
    is 16 x of), the padding of an amalgamated front, and the per-front report on a perturbed entry of the oracle's factor."""
    import test_gpu_factor_shapes as g
    case = next(c for c in fs.syrk_cases() if c["name"] == "syrk_kids3")
    be, Q, blocks = _handle(case, monkeypatch, fs.DEFAULTS)
    n = Q.shape[0]
    perm = be.ordering_permutation()
    hi, lo, _ = fs.reference_factor(Q, perm)
    assert fs.residual(Q, perm, hi, lo) <= g.BOUND / 100
    bad = hi.copy()
    bad[n - 1, n - 2] += 1e-12
    assert fs.residual(Q, perm, bad, lo) > g.BOUND / 100          # the residual sees one wrong entry
    full = np.ones((n, n), dtype=bool)
    el = fs.errors(np.linalg.cholesky(Q.toarray()[np.ix_(perm, perm)]), full, hi, lo).max()
    Lo = np.tril(orc.OracleFactor(Q, perm).L().toarray())
    eo = fs.errors(Lo, full, hi, lo).max()
    assert 1e-18 < el <= g.WITNESS_ERR_MAX and 1e-18 < eo <= g.WITNESS_ERR_MAX
    # the panels of the oracle's factor, in the device's layout; a perturbed entry: row 75 of the 3-children parent, column 11
    sym = be.symbolic()
    fr = ws.fronts(be)
    vals = np.zeros(int(sym.panel_ptr[-1]))
    for s, c, m, _, _, _ in fr:
        rows = sym.rows[sym.row_ptr[s]:sym.row_ptr[s + 1]]
        f, ld, pp = int(sym.super_first[s]), int(sym.panel_ld[s]), int(sym.panel_ptr[s])
        for j in range(c):
            vals[pp + j * ld:pp + j * ld + c + m] = Lo[rows, f + j]
    Lg, stored = fs.panels(sym, vals, n)
    assert np.array_equal(Lg, Lo) and stored.sum() == sum(c * (c + m) - c * (c - 1) // 2 for _, c, m, _, _, _ in fr)
    par = [f for f in fr if (f[1], f[2], f[4]) == (70, 150, 3)][0]
    vals[int(sym.panel_ptr[par[0]]) + 11 * int(sym.panel_ld[par[0]]) + 75] += 2 * g.BOUND * np.abs(hi[:, int(sym.super_first[par[0]]) + 11]).max()
    Lg, stored = fs.panels(sym, vals, n)
    err, where = fs.describe(fs.per_front(be, fs.errors(Lg, stored, hi, lo)))
    assert err > g.BOUND and where.startswith(f"front {par[0]} (c=70, m=150, level {par[3]}, 3 children): row 75 of the front, column 11"), where
    be.close()
    # padding: the stored entries of a merged front that the true factor does not have
    for case in fs.amalgamated_cases():
        be, Q, blocks = _handle(case, monkeypatch, fs.DEFAULTS)
        perm = be.ordering_permutation()
        hi, lo, _ = fs.reference_factor(Q, perm)
        sym = be.symbolic()
        _, stored = fs.panels(sym, np.zeros(int(sym.panel_ptr[-1])), Q.shape[0])
        cd, md = case["children"][0][3][0][:2]
        cp, mp = case["children"][0][:2]
        assert fs.padding(stored, hi).sum() == cd * (cp + mp - md) > 0, case["name"]
        be.close()
