"""The case list of test_gpu_sweep_shapes.py, verified WITHOUT a device: on symbolic-only handles every new matrix of
tests/sweep_shapes.py must come out with exactly the fronts it was built for, the restated small-front / task
classification must agree with the analysis, and the restated per-level plan, walked over every (case, knob setting,
width) the GPU test runs, must reach every class of sweep_shapes.WANT -- by a front alone in its launch wherever the
variant allows one. A change of the analysis or of a threshold that silently stops a shape from occurring fails here."""
import numpy as np
import pytest

import gmrfx
import orc
import selinv_shapes as ss
import sweep_shapes as ws


def _handle(case, monkeypatch, setting):
    ws.apply_setting(monkeypatch, setting)
    Q, blocks = ss.make(case)
    be = gmrfx.MI355XBackend(Q, symbolic_only=True, **ss.KW)
    return be, Q, blocks


def test_new_cases_have_their_fronts(monkeypatch):
    for case in ws.new_cases():
        be, Q, blocks = _handle(case, monkeypatch, ws.DEFAULTS)
        assert Q.shape[0] <= ws.N_MAX, case["name"]
        got = ss.check_shapes(be, blocks)
        fr = ws.fronts(be)
        kids = [g for name, g in got.items() if name != "root" and "." not in name]
        if case.get("alone"):
            lv = [g[2] for g in got.values()]
            assert len(set(lv)) == len(lv), case["name"]
        if case["name"].startswith("rec_"):
            big = [g for g in kids if ws.small_class(g[0], g[1], 64) == 4]
            tiles = ws.cdiv(max(g[1] for g in big), 32) * len(big)
            assert (tiles > ws.K_FWD16_MAX_TILES) == (case["name"] == "rec_over") and 100 < tiles < 200
            assert len({g[2] for g in kids}) == 1 and min(g[1] for g in big) < 32 and max(g[1] for g in big) == 131 and max(g[0] for g in big) <= 70
            assert sorted(f[4] for f in fr if f[3] == kids[0][2] and f[4])[-2:] == [3, 5]
        if "parent" in case:
            c, m, k = case["parent"]
            par = [f for f in fr if (f[1], f[2]) == (c, m)]
            assert len(par) == 1 and par[0][4] == k and sum(f[3] == par[0][3] for f in fr) == 1
            sym, s = be.symbolic(), par[0][0]
            for d in np.nonzero(sym.super_parent == s)[0]:      # each child reaches the parent's columns AND its trailing rows
                rel = sym.rel[sym.row_ptr[d] + (sym.super_first[d + 1] - sym.super_first[d]):sym.row_ptr[d + 1]]
                assert rel.min() < c <= rel.max(), (case["name"], d)
        if case["name"].startswith("bwd_"):
            assert len(kids) == case["nsib"] + 1 and len({g[2] for g in kids}) == 1 and max(g[0] for g in kids) == 40
        if case["name"] == "wide_level":
            assert len({g[2] for g in kids}) == 1 and sorted({g[0] for g in kids if g[0] != 40}) == list(ws.WIDE_C)
        if case["name"] == "tasks":
            cap, first, last, _ = be.sweep_tasks()
            c = np.diff(be.symbolic().super_first)
            rows = sorted(int(c[f:l + 1].sum()) + fr[l][2] for f, l in zip(first, last))
            assert cap == 288 and rows == list(ws.TASK_ROWS)
            incols = {int(v) for f, l in zip(first, last) for v in c[f:l + 1]}
            assert set(ws.TASK_COLS) <= incols
            ch = be.sweep_chunks()
            assert len(ch["task_ptr"]) == 6 and len(ch["bwd"]) == sum(ws.cdiv(int(v), 16) for f, l in zip(first, last) for v in c[f:l + 1])
        be.close()


def test_every_class_of_the_coverage_table_is_reached(monkeypatch):
    got, taskgot = set(), set()
    for group, cases, settings in ws.runs():
        for case in cases:
            for setting, widths in settings:
                be, Q, blocks = _handle(case, monkeypatch, setting)
                k = ws.knobs(setting)
                fr = ws.fronts(be)
                levels, tasks = ws.sweep_levels(fr, k)
                # the restated classification against the analysis
                _, first, last, _ = be.sweep_tasks()
                assert sorted(tasks.items()) == sorted((int(l), int(f)) for f, l in zip(first, last)), (case["name"], setting)
                in_task = sum(r - f + 1 for r, f in tasks.items())
                nsmall = sum(len(q) for L in levels.values() for q in L.small)
                assert be.stats()["n_small_fronts"] == sum(ws.small_class(f[1], f[2], k["small_rows"]) < 4 for f in fr), (case["name"], setting)
                assert nsmall + in_task + sum(len(L.big) for L in levels.values()) == len(fr)
                for w in widths:
                    for t in ws.reached(fr, Q.shape[0], k, w):
                        got.add(ws.classes(t))
                        if t[0].startswith("task_"):
                            taskgot.add((t[0], ws.nr_class(t[4]), t[1], setting.get("GMRFX_TASK_MODE")))
                be.close()
    miss = ws.missing(got)
    assert not miss, f"{len(miss)} classes of the coverage table are not reached, the first: {miss[:8]}"
    assert set(ws.LEFT_TO_MESH_TESTS) <= {"k_bwd_gemm_longk<2,4>"}
    # sweep tasks: every local-vector class in both forms at every width class, every chunk width edge
    for mode in (None, "wg", "wave"):
        have = {(v, nrc) for v, nrc, _, md in taskgot if md == mode}
        for rows in ws.TASK_ROWS:
            assert ws.task_variants(rows, mode) <= have, (mode, rows, sorted(ws.task_variants(rows, mode) - have))
    for form in ("task_chunk", "task_wave"):
        assert set(ws.TASK_COLS) <= {c for v, _, c, _ in taskgot if v.startswith(form)}


def test_wanted_variants_name_every_launch_of_the_issue():
    names = {w[0].split(":")[0].split("[")[0] for w in ws.WANT}
    for v in ("k_fwd_front", "k_fwd_assemble", "k_xmul<8>", "k_xmul_narrow<8>", "k_fwd_own_update", "k_fwd_update_wave<1>", "k_fwd_update_wave<4>",
              "k_fwd_update_rec", "k_fwd_update_longk<1>", "k_fwd_update_longk<2>", "k_bwd_front", "k_bwd_wave<1>", "k_bwd_wave<4>",
              "k_bwd_gemm_longk<1,8>", "k_bwd_gemm_longk<2,8>", "k_bwd_gemm_longk<2,4>", "k_copy_own", "k_permute", "k_permute_narrow",
              "k_fwd_small<48>", "k_fwd_small<64>", "k_fwd_small<96>", "k_fwd_small<128>"):
        assert v in names, v


def test_references_check_themselves_and_a_perturbed_entry_names_its_front(monkeypatch):
    """Both references on the 3-children case: their own residuals, the oracle's err against them (what the device bound
    is 16 x of), and the per-front report on a perturbed entry."""
    import test_gpu_sweep_shapes as g
    case = ws.children_cases()[7]
    assert case["parent"] == (40, 60, 3)
    be, Q, blocks = _handle(case, monkeypatch, ws.LEVEL)
    n = Q.shape[0]
    perm = be.ordering_permutation()
    B = ws.rhs(n, case["seed"])
    X, dX, res = ws.reference_solve(Q, B)
    Xb, dXb, resb = ws.reference_backward(Q, perm, B, B, X, dX)
    assert res.max() <= g.BOUND / 100 and resb.max() <= g.BOUND / 100
    # LAPACK alone (no correction) agrees to float64 accuracy, far above the references' own error
    Lc = np.linalg.cholesky(Q.toarray()[np.ix_(perm, perm)])
    import scipy.linalg as sl
    Yb = np.empty_like(B); Yb[perm] = sl.solve_triangular(Lc, B, lower=True, trans="T")
    assert 1e-18 < ws.errors(Yb, Xb, dXb).max() < 1e-14
    F = orc.OracleFactor(Q, perm)
    eo = max(ws.errors(F.solve(B), X, dX).max(), ws.errors(F.backward_solve(B), Xb, dXb).max())
    assert 0 < eo <= g.ORACLE_ERR_MAX
    # a perturbed entry: row 5 of the 3-children parent, column 11
    fr = ws.fronts(be)
    par = [f for f in fr if (f[1], f[2], f[4]) == (40, 60, 3)][0]
    G = F.solve(B)
    i = perm[be.symbolic().super_first[par[0]] + 5]
    G[i, 11] += 2 * g.BOUND * np.abs(X[:, 11]).max()
    err, where = ws.describe(ws.per_front(be, ws.errors(G, X, dX)))
    assert err > g.BOUND and where.startswith(f"front {par[0]} (c=40, m=60, level {par[3]}, 3 children): row 5 of the front, column 11"), where
    be.close()
