"""The shape list of test_gpu_selinv_shapes.py, verified WITHOUT a device: every matrix of tests/selinv_shapes.py is built
on a symbolic-only handle and every block must come out as one front with exactly the (c, m) it was built for, one level
below its parent; the union of the lists must cover the code classes of the selected-inversion kernels. A change of the
amalgamation that silently alters the shapes fails here, not on other shapes on the GPU."""
import numpy as np
import pytest

import gmrfx
import orc
import selinv_shapes as ss


def _fronts(case, monkeypatch, small_rows=None):
    if small_rows is None:
        monkeypatch.delenv("GMRFX_SMALL_ROWS", raising=False)
    else:
        monkeypatch.setenv("GMRFX_SMALL_ROWS", str(small_rows))
    Q, blocks = ss.make(case)
    be = gmrfx.MI355XBackend(Q, symbolic_only=True, **ss.KW)
    got = ss.check_shapes(be, blocks)
    rows = 64 if small_rows is None else small_rows
    assert be.stats()["n_small_fronts"] == sum(ss.is_small(c, m, rows) for c, m, _, _ in got.values())
    be.close()
    return got


def test_grid_cases_have_their_fronts_alone_and_cover_every_class(monkeypatch):
    dense, small, alone = set(), set(), set()
    for case in ss.chain_cases() + ss.lone_cases() + ss.small_path_cases():
        for small_rows in (None, 0, 128):
            got = _fronts(case, monkeypatch, small_rows)
            rows = 64 if small_rows is None else small_rows
            for c, m, _, _ in got.values():
                (small if ss.is_small(c, m, rows) else dense).add((c, m))
        if case.get("alone"):
            lv = [g[2] for g in got.values()]
            assert len(set(lv)) == len(lv), case["name"]
            alone.update(g[:2] for g in got.values())
    # (a): every listed pair alone on its level at least once
    assert {(c, m) for c in ss.C_LIST for m in [0] + ss.M_LIST} <= alone
    # the 64 code classes of k_sel_dense, and m = 0 / 0 < m < 8 with every c mod 4 on both sides of 64 columns
    want = {ss.dense_class(c, m) for c in range(1, 300) for m in range(0, 140)}
    assert len(want) == 64
    assert {ss.dense_class(c, m) for c, m in dense} == want
    for wide in (False, True):
        for c4 in range(4):
            assert any(c % 4 == c4 and (c > 64) == wide and m == 0 for c, m in dense)
            assert any(c % 4 == c4 and (c > 64) == wide and 0 < m < 8 for c, m in dense)
    # the small path: every c in 1..64 at m = 0 and at c + m in {63, 64, 65, 127, 128}
    for c in range(1, 65):
        assert (c, 0) in small
        for r in (63, 64, 65, 127, 128):
            assert r - c < 1 or (c, r - c) in small, (c, r)


def test_mixed_gather_inverse_and_big_cases_have_their_fronts(monkeypatch):
    for case in ss.mixed_cases() + ss.gather_cases() + ss.inverse_cases() + ss.big_cases():
        got = _fronts(case, monkeypatch)
        kids = [g for name, g in got.items() if name != "root" and "." not in name]
        if case["name"] == "mixed_narrow":
            assert max(g[0] for g in kids) <= 64 and len({g[2] for g in kids}) == 1
            assert any(ss.is_small(g[0], g[1], 64) for g in kids) and any(not ss.is_small(g[0], g[1], 64) for g in kids)
        if case["name"] == "mixed_joined":
            assert max(g[0] for g in kids) == 65
        if case["name"] == "mixed_spread":
            assert min(g[1] for g in kids) == 1 and max(g[1] for g in kids) == 131
        if case["name"].startswith("gather"):
            nthr = int(case["name"][6:])
            trails = [g[1] for name, g in got.items() if name.count(".") == 1]
            assert sorted(set(trails)) == list(ss.GATHER_TRAILS[nthr])
        if case["name"].startswith("z21"):
            assert len(kids) == 2 and len({g[2] for g in kids}) == 1 and min(min(g[:2]) for g in kids) >= 1024


def test_reference_inverse_both_ways_agree_and_measure_the_oracle():
    """The exact-residual Newton step used above n = 600 gives the extended-precision one's answer; the float64 oracle's
    err against it is what the device bound is 16 x of (test_gpu_selinv_shapes.ORACLE_ERR_MAX)."""
    Q, _ = ss.make(ss.mixed_cases()[0])
    assert Q.shape[0] <= 600
    X, dX, res = ss.reference_inverse(Q)
    Qd = Q.toarray()
    X0 = np.linalg.inv(Qd); X0 = 0.5 * (X0 + X0.T)
    R = ss._exact_residual(Qd, X0)
    # (the extended-precision products round at 1e-19 per term: that route's true residual is of order 1e-18)
    assert res <= 1e-25 and float(np.abs(ss._exact_residual(Qd, X, dX)).max()) <= 1e-17
    assert np.abs((X0 - X) + (X0 @ np.asarray(R, dtype=np.float64) - dX)).max() <= 1e-17 * np.abs(X).max()
    be = gmrfx.MI355XBackend(Q, symbolic_only=True, **ss.KW)
    e = ss.entry_errors(orc.OracleFactor(Q, be.ordering_permutation()).selinv(), X, dX)[2].max()
    assert 0 < e <= 1.33e-14
