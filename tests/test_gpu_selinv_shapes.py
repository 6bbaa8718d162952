"""Selected inversion ENTRY BY ENTRY on fronts of prescribed shape (run with -m gpu on an MI355X).

tests/selinv_shapes.py builds precisions whose fronts have exactly the (columns c, trailing rows m) the kernels of
csrc/selinv.hip and csrc/inverse.hip branch on (test_selinv_shapes_host.py checks the shapes and their coverage without a
device). Here every stored entry of get_selinv() -- amalgamation's extra entries included -- is compared with the dense
inverse of Q (LAPACK + one Newton step in extended precision, selinv_shapes.reference_inverse) in the measure

    err = |Z[i,j] - Sigma[i,j]| / sqrt(Sigma[i,i] Sigma[j,j])

per front, so that a failure names the front's (c, m), its level and the entry inside it; the CPU oracle is a second
witness on its own pattern. Plus: exact symmetry, diag(get_selinv()) == get_selinv_diag() and selinv_extract_at(Q) ==
the same entries of get_selinv() bit for bit, |selinv_dot(Q) - n| <= 1e-8 n.

BOUND = 16 x the largest err of the float64 CPU oracle against the same reference over the same case list (both run the
same recursion in float64, the sums of up to c + m terms in another order). Measured oracle err per case group:
    chains (a)        4.5e-15        lone fronts (a)     2.7e-15       small-path sets (a)   6.1e-15
    mixed levels (b)  2.6e-15        gather (c)          2.9e-15       doubling inverse (d)  9.5e-15 (c = 2049)
    k_sel_z21_big (e) 1.0e-14 off the grid, 1.33e-14 for the (1024, 4100) pair: the maximum, ORACLE_ERR_MAX
(LAPACK's own inverse: 0.7e-15 .. 1.3e-15.) On the device the oracle is a second witness up to ORACLE_NNZ_MAX entries of Q.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import orc
import selinv_shapes as ss

pytestmark = pytest.mark.gpu

ORACLE_ERR_MAX = 1.33e-14
BOUND = 16 * ORACLE_ERR_MAX
ORACLE_NNZ_MAX = 2_500_000          # the oracle is a second witness where it is affordable (dense n = 1500)

_ref_cache = {}


def _reference(case):
    """(Q, blocks, X, dX, oracle selinv or None): once per case, shared by the GMRFX_SMALL_ROWS settings."""
    if case["name"] not in _ref_cache:
        Q, blocks = ss.make(case)
        X, dX, res = ss.reference_inverse(Q)
        assert res <= 1e-20, f"reference residual {res:.2e}"      # its own err is then far more than 100 x below BOUND
        _ref_cache.clear()          # cases come grouped by name: keep one
        _ref_cache[case["name"]] = (Q, blocks, X, dX)
    return _ref_cache[case["name"]]


def _check_selinv(be, Q, X, dX, label):
    n = Q.shape[0]
    Z = be.get_selinv()
    pf = ss.per_front_errors(be, Z, X, dX)
    err, where = ss.worst(pf)
    print(f"{label}: n={n} fronts={len(pf)} gpu_err={err:.3e}")
    assert err <= BOUND, f"{label}: {where} (bound {BOUND:.2e})"
    assert abs(Z - Z.T).max() == 0.0
    d = be.get_selinv_diag()
    assert np.array_equal(Z.diagonal(), d)
    Se = be.selinv_extract_at(Q)
    assert np.array_equal(Se.indptr, Q.indptr) and np.array_equal(Se.indices, Q.indices)
    if np.array_equal(Z.indptr, Q.indptr) and np.array_equal(Z.indices, Q.indices):       # nothing stored beyond pattern(Q)
        assert np.array_equal(Se.data, Z.data)
    else:
        assert np.array_equal(np.asarray(Se[Q.nonzero()]).ravel(), np.asarray(Z[Q.nonzero()]).ravel())
    assert abs(be.selinv_dot(Q) - n) <= 1e-8 * n
    if Q.nnz <= ORACLE_NNZ_MAX:
        Zo = orc.OracleFactor(Q, be.ordering_permutation()).selinv()
        Zo_p = Zo.copy(); Zo_p.data[:] = 1.0
        diff = (Z.multiply(Zo_p) - Zo).tocoo()
        sd = np.sqrt(np.diag(X))
        eo = (np.abs(diff.data) / (sd[diff.row] * sd[diff.col])).max() if diff.nnz else 0.0
        assert eo <= BOUND + ORACLE_ERR_MAX, f"{label}: against the CPU oracle {eo:.3e}"
    return err


def _handle(case, monkeypatch, small_rows):
    if small_rows is None:
        monkeypatch.delenv("GMRFX_SMALL_ROWS", raising=False)
    else:
        monkeypatch.setenv("GMRFX_SMALL_ROWS", str(small_rows))
    Q, blocks, X, dX = _reference(case)
    be = gmrfx.MI355XBackend(Q, device=0, **ss.KW)
    assert be.last_info == 0
    got = ss.check_shapes(be, blocks)
    rows = 64 if small_rows is None else small_rows
    assert be.stats()["n_small_fronts"] == sum(ss.is_small(c, m, rows) for c, m, _, _ in got.values())
    if case.get("alone"):
        lv = [g[2] for g in got.values()]
        assert len(set(lv)) == len(lv), "every front of this case is alone on its level"
    return be, Q, X, dX, got


GRID = ss.chain_cases() + ss.lone_cases() + ss.small_path_cases()


@pytest.mark.parametrize("case", GRID, ids=[c["name"] for c in GRID])
def test_every_remainder_of_columns_and_trailing_rows(case, monkeypatch):
    """(a) c in C_LIST x m in {0} + M_LIST, each pair alone on its level (chains, lone fronts), and the small-path sets, with
    GMRFX_SMALL_ROWS unset (fronts of <= 64 rows fused), 0 (everything through k_sel_dense) and 128 (65..128 rows through
    k_sel_symm / k_sel_diag)."""
    for small_rows in (None, 0, 128):
        be, Q, X, dX, _ = _handle(case, monkeypatch, small_rows)
        _check_selinv(be, Q, X, dX, f"{case['name']}[SMALL_ROWS={small_rows}]")
        be.close()


MIXED = ss.mixed_cases() + ss.gather_cases()


@pytest.mark.parametrize("case", MIXED, ids=[c["name"] for c in MIXED])
def test_mixed_levels_and_gather_sources(case, monkeypatch):
    """(b) levels that mix narrow and wide, short and tall, small-path and dense-path fronts; (c) trailing blocks gathered
    from the parent's panel, its trailing block or both, at the three thread counts of launch_sel_gather."""
    for small_rows in (None, 0):
        be, Q, X, dX, got = _handle(case, monkeypatch, small_rows)
        if small_rows is None and case["name"] == "mixed_narrow":
            kids = [g for name, g in got.items() if name != "root"]
            assert max(g[0] for g in kids) <= 64 and be.stats()["n_small_fronts"] >= 2 and len({g[2] for g in kids}) == 1
        if case["name"] == "mixed_joined":
            assert sorted(g[0] for name, g in got.items() if name != "root")[-1] == 65
        if case["name"].startswith("gather"):
            nthr = int(case["name"][6:])
            trails = [g[1] for name, g in got.items() if name.count(".") == 1]
            assert len(trails) == 3 * len(ss.GATHER_TRAILS[nthr]) and nthr // 2 < max(trails) <= (nthr if nthr < 256 else 1 << 30)
        _check_selinv(be, Q, X, dX, f"{case['name']}[SMALL_ROWS={small_rows}]")
        be.close()


INV = ss.inverse_cases()


@pytest.mark.parametrize("case", INV, ids=[c["name"] for c in INV])
def test_doubling_inverse_between_and_beyond_its_powers_of_two(case, monkeypatch):
    """(d) c = 127 .. 2115 (past the 2048-column cap of the sweeps' inverses): the selected inverse entry by entry, and the
    solves that read the same inverse (k_xmul / k_xmul_narrow) against LAPACK at the parity suite's 1e-10."""
    import scipy.linalg as sl
    be, Q, X, dX, _ = _handle(case, monkeypatch, None)
    n = Q.shape[0]
    perm = be.ordering_permutation()
    Qd = Q.toarray()
    Lc = np.linalg.cholesky(Qd[np.ix_(perm, perm)])
    for nrhs in (1, 17, 64):
        B = np.random.default_rng(nrhs).standard_normal((n, nrhs))
        Xs = sl.cho_solve((Lc, True), B[perm])
        want = np.empty_like(Xs); want[perm] = Xs
        got = be.backend_solve(B[:, 0] if nrhs == 1 else B).reshape(n, -1)
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
        Yb = sl.solve_triangular(Lc, B, lower=True, trans="T")          # F.UP \ z = P' L^-T z
        wantb = np.empty_like(Yb); wantb[perm] = Yb
        gotb = be.backend_backward_solve(B[:, 0] if nrhs == 1 else B).reshape(n, -1)
        assert np.abs(gotb - wantb).max() <= 1e-10 * np.abs(wantb).max()
    _check_selinv(be, Q, X, dX, case["name"])
    be.close()


BIG = ss.big_cases()


@pytest.mark.parametrize("case", BIG, ids=[c["name"] for c in BIG])
def test_z21_on_staged_tiles_off_and_on_the_grid(case, monkeypatch):
    """(e) k_sel_z21_big: (1027, 1030) and (1025, 1101) under 1200 columns -- ragged tiles in both directions --, and the
    (1024, 4100) pair of test_two_huge_fronts_take_the_two_pass_contribution_product with ALL entries compared."""
    be, Q, X, dX, got = _handle(case, monkeypatch, None)
    kids = [g for name, g in got.items() if name != "root"]
    assert len(kids) == 2 and len({g[2] for g in kids}) == 1 and min(g[0] for g in kids) >= 1024 and min(g[1] for g in kids) >= 1024
    _check_selinv(be, Q, X, dX, case["name"])
    be.close()


def test_batched_handle_runs_the_same_kernels():
    """(f) three members of the mixed_joined pattern with different values in one batched handle: selinv_diag per member."""
    Q0, _ = ss.make(ss.mixed_cases()[1])
    members = [Q0, ss.with_values(Q0, 71), ss.with_values(Q0, 72)]
    bb = gmrfx.MI355XBatchBackend(Q0, 3, ordering="natural", device=0)
    assert not bb.refactorize_values(np.stack([q.data for q in members], axis=1)).any()
    D = bb.selinv_diag()
    for k, q in enumerate(members):
        X, dX, _ = ss.reference_inverse(q)
        e = np.abs((D[:, k] - np.diag(X)) - np.diag(dX)) / np.diag(X)
        print(f"batched member {k}: gpu_err={e.max():.3e}")
        assert e.max() <= BOUND, f"member {k}: row {int(e.argmax())}, err {e.max():.3e}"
    bb.close()
