"""What tests/test_gpu_refresh.py rests on, verified WITHOUT a device (tests/refresh_cases.py): the two problems have every structure
the handle's caches serve and are the smallest of their families that do (symbolic-only handles; pytest -rP prints the counts); the
value sets A and B are at least 1e-3 apart in the dense float64 counterpart of every read-out; prior - H reproduces B's bits; the
route and read-out tables name every method of the two backend classes or exclude it with a reason; and the protocol itself fails,
at its step 5, on a mock handle whose route forgets to bump the serial its caches are keyed on."""
import numpy as np
import pytest

import gmrfx
import refresh_cases as rc
from layout_buffers import same_bits


# ---- the problems ---------------------------------------------------------------------------------------------------------------------
def test_p_small_has_every_structure_and_is_the_smallest_square_grid():
    s = rc.structure(rc.grid(*rc.P_SMALL_SHAPE), {})
    print(f"P_small grid{rc.P_SMALL_SHAPE}: {s}")
    assert rc.small_ok(s) and not s["identity"]
    assert s["tasks"] >= 1 and s["chunks"] >= 1 and sum(s["small"]) >= 1 and s["big"] >= 1 and s["max_cols"] > 64
    k = rc.P_SMALL_SHAPE[0]
    assert rc.P_SMALL_SHAPE == (k, k)
    for j in range(2, k):
        t = rc.structure(rc.grid(j, j), {})
        assert not rc.small_ok(t), (j, t)
    t = rc.structure(rc.grid(k - 1, k - 1), {})
    print(f"one smaller, grid({k - 1}, {k - 1}): {t}")


def test_p_cap_has_a_front_wider_than_two_caps_and_is_the_smallest_slab():
    a, b, c = rc.P_CAP_SHAPE
    s = rc.structure(rc.grid3(a, b, c), rc.CAP_ENV)
    print(f"P_cap grid3{rc.P_CAP_SHAPE} under {rc.CAP_ENV}: {s}")
    assert rc.cap_ok(s) and not s["identity"] and s["tasks"] >= 1
    assert 128 < s["max_cols"] <= 256           # two doubling stages (64 -> 128 -> 256) are left to the selected inversion
    n0 = a * b * c
    # every a x a x c slab (c <= a) with fewer nodes: a front has at most a * a columns' worth of separator, so a >= 12 is needed
    # for 129 columns unless amalgamation merges separators; every slab below n0 is looked at
    seen = 0
    for aa in range(2, 36):
        for cc in range(1, aa + 1):
            if aa * aa * cc < n0 and aa * aa >= 100:
                t = rc.structure(rc.grid3(aa, aa, cc), rc.CAP_ENV)
                seen += 1
                assert not rc.cap_ok(t), ((aa, aa, cc), t)
    print(f"{seen} smaller slabs, none with a front wider than 128 columns")


def test_the_cap_knob_is_the_one_the_sweep_tests_use():
    import sweep_shapes as sw
    assert sw.CAP64 == rc.CAP_ENV and sw.knobs(rc.CAP_ENV)["inv_cap"] == 64 and "GMRFX_INV_CAP" in sw.KNOB_VARS


# ---- the value sets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P_small", "P_cap"])
def test_a_and_b_are_far_apart_in_every_readout(name):
    p = rc.problem(name)
    assert np.array_equal(p.A, p.Q.data) and p.B.shape == p.A.shape
    ratio = p.B[p.dpos] / p.A[p.dpos]
    assert (p.B[p.dpos] > 1.5 * p.A[p.dpos]).all() and len(np.unique(ratio)) >= 7          # positive, non-constant: no rescaling of A
    off = np.ones(p.nnz, bool)
    off[p.dpos] = False
    assert np.array_equal(p.B[off], 1.5 * p.A[off])
    da, db = rc.dense_readouts(p, p.A), rc.dense_readouts(p, p.B)
    for key in da:
        sep = np.abs(da[key] - db[key]).max() / np.abs(db[key]).max()
        print(f"{name} {key}: max |at A - at B| / max |at B| = {sep:.3g}")
        assert sep >= 1e-3, (key, sep)


@pytest.mark.parametrize("name", ["P_small", "P_cap"])
def test_prior_minus_h_is_b_bit_for_bit(name):
    p = rc.problem(name)
    assert same_bits(p.H, p.prior[p.dpos] - p.B[p.dpos])
    assert same_bits(rc.newton_values(p.prior, p.dpos, p.H), p.B)
    assert (p.H > 0).all()


def test_the_constraints_and_the_likelihoods_are_what_the_issue_names():
    p = rc.problem("P_small")
    assert p.con1[0].shape == (3, p.n) and p.con2[0].shape == (1, p.n) and np.linalg.matrix_rank(p.con1[0].toarray()) == 3
    assert p.Zr.shape == (p.n, 32) and p.R.shape == (p.n, 65)
    assert p.obs_design.shape[0] != len(p.obs_idx) and len(p.obs_idx) < p.n
    # pattern(A'A) of the design lies inside pattern(Q)
    AtA = (p.obs_design.T @ p.obs_design).tocoo()
    Qc = p.Q.tocsr()
    assert all(Qc[i, j] != 0 for i, j in zip(AtA.row, AtA.col))
    b = rc.BatchProblem()
    assert b.A.shape == (b.nnz, 3) and b.con[0].shape == (2, 72)


# ---- the tables name every method -------------------------------------------------------------------------------------------------------
def test_every_method_of_the_plain_backend_is_in_a_table_or_excluded():
    methods = set(rc.public_methods(gmrfx.MI355XBackend))
    cov = rc.covered(rc.ROUTES, rc.READOUTS, rc.OTHER_TESTS.values())
    assert not (cov - methods), f"tables name methods the backend does not have: {sorted(cov - methods)}"
    assert not (set(rc.EXCLUDED) - methods), sorted(set(rc.EXCLUDED) - methods)
    assert not (cov & set(rc.EXCLUDED)), sorted(cov & set(rc.EXCLUDED))
    missing = methods - cov - set(rc.EXCLUDED)
    assert not missing, f"neither a route, a read-out nor excluded with a reason: {sorted(missing)}"
    assert all(isinstance(v, str) and v for v in rc.EXCLUDED.values())
    # every factorising entry point is a route
    factorising = {m for m in methods if m.startswith("refactorize")} - {"refactorize_phase_dev"}
    routes = set().union(*(set(v[1]) for v in rc.ROUTES.values()))
    assert factorising <= routes, sorted(factorising - routes)


def test_every_method_of_the_batch_backend_is_in_a_table_or_excluded():
    methods = set(rc.public_methods(gmrfx.MI355XBatchBackend))
    cov = rc.covered(rc.BATCH_ROUTES, rc.BATCH_READOUTS)
    assert not (cov - methods) and not (set(rc.BATCH_EXCLUDED) - methods) and not (cov & set(rc.BATCH_EXCLUDED))
    missing = methods - cov - set(rc.BATCH_EXCLUDED)
    assert not missing, f"neither a route, a read-out nor excluded with a reason: {sorted(missing)}"
    routes = set().union(*(set(v[1]) for v in rc.BATCH_ROUTES.values()))
    assert {m for m in methods if m.startswith("refactorize") or m.startswith("constrained_logpdf")} <= routes


def test_the_tables_hold_what_the_issue_lists():
    assert {f"solve{k}" for k in (1, 16, 17, 64, 65)} | {"bsolve1", "bsolve17", "rbmc_plain", "rbmc_block"} <= set(rc.READOUTS)
    assert set(rc.NEEDS_VALUES) <= set(rc.READOUTS) and set(rc.NEEDS_CONSTRAINT) <= set(rc.READOUTS)
    assert set(rc.table(con=False)) == set(rc.READOUTS) - set(rc.NEEDS_CONSTRAINT)
    assert set(rc.table(con=True)) == set(rc.READOUTS) - set(rc.NEEDS_NO_CONSTRAINT) and set(rc.NEEDS_NO_CONSTRAINT) <= set(rc.table(con=False))
    assert {f"refactorize_solve[{k}]" for k in (1, 17, 65)} | {f"refactorize_solve_dev[{k}]" for k in (1, 17, 65)} <= set(rc.ROUTES)
    assert list(rc.BATCH_READOUTS) == ["info", "logdet", "solve", "backward_solve", "selinv_diag", "constraint_info", "constrained_mean",
                                       "constrained_var", "sample", "rbmc_var", "logpdf_grad"]


# ---- the protocol catches the bug class it is written for ---------------------------------------------------------------------------------
class MockHandle:
    """A dense numpy 'handle' with the real one's habits: the factor is replaced by every route, the 'selected inverse' and 'Bt' are
    built lazily and keyed on a serial. route_broken replaces the factor and forgets the serial."""

    def __init__(self, n):
        self.n, self.serial, self.sel_for, self.bt_for = n, 0, -1, -1
        self.L = self.sel = self._bt = None

    def _factor(self, vals):
        self.L = np.linalg.cholesky(np.diag(vals) + 0.1)

    def refactorize_values(self, vals):
        self._factor(vals)
        self.serial += 1

    def route_broken(self, vals):
        self._factor(vals)          # (no serial bump)

    def solve(self, b):
        return np.linalg.solve(self.L.T, np.linalg.solve(self.L, b))

    def selinv(self):
        if self.sel_for != self.serial:
            Li = np.linalg.inv(self.L)
            self.sel, self.sel_for = Li.T @ Li, self.serial
        return self.sel

    def bt(self, a):
        if self.bt_for != self.serial:
            self._bt, self.bt_for = self.solve(a), self.serial
        return self._bt

    def close(self):
        pass


def _mock_run(h, order, nz):
    b = np.arange(1.0, h.n + 1)
    tab = {"solve": lambda: (h.solve(b),), "selinv": lambda: (h.selinv(),), "bt": lambda: (h.bt(b[::-1].copy()),)}
    names = list(tab) if order == "table" else list(tab)[::-1]
    return {k: tab[k]() for k in names}


@pytest.mark.parametrize("order", ["table", "reverse"])
def test_the_protocol_fails_on_a_route_that_forgets_the_serial(order):
    n = 12
    A, B = np.linspace(1.0, 2.0, n), np.linspace(2.0, 5.0, n)
    good = lambda h: (h.refactorize_values(B), rc.RouteResult(B, True))[1]           # noqa: E731
    broken = lambda h: (h.route_broken(B), rc.RouteResult(B, True))[1]               # noqa: E731
    rc.protocol(lambda: MockHandle(n), A, good, _mock_run, order)
    with pytest.raises(AssertionError) as ei:
        rc.protocol(lambda: MockHandle(n), A, broken, _mock_run, order)
    msg = str(ei.value)
    assert "not the fresh handle's bits" in msg and "selinv" in msg and "bt" in msg and "'solve'" not in msg     # step 5; the solve is fresh
    # a route that does nothing at all is caught by step 6
    with pytest.raises(AssertionError, match="not the fresh handle's bits|unchanged by the route"):
        rc.protocol(lambda: MockHandle(n), A, lambda h: rc.RouteResult(B, True), _mock_run, order)
    # and by step 6 alone when the oracle is (wrongly) told the old values
    with pytest.raises(AssertionError, match="unchanged by the route"):
        rc.protocol(lambda: MockHandle(n), A, lambda h: rc.RouteResult(A, True), _mock_run, order)
