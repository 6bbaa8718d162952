"""gmrfx_batch_gaussian_approximation in design form on the device against the restatement of the reference's loop with a design matrix
(tests/fisher_design_ref.py: newton_loop), member by member, on the cases of tests/batch_design_cases.py (selected on the CPU:
tests/test_batch_design_host.py).

Per member: iteration count, convergence flag, frozen-finish flag, the three logical counters and the alpha trace EXACTLY as the
float64 restatement of that member alone; the mode and H (cnt values in map order, against the restatement's A' D A at its mode) within
64 x max(the float64 restatement's own error against the long-double one, eps x scale) -- the rule of tests/test_gpu_batch_laplace.py,
both figures printed. Independence: a member's x, H and decrement trace are, bit for bit, those it has in a batch of copies of itself,
also beside a member whose factorisation fails. The failing member: info > 0, no exception, x = its last accepted iterate, H NaN, the
others complete. Factor state: with refactorize_final the read-outs have the bits of a fresh batched handle factorised once at
Q_p,k - A' D_k A from the returned H; without it every member holds the factor of its own last iterate. laplace_terms() against the
plain handle's design loop on Q_p,k. Degenerate shapes: the batch calls on a plain handle (a batch of one), a plan with cnt = 0."""
import numpy as np
import pytest

import batch_design_cases as dc
import batch_laplace_cases as bc
import fisher_design_ref as dref
import fisher_ref as ref
import gmrfx
from layout_buffers import same_bits

pytestmark = pytest.mark.gpu
CASES = dc.loop_cases()
LOOPS = list(dc.LOOP_SC)


def _batch(c, Qs=None, params=None, scale=1.0, cls=None):
    Qs = c["Qs"] if Qs is None else Qs
    b, o = c["base"], c["obs"]
    bb = gmrfx.MI355XBatchLaplace(Qs[0], len(Qs), device=0, uplo=b["uplo"])
    bb.set_design_observations(o.family, o.y, b["A"], b["b"], o.aux, c["params"] if params is None else params)
    bb.set_prior(scale * bc.values(Qs))
    return bb


@pytest.fixture(scope="module")
def runs():
    """name -> (X, H, info) of the case's loop, computed once"""
    out = {}
    for name, c in CASES.items():
        bb = _batch(c)
        try:
            out[name] = bb.gaussian_approximation(x0=c["x0"], **c["kw"])
        finally:
            bb.close()
    return out


@pytest.fixture(scope="module")
def maps():
    """name -> (map, (j, k) of every position) of the case's plan, restated in Python"""
    out = {}
    for name, c in CASES.items():
        b = c["base"]
        tm = dref.hess_map(b["Q"], b["uplo"], b["A"])
        first = tm[1][:-1]
        out[name] = (tm[0], tm[5][first], tm[6][first])
    return out


@pytest.mark.parametrize("name", LOOPS)
def test_every_member_follows_its_own_plain_loop(runs, maps, name):
    c = CASES[name]
    X, H, info = runs[name]
    m, pj, pk = maps[name]
    assert info["posdef"] and (info["info"] == 0).all() and H.shape == (len(m), len(c["Qs"]))
    for k in range(len(c["Qs"])):
        a, b = dc.restate(c, k, np.float64), dc.restate(c, k, ref.LD)
        assert info["iterations"][k] == a["iterations"] and info["converged"][k] == a["converged"] and info["frozen_finish"][k] == a["frozen"]
        assert np.array_equal(info["alpha_trace"][k], a["alpha_trace"]), (k, info["alpha_trace"][k], a["alpha_trace"])
        assert (info["factorizations"][k], info["solves"][k], info["merit_evaluations"][k]) == (
            a["factorizations"], a["solves"], a["merit_evaluations"]), k
        Ha, Hb = np.asarray(a["hess_dense"], ref.LD)[pj, pk], np.asarray(b["hess_dense"], ref.LD)[pj, pk]
        own_x = float(np.abs(np.asarray(a["x"], ref.LD) - b["x"]).max())
        own_h = float(np.abs(Ha - Hb).max())
        tol_x = 64 * max(own_x, ref.EPS * float(np.abs(b["x"]).max()))
        tol_h = 64 * max(own_h, ref.EPS * float(np.abs(Hb).max()))
        err_x = float(np.abs(X[:, k] - b["x"]).max())
        err_h = float(np.abs(H[:, k] - Hb).max())
        print(f"{name}[{k}]: restatement f64-vs-ld x {own_x:.2e} H {own_h:.2e}; device-vs-ld x {err_x:.2e} H {err_h:.2e}")
        assert err_x <= tol_x and err_h <= tol_h, k
    assert info["totals"]["factorizations"] == info["factorizations"].max()


@pytest.mark.parametrize("name", ["mesh_far0", "one_fails"])
def test_a_member_does_not_depend_on_the_others(runs, name):
    c = CASES[name]
    X, H, info = runs[name]
    B = len(c["Qs"])
    for k in range(B):
        if info["info"][k] != 0:
            continue
        bb = _batch(c, [c["Qs"][k]] * B, np.full(B, c["params"][k]))
        try:
            Xc, Hc, ic = bb.gaussian_approximation(x0=np.repeat(c["x0"][:, k:k + 1], B, axis=1), **c["kw"])
        finally:
            bb.close()
        for j in range(B):
            assert same_bits(Xc[:, j], X[:, k]) and same_bits(Hc[:, j], H[:, k]) and same_bits(ic["dec_trace"][j], info["dec_trace"][k]), (k, j)


def test_one_failing_member_stops_alone(runs):
    c = CASES["one_fails"]
    X, H, info = runs["one_fails"]
    assert not info["posdef"]
    assert info["info"][1] > 0 and info["info"][0] == 0 and info["info"][2] == 0
    assert np.array_equal(X[:, 1], c["x0"][:, 1]) and info["iterations"][1] == 0 and not info["converged"][1] and np.isnan(H[:, 1]).all()
    for k in (0, 2):
        a = dc.restate(c, k, np.float64)
        assert info["converged"][k] and info["iterations"][k] == a["iterations"] and np.array_equal(info["alpha_trace"][k], a["alpha_trace"])
        assert np.isfinite(H[:, k]).all() and np.isfinite(X[:, k]).all()
    # the handle stays usable
    bb = _batch(c)
    try:
        bb.gaussian_approximation(x0=c["x0"])
        bb.set_prior(bc.values([c["Qs"][0]] * 3))
        X2, _, i2 = bb.gaussian_approximation(x0=c["x0"])
        assert i2["posdef"] and i2["converged"].all() and same_bits(X2[:, 0], X[:, 0])
    finally:
        bb.close()


@pytest.mark.parametrize("name", ["mesh_far0", "one_fails"])
def test_refactorize_final_leaves_the_factor_of_the_mode(name):
    c = CASES[name]
    b = c["base"]
    B = len(c["Qs"])
    NZ = bc.values(c["Qs"])
    bb, fresh = _batch(c, scale=2.0), gmrfx.MI355XBatchBackend(c["Qs"][0], B, device=0, uplo=b["uplo"])
    try:
        if name == "mesh_far0":        # another value set first: nothing of it may survive
            bb.gaussian_approximation(x0=c["x0"], refactorize_final=True)
        bb.set_prior(NZ)
        m = bb.observations_hess_map()
        X, H, info = bb.gaussian_approximation(x0=c["x0"], refactorize_final=True, **c["kw"])
        ok = info["info"] == 0
        assert info["totals"]["factorizations"] == (info["factorizations"] - 1)[ok].max() + 1
        NZpost = NZ.copy(order="F")
        NZpost[m, :] -= np.where(np.isnan(H), 0.0, H)          # Q_p,k - A' D_k A on the plan's positions
        finfo = fresh.refactorize_values(NZpost)
        assert np.array_equal(finfo != 0, ~ok) and np.array_equal(bb.info() != 0, ~ok)
        assert same_bits(bb.logdet()[ok], fresh.logdet()[ok])
        assert same_bits(np.ascontiguousarray(bb.selinv_diag()[:, ok]), np.ascontiguousarray(fresh.selinv_diag()[:, ok]))
        t = bb.laplace_terms()
        assert same_bits(t["energy"], info["energy"]) and same_bits(t["loglik"], info["loglik"]) and same_bits(t["logdet"][ok], fresh.logdet()[ok])
    finally:
        bb.close()
        fresh.close()


def test_without_the_flag_every_member_holds_its_last_iterates_factor():
    c = CASES["mesh_far0"]
    b = c["base"]
    B, n = len(c["Qs"]), b["Q"].shape[0]
    NZ = bc.values(c["Qs"])
    bb, fresh = _batch(c), gmrfx.MI355XBatchBackend(c["Qs"][0], B, device=0, uplo=b["uplo"])
    try:
        m = bb.observations_hess_map()
        X, H, info = bb.gaussian_approximation(x0=c["x0"], **c["kw"])
        # the iterate every member's last factorisation was formed at: x_{factorizations - 1}, from the restatement run that far
        Xlast = np.empty((n, B), order="F")
        for k in range(B):
            a = dc.restate(c, k, np.float64)
            r = dc.restate(c, k, np.float64, max_iter=a["factorizations"] - 1, predictive=False, mean_tol=0.0, dec_tol=0.0)
            Xlast[:, k] = np.asarray(r["x"], float)
        Hlast = bb.fisher_eval(Xlast, want_score=False)[1]
        NZlast = NZ.copy(order="F")
        NZlast[m, :] -= Hlast
        la, sa = bb.logdet(), bb.selinv_diag()
        fresh.refactorize_values(NZlast)
        lb, sb = fresh.logdet(), fresh.selinv_diag()
        rel_sd = np.abs(sa - sb).max(0) / np.abs(sb).max(0)
        print("logdet rel", np.abs(la - lb) / np.abs(lb), "selinv_diag rel", rel_sd)
        # the factor test's bounds (tests/test_gpu_batch.py): log det 1e-12 relative, diag of the selected inverse 1e-8 in the max norm
        assert (np.abs(la - lb) <= 1e-12 * np.abs(lb)).all() and (rel_sd < 1e-8).all()
        # and it is NOT the factor of the mode for the members that ran more than one iterate past it
        NZpost = NZ.copy(order="F")
        NZpost[m, :] -= H
        fresh.refactorize_values(NZpost)
        assert (np.abs(la - fresh.logdet()) > 0).any()
    finally:
        bb.close()
        fresh.close()


def _plain(b, Q):
    be = gmrfx.MI355XBackend(Q, device=0, uplo=b["uplo"], factorize=False)
    o = b["obs"]
    be.set_design_observations(o.family, o.y, b["A"], b["b"], o.aux, o.param)
    be.set_prior(Q.data, be.observations_hess_map())
    return be


@pytest.mark.parametrize("name", ["intercept_far0"])
def test_laplace_terms_against_the_plain_design_loop(name):
    c = CASES[name]
    b = c["base"]
    bb = _batch(c)
    try:
        X, H, info = bb.gaussian_approximation(x0=c["x0"], refactorize_final=True, **c["kw"])
        t = bb.laplace_terms()
        for k, Q in enumerate(c["Qs"]):
            be = _plain(b, Q)
            try:
                x, h, pi = be.gaussian_approximation(x0=c["x0"][:, k], refactorize_final=True, **c["kw"])
                _, _, en, ll = be.fisher_eval(x, want_score=False, want_hess=False)
                ld = be.compute_logdet()
            finally:
                be.close()
            assert same_bits(x, X[:, k]) and same_bits(h, H[:, k]), k              # the lockstep invariant: the plain loop's own bits
            assert pi["iterations"] == info["iterations"][k] and same_bits(pi["dec_trace"], info["dec_trace"][k])
            assert en == t["energy"][k] and ll == t["loglik"][k], k
            # (the batch sums a member's log pivots in its own kernel: the bound of tests/test_gpu_batch.py, 1e-12 relative)
            assert abs(ld - t["logdet"][k]) <= 1e-12 * abs(ld), (k, ld, t["logdet"][k])
    finally:
        bb.close()


class _BatchOfOne(gmrfx.MI355XBatchLaplace):
    """the batch entry points of a plain handle (its own handle pointer, not owned)"""

    def __init__(self, plain):
        self.n, self.nbatch, self._nnz, self._h = plain.n, 1, plain._nnz, plain._h
        self._info = np.zeros(1, np.int64)

    def close(self):
        self._h = None


def test_the_batch_calls_on_a_plain_handle_are_a_batch_of_one():
    c = CASES["mesh_far8"]
    b = c["base"]
    Q, o = c["Qs"][0], c["obs"]
    plain = gmrfx.MI355XBackend(Q, device=0, uplo=b["uplo"], factorize=False)
    ref_be = _plain(b, Q)
    try:
        one = _BatchOfOne(plain)
        one.set_design_observations(o.family, o.y, b["A"], b["b"], o.aux, 0.0)
        one.set_prior(Q.data[:, None])
        assert np.array_equal(one.observations_hess_map(), ref_be.observations_hess_map())
        X, H, info = one.gaussian_approximation(x0=c["x0"][:, :1], refactorize_final=True)
        x, h, pi = ref_be.gaussian_approximation(x0=c["x0"][:, 0], refactorize_final=True)
        assert same_bits(X[:, 0], x) and same_bits(H[:, 0], h) and info["iterations"][0] == pi["iterations"]
        assert same_bits(info["dec_trace"][0], pi["dec_trace"]) and np.array_equal(info["alpha_trace"][0], pi["alpha_trace"])
        S, Hs, en, ll = one.fisher_eval(X)
        ps, ph, pe, pl = ref_be.fisher_eval(x)
        assert same_bits(S[:, 0], ps) and same_bits(Hs[:, 0], ph) and en[0] == pe and ll[0] == pl
    finally:
        ref_be.close()
        plain.close()


@pytest.mark.parametrize("B", [1, 3])
def test_a_plan_without_entries_runs_with_the_prior_as_posterior_precision(B):
    e = dc.empty_case()
    Q, n = e["Q"], e["Q"].shape[0]
    Qs = dc.eval_members(Q, B, seed=6)
    y = np.array([1.0, 0.0, 3.0, 2.0, 1.0])
    bb, fresh = gmrfx.MI355XBatchLaplace(Q, B, device=0), gmrfx.MI355XBatchBackend(Q, B, device=0)
    try:
        bb.set_design_observations(1, y, e["A"], e["b"], None, np.zeros(B))
        assert bb.observations_design_info() == {"nnz": 0, "cnt": 0, "terms": 0} and bb.observations_hess_map().size == 0
        bb.set_prior(bc.values(Qs))
        mean = np.asfortranarray(np.random.default_rng(1).standard_normal((n, B)))
        S, H, en, ll = bb.fisher_eval(mean, mean)
        assert H.shape == (0, B) and S.shape == (n, B) and np.isfinite(S).all() and np.isfinite(ll).all()
        # eta = b does not depend on x: loglik = sum y b - exp(b) - lgamma(y + 1) for every member, the score is Q_p (x - mu)
        from math import lgamma
        want = float(sum(yi * bi - np.exp(bi) - lgamma(yi + 1.0) for yi, bi in zip(y, e["b"])))
        assert np.abs(ll - want).max() <= 64 * ref.EPS * sum(abs(yi * bi) + np.exp(bi) + lgamma(yi + 1.0) for yi, bi in zip(y, e["b"]))
        assert np.abs(S).max() == 0.0
        X, Hm, info = bb.gaussian_approximation(mean=mean, refactorize_final=True)
        assert Hm.shape == (0, B) and info["converged"].all() and (info["iterations"] == 1).all() and same_bits(X, mean)
        fresh.refactorize_values(bc.values(Qs))
        assert same_bits(bb.logdet(), fresh.logdet()) and same_bits(bb.selinv_diag(), fresh.selinv_diag())
    finally:
        bb.close()
        fresh.close()
