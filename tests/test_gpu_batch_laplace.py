"""gmrfx_batch_gaussian_approximation on the device against the restatement of the reference's loop (tests/fisher_ref.py: newton_loop), member
by member, on the cases of tests/batch_laplace_cases.py.

Per member: the same iteration count, convergence flag, frozen-finish flag, alpha trace EXACTLY and the same three logical counters as
the float64 restatement of that member alone; decrement trace and mode against the long-double restatement under the rule of
tests/test_gpu_fisher_loop.py (64 x max(the float64 restatement's own error, eps x scale), printed beside the device's); the long-double
Newton decrement at every converged member's mode is below newton_dec_tol. Independence: a member's x, hess and decrement trace are,
bit for bit, those it has in a batch of B copies of itself, also beside a member whose factorisation fails. Freshness: after
refactorize_final the handle's read-outs have the bits of a fresh MI355XBatchBackend refactorised at Q_p - diag(H); without it every
converged member holds the factor of its own last iterate. totals[0] = the largest logical factorisation count (+ 1 with the flag)."""
import numpy as np
import pytest

import batch_laplace_cases as bc
import fisher_loop_cases as lc
import fisher_ref as ref
import gmrfx
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
CASES = bc.loop_cases()


def _batch(c, Qs=None, params=None, scale=1.0):
    Qs = c["Qs"] if Qs is None else Qs
    bb = gmrfx.MI355XBatchLaplace(Qs[0], len(Qs), device=0)
    bb.set_prior(scale * bc.values(Qs))
    o = c["obs"]
    bb.set_observations(o.family, o.y, o.idx, o.aux, c["params"] if params is None else params)
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


@pytest.mark.parametrize("name", ["mixed", "negbin3"])
def test_every_member_follows_its_own_plain_loop(runs, name):
    c = CASES[name]
    X, H, info = runs[name]
    assert info["posdef"] and (info["info"] == 0).all()
    for k in range(len(c["Qs"])):
        a, b = bc.restate(c, k, np.float64), bc.restate(c, k, ref.LD)
        assert info["iterations"][k] == a["iterations"] and info["converged"][k] == a["converged"] and info["frozen_finish"][k] == a["frozen"]
        assert np.array_equal(info["alpha_trace"][k], a["alpha_trace"]), (k, info["alpha_trace"][k], a["alpha_trace"])
        assert (info["factorizations"][k], info["solves"][k], info["merit_evaluations"][k]) == (
            a["factorizations"], a["solves"], a["merit_evaluations"]), k
        decb = np.asarray(b["dec_trace"], ref.LD)
        own_dec = float(np.abs(np.asarray(a["dec_trace"], ref.LD) - decb).max())
        own_x = float(np.abs(np.asarray(a["x"], ref.LD) - b["x"]).max())
        tol_dec = 64 * max(own_dec, ref.EPS * float(np.abs(decb).max()))
        tol_x = 64 * max(own_x, ref.EPS * float(np.abs(b["x"]).max()))
        err_dec = float(np.abs(info["dec_trace"][k] - decb).max())
        err_x = float(np.abs(X[:, k] - b["x"]).max())
        print(f"{name}[{k}]: restatement f64-vs-ld dec {own_dec:.2e} x {own_x:.2e}; device-vs-ld dec {err_dec:.2e} x {err_x:.2e}")
        assert err_dec <= tol_dec and err_x <= tol_x, k
        if a["converged"]:
            assert ref.decrement_at(lc.dense(c["Qs"][k]), None, bc.member_obs(c, k), X[:, k]) < 1e-5
    assert info["totals"]["factorizations"] == info["factorizations"].max()


@pytest.mark.parametrize("name", ["mixed", "one_fails"])
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
        a = bc.restate(c, k, np.float64)
        assert info["converged"][k] and info["iterations"][k] == a["iterations"] and np.array_equal(info["alpha_trace"][k], a["alpha_trace"])
    # the handle stays usable
    bb = _batch(c)
    try:
        bb.gaussian_approximation(x0=c["x0"])
        bb.set_prior(bc.values([c["Qs"][0]] * 3))
        X2, _, i2 = bb.gaussian_approximation(x0=c["x0"])
        assert i2["posdef"] and i2["converged"].all() and same_bits(X2[:, 0], X[:, 0])
    finally:
        bb.close()


def _readouts(b, NZpost, z):
    g = b.logpdf_grad(z, nzval=NZpost)
    return [b.logdet(), b.solve(z), b.selinv_diag()] + [np.asarray(t) for t in g]


@pytest.mark.parametrize("name", ["mixed", "one_fails"])
def test_refactorize_final_leaves_fresh_readouts(name):
    c = CASES[name]
    B, n = len(c["Qs"]), c["M"].shape[0]
    NZ = bc.values(c["Qs"])
    dpos = diag_positions(c["Qs"][0])
    z = np.asfortranarray(np.random.default_rng(2).standard_normal((n, B)))
    bb, fresh = _batch(c, scale=2.0), gmrfx.MI355XBatchBackend(c["Qs"][0], B, device=0)
    try:
        if name == "mixed":        # another value set first: nothing of it may survive
            bb.gaussian_approximation(x0=c["x0"], refactorize_final=True)
        bb.set_prior(NZ)
        cl = bb.clone()
        cl.set_prior(NZ)
        X, H, info = bb.gaussian_approximation(x0=c["x0"], refactorize_final=True, **c["kw"])
        ok = info["info"] == 0
        assert info["totals"]["factorizations"] == (info["factorizations"] - 1)[ok].max() + 1
        NZpost = NZ.copy(order="F")
        Hz = np.where(np.isnan(H), 0.0, H)
        NZpost[dpos, :] -= Hz
        finfo = fresh.refactorize_values(NZpost)
        assert np.array_equal(finfo != 0, ~ok) and np.array_equal(bb.info() != 0, ~ok)
        for a, b in zip(_readouts(bb, NZpost, z), _readouts(fresh, NZpost, z)):
            a, b = np.asarray(a), np.asarray(b)
            sel = (..., ok) if a.ndim >= 1 and a.shape[-1] == B else ...
            assert same_bits(np.ascontiguousarray(a[sel]), np.ascontiguousarray(b[sel]))
        t = bb.laplace_terms()
        assert same_bits(t["energy"], info["energy"]) and same_bits(t["loglik"], info["loglik"]) and same_bits(t["logdet"][ok], fresh.logdet()[ok])
        # a clone made before the call runs the same loop to the same bits
        Xc, Hc, ic = cl.gaussian_approximation(x0=c["x0"], refactorize_final=True, **c["kw"])
        assert same_bits(Xc, X) and same_bits(Hc[:, ok], H[:, ok]) and same_bits(cl.logdet()[ok], bb.logdet()[ok])
        cl.close()
    finally:
        bb.close()
        fresh.close()


def test_without_the_flag_every_member_holds_its_last_iterates_factor():
    c = CASES["mixed"]
    B, n = 5, 256
    NZ = bc.values(c["Qs"])
    dpos = diag_positions(c["Qs"][0])
    bb, fresh = _batch(c), gmrfx.MI355XBatchBackend(c["Qs"][0], B, device=0)
    try:
        X, H, info = bb.gaussian_approximation(x0=c["x0"], **c["kw"])
        NZlast = NZ.copy(order="F")
        for k in range(B):
            a = bc.restate(c, k, np.float64)
            # the iterate the member's last factorisation was formed at: x_{factorizations - 1}, from the restatement run that far
            r = ref.newton_loop(lc.dense(c["Qs"][k]), None, bc.member_obs(c, k), x0=c["x0"][:, k], max_iter=a["factorizations"] - 1,
                                predictive=False, mean_tol=0.0, dec_tol=0.0)
            xl = np.asarray(r["x"], float)
            NZlast[dpos, k] += np.exp(xl)            # Q_p - H, H = -exp(x) for Poisson
        fresh.refactorize_values(NZlast)
        la, lb = bb.logdet(), fresh.logdet()
        sa, sb = bb.selinv_diag(), fresh.selinv_diag()
        rel_sd = np.abs(sa - sb).max(0) / np.abs(sb).max(0)
        print("logdet rel", np.abs(la - lb) / np.abs(lb), "selinv_diag rel", rel_sd)
        # the factor test's bounds (tests/test_gpu_batch.py): log det 1e-12 relative, diag of the selected inverse 1e-8 in the max norm
        assert (np.abs(la - lb) <= 1e-12 * np.abs(lb)).all() and (rel_sd < 1e-8).all()
        # and it is NOT the factor of the mode for the members that ran more than one iterate past it
        NZpost = NZ.copy(order="F")
        NZpost[dpos, :] -= H
        fresh.refactorize_values(NZpost)
        assert (np.abs(bb.logdet() - fresh.logdet()) > 0).any()
    finally:
        bb.close()
        fresh.close()
