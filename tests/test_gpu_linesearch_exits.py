"""The line-search exits of the Newton loop on the device (csrc/device_fisher.cpp, csrc/device_batch_fisher.cpp) on the cases of
tests/linesearch_exit_cases.py: an exhausted search, the tiny-step exit and max_linesearch_iter = 0, on plain handles (node form, with
a constraint, design form, the sqrt recovery) and in batches where a member that exhausts sits beside members that accept.

Per loop (per member of a batch), as tests/test_gpu_fisher_loop.py: iterations, converged and frozen flags, the alpha trace EXACTLY and
the three logical counters of the float64 restatement; decrement trace and mode against the long-double restatement within 64 x
max(the float64 restatement's own error, eps x scale), printed beside the device's error. Batches: every member has the bits of a plain
handle of Q_k, param[k] under the same keywords, and of itself in a batch of B copies; the forest totals are the rounds the
restatements imply (linesearch_exit_cases.forest_totals); after refactorize_final the read-outs have the bits of a fresh handle
refactorised at Q_p - H."""
import numpy as np
import pytest
import scipy.sparse as sp

import batch_laplace_cases as bc
import fisher_ref as ref
import gmrfx
import linesearch_exit_cases as le
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
PLAIN, BATCH = le.plain_cases(), le.batch_cases()


def _kw(kw):
    """the restatement's keywords as the handle's"""
    names = {"max_iter": "max_iter", "max_ls": "max_linesearch_iter", "dec_tol": "newton_dec_tol"}
    out = {names[k]: v for k, v in kw.items() if k in names}
    if kw.get("retry_full") is False:
        out["step_recovery"] = "sqrt"
    assert set(kw) <= set(names) | {"retry_full"}
    return out


def _plain(Q, obs, param, A=None, design=None):
    """a plain handle of Q with the likelihood in node form, or through the design case's matrix; A: a constraint A x = 0"""
    be = gmrfx.MI355XBackend(Q, device=0, uplo=design["uplo"] if design else "U", factorize=False)
    try:
        if design:
            be.set_design_observations(obs.family, obs.y, design["A"], design["b"], obs.aux, param)
            be.set_prior(Q.data, be.observations_hess_map())
        else:
            be.set_prior(Q.data, diag_positions(Q))
            be.set_observations(obs.family, obs.y, obs.idx, obs.aux, param)
        if A is not None:
            be.set_constraints(sp.csr_matrix(A), np.zeros(A.shape[0]))
    except Exception:
        be.close()
        raise
    return be


def _batch(case, Qs=None, params=None):
    c = case["c"]
    Qs = c["Qs"] if Qs is None else Qs
    p = c["params"] if params is None else params
    o = c["obs"]
    design = {"node": None, "design": c.get("base"), "con": c.get("design")}[case["kind"]]
    bb = gmrfx.MI355XBatchLaplace(Qs[0], len(Qs), device=0, uplo=design["uplo"] if design else "U")
    try:
        if design:
            bb.set_design_observations(o.family, o.y, design["A"], design["b"], o.aux, p)
        else:
            bb.set_observations(o.family, o.y, o.idx, o.aux, p)
        if case["kind"] == "con":
            bb.set_constraints(c["A"], np.zeros(c["A"].shape[0]))
        bb.set_prior(bc.values(Qs))
    except Exception:
        bb.close()
        raise
    return bb, design


def _follows(tag, x, info, a, b):
    """the assertions of tests/test_gpu_fisher_loop.py: test_whole_loop on one loop's results (info: the plain handle's dict)"""
    assert info["iterations"] == a["iterations"] and info["converged"] == a["converged"] and info["frozen_finish"] == a["frozen"], tag
    assert np.array_equal(info["alpha_trace"], a["alpha_trace"]), (tag, info["alpha_trace"], a["alpha_trace"])
    assert (info["factorizations"], info["solves"], info["merit_evaluations"]) == (a["factorizations"], a["solves"], a["merit_evaluations"]), tag
    decb = np.asarray(b["dec_trace"], ref.LD)
    own_dec = float(np.abs(np.asarray(a["dec_trace"], ref.LD) - decb).max())
    own_x = float(np.abs(np.asarray(a["x"], ref.LD) - b["x"]).max())
    tol_dec = 64 * max(own_dec, ref.EPS * float(np.abs(decb).max()))
    tol_x = 64 * max(own_x, ref.EPS * float(np.abs(b["x"]).max()))
    err_dec = float(np.abs(info["dec_trace"] - decb).max())
    err_x = float(np.abs(x - b["x"]).max())
    print(f"{tag}: restatement f64-vs-ld dec {own_dec:.2e} x {own_x:.2e}; device-vs-ld dec {err_dec:.2e} x {err_x:.2e}")
    assert err_dec <= tol_dec and err_x <= tol_x, tag


def _member_info(info, k):
    return {"iterations": int(info["iterations"][k]), "converged": bool(info["converged"][k]), "frozen_finish": bool(info["frozen_finish"][k]),
            "alpha_trace": info["alpha_trace"][k], "dec_trace": info["dec_trace"][k], "factorizations": int(info["factorizations"][k]),
            "solves": int(info["solves"][k]), "merit_evaluations": int(info["merit_evaluations"][k]), "alpha": float(info["alpha"][k])}


@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_loop_takes_the_exit(name):
    c = PLAIN[name]
    (a, b), = le.restated(name)
    assert c["events"] <= set(a["events"])
    be = _plain(c["Q"], c["obs"], c["obs"].param, c["A"], c.get("base"))
    try:
        x, hess, info = be.gaussian_approximation(x0=c["x0"], **_kw(c["kw"]))
        _follows(name, x, info, a, b)
        assert info["alpha"] == a["alpha"]
        if c["A"] is not None:       # the projected step fed the exhausted candidate: the iterates never leave the null space (x0 = 0)
            assert np.abs(c["A"] @ x).max() <= 64 * info["solves"] * ref.EPS * np.abs(c["A"]).sum() * max(np.abs(x).max(), 1.0)
        x2, h2, i2 = be.gaussian_approximation(x0=c["x0"], **_kw(c["kw"]))
        assert same_bits(x, x2) and same_bits(hess, h2) and same_bits(info["dec_trace"], i2["dec_trace"])
    finally:
        be.close()


def test_tiny_step_exit_keeps_the_rejected_full_step():
    """one iterate of matern200_tiny: the mode is x0 - 1 step bit for bit (the candidate the merit rejected), not x0 - 0.1 step"""
    c = PLAIN["matern200_tiny"]
    be = _plain(c["Q"], c["obs"], 0.0)
    try:
        n = c["Q"].shape[0]
        kw = dict(_kw(c["kw"]), max_iter=1)
        x, _, info = be.gaussian_approximation(x0=np.zeros(n), **kw)
        full, _, _ = be.gaussian_approximation(x0=np.zeros(n), max_iter=1, adaptive_stepsize=False, predictive_convergence=False,
                                               mean_change_tol=0.0, newton_dec_tol=0.0)
        assert info["alpha"] == 0.1 and info["merit_evaluations"] == 1 and same_bits(x, full)
        # and an exhausted search (max_linesearch_iter = 1, the default tolerance) does move to x0 - 0.1 step
        xe, _, ie = be.gaussian_approximation(x0=np.zeros(n), max_iter=1, max_linesearch_iter=1)
        assert ie["alpha"] == 0.1 and ie["merit_evaluations"] == 1 and same_bits(xe, 0.0 - 0.1 * (0.0 - full))
    finally:
        be.close()


@pytest.fixture(scope="module")
def runs():
    """name -> (X, H, info) of the batch's loop, computed once and left unchanged"""
    out = {}
    for name, case in BATCH.items():
        bb, _ = _batch(case)
        try:
            out[name] = bb.gaussian_approximation(x0=case["c"]["x0"], **_kw(case["c"]["kw"]))
        finally:
            bb.close()
    return out


@pytest.mark.parametrize("name", list(BATCH))
def test_every_member_follows_its_restatement(runs, name):
    X, H, info = runs[name]
    assert info["posdef"] and (info["info"] == 0).all()
    pairs = le.restated(name)
    for k, (a, b) in enumerate(pairs):
        assert BATCH[name]["events"][k] <= set(a["events"])
        mi = _member_info(info, k)
        _follows(f"{name}[{k}]", X[:, k], mi, a, b)
        assert mi["alpha"] == a["alpha"], k
    t = info["totals"]
    assert (t["factorizations"], t["solves"], t["evaluations"]) == le.forest_totals([a for a, _ in pairs])
    if BATCH[name]["kind"] == "con":
        assert (info["cinfo"] == 0).all()


@pytest.mark.parametrize("name", list(BATCH))
def test_every_member_has_the_bits_of_its_plain_handle(runs, name):
    case = BATCH[name]
    c = case["c"]
    X, H, info = runs[name]
    design = {"node": None, "design": c.get("base"), "con": c.get("design")}[case["kind"]]
    A = c["A"].toarray() if case["kind"] == "con" else None
    for k in range(len(c["Qs"])):
        be = _plain(c["Qs"][k], c["obs"], float(c["params"][k]), A, design)
        try:
            x, h, pi = be.gaussian_approximation(x0=c["x0"][:, k], **_kw(c["kw"]))
        finally:
            be.close()
        mi = _member_info(info, k)
        if case["kind"] == "con":
            # the two routes prepare W_k by different arithmetic (tests/test_gpu_batch_con_laplace.py:
            # test_laplace_terms_against_the_plain_constrained_loop), so the numbers are not compared bit for bit: the plain loop is
            # held to the same restatement under the same rule, and decisions and counts agree exactly
            _follows(f"{name}[{k}] plain", x, pi, *le.restated(name)[k])
        else:
            assert same_bits(x, X[:, k]) and same_bits(h, H[:, k]) and same_bits(pi["dec_trace"], mi["dec_trace"]), k
        assert same_bits(pi["alpha_trace"], mi["alpha_trace"]) and pi["alpha"] == mi["alpha"], k
        assert all(pi[q] == mi[q] for q in ("iterations", "converged", "frozen_finish", "factorizations", "solves", "merit_evaluations")), k


@pytest.mark.parametrize("name", list(BATCH))
def test_a_member_does_not_depend_on_the_others(runs, name):
    """in the batch of copies everybody exhausts (or accepts) together; in the case's batch the exhausted members' candidate launch and
    the tiny-step test run beside members that are masked out: the same bits either way"""
    case = BATCH[name]
    c = case["c"]
    X, H, info = runs[name]
    B = len(c["Qs"])
    for k in range(B):
        bb, _ = _batch(case, [c["Qs"][k]] * B, np.full(B, c["params"][k]))
        try:
            Xc, Hc, ic = bb.gaussian_approximation(x0=np.repeat(c["x0"][:, k:k + 1], B, axis=1), **_kw(c["kw"]))
        finally:
            bb.close()
        for j in range(B):
            assert same_bits(Xc[:, j], X[:, k]) and same_bits(Hc[:, j], H[:, k]) and same_bits(ic["dec_trace"][j], info["dec_trace"][k]), (k, j)
            assert same_bits(ic["alpha_trace"][j], info["alpha_trace"][k]) and ic["merit_evaluations"][j] == info["merit_evaluations"][k], (k, j)


def test_refactorize_final_after_an_exhausted_search_leaves_fresh_readouts(runs):
    case = BATCH["mixed_ls1"]
    c = case["c"]
    B, n = len(c["Qs"]), c["Qs"][0].shape[0]
    NZ = bc.values(c["Qs"])
    dpos = diag_positions(c["Qs"][0])
    z = np.asfortranarray(np.random.default_rng(2).standard_normal((n, B)))
    bb, _ = _batch(case)
    fresh = gmrfx.MI355XBatchBackend(c["Qs"][0], B, device=0)
    try:
        X, H, info = bb.gaussian_approximation(x0=c["x0"], refactorize_final=True, **_kw(c["kw"]))
        X0, H0, i0 = runs["mixed_ls1"]
        assert same_bits(X, X0) and same_bits(H, H0)
        assert np.array_equal(info["factorizations"], i0["factorizations"] + 1)
        assert info["totals"]["factorizations"] == i0["totals"]["factorizations"] + 1
        NZpost = NZ.copy(order="F")
        NZpost[dpos, :] -= H
        assert (fresh.refactorize_values(NZpost) == 0).all()
        assert same_bits(bb.logdet(), fresh.logdet()) and same_bits(bb.solve(z), fresh.solve(z)) and same_bits(bb.selinv_diag(), fresh.selinv_diag())
    finally:
        bb.close()
        fresh.close()
