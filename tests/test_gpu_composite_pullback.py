"""The pullback of gaussian_approximation under a composite likelihood on the device (gmrfx_ga_pullback_composite[_dev];
csrc/ga_pullback.hip: k_gap_point_comp, k_gap_param_comp, k_gap_final_comp) against tests/composite_pullback_ref.py.

Reference: the rule restated in np.longdouble per component, fed the handle's own lam, and the per-entry bounds derived in
tests/ga_pullback_ref.py (times the project's factor 16); param[c] is held to the single-family bound over c's rows. lam itself: the
normwise bound of the one-right-hand-side solve tests, |Q_post lam - xbar| / |xbar| < 1e-10; xbar, recovered as Q_post lam, is held to
its own bound plus that residual. The point is not the mode: the rule's arithmetic is the same at any x, and flag bit 1 factorises
Q_prior - H(x) there (H is negative semi-definite for all six families).

 1. every output entry by entry on one, same_nodes, cuts, six, sixteen and long           6. projection on the joint model at its mode
 2. one component, each family: the bits of be.ga_pullback under set_design_observations   7. set_composite_param = a fresh handle
 3. one family in five components, cuts off the 16-row grid: arrays bit-equal, sums agree  8. logdet / selinv_diag after refactorize
 4. zeros for components without a parameter; absent cotangents                           9. logit components at eta = +-700
 5. host = _dev, repeats, the factor in hand                                              10. refusals on a live handle"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import composite_pullback_ref as pref
import composite_ref as cref
import constraint_ref as conref
import fisher_design_ref as dref
import fisher_ref as ref
import ga_pullback_ref as gref
import gmrfx
from gmrfx import composite as gc
from layout_buffers import same_bits

pytestmark = pytest.mark.gpu
LD = pref.LD
DEV = "cuda:0"
NAMES = ("one", "same_nodes", "cuts", "six", "sixteen", "long")


def _handle(c, factorize=False):
    o = c["obs"]
    comp = gmrfx.CompositeObservations(c["Q"].shape[0])
    A = sp.csr_matrix(c["A"])
    for k in range(o.ncomp):
        r0, r1 = int(o.rowptr[k]), int(o.rowptr[k + 1])
        comp.add(o.families[k], o.y[r0:r1], A=A[r0:r1], offset=None if c["b"] is None else c["b"][r0:r1],
                 aux=None if o.aux is None else o.aux[r0:r1], param=o.params[k])
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=factorize)
    gmrfx.set_composite_observations(be, comp)
    be.set_prior(c["Q"].data, be.observations_hess_map())
    return be


def _single(c, family, param, y, aux):
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=False)
    be.set_design_observations(family, y, c["A"], c["b"], aux, param)
    be.set_prior(c["Q"].data, be.observations_hess_map())
    return be


def _check(tag, c, S, Ad, krow, x, mu, mubar, Gd, got, projected=False):
    """got = (Qbar_prior, mubar_prior, lam, param, check) of the handle against the restatement fed the handle's lam; the ratios"""
    qp, mp, lam, par, chk = got
    assert np.isfinite(lam).all()
    r = pref.restate(S, mu, Ad, c["b"], c["obs"], x, mubar, Gd, lam=lam)
    bd = pref.bounds(S, Ad, c["b"], c["obs"], x, mubar, Gd, r, lam, krow=krow)
    xb = r["xbar"]
    nx = float(np.sqrt((xb * xb).sum()))
    rat = {}
    if not projected:           # (a projected lam solves another system)
        resid = r["Qpost"] @ np.asarray(lam, LD) - xb
        rel = float(np.sqrt((resid * resid).sum())) / nx
        assert rel < gref.SOLVE_RESIDUAL, rel
        rat["xbar"] = float(np.max(np.abs(resid) / (bd["xbar"] + gref.SOLVE_RESIDUAL * nx)))
    got_d = {"param": par, "check": chk}
    if qp is not None:
        got_d["Qbar_prior"] = qp
        r, bd = dict(r, Qbar_prior=gref.to_pattern(c["Q"], r["Qbar_prior"])), dict(bd, Qbar_prior=gref.to_pattern(c["Q"], bd["Qbar_prior"]))
    if mp is not None:
        got_d["mubar_prior"] = mp
    rat.update(pref.ratios(got_d, r, bd))
    print(f"{tag}: err/bound " + " ".join(f"{k} {v:.3f}" for k, v in rat.items()))
    assert all(np.isfinite(np.asarray(v)).all() for v in got_d.values())
    assert max(rat.values()) <= 1.0, rat
    for k, f in enumerate(c["obs"].families):
        assert f in pref.HAS_PARAM or (par[k] == 0.0 and not np.signbit(par[k]))
    return r


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_output_entry_by_entry(name):
    c = pref.cases()[name]
    S, Ad, krow, mubar, Gv, Gd = pref.dense(name)
    be = _handle(c)
    try:
        got = gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv, refactorize=True)
        assert got[3].shape == (c["obs"].ncomp,)
        _check(name, c, S, Ad, krow, c["x"], c["mu"], mubar, Gd, got)
    finally:
        be.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", range(6))
def test_one_component_has_the_bits_of_the_single_family_pullback(family):
    c = dict(pref.cases()["one"])
    S, Ad, krow, mubar, Gv, Gd = pref.dense("one")
    o = dref.make_obs(family, c["A"].shape[0], 10 * family + 1)
    c["obs"] = cref.CompObs([family], [o.param], [0, len(o.y)], o.y, o.aux)
    a, b = _handle(c), _single(c, family, o.param, o.y, o.aux)
    try:
        ga = gc.ga_pullback(a, c["x"], c["mu"], mubar, Gv, refactorize=True)
        gb = b.ga_pullback(c["x"], c["mu"], mubar, Gv, refactorize=True)
        assert all(same_bits(u, v) for u, v in zip(ga[:3], gb[:3]))
        assert same_bits(ga[3], [gb[3]]) and same_bits([ga[4]], [gb[4]])
        ga, gb = gc.ga_pullback(a, c["x"], c["mu"], None, Gv), b.ga_pullback(c["x"], c["mu"], None, Gv)
        assert all(same_bits(u, v) for u, v in zip(ga[:3], gb[:3])) and same_bits(ga[3], [gb[3]]) and same_bits([ga[4]], [gb[4]])
        ga, gb = gc.ga_pullback(a, c["x"], c["mu"], mubar, None), b.ga_pullback(c["x"], c["mu"], mubar, None)
        assert all(same_bits(u, v) for u, v in zip(ga[:3], gb[:3])) and same_bits(ga[3], [gb[3]]) and same_bits([ga[4]], [gb[4]])
    finally:
        a.close()
        b.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [0, 4, 5])
def test_one_family_in_five_components_off_the_grid(family):
    base = pref.cases()["one"]
    S, Ad, krow, mubar, Gv, Gd = pref.dense("one")
    nobs = base["A"].shape[0]
    o = dref.make_obs(family, nobs, 10 * family + 2)
    rowptr = [0, 1, 15, 18, 32, nobs]            # cuts at 1, 15, 18 and 32 (a cut ON the grid too), nobs = 33
    assert nobs == 33 and any(r % pref.ROWS for r in rowptr[1:-1])
    c = dict(base, obs=cref.CompObs([family] * 5, [o.param] * 5, rowptr, o.y, o.aux))
    a, b = _handle(c), _single(c, family, o.param, o.y, o.aux)
    try:
        ga = gc.ga_pullback(a, c["x"], c["mu"], mubar, Gv, refactorize=True)
        gb = b.ga_pullback(c["x"], c["mu"], mubar, Gv, refactorize=True)
        assert all(same_bits(u, v) for u, v in zip(ga[:3], gb[:3])) and same_bits([ga[4]], [gb[4]])
        # the split sum against the whole one: each within its own bound of the exact value (the handles' lam agree bit for bit)
        one = dict(base, obs=cref.CompObs([family], [o.param], [0, nobs], o.y, o.aux))
        r5 = pref.restate(S, c["mu"], Ad, c["b"], c["obs"], c["x"], mubar, Gd, lam=ga[2])
        b5 = pref.bounds(S, Ad, c["b"], c["obs"], c["x"], mubar, Gd, r5, ga[2], krow=krow)["param"]
        r1 = pref.restate(S, c["mu"], Ad, c["b"], one["obs"], c["x"], mubar, Gd, lam=ga[2])
        b1 = pref.bounds(S, Ad, c["b"], one["obs"], c["x"], mubar, Gd, r1, ga[2], krow=krow)["param"]
        assert (np.abs(ga[3] - r5["param"]) <= b5).all()
        err = abs(np.asarray(ga[3], LD).sum() - LD(gb[3]))
        print(f"family {family}: |sum(param_bar) - out[0]| {float(err):.3e} bound {float(b5.sum() + b1[0]):.3e}")
        assert err <= b5.sum() + b1[0]
    finally:
        a.close()
        b.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------------
def test_zeros_and_absent_cotangents():
    c = pref.cases()["six"]
    S, Ad, krow, mubar, Gv, Gd = pref.dense("six")
    be = _handle(c)
    try:
        full = gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv, refactorize=True)
        assert [p == 0.0 for p in full[3]] == [f not in pref.HAS_PARAM for f in c["obs"].families]
        _check("six no Qbar", c, S, Ad, krow, c["x"], c["mu"], mubar, None, gc.ga_pullback(be, c["x"], c["mu"], mubar, None))
        _check("six no mubar", c, S, Ad, krow, c["x"], c["mu"], None, Gd, gc.ga_pullback(be, c["x"], c["mu"], None, Gv))
        for want in ((True, False, False), (False, True, False), (False, False, True)):
            got = gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv, want_Qbar_prior=want[0], want_mubar_prior=want[1], want_lambda=want[2])
            for w, u, v in zip(want, got[:3], full[:3]):
                assert (u is None) if not w else same_bits(u, v)
            assert same_bits(got[3], full[3]) and got[4] == full[4]
    finally:
        be.close()
    # no parametrised component: Poisson, Bernoulli and Binomial rows of `six`
    o = c["obs"]
    rows = np.arange(int(o.rowptr[1]), int(o.rowptr[4]))
    A = sp.csr_matrix(c["A"])[rows]
    c3 = dict(c, A=A, b=None, obs=cref.CompObs([1, 2, 3], [0.0] * 3, [0, 7, 14, 21], o.y[rows], o.aux[rows]))
    be = _handle(c3)
    try:
        got = gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv, refactorize=True)
        assert got[3].tolist() == [0.0, 0.0, 0.0] and not np.signbit(got[3]).any() and np.isfinite(got[2]).all() and np.isfinite(got[4])
    finally:
        be.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize("name", ["cuts", "long"])
def test_host_and_dev_forms_agree_and_repeat_bit_for_bit(name):
    c = pref.cases()[name]
    _, _, _, mubar, Gv, _ = pref.dense(name)
    n, nnz = c["Q"].shape[0], c["Q"].nnz
    be = _handle(c)
    try:
        host = gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv, refactorize=True)
        again = gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv, refactorize=True)
        in_hand = gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv)
        for other in (again, in_hand):
            assert all(same_bits(u, v) for u, v in zip(host[:4], other[:4])) and host[4] == other[4]
        dx, dm, db, dq = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (c["x"], c["mu"], mubar, Gv))
        oq, om, ol = (torch.full((k,), float("nan"), dtype=torch.float64, device=DEV) for k in (nnz, n, n))
        torch.cuda.synchronize()
        par, chk = gc.ga_pullback_dev(be, _ptr(dx), _ptr(dm), _ptr(db), _ptr(dq), _ptr(oq), _ptr(om), _ptr(ol))
        torch.cuda.synchronize()
        assert same_bits(par, host[3]) and chk == host[4]
        assert all(same_bits(t.cpu().numpy(), v) for t, v in ((oq, host[0]), (om, host[1]), (ol, host[2])))
        par2, chk2 = gc.ga_pullback_dev(be, _ptr(dx), _ptr(dm), _ptr(db), _ptr(dq), _ptr(dq), 0, 0, refactorize=True)     # Qbar_prior over Qbar
        torch.cuda.synchronize()
        assert same_bits(par2, host[3]) and chk2 == host[4] and same_bits(dq.cpu().numpy(), host[0])
    finally:
        be.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------------
def test_projection_on_the_joint_model_at_its_mode():
    c = cref.loop_cases()["joint_sum0"]
    n = c["Q"].shape[0]
    rng = np.random.default_rng(6)
    mubar = rng.standard_normal(n)
    Gv, Gd = gref.random_cotangent(c["Q"], rng)
    S, Ad, krow = gref._sym(c["Q"], c["uplo"]), c["A"].toarray(), ref.symmetric_coo(c["Q"], c["uplo"])[3]
    Cm = sp.csr_matrix(c["C"])
    be = _handle(c)
    try:
        be.set_constraints(Cm, np.zeros(1))
        x, _, info = be.gaussian_approximation(refactorize_final=True)
        assert info["converged"]
        plain = gc.ga_pullback(be, x, None, mubar, Gv)
        proj = gc.ga_pullback(be, x, None, mubar, Gv, project=True)
        At, _ = be.constraint_fields()
        cc = conref.prepare(Cm, np.zeros(1), At)
        rr = conref.correct(cc, plain[2])
        assert (np.abs(np.asarray(proj[2], LD) - rr["Xc"][:, 0]) <= conref.bound_X(cc, rr)[:, 0]).all()
        assert conref.residual_ratio(Cm, np.zeros(1), proj[2]) <= 1.0
        mu0 = np.zeros(n)
        _check("joint_sum0 plain", c, S, Ad, krow, x, mu0, mubar, Gd, plain)
        _check("joint_sum0 projected", c, S, Ad, krow, x, mu0, mubar, Gd, proj, projected=True)
        assert proj[3][1] == 0.0 and proj[3][2] == 0.0 and proj[3][0] != 0.0
    finally:
        be.close()


# ---- 7, 8 ---------------------------------------------------------------------------------------------------------------------------------------
def test_set_param_then_the_pullback_has_the_bits_of_a_fresh_handle_and_so_has_the_factor():
    c = pref.cases()["six"]
    _, _, _, mubar, Gv, _ = pref.dense("six")
    p = [1.3, 0.0, 0.0, 0.0, 4.0, 0.5]
    fresh_case = dict(c, obs=cref.CompObs(c["obs"].families, p, c["obs"].rowptr, c["obs"].y, c["obs"].aux))
    a, b, f = _handle(c), _handle(fresh_case), _handle(fresh_case, True)
    try:
        before = gc.ga_pullback(a, c["x"], c["mu"], mubar, Gv, refactorize=True)        # (the tiling's tables exist before the parameters change)
        gmrfx.set_composite_param(a, p)
        ga = gc.ga_pullback(a, c["x"], c["mu"], mubar, Gv, refactorize=True)
        gb = gc.ga_pullback(b, c["x"], c["mu"], mubar, Gv, refactorize=True)
        assert all(same_bits(u, v) for u, v in zip(ga[:4], gb[:4])) and ga[4] == gb[4]
        assert not same_bits(ga[3], before[3])
        # the state refactorize=True leaves: Q_prior - H(x), as a fresh handle factorises it from the evaluation's Hessian values
        f.refactorize_update(f.fisher_eval(c["x"], c["mu"])[1])
        assert a.compute_logdet() == f.compute_logdet() and same_bits(a.get_selinv_diag(), f.get_selinv_diag())
    finally:
        for be in (a, b, f):
            be.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------------
def test_logit_components_at_eta_700():
    c = dict(pref.cases()["six"])
    S, Ad, krow, mubar, Gv, Gd = pref.dense("six")
    o = c["obs"]
    # the Bernoulli and Binomial components (2 and 3) observe their private nodes 4 c and 4 c + 1 through selection rows, the nodes at
    # +700 and -700: eta = +-700 on their rows, no other component reaches those nodes, the pattern already holds the diagonal
    A = sp.lil_matrix(c["A"])
    x = c["x"].copy()
    for k in (2, 3):
        for i in range(int(o.rowptr[k]), int(o.rowptr[k + 1])):
            A[i, :] = 0
            A[i, 4 * k + i % 2] = 1.0
        x[4 * k], x[4 * k + 1] = 700.0, -700.0
    A = sp.csr_matrix(A)
    c.update(A=A, b=None)
    eta = A @ x
    assert set(eta[int(o.rowptr[2]):int(o.rowptr[4])]) == {700.0, -700.0} and np.abs(np.delete(eta, np.arange(14, 28))).max() < 3
    Ad = A.toarray()
    be = _handle(c)
    try:
        got = gc.ga_pullback(be, x, c["mu"], mubar, Gv, refactorize=True)
        assert all(np.isfinite(v).all() for v in got[:4]) and np.isfinite(got[4])
        _check("six at eta +-700", c, S, Ad, krow, x, c["mu"], mubar, Gd, got)
    finally:
        be.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_live_handle_usable():
    c = pref.cases()["six"]
    _, _, _, mubar, Gv, _ = pref.dense("six")
    n = c["Q"].shape[0]
    be = _handle(c, True)
    try:
        before = be.fisher_eval(c["x"], c["mu"])
        with pytest.raises(ValueError, match="flag bit 0 .* needs a constraint"):
            gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv, project=True)
        with pytest.raises(ValueError, match="ga_pullback: composite likelihoods are not supported"):
            be.ga_pullback(c["x"], c["mu"], mubar, Gv)
        after = be.fisher_eval(c["x"], c["mu"])
        assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2:] == after[2:]
        # no composite set: a single-family design likelihood on the same handle
        o = dref.make_obs(1, c["A"].shape[0], 3)
        be.set_design_observations(1, o.y, c["A"], c["b"], o.aux, 0.0)
        be.set_prior(c["Q"].data, be.observations_hess_map())
        with pytest.raises(ValueError, match="no composite likelihood is set"):
            gc.ga_pullback(be, c["x"], c["mu"], mubar, Gv)
        assert np.isfinite(be.fisher_eval(c["x"], c["mu"])[2])
        assert np.isfinite(be.ga_pullback(c["x"], c["mu"], mubar, Gv, refactorize=True)[4])
    finally:
        be.close()
    Q = sp.csc_matrix(ref.banded(12, 2))
    Q.sort_indices()
    bb = gmrfx.MI355XBatchBackend(Q, 2, device=0)
    try:
        with pytest.raises(ValueError, match="batched handles are not supported"):
            gc.ga_pullback(bb, np.zeros(12), None, np.ones(12), None)
        assert (bb.refactorize_values(np.stack([Q.data, 2 * Q.data], axis=1)) == 0).all() and np.isfinite(bb.logdet()).all()
    finally:
        bb.close()
