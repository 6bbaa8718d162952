"""gmrfx_predictor_marginals / gmrfx_predictive_scores / gmrfx_obs_pointwise_const without a device: the refusals of the C ABI on
symbolic_only handles, the per-observation constants against their restatement, and the conditions tests/test_gpu_predictive.py rests
on -- every case reaches the edge it is named for, the float64 control stays inside the bounds of tests/predictive_ref.py without the
factor 16, every named mutant leaves them (with the factor) on at least one case. Where the GPU tests feed the restatement the handle's
own Sigma and At, these feed it a dense inverse rounded to float64."""
import numpy as np
import pytest
import scipy.sparse as sp

import constraint_ref as cref
import fisher_ref as ref
import gmrfx
import predictive_ref as pref
from gmrfx._lib import ERR_NO_DEVICE, NoDeviceError, lib, ptr

LD = pref.LD
GRID = pref.grid()
N = GRID.shape[0]


def _handle(Q=GRID, uplo="U"):
    return gmrfx.MI355XBackend(Q, symbolic_only=True, uplo=uplo)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_marginals_in_the_order_of_the_header():
    be = _handle()
    x, out = np.zeros(N), np.full(N, 7.0)
    with pytest.raises(ValueError, match="no observation likelihood"):
        be.predictor_marginals(x)
    with pytest.raises(ValueError, match="no observation likelihood"):
        be.observations_pointwise_const()
    obs = ref.make_obs(1, N, np.random.default_rng(0), "subset")
    be.set_observations(1, obs.y, obs.idx, obs.aux)
    L, h = lib(), be._h
    k = len(obs.y)
    out = np.full(k, 7.0)
    for args, msg in (((None, 0, ptr(out), None, None), "x is null"), ((ptr(x), 0, None, None, None), "every output is null"),
                      ((ptr(x), 2, ptr(out), None, None), "unknown flag bits"), ((ptr(x), -1, ptr(out), None, None), "unknown flag bits"),
                      ((ptr(x), 1, ptr(out), None, None), "needs a constraint")):
        for fn in (L.gmrfx_predictor_marginals, L.gmrfx_predictor_marginals_dev):
            assert fn(h, *args) == 1 and msg in L.gmrfx_last_error(h).decode()
    # the arguments are fine: what is missing is the device
    with pytest.raises(NoDeviceError):
        be.predictor_marginals(x)
    with pytest.raises(NoDeviceError):
        be.predictor_marginals(x, want_var=False)
    assert (out == 7.0).all()
    be.set_constraints(sp.csr_matrix(np.ones((1, N))), np.zeros(1))
    with pytest.raises(NoDeviceError):
        be.predictor_marginals(x, constraint_correction=True)
    be.close()


def test_refusals_of_the_scores():
    be = _handle()
    obs = ref.make_obs(0, N, np.random.default_rng(0), "all")
    k = N
    mu, v = np.zeros(k), np.ones(k)
    z, w = gmrfx.MI355XBackend.gauss_hermite(5)
    L, h = lib(), be._h
    out = np.full(4, 7.0)
    assert L.gmrfx_predictive_scores(h, ptr(mu), ptr(v), 5, ptr(z), ptr(w), None, None, None, None, ptr(out)) == 1
    assert "no observation likelihood" in L.gmrfx_last_error(h).decode()
    be.set_observations(0, obs.y, None, None, obs.param)
    z65, w65 = np.zeros(65), np.ones(65)

    def call(fn, m=mu, vv=v, K=5, zz=z, ww=w, o=out):
        return fn(h, ptr(m), ptr(vv), K, ptr(zz), ptr(ww), None, None, None, None, ptr(o))
    for fn in (L.gmrfx_predictive_scores, L.gmrfx_predictive_scores_dev):
        for kw, msg in ((dict(m=None), "mu_eta / v_eta is null"), (dict(vv=None), "mu_eta / v_eta is null"), (dict(o=None), "out is null"),
                        (dict(K=0), "K must be 1 .. 64"), (dict(K=65, zz=z65, ww=w65), "K must be 1 .. 64"), (dict(zz=None), "are null"),
                        (dict(zz=np.array([0, np.inf, 1, 2, 3.0])), "not finite"), (dict(ww=np.array([1, np.nan, 1, 1, 1.0])), "not finite"),
                        (dict(ww=np.array([1, 0.0, 1, 1, 1])), "must be positive"), (dict(ww=np.array([1, -1.0, 1, 1, 1])), "must be positive")):
            assert call(fn, **kw) == 1 and msg in L.gmrfx_last_error(h).decode(), (kw, L.gmrfx_last_error(h))
        assert call(fn) == ERR_NO_DEVICE
    assert (out == 7.0).all()
    be.close()


def test_batched_handles_are_refused():
    bb = gmrfx.MI355XBatchBackend(GRID, 2, symbolic_only=True)
    L = lib()
    x, out = np.zeros(2 * N), np.zeros(2 * N)
    assert L.gmrfx_predictor_marginals(bb._h, ptr(x), 0, ptr(out), None, None) == 1
    assert "batched handles are not supported" in L.gmrfx_last_error(bb._h).decode()
    z, w = gmrfx.MI355XBackend.gauss_hermite(3)
    tot = np.full(4, 7.0)
    assert L.gmrfx_predictive_scores(bb._h, ptr(x), ptr(out), 3, ptr(z), ptr(w), None, None, None, None, ptr(tot)) == 1
    assert "batched handles are not supported" in L.gmrfx_last_error(bb._h).decode() and (tot == 7.0).all()
    bb.close()


def test_sharded_handles_are_refused():
    be = gmrfx.MI355XBackend(GRID, symbolic_only=True, shard_min_top=8)
    assert be.shard_info() is not None
    L = lib()
    x, out = np.zeros(N), np.full(N, 7.0)
    for fn in (L.gmrfx_predictor_marginals, L.gmrfx_predictor_marginals_dev):
        assert fn(be._h, ptr(x), 0, ptr(out), None, None) == 1
        assert "sharded handles are not supported" in L.gmrfx_last_error(be._h).decode()
    z, w = gmrfx.MI355XBackend.gauss_hermite(3)
    tot = np.full(4, 7.0)
    for fn in (L.gmrfx_predictive_scores, L.gmrfx_predictive_scores_dev):
        assert fn(be._h, ptr(x), ptr(out), 3, ptr(z), ptr(w), None, None, None, None, ptr(tot)) == 1
        assert "sharded handles are not supported" in L.gmrfx_last_error(be._h).decode()
    assert (out == 7.0).all() and (tot == 7.0).all()
    be.close()


def test_gauss_hermite_is_normalised_and_integrates_moments():
    for K in pref.SCORE_K:
        z, w = gmrfx.MI355XBackend.gauss_hermite(K)
        assert z.size == w.size == K and abs(w.sum() - 1) < 4e-16 and (w > 0).all()
        if K >= 3:
            assert abs((w * z ** 2).sum() - 1) < 1e-13 and abs((w * z ** 4).sum() - 3) < 1e-12


# ---- the constants ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", [False, True])
@pytest.mark.parametrize("family", range(6))
def test_pointwise_constants_and_their_sum(family, design):
    """each c_i within eps sum |its terms| of the 40-digit value (long-double terms, one rounding to double); their long-double sum
    within an ulp of loglik_const"""
    if design:
        c = pref.design_case(GRID, 33, family, True)
        be = _handle(c["Q"], c["uplo"])
        be.set_design_observations(family, c["obs"].y, c["A"], c["b"], c["obs"].aux, c["obs"].param)
    else:
        c = pref.node_case(GRID, 257, family)
        be = _handle()
        be.set_observations(family, c["obs"].y, c["obs"].idx, c["obs"].aux, c["obs"].param)
    got = be.observations_pointwise_const()
    want, size = pref.pointwise_const(c["obs"])
    err = np.abs(np.asarray(got, LD) - want)
    print(f"family {family}: max err / (eps sum |terms|) {float(np.max(err / (pref.EPS * size + LD(1e-300)))):.3f}")
    assert (err <= pref.EPS * size).all()
    total = np.asarray(got, LD).sum(dtype=LD)
    const = be.observations_info()["loglik_const"]
    assert abs(float(total) - const) <= np.spacing(abs(const)), (float(total), const)
    be.close()


# ---- the cases reach their edges ----------------------------------------------------------------------------------------------------------
def test_cases_reach_the_edges_they_are_named_for():
    for nobs in pref.NODE_NOBS:
        c = pref.node_case(GRID, nobs, 1)
        idx = c["obs"].idx
        assert len(idx) == nobs < N and len(set(idx)) == nobs and (nobs == 1 or (np.diff(idx) < 0).any())
    assert {1, 255, 256, 257} == set(pref.NODE_NOBS)           # one thread, a workgroup less one, exactly one, one more
    seen = set()
    for nobs in pref.DESIGN_NOBS:
        for off in (False, True):
            c = pref.design_case(GRID, nobs, 1, off)
            A = sp.csr_matrix(c["A"])
            counts = np.diff(A.indptr)
            seen |= set(counts)
            assert A.shape == (nobs, N) and (c["b"] is None) == (not off)
            if nobs > 1:
                assert (A.data == 0).any()                      # an explicit zero, stored
                assert np.bincount(A.indices, minlength=N).max() > 1       # a node in more than one row
    assert set(pref.ROW_COUNTS) <= seen
    assert [k * (k + 1) // 2 for k in pref.ROW_COUNTS] == [0, 1, 6, 136, 153, 561]
    assert {1, 15, 16, 17, 33} == set(pref.DESIGN_NOBS)        # one lane group, a workgroup less one, exactly one, one more, three
    for m in pref.CON_M:
        Cm = pref.constraint_rows(N, m)
        assert Cm.shape == (m, N) and (Cm.sum(axis=1) == N // m).all() and (Cm.sum(axis=0) <= 1).all()


# ---- control and mutants ------------------------------------------------------------------------------------------------------------------
def _marginal_setup(c, m=0):
    P, inv = pref.dense_posterior(c)
    cc = np.asarray(pref.pointwise_const(c["obs"])[0], np.float64)
    con = None
    if m > 0:
        Cm = c["C"]
        At = np.asarray(inv @ np.asarray(Cm, LD).T, np.float64)
        con = cref.prepare(sp.csr_matrix(Cm), np.zeros(m), At)
        assert con["kappa"] <= 1e3, con["kappa"]
    return P, cc, con


def _marginal_case(kind, family=1):
    """the cases the mutants are tried on: node form, design form with an offset, the constrained design form with rows equal to the
    constraint's, a stand-in Sigma with a negative entry (what only a clamp without a constraint would hide)"""
    if kind == "node":
        return pref.node_case(GRID, 257, family), 0
    if kind == "design":
        return pref.design_case(GRID, 33, family, True), 0
    m = 4
    Cm = pref.constraint_rows(N, m)
    c = pref.design_case(GRID, 17 + 3 * m, family, True, extra_rows=np.vstack([Cm, 2.0 * Cm, -0.5 * Cm]))
    c["C"] = Cm
    return c, m


@pytest.mark.parametrize("kind", ["node", "design", "constrained"])
@pytest.mark.parametrize("family", range(6))
def test_float64_control_of_the_marginals_stays_inside_the_bounds_without_the_factor(kind, family):
    c, m = _marginal_case(kind, family)
    P, cc, con = _marginal_setup(c, m)
    kw = dict(con=con, correct=m > 0)
    r = pref.marginals(c["Ad"], c["b"], c["x"], P, c["obs"], cc, node=c["node"], **kw)
    bd = pref.marginal_bounds(c["Ad"], c["b"], c["x"], P, c["obs"], cc, r, factor=1, **kw)
    r64 = pref.marginals(c["Ad"], c["b"], c["x"], P, c["obs"], cc, dtype=np.float64, node=c["node"], **kw)
    rat = {k: pref.ratio(r64[k], r[k], bd[k]) for k in bd}
    print(f"{kind} family {family}: control err / bound {rat}")
    assert max(rat.values()) <= 1.0, rat


def _marginal_mutant_exceeds(mutant):
    for kind in ("node", "design", "constrained", "negative"):
        c, m = _marginal_case("design" if kind == "negative" else kind)
        P, cc, con = _marginal_setup(c, m)
        if kind == "negative":
            P[np.diag_indices(N)] = -50.0
        for correct in ((False, True) if m > 0 else (False,)):
            kw = dict(con=con, correct=correct)
            r = pref.marginals(c["Ad"], c["b"], c["x"], P, c["obs"], cc, node=c["node"], **kw)
            bd = pref.marginal_bounds(c["Ad"], c["b"], c["x"], P, c["obs"], cc, r, **kw)
            rm = pref.marginals(c["Ad"], c["b"], c["x"], P, c["obs"], cc, node=c["node"], mutant=mutant, **kw)
            if max(pref.ratio(rm[k], r[k], bd[k], nonnegative=correct and k == "v_eta") for k in bd) > 1.0:
                return True
    return False


def _score_mutant_exceeds(mutant):
    for family in (1, 0):
        for K in (17, 2):
            obs, mu, v = pref.score_inputs(family, 33)
            mu[0] = 200.0 if family == 0 else mu[0]         # a log density far below the underflow of exp
            cc = np.asarray(pref.pointwise_const(obs)[0], np.float64)
            z, w = gmrfx.MI355XBackend.gauss_hermite(K)
            r = pref.scores(mu, v, z, w, obs, cc)
            bd = pref.score_bounds(z, w, obs, r)
            rm = pref.scores(mu, v, z, w, obs, cc, mutant=mutant)
            if max(pref.ratio(rm[k], r[k], bd[k]) for k in bd) > 1.0:
                return True
    return False


@pytest.mark.parametrize("mutant", pref.MUTANTS)
def test_every_mutant_leaves_the_bounds_on_some_case(mutant):
    marginal = mutant in ("no_factor_2", "no_clamp", "always_clamp", "no_offset", "At_for_B")
    if mutant == "no_const":
        assert _marginal_mutant_exceeds(mutant) and _score_mutant_exceeds(mutant)
    else:
        assert _marginal_mutant_exceeds(mutant) if marginal else _score_mutant_exceeds(mutant)


@pytest.mark.parametrize("K", pref.SCORE_K)
@pytest.mark.parametrize("family", range(6))
def test_float64_control_of_the_scores_stays_inside_the_bounds_without_the_factor(family, K):
    obs, mu, v = pref.score_inputs(family, 33)
    cc = np.asarray(pref.pointwise_const(obs)[0], np.float64)
    z, w = gmrfx.MI355XBackend.gauss_hermite(K)
    r = pref.scores(mu, v, z, w, obs, cc)
    bd = pref.score_bounds(z, w, obs, r, factor=1)
    r64 = pref.scores(mu, v, z, w, obs, cc, dtype=np.float64)
    rat = {k: pref.ratio(r64[k], r[k], bd[k]) for k in bd}
    print(f"family {family} K {K}: control err / bound {rat}")
    assert max(rat.values()) <= 1.0, rat
    assert np.isnan(r["lpd"][[3, 5]]).all() and np.isfinite(r["lpd"][1])
    # v = 0: every node sits on the mean
    one = float((np.asarray(w, LD)).sum())
    l1 = pref.marginals(np.eye(33), None, mu, np.zeros((33, 33)), obs, cc, node=True)["pll"][1]
    for k in ("lpd", "lcpo", "elp"):
        assert abs(r[k][1] - l1) <= abs(one - 1) * abs(l1) + 8 * pref.EPS * abs(l1) + 8 * pref.EPS
    assert r["vlp"][1] <= (abs(one - 1) * abs(l1) + 8 * pref.EPS * abs(l1)) ** 2 * 2


def test_normal_closed_forms_agree_with_the_restated_quadrature():
    obs, mu, v = pref.score_inputs(0, 33)
    v = np.where(v >= 0, np.minimum(v, obs.param ** 2), v)
    cc = np.asarray(pref.pointwise_const(obs)[0], np.float64)
    good = v >= 0
    for K in (16, 17, 64):
        z, w = gmrfx.MI355XBackend.gauss_hermite(K)
        r = pref.scores(mu, v, z, w, obs, cc)
        elp, vlp, lpd = pref.normal_closed(mu, v, obs.y, obs.param)
        assert np.abs(r["elp"] - elp)[good].max() < 1e-13 and np.abs(r["vlp"] - vlp)[good].max() < 1e-12
        if K == 64:
            assert np.abs(r["lpd"] - lpd)[good].max() < 1e-9
