"""The linear predictor's marginals and the predictive scores on the device (csrc/predictive.hip; gmrfx_predictor_marginals[_dev],
gmrfx_predictive_scores[_dev]).

Reference: tests/predictive_ref.py -- both restated in np.longdouble, fed the handle's own Sigma on pattern(Q) (gmrfx_selinv_extract),
its constants and, under a constraint, its At and W (B = At L_c^-T through tests/constraint_ref.py), and the per-entry bounds derived
there (times the project's factor 16). Cases: tests/predictive_ref.py (what each reaches: tests/test_predictive_host.py) on a 17 x 17
Matern grid, n = 289; the handle is factorised at the case's Q itself -- the arithmetic is the same for any factor it holds."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import constraint_ref as cref
import fisher_ref as ref
import gmrfx
import predictive_ref as pref
from layout_buffers import same_bits

pytestmark = pytest.mark.gpu
LD = pref.LD
GRID = pref.grid()
N = GRID.shape[0]
GH = gmrfx.MI355XBackend.gauss_hermite
_BE = {}


def _node_backend():
    if "node" not in _BE:
        _BE["node"] = gmrfx.MI355XBackend(GRID, device=0)
    return _BE["node"]


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    for be in _BE.values():
        be.close()
    _BE.clear()


def _sigma(be, Q):
    """the handle's Sigma on pattern(Q), dense"""
    Z = be.selinv_extract_at(Q).tocoo()
    S = np.zeros(Q.shape)
    S[Z.row, Z.col] = Z.data
    return S


def _set(be, c):
    o = c["obs"]
    if c["node"]:
        be.set_observations(o.family, o.y, o.idx, o.aux, o.param)
    else:
        be.set_design_observations(o.family, o.y, c["A"], c["b"], o.aux, o.param)


def _check(tag, be, c, got, con=None, correct=False):
    cc = be.observations_pointwise_const()
    S = _sigma(be, c["Q"])
    kw = dict(con=con, correct=correct)
    r = pref.marginals(c["Ad"], c["b"], c["x"], S, c["obs"], cc, node=c["node"], **kw)
    bd = pref.marginal_bounds(c["Ad"], c["b"], c["x"], S, c["obs"], cc, r, **kw)
    rat = {k: pref.ratio(g, r[k], bd[k], nonnegative=correct and k == "v_eta") for k, g in zip(("mu_eta", "v_eta", "pll"), got)}
    print(f"{tag}: err/bound {rat}")
    assert max(rat.values()) <= 1.0, rat
    return r


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("nobs", pref.NODE_NOBS)
def test_node_form_entry_by_entry_in_the_callers_order(nobs, family):
    be = _node_backend()
    c = pref.node_case(GRID, nobs, family)
    _set(be, c)
    got = be.predictor_marginals(c["x"])
    _check(f"node nobs {nobs} family {family}", be, c, got)
    idx = c["obs"].idx
    assert same_bits(got[0], c["x"][idx]) and same_bits(got[1], be.get_selinv_diag()[idx])
    for want in ((True, False, False), (False, True, False), (False, False, True)):      # each output on its own, bit for bit
        one = be.predictor_marginals(c["x"], want_mean=want[0], want_var=want[1], want_pll=want[2])
        assert all((a is None) if not w else same_bits(a, b) for w, a, b in zip(want, one, got))


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("nobs", pref.DESIGN_NOBS)
def test_design_form_entry_by_entry(nobs, offset, family):
    c = pref.design_case(GRID, nobs, family, offset)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"])
    try:
        _set(be, c)
        got = be.predictor_marginals(c["x"])
        _check(f"design nobs {nobs} offset {offset} family {family}", be, c, got)
        empty = np.flatnonzero(np.diff(sp.csr_matrix(c["A"]).indptr) == 0)
        assert all(got[1][i] == 0.0 and not np.signbit(got[1][i]) for i in empty)
        if family != 1:
            return
        # against the truth and against selinv_row_diag, to the tolerance of tests/test_gpu_parity.py for row_diag_ASigmaAt
        inv = pref.dense_posterior(c)[1]
        want = np.asarray(np.einsum("ij,jk,ik->i", np.asarray(c["Ad"], LD), inv, np.asarray(c["Ad"], LD)), float)
        tol = 1e-10 * max(np.abs(want).max(), 1e-300)
        assert np.abs(got[1] - want).max() <= tol
        assert np.abs(got[1] - be.row_diag_ASigmaAt(c["A"])).max() <= tol
    finally:
        be.close()


@pytest.mark.parametrize("family", range(6))
def test_a_selection_matrix_has_the_bits_of_the_node_form(family):
    be = _node_backend()
    c = pref.node_case(GRID, 257, family)
    _set(be, c)
    node = be.predictor_marginals(c["x"])
    o = c["obs"]
    A = sp.csr_matrix((np.ones(257), (np.arange(257), o.idx)), shape=(257, N))
    be.set_design_observations(o.family, o.y, A, None, o.aux, o.param)
    des = be.predictor_marginals(c["x"])
    assert all(same_bits(a, b) for a, b in zip(node, des))


@pytest.mark.parametrize("offset", [False, True])
def test_mu_eta_has_the_bits_of_the_eta_of_fisher_eval(offset):
    """The eta of k_design_eta cannot be read back bit for bit through gmrfx_fisher_eval: its score adds (Q_p x)_j to A' g and its
    loglik squares and sums. So mu_eta is compared, bit for bit, with a restatement of the lane-group order in exact rational
    arithmetic rounded once per operation: lane l adds entries l, l + 16, ... by fused multiply-adds, the 16 sums meet in the xor
    butterfly, then + b_i. That the evaluation sees the same eta is checked through its loglik (y = 0, sigma = 1: -0.5 sum eta^2)."""
    from fractions import Fraction

    def fma(a, b, c_):
        return float(Fraction(a) * Fraction(b) + Fraction(c_))
    c = pref.design_case(GRID, 33, 0, offset)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"])
    try:
        _set(be, c)
        got = be.predictor_marginals(c["x"], want_var=False, want_pll=False)[0]
        A = sp.csr_matrix(c["A"])
        want = np.empty(33)
        for i in range(33):
            cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
            lanes = [0.0] * 16
            for q in range(len(cols)):
                a, xx = float(vals[q]), float(c["x"][cols[q]])
                lanes[q % 16] = fma(a, xx, lanes[q % 16])
            for sh in (8, 4, 2, 1):
                lanes = [lanes[k] + lanes[k ^ sh] for k in range(16)]
            want[i] = lanes[0] + c["b"][i] if offset else lanes[0]
        assert same_bits(got, want)
        # and the evaluation sees the same eta: with y = 0, sigma = 1 the x-dependent loglik is -0.5 sum eta^2, to the reduction's bound
        be.set_design_observations(0, np.zeros(33), c["A"], c["b"], None, 1.0)
        be.set_prior(c["Q"].data, be.observations_hess_map())
        ll = be.fisher_eval(c["x"], want_score=False, want_hess=False)[3] - be.observations_info()["loglik_const"]
        ref_ll = -0.5 * (np.asarray(got, LD) ** 2).sum()
        assert abs(ll - ref_ll) <= 16 * 12 * pref.EPS * float((0.5 * np.asarray(got, LD) ** 2).sum())
    finally:
        be.close()


@pytest.mark.parametrize("m", pref.CON_M)
def test_constraint_correction_and_clamp(m):
    """design rows followed by the constraint's own rows (and multiples of them): there v - correction is 0 in exact arithmetic and
    of either sign by rounding; with bit 0 it comes back within its bound of 0, never negative, never -0.0"""
    Cm = pref.constraint_rows(N, m)
    extra = np.vstack([Cm, 2.0 * Cm[: min(m, 8)], -0.5 * Cm[: min(m, 8)]])
    c = pref.design_case(GRID, 17 + len(extra), 1, True, extra_rows=extra)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"])
    try:
        _set(be, c)
        raw = be.predictor_marginals(c["x"])
        be.set_constraints(sp.csr_matrix(Cm), np.zeros(m))
        At, _ = be.constraint_fields()
        con = cref.prepare(sp.csr_matrix(Cm), np.zeros(m), At)
        assert con["kappa"] <= 1e3
        again = be.predictor_marginals(c["x"])                 # without the bit: the raw value, no clamp
        assert all(same_bits(a, b) for a, b in zip(raw, again))
        got = be.predictor_marginals(c["x"], constraint_correction=True)
        _check(f"constraint m {m}", be, c, got, con=con, correct=True)
        assert same_bits(got[0], raw[0]) and same_bits(got[2], raw[2])
        tail = got[1][17:]
        assert (tail >= 0).all() and not np.signbit(tail).any() and (tail < 1e-12 * raw[1][17:]).all()
        print(f"m {m}: {int((tail == 0).sum())} of {len(tail)} rows clamped to +0.0")
        assert (tail == 0).any()            # the clamp itself: a difference that rounding left negative comes back as +0.0
        # against the truth: diag(A Sigma_c A') with Sigma_c = Sigma - Sigma C' (C Sigma C')^-1 C Sigma from a dense long-double
        # inverse, nothing of the handle's in it; the tolerance tests/test_gpu_parity.py applies to row_diag_ASigmaAt. The rows equal
        # to constraint rows have truth 0: they are held to the scale of their uncorrected values
        inv = pref.dense_posterior(c)[1]
        Cl = np.asarray(Cm, LD)
        SC = inv @ Cl.T
        Sc = inv - SC @ ref._solve(Cl @ SC, np.ascontiguousarray(SC.T))
        Al = np.asarray(c["Ad"], LD)
        want = np.asarray(np.einsum("ij,jk,ik->i", Al, Sc, Al), float)
        assert np.abs(want[17:]).max() <= 1e-14 * raw[1][17:].max()
        assert np.abs(got[1][:17] - want[:17]).max() <= 1e-10 * np.abs(want[:17]).max()
        assert np.abs(got[1][17:]).max() <= 1e-10 * raw[1][17:].max()
        # node form under the same constraint: against constrained_var bit for bit, against the restatement and against the truth
        cn = pref.node_case(c["Q"], 257, 1)
        cn["uplo"] = c["uplo"]
        _set(be, cn)
        gn = be.predictor_marginals(cn["x"], constraint_correction=True)
        _check(f"constraint m {m} node", be, cn, gn, con=con, correct=True)
        assert same_bits(gn[1], be.constrained_var()[cn["obs"].idx])
        wn = np.asarray(np.diag(Sc), float)[cn["obs"].idx]
        assert np.abs(gn[1] - wn).max() <= 1e-10 * np.abs(wn).max()
    finally:
        be.close()


# ---- the scores ---------------------------------------------------------------------------------------------------------------------------
def _score_check(tag, be, obs, mu, v, K):
    z, w = GH(K)
    cc = be.observations_pointwise_const()
    arrs, tot = be.predictive_scores(mu, v, z, w)
    r = pref.scores(mu, v, z, w, obs, cc)
    bd = pref.score_bounds(z, w, obs, r)
    rat = {k: pref.ratio(a, r[k], bd[k]) for k, a in zip(("lpd", "lcpo", "elp", "vlp"), arrs)}
    print(f"{tag}: err/bound {rat}")
    assert max(rat.values()) <= 1.0, rat
    return arrs, tot, r


def _totals_check(arrs, tot):
    for a, k in zip(arrs, ("lpd", "lcpo", "elp", "p_waic")):
        if np.isfinite(a).all():
            assert abs(LD(tot[k]) - np.asarray(a, LD).sum()) <= pref.total_bound(a)
        else:
            assert not np.isfinite(tot[k])


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("K", pref.SCORE_K)
@pytest.mark.parametrize("nobs", [15, 17, 257])
def test_scores_entry_by_entry(nobs, K, family):
    be = _node_backend()
    obs, mu, v = pref.score_inputs(family, nobs)
    obs.idx = np.random.default_rng(nobs).permutation(N)[:nobs]
    be.set_observations(obs.family, obs.y, obs.idx, obs.aux, obs.param)
    arrs, tot, r = _score_check(f"scores nobs {nobs} K {K} family {family}", be, obs, mu, v, K)
    assert all(np.isnan(a[[3, 5]]).all() for a in arrs)            # v = NaN, v < 0
    assert all(np.isnan(tot[k]) for k in ("lpd", "lcpo", "elp", "p_waic", "waic"))
    good = np.isfinite(v) & (v >= 0)
    mu2, v2 = mu[good], v[good]
    o2 = ref.Obs(obs.family, obs.idx[good], obs.y[good], None if obs.aux is None else obs.aux[good], obs.param)
    be.set_observations(o2.family, o2.y, o2.idx, o2.aux, o2.param)
    arrs, tot, r = _score_check("finite rows", be, o2, mu2, v2, K)
    _totals_check(arrs, tot)
    assert tot["waic"] == -2.0 * (tot["lpd"] - tot["p_waic"])
    z, w = GH(K)
    none, tot2 = be.predictive_scores(mu2, v2, z, w, want_arrays=False)           # totals with and without the arrays, and again
    assert none == (None,) * 4 and tot2 == tot and be.predictive_scores(mu2, v2, z, w)[1] == tot


def test_more_than_256_workgroup_partials_and_the_design_form():
    """nobs = 33 rows tiled to 4113 observations: 258 workgroups, the final kernel's strided loop"""
    c = pref.design_case(GRID, 33, 1, True)
    reps = 4113 // 33 + 1
    A = sp.vstack([c["A"]] * reps).tocsr()[:4113]
    o = c["obs"]
    obs = ref.Obs(1, None, np.tile(o.y, reps)[:4113], np.tile(o.aux, reps)[:4113], 0.0)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"])
    try:
        be.set_design_observations(1, obs.y, A, np.tile(c["b"], reps)[:4113], obs.aux)
        mu, v, _ = be.predictor_marginals(c["x"])
        arrs, tot, _ = _score_check("4113 observations", be, obs, mu, v, 16)
        _totals_check(arrs, tot)
        assert same_bits(arrs[0][:33], arrs[0][33:66])
    finally:
        be.close()


@pytest.mark.parametrize("family", [2, 3])
def test_logit_families_are_finite_at_mu_700(family):
    be = _node_backend()
    obs, mu, v = pref.score_inputs(family, 17)
    obs.idx = np.arange(17)
    mu[::2], mu[1::2] = 700.0, -700.0
    v = np.abs(np.nan_to_num(v, nan=0.3))
    be.set_observations(obs.family, obs.y, obs.idx, obs.aux, obs.param)
    arrs, tot, _ = _score_check(f"mu = +-700 family {family}", be, obs, mu, v, 17)
    assert all(np.isfinite(a).all() for a in arrs)


def test_poisson_at_zero_counts_and_at_an_overflowing_mean():
    be = _node_backend()
    nobs = 17
    obs = ref.Obs(1, np.arange(nobs), np.r_[np.zeros(9), np.full(8, 3.0)], None, 0.0)
    mu, v = np.full(nobs, 0.3), np.full(nobs, 0.2)
    mu[[2, 12]], v[[2, 12]] = 800.0, 0.0          # exp(800) overflows at every node
    mu[[4, 14]] = 708.5                           # ... at the upper nodes only
    be.set_observations(1, obs.y, obs.idx, None)
    z, w = GH(17)
    arrs, tot = be.predictive_scores(mu, v, z, w)
    lpd, lcpo, elp, vlp = arrs
    # the ordinary rows against the restatement (long double does not overflow where float64 does: the others are checked below)
    keep = np.setdiff1d(np.arange(nobs), [2, 12, 4, 14])
    r = pref.scores(mu, v, z, w, obs, be.observations_pointwise_const())
    bd = pref.score_bounds(z, w, obs, r)
    assert max(pref.ratio(a[keep], r[k][keep], bd[k][keep]) for k, a in zip(("lpd", "lcpo", "elp", "vlp"), arrs)) <= 1.0
    assert (lpd[[2, 12]] == -np.inf).all() and (lcpo[[2, 12]] == -np.inf).all() and (elp[[2, 12]] == -np.inf).all()
    assert not np.isnan(lpd).any() and not np.isnan(lcpo).any()
    assert np.isfinite(lpd[[4, 14]]).all() and (lcpo[[4, 14]] == -np.inf).all()
    assert np.isfinite(np.delete(lpd, [2, 12])).all() and tot["lpd"] == -np.inf


def test_zero_variance_puts_every_node_on_the_mean():
    be = _node_backend()
    obs, mu, _ = pref.score_inputs(4, 33)
    obs.idx = np.arange(33)
    be.set_observations(obs.family, obs.y, obs.idx, obs.aux, obs.param)
    pll = be.predictor_marginals(np.r_[mu, np.zeros(N - 33)], want_mean=False, want_var=False)[2]
    for K in pref.SCORE_K:
        z, w = GH(K)
        (lpd, lcpo, elp, vlp), _ = be.predictive_scores(mu, np.zeros(33), z, w)
        slack = (abs(float(np.asarray(w, LD).sum()) - 1) + 16 * (K // 16 + 8) * pref.EPS) * np.abs(pll) + 16 * 8 * pref.EPS
        assert (np.abs(lpd - pll) <= slack).all() and (np.abs(lcpo - pll) <= slack).all() and (np.abs(elp - pll) <= slack).all()
        assert (vlp >= 0).all() and (vlp <= 2 * slack ** 2).all()


@pytest.mark.parametrize("K", [16, 17, 64])
def test_normal_family_against_the_closed_forms(K):
    be = _node_backend()
    obs, mu, v = pref.score_inputs(0, 257)
    v = np.minimum(np.abs(np.nan_to_num(v, nan=0.3)), obs.param ** 2)
    obs.idx = np.arange(257)
    be.set_observations(0, obs.y, obs.idx, None, obs.param)
    arrs, tot, r = _score_check(f"normal K {K}", be, obs, mu, v, K)
    z, w = GH(K)
    bd = pref.score_bounds(z, w, obs, r)
    elp, vlp, lpd = pref.normal_closed(mu, v, obs.y, obs.param)
    # the rule is exact to degree 2 K - 1 >= 4: what remains is the restated rule's own rounding (its weights are float64) plus the bound
    # -- and that is at the rounding level: nodes and weights each carry an ulp or so of their exact values, the sums are in long double
    for got, want, k in ((arrs[2], elp, "elp"), (arrs[3], vlp, "vlp")):
        assert (np.abs(r[k] - want) <= pref.FACTOR * pref.EPS * (1 + np.abs(want))).all()
        assert (np.abs(np.asarray(got, LD) - want) <= np.abs(r[k] - want) + bd[k]).all()
    if K == 64:     # lpd: the quadrature's own truncation error, from the long-double restatement, plus the rounding bound
        assert (np.abs(np.asarray(arrs[0], LD) - lpd) <= np.abs(r["lpd"] - lpd) + bd["lpd"]).all()
        assert float(np.abs(r["lpd"] - lpd).max()) < 1e-9


# ---- forms and states ---------------------------------------------------------------------------------------------------------------------
def _dev(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize("design", [False, True])
def test_host_device_and_misaligned_forms_agree_bit_for_bit(design):
    c = pref.design_case(GRID, 33, 4, True) if design else pref.node_case(GRID, 257, 4)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"])
    try:
        _set(be, c)
        nobs = len(c["obs"].y)
        host = be.predictor_marginals(c["x"])
        z, w = GH(17)
        harr, htot = be.predictive_scores(host[0], host[1], z, w)
        dev = torch.device("cuda:0")
        for off in (0, 1, 3):           # doubles: offsets 1 and 3 are 8-byte aligned only
            lens = (N,) + (nobs,) * 7
            bufs = [torch.full((k + 8,), float("nan"), dtype=torch.float64, device=dev) for k in lens]
            dx, dm, dv, dp, o0, o1, o2, o3 = (b[off:off + k] for b, k in zip(bufs, lens))
            dx.copy_(torch.from_numpy(c["x"]))
            torch.cuda.synchronize()
            be.predictor_marginals_dev(_dev(dx), _dev(dm), _dev(dv), _dev(dp))
            tot = be.predictive_scores_dev(_dev(dm), _dev(dv), z, w, _dev(o0), _dev(o1), _dev(o2), _dev(o3))
            torch.cuda.synchronize()
            assert tot == htot and tot == be.predictive_scores_dev(_dev(dm), _dev(dv), z, w)
            for t, a in zip((dm, dv, dp, o0, o1, o2, o3), host + harr):
                assert same_bits(t.cpu().numpy(), a)
            for b, k in zip(bufs[1:], lens[1:]):        # nothing is written outside the window
                assert bool(torch.isnan(torch.cat([b[:off], b[off + k:]])).all())
    finally:
        be.close()


def test_states_factorisation_selected_inverse_and_a_new_likelihood():
    c = pref.node_case(GRID, 256, 1)
    be = gmrfx.MI355XBackend(GRID, device=0, factorize=False)
    try:
        _set(be, c)
        mu, v, pll = be.predictor_marginals(c["x"], want_var=False)            # neither a factorisation nor a selected inverse
        assert v is None and same_bits(mu, c["x"][c["obs"].idx])
        with pytest.raises(gmrfx._lib.GmrfxError, match="refactorize"):
            be.predictor_marginals(c["x"])
        be.refactorize_values(GRID.data)
        v1 = be.predictor_marginals(c["x"])[1]
        be.refactorize_values(2.0 * GRID.data)                                  # a new factorisation: the selected inverse is computed again
        v2 = be.predictor_marginals(c["x"])[1]
        assert same_bits(v2, be.get_selinv_diag()[c["obs"].idx]) and np.abs(2 * v2 / v1 - 1).max() < 1e-12
        c2 = pref.node_case(GRID, 255, 3)                                       # obs_set drops the tables
        _set(be, c2)
        _check("after a new likelihood", be, dict(c2, Q=GRID), be.predictor_marginals(c2["x"]))
    finally:
        be.close()


def test_a_rank_deficient_constraint_is_refused_with_the_outputs_untouched():
    """two equal constraint rows: W = A Q^-1 A' has a pivot within rounding of zero, which con_prepare reports (no fault)"""
    c = pref.design_case(GRID, 17, 1, True)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"])
    try:
        _set(be, c)
        row = pref.constraint_rows(N, 1)
        be.set_constraints(sp.csr_matrix(np.vstack([row, row])), np.zeros(2))
        dev = torch.device("cuda:0")
        dx = torch.from_numpy(c["x"]).to(dev)
        outs = [torch.full((17,), 7.0, dtype=torch.float64, device=dev) for _ in range(3)]
        with pytest.raises(gmrfx.PosDefException, match="not positive definite"):
            be.predictor_marginals_dev(dx.data_ptr(), *(t.data_ptr() for t in outs), constraint_correction=True)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in outs)
        host = [np.full(17, 7.0) for _ in range(3)]
        rc = gmrfx._lib.lib().gmrfx_predictor_marginals(be._h, gmrfx._lib.ptr(c["x"]), 1, *(gmrfx._lib.ptr(a) for a in host))
        assert rc == gmrfx._lib.ERR_NOT_POSDEF and all((a == 7.0).all() for a in host)
        mu, v, pll = be.predictor_marginals(c["x"])            # without the bit the constraint is not looked at
        assert np.isfinite(mu).all() and (v[np.diff(sp.csr_matrix(c["A"]).indptr) > 0] > 0).all()
    finally:
        be.close()


def test_after_the_loop_with_refactorize_final_as_after_an_explicit_refactorisation():
    c = pref.design_case(GRID, 33, 1, True)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=False)
    try:
        _set(be, c)
        prior = c["Q"].data.copy()
        be.set_prior(prior, be.observations_hess_map())
        x, hess, info = be.gaussian_approximation(refactorize_final=True)
        assert info["converged"]
        a = be.predictor_marginals(x)
        be.refactorize_update(hess)
        b = be.predictor_marginals(x)
        assert all(same_bits(u, w) for u, w in zip(a, b))
        _check("posterior", be, dict(c, x=x), a)
    finally:
        be.close()
