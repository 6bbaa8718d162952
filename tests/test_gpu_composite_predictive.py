"""The predictive read-outs of a composite likelihood on the device (csrc/predictive.hip: k_pred_design_comp, k_pred_scores_comp;
gmrfx_predictor_marginals[_dev], gmrfx_predictive_scores[_dev] after gmrfx_obs_set_composite) against tests/composite_predictive_ref.py.

The restatement is fed the handle's own Sigma on pattern(Q) (gmrfx_selinv_extract), its constants and, under a constraint, its At
(gmrfx_constraints_get; B = At L_c^-T through tests/constraint_ref.py), as tests/test_gpu_predictive.py does: the bounds -- those of
tests/predictive_ref.py with the project's factor 16, per component -- cover the new arithmetic only. What each case reaches, the
float64 control and the mutants: tests/test_composite_predictive_host.py.

a. marginals entry by entry on `cuts`, `sixteen`, `rows`; the _dev form has the bits of the host form
b. scores entry by entry for every K of SCORE_K, the totals against the sums of the returned arrays, the special rows of `cuts`
c. the constraint correction under a composite: uncorrected and corrected bounds, the clamp rows never negative, never -0.0 and
   +0.0 on some row of every case; a composite of one family and parameter in five components has the bits of the design form on the
   same A, clamped rows among them (the guard of "KEEP THE TWO IN STEP" on the m > 0 branch of k_pred_design_comp)
d. each output on its own has the bits of the full call; the variance alone on an unfactorised handle is refused
e. a likelihood replaced on one handle: composite, design form, another composite, set_param -- each state has the bits of a fresh handle
f. after the loop with refactorize_final on the joint model under a sum-to-zero constraint"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import composite_predictive_ref as cp
import composite_ref as cref
import constraint_ref as conref
import gmrfx
import predictive_ref as pref
from layout_buffers import same_bits

pytestmark = pytest.mark.gpu
LD = pref.LD
GH = gmrfx.MI355XBackend.gauss_hermite
CASES = cp.cases()
DEV = "cuda:0"
TOT = ("lpd", "lcpo", "elp", "p_waic")


def _set_composite(be, c):
    o = c["obs"]
    comp = gmrfx.CompositeObservations(c["Q"].shape[0])
    A = sp.csr_matrix(c["A"])
    for k in range(o.ncomp):
        r0, r1 = int(o.rowptr[k]), int(o.rowptr[k + 1])
        comp.add(o.families[k], o.y[r0:r1], A=A[r0:r1], offset=None if c["b"] is None else c["b"][r0:r1],
                 aux=None if o.aux is None else o.aux[r0:r1], param=o.params[k])
    gmrfx.set_composite_observations(be, comp)


def _composite(c, factorize=True):
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=factorize)
    _set_composite(be, c)
    be.set_prior(c["Q"].data, be.observations_hess_map())
    return be


def _sigma(be, Q):
    """the handle's Sigma on pattern(Q), dense"""
    Z = be.selinv_extract_at(Q).tocoo()
    S = np.zeros(Q.shape)
    S[Z.row, Z.col] = Z.data
    return S


def _constrain(be, c):
    m = c["C"].shape[0]
    be.set_constraints(sp.csr_matrix(c["C"]), np.zeros(m))
    At, _ = be.constraint_fields()
    con = conref.prepare(sp.csr_matrix(c["C"]), np.zeros(m), At)
    assert con["kappa"] <= 1e3
    return con


def _check_marginals(tag, be, c, got, con=None, correct=False, x=None):
    cc, S = be.observations_pointwise_const(), _sigma(be, c["Q"])
    r = cp.marginals(c, S, cc, con=con, correct=correct, x=x)
    bd = cp.marginal_bounds(c, S, cc, r, con=con, correct=correct, x=x)
    rat = cp.marginal_ratios(got, r, bd, correct)
    print(f"{tag}: err/bound " + " ".join(f"{k} {v:.3f}" for k, v in rat.items()))
    assert max(rat.values()) <= 1.0, rat
    return rat


def _check_scores(tag, be, obs, mu, v, K):
    z, w = GH(K)
    arrs, tot = be.predictive_scores(mu, v, z, w)
    r = cp.scores(obs, mu, v, z, w, be.observations_pointwise_const())
    bd = cp.score_bounds(z, w, r)
    rat = cp.score_ratios(arrs, r, bd)
    print(f"{tag}: err/bound " + " ".join(f"{k} {v:.3f}" for k, v in rat.items()))
    assert max(rat.values()) <= 1.0, rat
    for a, k in zip(arrs, TOT):         # the totals against the sums of the returned arrays
        if np.isfinite(a).all():
            assert abs(LD(tot[k]) - np.asarray(a, LD).sum()) <= pref.total_bound(a), k
        else:
            assert not np.isfinite(tot[k]), k
    arrs2, tot2 = be.predictive_scores(mu, v, z, w)            # and again: the same bits
    assert all(same_bits(a, b) for a, b in zip(arrs, arrs2))
    assert all(same_bits(np.float64(tot[k]), np.float64(tot2[k])) for k in tot)
    return arrs, tot, r, rat


def _readouts(be, x, K=16, correct=False):
    """(mu_eta, v_eta, pll, lpd, lcpo, elp, vlp, totals as an array)"""
    m = be.predictor_marginals(x, constraint_correction=correct)
    z, w = GH(K)
    arrs, tot = be.predictive_scores(m[0], m[1], z, w)
    return tuple(m) + tuple(arrs) + (np.array([tot[k] for k in sorted(tot)]),)


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


# ---- a. the marginals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_marginals_entry_by_entry(name):
    c = CASES[name]
    be = _composite(c)
    try:
        got = be.predictor_marginals(c["x"])
        _check_marginals(f"marginals {name}", be, c, got)
        empty = np.flatnonzero(np.diff(sp.csr_matrix(c["A"]).indptr) == 0)
        assert all(got[1][i] == 0.0 and not np.signbit(got[1][i]) for i in empty)
        nobs = len(c["obs"].y)
        dx = torch.from_numpy(c["x"]).to(DEV)
        outs = [torch.full((nobs,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(3)]
        torch.cuda.synchronize()
        be.predictor_marginals_dev(dx.data_ptr(), *(t.data_ptr() for t in outs))
        torch.cuda.synchronize()
        assert _same([t.cpu().numpy() for t in outs], got)
        assert _same(be.predictor_marginals(c["x"]), got)
    finally:
        be.close()


# ---- b. the scores --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_scores_entry_by_entry(name):
    c = CASES[name]
    obs = c["obs"]
    be = _composite(c, factorize=False)
    try:
        mu, v = cp.score_inputs(obs)
        bad = ~(v >= 0)
        for K in pref.SCORE_K:
            arrs, tot, r, _ = _check_scores(f"scores {name} K {K}", be, obs, mu, v, K)
            assert all(np.array_equal(np.isnan(a), bad) for a in arrs)
            if bad.any():           # the totals are NaN: the same rows with their variances repaired
                assert all(np.isnan(tot[k]) for k in tot)
                arrs, tot, _, _ = _check_scores(f"scores {name} K {K} finite rows", be, obs, mu, cp.repaired(v), K)
                assert all(np.isfinite(a).all() for a in arrs) and tot["waic"] == -2.0 * (tot["lpd"] - tot["p_waic"])
    finally:
        be.close()


def test_special_rows_stay_in_their_own_rows():
    """v = 0, NaN, -1, a Poisson mean of exp(800) and mu = 700 on logit rows, on and beside the component edges at rows 16 and 32"""
    c = CASES["cuts"]
    obs, S = c["obs"], cp.SPECIAL
    be = _composite(c, factorize=False)
    try:
        mu, v = cp.special_inputs(obs)
        arrs, tot, r, _ = _check_scores("special rows", be, obs, mu, v, cp.SPECIAL_K)
        nan_rows = np.flatnonzero(np.all([np.isnan(a) for a in arrs], axis=0))
        assert nan_rows.tolist() == sorted([S["nan"], S["negative"]])
        assert all(np.isnan(tot[k]) for k in tot)
        lpd, lcpo, elp, vlp = arrs
        assert lpd[S["overflow"]] == -np.inf and lcpo[S["overflow"]] == -np.inf and elp[S["overflow"]] == -np.inf
        assert all(np.isfinite(a[[S["zero"], *S["logit"][1:]]]).all() for a in arrs)
        # every other row has the bits it has without the special rows
        z, w = GH(cp.SPECIAL_K)
        mu0, v0 = cp.score_inputs(obs)
        plain, _ = be.predictive_scores(mu0, cp.repaired(v0), z, w)
        same = np.setdiff1d(np.arange(len(obs.y)), [S["zero"], S["nan"], S["negative"], S["overflow"], *S["logit"]])
        assert all(same_bits(a[same], b[same]) for a, b in zip(arrs, plain))
    finally:
        be.close()


def test_logit_rows_are_finite_at_mu_700():
    """`sixteen`: mu = 700 and -700 on Bernoulli and Binomial rows with finite variances, between components of other families"""
    c = CASES["sixteen"]
    obs = c["obs"]
    be = _composite(c, factorize=False)
    try:
        mu, v, rows = cp.logit_inputs(obs)
        arrs, tot, _, _ = _check_scores("logit rows", be, obs, mu, v, cp.LOGIT_K)
        assert all(np.isfinite(a).all() for a in arrs) and all(np.isfinite(tot[k]) for k in tot)
    finally:
        be.close()


# ---- c. the constraint correction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m", cp.CON)
def test_constraint_correction_and_clamp_under_a_composite(name, m):
    """rows equal to the constraint's rows and multiples of them (composite_predictive_ref.CLAMP_SCALES) in two components: v -
    correction is 0 in exact arithmetic and of either sign by rounding; with bit 0 it comes back within its bound of 0, never negative,
    never -0.0, and on some row of every case as +0.0"""
    c = cp.con_case(name, m, base=CASES[name])
    clamp = c["clamp"]
    be = _composite(c)
    try:
        raw = be.predictor_marginals(c["x"])
        con = _constrain(be, c)
        again = be.predictor_marginals(c["x"])                 # without the bit: the raw value, no clamp
        assert _same(raw, again)
        _check_marginals(f"con {name} m {m} uncorrected", be, c, raw)
        got = be.predictor_marginals(c["x"], constraint_correction=True)
        _check_marginals(f"con {name} m {m} corrected", be, c, got, con=con, correct=True)
        assert same_bits(got[0], raw[0]) and same_bits(got[2], raw[2])
        tail = got[1][clamp]
        assert (tail >= 0).all() and not np.signbit(tail).any() and (tail < 1e-12 * raw[1][clamp]).all()
        assert not np.signbit(got[1][~np.isnan(got[1])]).any()
        print(f"con {name} m {m}: {int((tail == 0).sum())} of {len(tail)} rows clamped to +0.0")
        assert (tail == 0).any()            # the clamp itself: a difference that rounding left negative comes back as +0.0
        # the scores over the corrected marginals: v = +0.0 rows among them
        _check_scores(f"con {name} m {m} scores", be, c["obs"], got[0], got[1], 16)
    finally:
        be.close()


@pytest.mark.parametrize("name,m", cp.CON)
def test_one_family_in_five_components_has_the_bits_of_the_design_form_under_a_constraint(name, m):
    c = cp.twin_case(cp.con_case(name, m, base=CASES[name]))
    o = c["obs"]
    a = _composite(c)
    b = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"])
    try:
        b.set_design_observations(1, o.y, c["A"], c["b"], o.aux, 0.0)
        assert gmrfx.composite_info(a)["family"].tolist() == [1] * 5 and gmrfx.composite_info(b)["family"].size == 0
        for be in (a, b):
            _constrain(be, c)
        for correct in (False, True):
            for K in (16, 17):
                ra, rb = _readouts(a, c["x"], K, correct), _readouts(b, c["x"], K, correct)
                assert _same(ra, rb), (correct, K)
        v = _readouts(a, c["x"], 16, True)[1]
        assert not np.signbit(v).any() and (v[c["clamp"]] < 1e-12 * _readouts(a, c["x"], 16, False)[1][c["clamp"]]).all()
        assert (v[c["clamp"]] == 0).any()           # the twins agree on rows that pred_clamp changed
    finally:
        a.close()
        b.close()


# ---- d. outputs left out ----------------------------------------------------------------------------------------------------------------------
def test_each_output_on_its_own_has_the_bits_of_the_full_call():
    c = CASES["cuts"]
    obs = c["obs"]
    nobs = len(obs.y)
    be = _composite(c, factorize=False)
    try:
        dx = torch.from_numpy(c["x"]).to(DEV)

        def buf():
            return torch.full((nobs,), float("nan"), dtype=torch.float64, device=DEV)
        d_mu, d_pll, d_v = buf(), buf(), buf()
        torch.cuda.synchronize()
        be.predictor_marginals_dev(dx.data_ptr(), 0, 0, d_pll.data_ptr())           # no factorisation: pll alone, mu_eta alone
        be.predictor_marginals_dev(dx.data_ptr(), d_mu.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        with pytest.raises(gmrfx._lib.GmrfxError, match="refactorize"):
            be.predictor_marginals_dev(dx.data_ptr(), 0, d_v.data_ptr(), 0)
        with pytest.raises(gmrfx._lib.GmrfxError, match="refactorize"):
            be.predictor_marginals(c["x"], want_mean=False, want_pll=False)
        torch.cuda.synchronize()
        assert bool(torch.isnan(d_v).all())
        be.refactorize_values(c["Q"].data)
        full = be.predictor_marginals(c["x"])
        be.predictor_marginals_dev(dx.data_ptr(), 0, d_v.data_ptr(), 0)
        torch.cuda.synchronize()
        assert same_bits(d_mu.cpu().numpy(), full[0]) and same_bits(d_v.cpu().numpy(), full[1]) and same_bits(d_pll.cpu().numpy(), full[2])
        for want in ((True, False, False), (False, True, False), (False, False, True)):
            one = be.predictor_marginals(c["x"], want_mean=want[0], want_var=want[1], want_pll=want[2])
            assert all((g is None) if not w else same_bits(g, f) for w, g, f in zip(want, one, full))
        # the scores: each array alone, none at all
        mu, v = cp.special_inputs(obs)
        z, w = GH(cp.SPECIAL_K)
        arrs, tot = be.predictive_scores(mu, v, z, w)
        dm, dv = torch.from_numpy(mu).to(DEV), torch.from_numpy(v).to(DEV)
        for k in range(4):
            out = buf()
            ptrs = [0, 0, 0, 0]
            ptrs[k] = out.data_ptr()
            torch.cuda.synchronize()
            t = be.predictive_scores_dev(dm.data_ptr(), dv.data_ptr(), z, w, *ptrs)
            torch.cuda.synchronize()
            assert same_bits(out.cpu().numpy(), arrs[k]), k
            assert all(same_bits(np.float64(t[q]), np.float64(tot[q])) for q in tot)
        v2 = cp.repaired(v)
        v2[cp.SPECIAL["overflow"]], mu2 = 0.3, mu.copy()
        mu2[cp.SPECIAL["overflow"]] = 0.3
        arrs, tot = be.predictive_scores(mu2, v2, z, w)
        assert all(np.isfinite(tot[k]) for k in tot)
        none, tot2 = be.predictive_scores(mu2, v2, z, w, want_arrays=False)
        dm.copy_(torch.from_numpy(mu2))
        dv.copy_(torch.from_numpy(v2))
        torch.cuda.synchronize()
        assert none == (None,) * 4 and tot2 == tot and be.predictive_scores_dev(dm.data_ptr(), dv.data_ptr(), z, w) == tot
    finally:
        be.close()


# ---- e. a likelihood replaced on one handle ---------------------------------------------------------------------------------------------------
def test_a_replaced_likelihood_has_the_bits_of_a_fresh_handle():
    """composite (9 components), the design form on the same A, a composite of 3 components, set_param: pred_ and the component table
    are rebuilt each time"""
    c9 = CASES["cuts"]
    o9 = c9["obs"]
    nobs = len(o9.y)
    rowptr = np.array([0, cp.ROWS, 2 * cp.ROWS, nobs])
    fam3 = [1, 0, 4]
    y3, aux3 = cref._values(fam3, rowptr, np.random.default_rng(9))
    c3 = dict(c9, obs=cref.CompObs(fam3, [cref.PARAM[f] for f in fam3], rowptr, y3, aux3))
    p4 = [0.0, 1.3, 4.0]
    c4 = dict(c9, obs=cref.CompObs(fam3, p4, rowptr, y3, aux3))

    def design(be):
        be.set_design_observations(0, o9.y, c9["A"], c9["b"], None, 0.7)

    def fresh(setter):
        f = gmrfx.MI355XBackend(c9["Q"], device=0, uplo=c9["uplo"])
        try:
            setter(f)
            return _readouts(f, c9["x"])
        finally:
            f.close()
    be = gmrfx.MI355XBackend(c9["Q"], device=0, uplo=c9["uplo"])
    try:
        seen = []
        for tag, setter in (("composite of 9", lambda h: _set_composite(h, c9)), ("design form", design),
                            ("composite of 3", lambda h: _set_composite(h, c3)), ("set_param", lambda h: gmrfx.set_composite_param(h, p4))):
            setter(be)
            got = _readouts(be, c9["x"])
            want = fresh((lambda h: _set_composite(h, c4)) if tag == "set_param" else setter)
            assert _same(got, want), tag
            assert not seen or not same_bits(got[2], seen[-1][2]), tag           # (the states differ: pll moved)
            seen.append(got)
        assert gmrfx.composite_info(be)["param"].tolist() == p4
        # the last state against the restatement as well
        _check_marginals("after set_param", be, c4, seen[-1][:3])
    finally:
        be.close()


# ---- f. after the loop ------------------------------------------------------------------------------------------------------------------------
def test_after_the_loop_on_the_joint_model_under_a_sum_to_zero_constraint():
    c = cref.loop_cases()["joint_sum0"]
    be = _composite(c, factorize=False)
    try:
        be.set_constraints(sp.csr_matrix(c["C"]), np.zeros(1))
        x, hess, info = be.gaussian_approximation(x0=c["x0"], refactorize_final=True)
        assert info["converged"]
        got = be.predictor_marginals(x, constraint_correction=True)
        At, _ = be.constraint_fields()
        con = conref.prepare(sp.csr_matrix(c["C"]), np.zeros(1), At)
        _check_marginals("joint_sum0 at the mode", be, c, got, con=con, correct=True, x=x)
        assert (got[1] > 0).all()
        arrs, tot, _, _ = _check_scores("joint_sum0 at the mode", be, c["obs"], got[0], got[1], 16)
        assert all(np.isfinite(a).all() for a in arrs)
    finally:
        be.close()
