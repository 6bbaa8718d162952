"""The conditions tests/test_gpu_composite_predictive.py rests on, without a device (tests/composite_predictive_ref.py):

1. the float64 control stays inside the bounds WITHOUT their factor 16 on every case: the marginals (constrained cases with and
   without the correction) and the scores at every K of predictive_ref.SCORE_K, the special rows included;
2. every named mutant leaves the factor-16 bounds on the case named for it here;
3. the cases reach what they claim: every row length in every component of `rows`, component edges on the workgroup edges of `cuts`,
   clamp rows in two components of every constrained case, and the special rows' NaN and -inf under the reference alone.
Where the GPU tests feed the restatement the handle's own Sigma, At and constants, these feed it a dense long-double inverse rounded
to float64 and the restated constants."""
import numpy as np
import pytest
import scipy.sparse as sp

import composite_predictive_ref as cp
import constraint_ref as conref
import gmrfx
import predictive_ref as pref

LD = pref.LD
GH = gmrfx.MI355XBackend.gauss_hermite
CASES = cp.cases()
CON = {key: cp.con_case(*key, base=CASES[key[0]]) for key in cp.CON}
_SETUP = {}


def _case(key):
    return CON[key] if isinstance(key, tuple) else CASES[key]


def _setup(key):
    """(Sigma on the pattern, constants, prepared constraint or None) of a case, computed once"""
    if key not in _SETUP:
        c = _case(key)
        P, inv = pref.dense_posterior(c)
        con = None
        if isinstance(key, tuple):
            At = np.asarray(inv @ np.asarray(c["C"], LD).T, np.float64)
            con = conref.prepare(sp.csr_matrix(c["C"]), np.zeros(c["m"]), At)
            assert con["kappa"] <= 1e3, con["kappa"]
        _SETUP[key] = (P, cp.pointwise_const(c["obs"]), con)
    return _SETUP[key]


def _marginal_ratio(key, correct, dtype=None, mutant=None, factor=cp.FACTOR):
    c = _case(key)
    P, cc, con = _setup(key)
    kw = dict(con=con, correct=correct)
    r = cp.marginals(c, P, cc, **kw)
    bd = cp.marginal_bounds(c, P, cc, r, factor=factor, **kw)
    got = cp.marginals(c, P, cc, mutant=mutant, **kw) if dtype is None else cp.marginals(c, P, cc, dtype=dtype, **kw)
    return cp.marginal_ratios([got[k] for k in ("mu_eta", "v_eta", "pll")], r, bd, correct)


def _score_ratio(key, K, dtype=None, mutant=None, factor=cp.FACTOR, special=False):
    obs = _case(key)["obs"]
    cc = _setup(key)[1]
    mu, v = cp.special_inputs(obs) if special else cp.score_inputs(obs)
    z, w = GH(K)
    r = cp.scores(obs, mu, v, z, w, cc)
    bd = cp.score_bounds(z, w, r, factor=factor)
    got = cp.scores(obs, mu, v, z, w, cc, mutant=mutant) if dtype is None else cp.scores(obs, mu, v, z, w, cc, dtype=dtype)
    return cp.score_ratios([got[k] for k in cp.KEYS], r, bd), r, got


# ---- 1. the control -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(CASES) + list(cp.CON), ids=str)
def test_float64_control_of_the_marginals_stays_inside_the_bounds_without_the_factor(key):
    for correct in ((False, True) if isinstance(key, tuple) else (False,)):
        rat = _marginal_ratio(key, correct, dtype=np.float64, factor=1)
        print(f"{key} correct {correct}: control err / bound {rat}")
        assert max(rat.values()) <= 1.0, rat


@pytest.mark.parametrize("K", pref.SCORE_K)
@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_control_of_the_scores_stays_inside_the_bounds_without_the_factor(name, K):
    rat, r, r64 = _score_ratio(name, K, dtype=np.float64, factor=1)
    print(f"{name} K {K}: control err / bound {rat}")
    assert max(rat.values()) <= 1.0, rat
    # the totals: the sums of the scattered arrays, NaN where a row is
    for k, t, t64 in zip(cp.KEYS, r["totals"], r64["totals"]):
        if np.isfinite(r[k]).all():
            assert abs(t64 - t) <= pref.total_bound(r[k], factor=1) + np.abs(r64[k] - r[k]).sum()
        else:
            assert not np.isfinite(t) and not np.isfinite(t64)


def test_float64_control_of_the_special_rows():
    rat, r, r64 = _score_ratio("cuts", cp.SPECIAL_K, dtype=np.float64, factor=1, special=True)
    print(f"special rows: control err / bound {rat}")
    assert max(rat.values()) <= 1.0, rat


# ---- 2. the mutants -------------------------------------------------------------------------------------------------------------------------
# mutant -> (case, what is compared: ("scores", K) or ("marginals", correction))
CAUGHT_BY = {"comp_of_next_row": ("cuts", ("scores", 17)),
             "logparam_of_component_0": ("cuts", ("marginals", False)),
             "param_of_component_0": ("rows", ("scores", 16)),
             "family_table_shifted_past_first_workgroup": ("cuts", ("scores", 2)),
             "const_of_component_0_param": ("rows", ("marginals", False)),
             "aux_dropped_in_scores": ("rows", ("scores", 1)),
             "At_for_B": (("rows", 3), ("marginals", True)),
             "no_clamp": (("cuts", 3), ("marginals", True))}


def _mutant_ratio(mutant, key, what):
    if what[0] == "scores":
        return max(_score_ratio(key, what[1], mutant=mutant)[0].values())
    return max(_marginal_ratio(key, what[1], mutant=mutant).values())


@pytest.mark.parametrize("mutant", cp.MUTANTS)
def test_every_mutant_leaves_the_bounds_on_its_named_case(mutant):
    key, what = CAUGHT_BY[mutant]
    worst = _mutant_ratio(mutant, key, what)
    print(f"{mutant} on {key} {what}: err / bound {worst:.3g}")
    assert worst > 1.0, worst


def test_the_table_mutants_are_seen_by_marginals_and_scores_alike():
    """each wrong table lookup leaves the bounds of pll AND of the scores (K = 17) on `cuts`: neither kernel's lookup is covered by the
    other's test alone. aux_dropped_in_scores is a rule of the scores only: pll stays clean."""
    for mutant in ("comp_of_next_row", "logparam_of_component_0", "param_of_component_0", "family_table_shifted_past_first_workgroup",
                   "const_of_component_0_param"):
        assert _mutant_ratio(mutant, "cuts", ("scores", 17)) > 1.0, mutant
        assert _marginal_ratio("cuts", False, mutant=mutant)["pll"] > 1.0, mutant
    assert _mutant_ratio("aux_dropped_in_scores", "cuts", ("scores", 17)) > 1.0
    assert max(_marginal_ratio("rows", False, mutant="aux_dropped_in_scores").values()) == 0.0
    assert set(CAUGHT_BY) == set(cp.MUTANTS)


def test_no_mutant_is_the_clean_rule_in_disguise_and_the_clean_rule_has_ratio_zero():
    for key in ("cuts", "rows"):
        assert max(_marginal_ratio(key, False).values()) == 0.0
        assert max(_score_ratio(key, 16)[0].values()) == 0.0


# ---- 3. the cases ---------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_what_they_claim():
    R = cp.ROWS
    assert R == 16
    for name, c in CASES.items():
        nobs, n = sp.csr_matrix(c["A"]).shape
        assert n <= 80 and nobs <= 48, name
    rows = CASES["rows"]
    A, o = sp.csr_matrix(rows["A"]), rows["obs"]
    counts = np.diff(A.indptr)
    assert o.families == [5, 4, 3] and o.rowptr.tolist() == [0, 6, 12, 18] and rows["b"] is not None and (A.data == 0).any()
    for k in range(3):
        assert sorted(counts[o.rowptr[k]:o.rowptr[k + 1]]) == sorted(pref.ROW_COUNTS), k
    # Q's pattern holds every pair of a row
    P = sp.csr_matrix(A, copy=True)
    P.data[:] = 1.0
    pairs, Qp = sp.coo_matrix(P.T @ P), sp.csc_matrix(rows["Q"])
    have = set(zip(*sp.coo_matrix(Qp).nonzero())) | set(zip(sp.coo_matrix(Qp).row, sp.coo_matrix(Qp).col))
    assert set(zip(pairs.row, pairs.col)) <= have
    cuts = CASES["cuts"]["obs"]
    comp = cuts.comp_of_row()
    assert len(cuts.y) == 2 * R + 8 and cuts.ncomp == 9 and set(cuts.families) == set(range(6))
    for edge in (R, 2 * R):         # one-row components on either side of the workgroups' edges
        assert comp[edge - 1] != comp[edge] and (comp == comp[edge - 1]).sum() == 1 and (comp == comp[edge]).sum() == 1
    assert CASES["sixteen"]["obs"].ncomp == 16
    for key, c in CON.items():
        o, m = c["obs"], c["m"]
        A = sp.csr_matrix(c["A"]).toarray()
        assert A.shape[1] <= 80 and A.shape[0] <= 48
        ccomp = o.comp_of_row()[c["clamp"]]
        assert len(set(ccomp)) >= 2 and len(c["clamp"]) == min(48 - len(CASES[key[0]]["obs"].y), cp.MAX_CLAMP) >= 8, key
        fams = {o.families[k] for k in set(ccomp)}
        assert len(fams) >= 2
        for q, i in enumerate(c["clamp"]):        # each is a multiple of a constraint row: C itself first, then -0.5 C, then 3 C ...
            assert np.array_equal(A[i], c["scales"][q] * c["C"][q % m]), (key, i)
        assert (c["scales"][:m] == 1.0).all() and (c["scales"][m:2 * m] == -0.5).all()
        # at least two draws of the rounded difference's sign that are independent of the unscaled rows': multiples that are no
        # power of two (a power of two scales v and the correction exactly: the copy rounds as the row itself)
        odd = {(float(s), q % m) for q, s in enumerate(c["scales"]) if np.frexp(abs(s))[0] != 0.5}
        assert len(odd) >= 2, key
        base = CASES[key[0]]
        nb = len(base["obs"].y)
        assert np.array_equal(A[:nb], sp.csr_matrix(base["A"]).toarray()) and np.array_equal(o.y[:nb], base["obs"].y)
    twin = cp.twin_case(CON[("cuts", 3)])["obs"]
    assert twin.rowptr.tolist()[:5] == [0, 1, R - 1, R, R + 1] and set(twin.families) == {1} and set(twin.params) == {0.0}


def test_logit_rows_of_sixteen_at_mu_700_under_the_reference_and_the_control():
    obs = CASES["sixteen"]["obs"]
    mu, v, rows = cp.logit_inputs(obs)
    fam = np.asarray(obs.families)[obs.comp_of_row()]
    assert set(fam[rows]) == {2, 3} and (np.abs(mu[rows]) == 700.0).all() and (mu[rows] > 0).any() and (mu[rows] < 0).any()
    assert ((fam[rows] == 2) & (mu[rows] == 700.0)).any() and ((fam[rows] == 2) & (mu[rows] == -700.0)).any()
    z, w = GH(cp.LOGIT_K)
    cc = _setup("sixteen")[1]
    r = cp.scores(obs, mu, v, z, w, cc)
    assert all(np.isfinite(np.asarray(r[k], np.float64)).all() for k in cp.KEYS)
    bd = cp.score_bounds(z, w, r, factor=1)
    r64 = cp.scores(obs, mu, v, z, w, cc, dtype=np.float64)
    rat = cp.score_ratios([r64[k] for k in cp.KEYS], r, bd)
    print(f"logit rows: control err / bound {rat}")
    assert max(rat.values()) <= 1.0, rat


def test_special_rows_under_the_reference_alone():
    obs = CASES["cuts"]["obs"]
    comp, fam = obs.comp_of_row(), np.asarray(obs.families)
    S = cp.SPECIAL
    assert fam[comp[S["zero"]]] == 1 and (comp == comp[S["zero"]]).sum() == 1 and S["zero"] == cp.ROWS
    assert fam[comp[S["overflow"]]] == 1 and fam[comp[S["nan"]]] == 2 and S["nan"] == cp.ROWS - 1 and S["negative"] == 2 * cp.ROWS - 1
    assert [fam[comp[i]] for i in S["logit"]] == [2, 3, 3]
    mu, v = cp.special_inputs(obs)
    z, w = GH(cp.SPECIAL_K)
    r = cp.scores(obs, mu, v, z, w, _setup("cuts")[1])
    nan_rows = np.flatnonzero(np.all([np.isnan(r[k]) for k in cp.KEYS], axis=0))
    assert nan_rows.tolist() == sorted([S["nan"], S["negative"]])
    assert np.isnan(r["totals"].astype(float)).all()
    assert (r["lcpo"] == -np.inf).sum() >= 1 and r["lcpo"][S["overflow"]] == -np.inf and r["lpd"][S["overflow"]] == -np.inf
    # a row's special value stays in its own row: every other row is what it is without the special rows
    mu0, v0 = cp.score_inputs(obs)
    r0 = cp.scores(obs, mu0, cp.repaired(v0), z, w, _setup("cuts")[1])
    same = np.setdiff1d(np.arange(len(obs.y)), [S["zero"], S["nan"], S["negative"], S["overflow"], *S["logit"]])
    assert all(np.array_equal(r[k][same], r0[k][same]) for k in cp.KEYS)
    for i in S["logit"][1:]:        # the Binomial rows at mu = 700 are finite
        assert all(np.isfinite(r[k][i]) for k in cp.KEYS)
    assert all(np.isfinite(r[k][S["zero"]]) for k in cp.KEYS)
