"""References for the predictive read-outs of a composite likelihood (csrc/predictive.hip: k_pred_design_comp, k_pred_scores_comp), no
device.

RESTATEMENT. The scores are independent per observation, so the composite's restatement is tests/predictive_ref.py run per component
and scattered back: `scores`, `score_bounds` hand predictive_ref.scores / score_bounds / ll_sizes that component's rows of mu, v, c, y
and aux with that component's family and parameter (a small record with .family, .y, .aux, .param). The totals are the long-double sums
of the scattered arrays (predictive_ref.total_bound bounds the handle's totals against the sum of the arrays it returned). For the
marginals mu_eta and v_eta do not depend on the family: they and their bounds are predictive_ref.marginals / marginal_bounds on the
stacked A; pll and its bound follow the per-component rule (4 eps S(eta) + |g| e_mu + eps (|l| + |c|), module docstring of
predictive_ref). Nothing of predictive_ref, fisher_ref or composite_ref is edited: `restated()` puts a proxy of fisher_ref in
predictive_ref's place for the duration of a call (as composite_ref.restated does for fisher_design_ref). The proxy does two things:
* it rounds l to the range of the output format: the device's l_k is a double, and a log density below -DBL_MAX (a Poisson mean of
  exp(800)) is -inf there -- the correctly rounded value -- where long double still holds -1e347. With it the non-finite entries of
  the restatement (lpd = lcpo = elp = -inf, vlp = NaN on such a row) are the device's, and predictive_ref.ratio compares them exactly;
* it evaluates the NegBin rule with log r taken from another parameter than r (the mutants below; k_pred_*_comp read tab.param and
  tab.logparam separately).
dtype=np.float64 gives the control, which has to stay inside the bounds WITHOUT the factor 16.

MUTANTS: deliberately wrong composites, each of which has to leave the factor-16 bounds on the case tests/test_composite_predictive_host.py
names for it.

CASES (at most 80 nodes, at most 48 observations): `cuts` and `sixteen` of composite_ref.eval_cases() unchanged; `rows`: rows of 0, 1, 3,
16, 17 and 33 entries (predictive_ref.ROW_COUNTS) in each of three components Gamma / NegBin / Binomial, with an offset; con_case(name,
m): `cuts` / `rows` under m constraint rows of ones over disjoint blocks, followed by design rows equal to the constraint's rows and
multiples of them (CLAMP_SCALES; v - correction = 0 in exact arithmetic: the clamp), which make up two further components (Poisson,
Gamma).

MEASURED (MI355X, largest error / bound with the factor 16, as tests/test_gpu_composite_predictive.py prints them): RATIOS below."""
import contextlib

import numpy as np
import scipy.sparse as sp

import composite_ref as cref
import fisher_design_ref as dref
import fisher_ref as ref
import predictive_ref as pref

LD, EPS, FACTOR = pref.LD, pref.EPS, pref.FACTOR
ROWS = dref.ROWS            # observations per workgroup of both kernels
KEYS = ("lpd", "lcpo", "elp", "vlp")
MARGINAL_MUTANTS = ("At_for_B", "no_clamp")
MUTANTS = ("comp_of_next_row", "logparam_of_component_0", "param_of_component_0", "family_table_shifted_past_first_workgroup",
           "const_of_component_0_param", "aux_dropped_in_scores") + MARGINAL_MUTANTS
DBL_MAX = np.finfo(np.float64).max

# largest error / bound (factor 16) seen on the MI355X. marginals: (mu_eta, v_eta, pll), `replaced`: the three-component composite of
# the replaced-likelihood test after set_param; scores: the largest over SCORE_K of (lpd, lcpo, elp, vlp), `con`: over the corrected
# marginals of the four constrained cases at K = 16; con: v_eta (uncorrected, corrected) per (case, m); clamped: (rows that came back
# as +0.0, clamp rows) per (case, m) -- the tests assert that there is one. None reaches 0.5; the largest of all is 0.026.
RATIOS = {"marginals": {"cuts": (0.010, 0.006, 0.007), "rows": (0.008, 0.001, 0.005), "sixteen": (0.015, 0.004, 0.010),
                        "joint_sum0": (0.010, 0.004, 0.009), "replaced": (0.010, 0.006, 0.026)},
          "scores": {"cuts": (0.008, 0.015, 0.006, 0.003), "rows": (0.008, 0.008, 0.007, 0.002), "sixteen": (0.014, 0.014, 0.011, 0.004),
                     "special": (0.003, 0.007, 0.005, 0.003), "logit": (0.006, 0.006, 0.006, 0.002), "con": (0.005, 0.013, 0.006, 0.008),
                     "joint_sum0": (0.004, 0.009, 0.006, 0.004)},
          "con": {("cuts", 1): (0.005, 0.003), ("cuts", 3): (0.004, 0.001), ("rows", 1): (0.003, 0.002), ("rows", 3): (0.003, 0.001)},
          "clamped": {("cuts", 1): (5, 8), ("cuts", 3): (6, 8), ("rows", 1): (6, 12), ("rows", 3): (9, 12)}}


# ---- the per-component rule -----------------------------------------------------------------------------------------------------------------
class Rec:
    """the rows of one component as predictive_ref reads an observation set"""

    def __init__(self, family, y, aux, param):
        self.family, self.y, self.aux, self.param = family, np.asarray(y, np.float64), aux, param


class _Split:
    """NegBin with r = param and log r = log(lr_param): what a kernel computes that takes the two from different table entries"""

    def __init__(self, lr_param):
        self.lr_param = lr_param


class _Ref:
    """fisher_ref with l rounded to the range of a double, and the split NegBin rule"""

    def __getattr__(self, name):
        return getattr(ref, name)

    @staticmethod
    def pointwise(family, eta, y, aux, param, dtype=LD):
        if isinstance(family, _Split):
            eta, y = np.asarray(eta, dtype), np.asarray(y, dtype)
            aux = np.zeros_like(eta) if aux is None else np.asarray(aux, dtype)
            p, e = dtype(param), eta + aux
            lr = np.log(dtype(family.lr_param))
            s, q = ref._logistic(e - lr), ref._logistic(lr - e)
            g, d, mean = y * q - p * s, -((p + y) * s * q), np.exp(e)
            ll = y * e - (p + y) * (np.maximum(lr, e) + np.log1p(np.exp(-np.abs(e - lr))))
        else:
            g, d, ll, mean = ref.pointwise(family, eta, y, aux, param, dtype)
        with np.errstate(invalid="ignore"):
            ll = np.where(ll < -DBL_MAX, -np.inf, ll)
        return g, d, ll, mean


@contextlib.contextmanager
def restated():
    """predictive_ref reaches fisher_ref through its module attribute `ref` alone; the assertion says so should that change"""
    assert pref.ref is ref and not hasattr(pref, "pointwise"), \
        "predictive_ref no longer reaches fisher_ref.pointwise through its attribute `ref`: restated() cannot dispatch"
    saved, pref.ref = pref.ref, _Ref()
    try:
        yield
    finally:
        pref.ref = saved


def _allows(f, y, aux, param):
    """may a row with these values be evaluated under family f (the checks of gmrfx_obs_set_composite)"""
    count = y >= 0 and y == np.floor(y)
    if f == 0:
        return param > 0
    if f == 1:
        return bool(count)
    if f == 2:
        return y in (0.0, 1.0)
    if f == 3:
        return bool(count and aux >= 1 and aux == np.floor(aux) and y <= aux)
    if f == 4:
        return bool(count and param > 0)
    return bool(y > 0 and param > 0)


def device_aux(obs):
    """aux as the handle stores it: the caller's on the rows of the components that read one, 0 elsewhere (NaN there is never read)"""
    nobs = len(obs.y)
    a = np.zeros(nobs)
    if obs.aux is not None:
        reads = np.isin(np.asarray(obs.families)[obs.comp_of_row()], cref.READS_AUX)
        a[reads] = np.asarray(obs.aux, np.float64)[reads]
    return a


def groups(obs, mutant=None, in_scores=False):
    """[(Rec, row indices)]: the rows that share (family, param, parameter of log r), under the named wrong rule where one is given"""
    nobs = len(obs.y)
    comp = obs.comp_of_row()
    if mutant == "comp_of_next_row":
        comp = np.r_[comp[1:], comp[-1]]
    fam = np.asarray(obs.families, np.int64)[comp]
    par = np.asarray(obs.params, np.float64)[comp]
    lpar = par.copy()
    aux = device_aux(obs)
    if mutant == "logparam_of_component_0":
        lpar[:] = obs.params[0]
    if mutant == "param_of_component_0":
        par[:] = obs.params[0]
    if mutant == "family_table_shifted_past_first_workgroup":
        for i in range(ROWS, nobs):
            f2 = (int(fam[i]) + 1) % 6
            fam[i] = f2 if _allows(f2, obs.y[i], aux[i], par[i]) else obs.families[0]
    drop = in_scores and mutant == "aux_dropped_in_scores"
    out = []
    for key in sorted({(int(f), float(p), float(lp) if f == 4 else float(p)) for f, p, lp in zip(fam, par, lpar)}):
        f, p, lp = key
        i = np.flatnonzero((fam == f) & (par == p) & ((lpar == lp) if f == 4 else True))
        family = _Split(lp) if (f == 4 and lp != p) else f
        out.append((Rec(family, obs.y[i], None if (drop or f not in cref.READS_AUX) else aux[i], p), i))
    assert sum(len(i) for _, i in out) == nobs
    return out


def pointwise_const(obs, mutant=None):
    """c_i in float64 (the long-double restatement rounded once): the stand-in for the handle's own where there is no device"""
    o = obs
    if mutant == "const_of_component_0_param":
        o = cref.CompObs(obs.families, [obs.params[0]] * obs.ncomp, obs.rowptr, obs.y, obs.aux)
    return np.asarray(cref.pointwise_const(o), np.float64)


def _consts(obs, cc, mutant):
    return pointwise_const(obs, mutant) if mutant == "const_of_component_0_param" else np.asarray(cc, np.float64)


# ---- the marginals --------------------------------------------------------------------------------------------------------------------------
def _neutral(nobs):
    return Rec(0, np.zeros(nobs), None, 1.0)


def marginals(c, Sigma, cc, con=None, correct=False, dtype=LD, mutant=None, x=None):
    """c: a case (A, b, obs, x); Sigma: dense symmetric, the handle's entries on pattern(Q); cc: the handle's constants; con:
    constraint_ref.prepare(...) of the handle's At. mu_eta, v_eta (and v0, corr) of predictive_ref.marginals on the stacked A; pll, g
    and l per component."""
    obs = c["obs"]
    nobs = len(obs.y)
    Ad = sp.csr_matrix(c["A"]).toarray()
    r = pref.marginals(Ad, c["b"], c["x"] if x is None else x, Sigma, _neutral(nobs), np.zeros(nobs), con=con, correct=correct, dtype=dtype,
                       mutant=mutant if mutant in MARGINAL_MUTANTS else None)
    g, ll = np.zeros(nobs, dtype), np.zeros(nobs, dtype)
    with restated():
        for rec, i in groups(obs, mutant):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                gi, _, li, _ = pref.ref.pointwise(rec.family, r["mu_eta"][i], rec.y, rec.aux, rec.param, dtype)
            g[i], ll[i] = gi, li
    ck = np.asarray(_consts(obs, cc, mutant), dtype)
    r.update(g=g, ll=ll, pll=ll + ck, cc=ck)
    return r


def marginal_bounds(c, Sigma, cc, r, con=None, correct=False, factor=FACTOR, x=None):
    obs = c["obs"]
    nobs = len(obs.y)
    Ad = sp.csr_matrix(c["A"]).toarray()
    bd = pref.marginal_bounds(Ad, c["b"], c["x"] if x is None else x, Sigma, _neutral(nobs), np.zeros(nobs), r, con=con, correct=correct,
                              factor=1)
    e_mu = bd["mu_eta"]
    S = np.zeros(nobs, LD)
    with restated():
        for rec, i in groups(obs):
            S[i] = pref.ll_sizes(rec.family, r["mu_eta"][i], rec.y, rec.aux, rec.param)
    e_pll = 4 * EPS * S + np.abs(r["g"]) * e_mu + EPS * (np.abs(r["ll"]) + np.abs(np.asarray(cc, LD)))
    return {"mu_eta": factor * e_mu, "v_eta": factor * bd["v_eta"], "pll": factor * e_pll}


def marginal_ratios(got, r, bd, correct=False):
    return {k: pref.ratio(g, r[k], bd[k], nonnegative=correct and k == "v_eta") for k, g in zip(("mu_eta", "v_eta", "pll"), got)
            if g is not None}


# ---- the scores -----------------------------------------------------------------------------------------------------------------------------
def scores(obs, mu, v, z, w, cc, dtype=LD, mutant=None):
    """lpd, lcpo, elp, vlp (nobs each) scattered from the components' runs, their totals, and `parts` for score_bounds()"""
    mu, v = np.asarray(mu, np.float64), np.asarray(v, np.float64)
    nobs = len(obs.y)
    ck = _consts(obs, cc, mutant)
    out = {k: np.full(nobs, np.nan, dtype) for k in KEYS}
    parts = []
    with restated():
        for rec, i in groups(obs, mutant, in_scores=True):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                r = pref.scores(mu[i], v[i], z, w, rec, ck[i], dtype)
            for k in KEYS:
                out[k][i] = r[k]
            parts.append((rec, i, r))
    out["totals"] = np.array([out[k].sum(dtype=dtype) for k in KEYS], dtype)
    out["parts"] = parts
    return out


def score_bounds(z, w, r, factor=FACTOR):
    nobs = sum(len(i) for _, i, _ in r["parts"])
    bd = {k: np.full(nobs, np.nan, LD) for k in KEYS}
    with restated():
        for rec, i, rk in r["parts"]:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                b = pref.score_bounds(z, w, rec, rk, factor)
            for k in KEYS:
                bd[k][i] = b[k]
    return bd


def score_ratios(arrs, r, bd):
    return {k: pref.ratio(a, r[k], bd[k]) for k, a in zip(KEYS, arrs)}


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def _rows_case():
    n = 48
    rng = np.random.default_rng(41)
    A = sp.csr_matrix(dref._rows_matrix(n, list(pref.ROW_COUNTS) * 3, rng, positive=False))
    A.data[1] = 0.0          # (stays stored)
    return cref._case(ref.banded(n, 2, seed=6), A, "full", [5, 4, 3], np.array([0, 6, 12, 18]), rng, True, False, 6)


def cases():
    """name -> dict(Q, uplo, A, b, obs, x, ...)"""
    ev = cref.eval_cases()
    return {"cuts": ev["cuts"], "sixteen": ev["sixteen"], "rows": _rows_case()}


CON = (("cuts", 1), ("cuts", 3), ("rows", 1), ("rows", 3))
CON_FAMILIES = [1, 5]


MAX_NOBS, MAX_CLAMP = 48, 12
# the multiples of the constraint's rows, in the order they are appended. 1, -0.5 and 2 are those of tests/test_gpu_predictive.py; they
# scale every operand of v and of the correction by a power of two, so the copies of one row round alike: ONE draw of the sign of the
# rounded difference per constraint row. The others are not powers of two (3, 5, 7: their squares are exact; the rest: the weight
# fl(s s) carries its own rounding, inside the "+ 6" of the bound of v_eta): a draw each, so that some row of every case rounds to or
# below zero and the clamp itself is seen.
CLAMP_SCALES = (1.0, -0.5, 3.0, -0.7, 1.3, 2.0, 0.3, 5.0, -1.7, 0.9, 7.0, -0.11)


def clamp_rows(Cm, count):
    """(rows, their scales): s C row by row for s in CLAMP_SCALES until `count` rows"""
    rows = [(s * Cm[j], s) for s in CLAMP_SCALES for j in range(len(Cm))][:count]
    return np.vstack([r for r, _ in rows]), np.array([s for _, s in rows])


def con_case(name, m, base=None):
    """the case under m constraint rows, followed by multiples of the constraint's rows (clamp_rows: as many as keep the case within
    MAX_NOBS observations, MAX_CLAMP at the most) as design rows in two further components; `clamp`: their indices, `scales`: their
    multiples, C: the constraint's rows (dense), e = 0"""
    base = cases()[name] if base is None else base
    A0, o = sp.csr_matrix(base["A"]), base["obs"]
    nobs0, n = A0.shape
    Cm = pref.constraint_rows(n, m)
    extra, scales = clamp_rows(Cm, min(MAX_NOBS - nobs0, MAX_CLAMP))
    ne = len(extra)
    k1 = (ne + 1) // 2
    A = sp.vstack([A0, sp.csr_matrix(extra)]).tocsr()
    rng = np.random.default_rng(100 * m + len(name))
    y2, aux2 = cref._values(CON_FAMILIES, np.array([0, k1, ne]), rng)
    aux0 = np.full(nobs0, np.nan) if o.aux is None else np.asarray(o.aux, np.float64)
    obs = cref.CompObs(o.families + CON_FAMILIES, o.params + [cref.PARAM[f] for f in CON_FAMILIES], np.r_[o.rowptr, nobs0 + k1, nobs0 + ne],
                       np.r_[o.y, y2], np.r_[aux0, aux2])
    Q, u = dref.with_pattern(base["Q"], A, "full")
    b = np.r_[base["b"], rng.uniform(-0.3, 0.3, ne)]
    return dict(Q=Q, uplo=u, A=A, b=b, obs=obs, x=base["x"], mu=base["mu"], pure=False, C=Cm, m=m, clamp=np.arange(nobs0, nobs0 + ne),
                scales=scales)


TWIN_CUTS = (1, ROWS - 1, ROWS, ROWS + 1)


def twin_case(c):
    """the stacked A of a case under ONE family and parameter (Poisson with exposure) cut into components at rows 1, 15, 16, 17: what
    the design form computes on the same A, bit for bit"""
    nobs = sp.csr_matrix(c["A"]).shape[0]
    o = ref.make_obs(1, nobs, np.random.default_rng(77), "all")
    rowptr = np.r_[0, TWIN_CUTS, nobs]
    ncomp = len(rowptr) - 1
    return dict(c, obs=cref.CompObs([1] * ncomp, [0.0] * ncomp, rowptr, o.y, o.aux))


def score_inputs(obs, seed=0):
    """(mu, v) drawn as predictive_ref.score_inputs draws them, component by component (a component of 8 rows or more gets a zero, a
    NaN and a negative variance among its rows)"""
    mu, v = np.zeros(len(obs.y)), np.zeros(len(obs.y))
    for k in range(obs.ncomp):
        r0, r1 = int(obs.rowptr[k]), int(obs.rowptr[k + 1])
        _, mu[r0:r1], v[r0:r1] = pref.score_inputs(obs.families[k], r1 - r0, seed=seed + k)
    return mu, v


def repaired(v):
    """the variances with every NaN or negative one replaced: the rows whose totals are finite"""
    v = np.asarray(v, np.float64)
    return np.where(v >= 0, v, 0.3)


SPECIAL_K = 17
SPECIAL = dict(zero=16, nan=15, negative=31, overflow=39, logit=(15, 14, 33))


def special_inputs(obs):
    """`cuts` at K = 17: repaired draws, then v = 0 on the one-row Poisson component at row 16, v = NaN on row 15 (the one Bernoulli
    row), v = -1 on row 31 (NegBin), a Poisson mean of exp(800) on row 39 (it overflows at every node), mu = 700 on the Bernoulli row
    (15: its outputs are NaN through v, the Binomial rows carry the check) and on the Binomial rows 14 (the last of its component) and
    33 (the first)"""
    mu, v = score_inputs(obs)
    v = repaired(v)
    v[SPECIAL["zero"]], v[SPECIAL["nan"]], v[SPECIAL["negative"]] = 0.0, np.nan, -1.0
    mu[SPECIAL["overflow"]] = 800.0
    mu[list(SPECIAL["logit"])] = 700.0
    return mu, v


LOGIT_K = 17


def logit_inputs(obs):
    """`sixteen` at K = 17: mu = 700 and mu = -700 on the first two rows of every Bernoulli and Binomial component (all its variances are
    finite: `cuts` has one Bernoulli row, the one whose variance is NaN); returns (mu, v, those rows)"""
    mu, v = score_inputs(obs)
    assert (v >= 0).all()
    rows = []
    for k in range(obs.ncomp):
        if obs.families[k] in (2, 3):
            r0, r1 = int(obs.rowptr[k]), int(obs.rowptr[k + 1])
            mu[r0] = 700.0
            rows.append(r0)
            if r1 - r0 > 1:
                mu[r0 + 1] = -700.0
                rows.append(r0 + 1)
    return mu, v, np.array(rows)
