"""References for the pullback of gaussian_approximation under a composite likelihood (gmrfx_ga_pullback_composite; csrc/ga_pullback.hip:
k_gap_point_comp, k_gap_param_comp, k_gap_final_comp), no device.

The rule is that of tests/ga_pullback_ref.py with d3, gp and dp of every row under the family and parameter of the row's component, and
the parameter cotangent split by component:  param[c] = sum_{i in c} (A lam)_i gp_i - sum_{i in c} c_i dp_i.

* restate() / bounds(): ga_pullback_ref.restate and bounds, run with fisher_ref.pointwise and ga_pullback_ref.point3 dispatched per
  component for the duration of the call (`restated()`, the idea of composite_ref.restated(); neither module is edited). `param` becomes
  a vector (split()). Its bound: a component's partial sums are its own -- no workgroup mixes components (tiles()) -- so param[c] is the
  single-family sum over c's rows alone: ga_pullback_ref.bounds is run on those rows and its `param` taken. That function takes the
  depth of the two-level sum from max(n, rows); the depth that belongs here is 8 + reduction_depth(rows of c), the workgroup tree and
  the final pass over c's OWN blocks. The two agree for every case of this file (asserted in bounds(): they differ only when n needs
  more passes of the final kernel than c's rows do). A component without a parameter has bound 0: the entry point returns exactly 0.0.
  The whole-array outputs (xbar, Qbar_prior, mubar_prior, check) do not see the components except through d3: their bounds are
  ga_pullback_ref's on the stacked A.
* tiles(): the component tiling of csrc/kernels.h (gap_comp_tiles, GapTiles) restated.
* MUTANTS: named wrong rules, each of which has to leave the bounds on at least one case.
* fd_case(), objective(), rule_derivatives(): the whole Laplace objective of a Normal + Gamma + NegBinomial + Poisson joint model and
  its derivatives by each component's parameter and along a direction of the prior's precision and mean.
  MEASURED (CPU, np.longdouble, relative steps 1e-3 and 5e-4): FD_MEASURED below, the relative discrepancy at the smaller step per
  derivative; the larger step's is 4.00 times that in every case.

MEASURED (MI355X, error / bounds(.., 16), the handle's own lam): RATIOS below, the largest per case as tests/test_gpu_composite_pullback.py
prints them."""
import contextlib
import functools

import numpy as np

import composite_ref as cref
import fisher_design_ref as dref
import fisher_ref as ref
import ga_pullback_ref as gref

LD, EPS, FACTOR = gref.LD, gref.EPS, gref.FACTOR
ROWS, FINAL = dref.ROWS, ref.FINAL
HAS_PARAM = gref.HAS_PARAM
MUTANTS = ("total_for_all", "boundary_row", "param0_for_all", "last_family_for_all", "no_dp", "grid_tiles")
# what composite_ref.CompObs.rows() applies to family and parameter; boundary_row: the first row of component 1 is a row of component 0
# there (its family, its parameter) AND in the split, as a tile of component 0 that runs one row over the cut would have it
_POINT_MUTANTS = ("param0_for_all", "last_family_for_all", "boundary_row")

# relative discrepancy between the rule and the central difference at the smaller step (tests/test_composite_pullback_host.py)
FD_MEASURED = {"param[0] Normal": 5.49e-7, "param[1] Gamma": 5.81e-7, "param[2] NegBinomial": 3.28e-8, "precision": 6.38e-9, "mean": 1.83e-8}
FD_BOUND = 5.81e-6           # the largest of them with a tenfold margin

# largest error / bound on the MI355X per case: (xbar, Qbar_prior, mubar_prior, param, check)
RATIOS = {"one": (0.000, 0.007, 0.003, 0.000, 0.000), "same_nodes": (0.000, 0.007, 0.003, 0.000, 0.001),
          "cuts": (0.000, 0.008, 0.003, 0.002, 0.000), "six": (0.000, 0.007, 0.003, 0.001, 0.001),
          "sixteen": (0.000, 0.006, 0.003, 0.001, 0.000), "long": (0.000, 0.008, 0.001, 0.001, 0.000)}

_POINT3 = gref.point3


# ---- the component tiling -------------------------------------------------------------------------------------------------------------------
def tiles(rowptr):
    """(bptr, [(component, first row, end row)] per workgroup): component c owns workgroups bptr[c] .. bptr[c + 1], ceil(rows_c / ROWS)
    of them; a workgroup's rows start at rowptr[c] + ROWS (b - bptr[c]) and are cut at rowptr[c + 1]"""
    bptr, out = [0], []
    for c in range(len(rowptr) - 1):
        r0, r1 = int(rowptr[c]), int(rowptr[c + 1])
        nb = -(-(r1 - r0) // ROWS)
        out += [(c, r0 + ROWS * b, min(r0 + ROWS * (b + 1), r1)) for b in range(nb)]
        bptr.append(bptr[-1] + nb)
    return np.array(bptr), out


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def point3(obs, eta, dtype=LD):
    """ga_pullback_ref.point3 per component of a CompObs"""
    eta = np.asarray(eta, dtype)
    out = [np.zeros(len(eta), dtype) for _ in range(7)]
    for f, p, i in obs.rows():
        if len(i):
            for o, v in zip(out, _POINT3(f, eta[i], obs.y[i], obs.aux_rows(f, i), p, dtype)):
                o[i] = v
    return tuple(out)


def _point3_dispatch(family, eta, y, aux, param, dtype=LD):
    return point3(family, eta, dtype) if isinstance(family, cref.CompObs) else _POINT3(family, eta, y, aux, param, dtype)


@contextlib.contextmanager
def restated():
    """ga_pullback_ref reaches the pointwise rule through its module attribute `ref` and the third derivatives through its own global
    `point3`: both are replaced by dispatchers on a CompObs for the duration of a call"""
    assert gref.ref is ref and gref.point3 is _POINT3 and not hasattr(gref, "pointwise"), \
        "ga_pullback_ref no longer reaches fisher_ref.pointwise through `ref` / point3 through its global: restated() cannot dispatch"
    gref.ref, gref.point3 = cref._Ref(), _point3_dispatch
    try:
        yield
    finally:
        gref.ref, gref.point3 = ref, _POINT3


def split(obs, r, mutant=None):
    """param[c] from the per-row terms of a restatement"""
    tg, tp = r["Alam"] * r["gp"], r["c"] * r["dp"]
    owner = obs.comp_of_row()
    if mutant == "grid_tiles":          # 16-row tiles over the stacked rows; a tile's sum goes to the component of its first row
        owner = owner[(np.arange(len(owner)) // ROWS) * ROWS]
    if mutant == "boundary_row" and obs.ncomp > 1:
        owner = owner.copy()
        owner[obs.rowptr[1]] = 0
    out = np.array([tg[owner == k].sum() - tp[owner == k].sum() for k in range(obs.ncomp)], tg.dtype)
    if mutant == "total_for_all":
        out[:] = tg.sum() - tp.sum()
    return out


def restate(S, mu, Ad, b, obs, x, mubar, G, dtype=LD, lam=None, C=None, project=False, mutant=None):
    """ga_pullback_ref.restate for a CompObs; `param` is the vector of the components' cotangents"""
    o = obs.with_mutant(mutant if mutant in _POINT_MUTANTS else None)
    with restated():
        r = gref.restate(S, mu, Ad, b, o, x, mubar, G, dtype=dtype, lam=lam, C=C, project=project, mutant="no_dp" if mutant == "no_dp" else None)
    r["param"] = split(obs, r, mutant)
    return r


def bounds(S, Ad, b, obs, x, mubar, G, r, lam, factor=FACTOR, krow=None):
    """ga_pullback_ref.bounds for a CompObs; `param`: per component, the single-family bound over the component's rows"""
    Ad = np.asarray(Ad, LD)
    with restated():
        bd = gref.bounds(S, Ad, b, obs, x, mubar, G, r, lam, factor=factor, krow=krow)
    par = np.zeros(obs.ncomp, LD)
    n = np.shape(S)[0]
    for k, (f, p, i) in enumerate(obs.rows()):
        if f not in HAS_PARAM:
            continue
        assert ref.reduction_depth(max(n, len(i))) == ref.reduction_depth(len(i)), "the depth of c's own blocks is not what bounds() takes"
        sub = ref.Obs(f, None, obs.y[i], obs.aux_rows(f, i), p)
        rs = dict(r, **{key: r[key][i] for key in ("eta", "c", "t", "d3", "Alam", "gp", "dp")})
        par[k] = gref.bounds(S, Ad[i], None if b is None else np.asarray(b)[i], sub, x, mubar, G, rs, lam, factor=factor)["param"]
    return dict(bd, param=par)


def ratios(got, r, bd):
    """ga_pullback_ref.ratios; a value that is not finite counts as outside every bound"""
    out = gref.ratios(got, r, bd)
    return {k: (v if np.isfinite(v) else np.inf) for k, v in out.items()}


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def long_case():
    """three components of 4113, 1 and 17 rows on 48 nodes, rows of 1 to 3 entries: the first has 258 workgroups, more than the final
    kernel's 256 threads (its strided loop takes a second trip); all three have a parameter"""
    rng = np.random.default_rng(41)
    n, rowptr = 48, np.array([0, 4113, 4114, 4131])
    A = dref._rows_matrix(n, list(1 + rng.integers(0, 3, int(rowptr[-1]))), rng)
    return cref._case(ref.banded(n, 2, seed=6), A, "U", [5, 0, 4], rowptr, rng, True, False, 6)


@functools.lru_cache(maxsize=None)
def cases():
    """composite_ref.eval_cases() and `long`; read-only"""
    return dict(cref.eval_cases(), long=long_case())


@functools.lru_cache(maxsize=None)
def dense(name):
    """(S, Ad, krow, mubar, Gv, Gd) of a case: the dense prior precision and design matrix, the stored entries per row of Symmetric(Q)
    and a random pair of cotangents"""
    c = cases()[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    Gv, Gd = gref.random_cotangent(c["Q"], rng)
    return gref._sym(c["Q"], c["uplo"]), c["A"].toarray(), ref.symmetric_coo(c["Q"], c["uplo"])[3], rng.standard_normal(c["Q"].shape[0]), Gv, Gd


# ---- the Laplace objective of a joint model and its derivatives ---------------------------------------------------------------------------------
def fd_case(seed=0):
    """Normal, Gamma, NegBinomial and Poisson components (4, 5, 4 and 5 rows of 3, 1 or 2 entries, an offset) on 11 nodes under a banded
    prior; a direction dS on the prior's pattern and a direction dmu"""
    rng = np.random.default_rng(700 + seed)
    n, fam, rowptr = 11, [0, 5, 4, 1], np.array([0, 4, 9, 13, 18])
    S = np.asarray(ref.banded(n, 2, seed=seed).toarray(), LD)
    Ad = np.asarray(dref._rows_matrix(n, [3] * 16 + [1, 2], rng).toarray(), LD)
    b = rng.uniform(-0.2, 0.2, 18)
    y, aux = cref._values(fam, rowptr, rng)
    D = rng.standard_normal((n, n))
    dS = np.asarray(0.1 * (D + D.T) * (S != 0), LD)
    return dict(S=S, Ad=Ad, b=b, fam=fam, rowptr=rowptr, y=y, aux=aux, params=[LD(cref.PARAM[f]) for f in fam],
                mu=np.asarray(0.3 * rng.standard_normal(n), LD), wlin=np.asarray(rng.standard_normal(n), LD), dS=dS,
                dmu=np.asarray(rng.standard_normal(n), LD))


def _obs(k, params):
    return cref.CompObs(k["fam"], params, k["rowptr"], k["y"], k["aux"])


def _mode(k, S, mu, obs, x0):
    with restated():
        return gref.mode(S, mu, k["Ad"], k["b"], obs, x0)


def objective(k, S, mu, params, x0):
    """logpdf(prior, x*) + loglik(x*) - logpdf(posterior, x*) + wlin' x* (constants dropped), the mode re-solved in long double"""
    obs = _obs(k, params)
    x = _mode(k, S, mu, obs, x0)
    eta = k["Ad"] @ x + np.asarray(k["b"], LD)
    d = cref.pointwise(obs, eta)[1]
    Qpost = S - k["Ad"].T @ (d[:, None] * k["Ad"])
    ll = sum(gref.loglik(ref.Obs(f, None, obs.y[i], obs.aux_rows(f, i), p), eta[i], p) for f, p, i in obs.rows())
    r = x - mu
    return gref._chol_logdet(S) / 2 - (r @ (S @ r)) / 2 + ll - gref._chol_logdet(Qpost) / 2 + k["wlin"] @ x


def rule_derivatives(k, x0, mutant=None):
    """(dL/dparam[c] per component, dL/ds along S + s dS, dL/ds along mu + s dmu) by the rule: the direct terms plus the pullback of
    (mubar, Qbar) = (dL/dx*, -Q_post^-1 / 2)"""
    S, mu, Ad, obs = k["S"], k["mu"], k["Ad"], _obs(k, k["params"])
    n = S.shape[0]
    x = _mode(k, S, mu, obs, x0)
    eta = Ad @ x + np.asarray(k["b"], LD)
    g, d = cref.pointwise(obs, eta)[:2]
    Qpost = S - Ad.T @ (d[:, None] * Ad)
    G = -ref._solve(Qpost, np.eye(n, dtype=LD)) / 2
    G = (G + G.T) / 2
    r = x - mu
    mubar = k["wlin"] + (Ad.T @ g - S @ r)              # (the second term vanishes at the mode)
    R = restate(S, mu, Ad, k["b"], obs, x, mubar, G, mutant=mutant)
    direct_Q = ref._solve(S, np.eye(n, dtype=LD)) / 2 - np.outer(r, r) / 2
    dpar = np.array([gref.dloglik_dparam(ref.Obs(f, None, obs.y[i], obs.aux_rows(f, i), p), eta[i], p) for f, p, i in obs.rows()], LD) + R["param"]
    return dpar, ((direct_Q + R["Qbar_prior"]) * k["dS"]).sum(), (S @ r + R["mubar_prior"]) @ k["dmu"]
