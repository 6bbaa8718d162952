"""References for composite likelihoods (gmrfx_obs_set_composite; csrc/fisher_design.hip: k_design_eta_comp), no device.

A composite is the design form with a family and a parameter per ROW. The restatement therefore is the design form's own
(tests/fisher_design_ref.py: eval_ref, eval_f64, bounds, newton_loop; mu_eta and v_eta of the predictive calls do not depend on the
family, but pll and the four scores do: their restatement per component is tests/composite_predictive_ref.py), run with
fisher_ref.pointwise and fisher_ref.loglik_const dispatched per component: `restated()` puts a proxy of fisher_ref in
fisher_design_ref's place for the duration of a call, which hands a CompObs to the per-component rule and everything else through.
Nothing of either module is edited. The bounds are those of fisher_design_ref.bounds: a row's g, d and l have the error of their own
family whatever the neighbouring rows hold, so the derivation there carries over term by term.

MUTANTS: deliberately wrong composites, each of which must leave the bounds on at least one case (tests/test_composite_host.py).

MEASURED (MI355X, error / bounds(r, 16) over all entries, mixed ones included, and the two scalars): RATIOS below; the joint-model loop
reached its long-double mode to 1.6e-16 against a bound of 1.7e-13."""
import contextlib

import numpy as np
import scipy.sparse as sp

import fisher_design_ref as dref
import fisher_ref as ref

LD = ref.LD
MAX_COMPONENTS = 16
READS_AUX = (1, 3, 4)
PARAM = {0: 0.7, 1: 0.0, 2: 0.0, 3: 0.0, 4: 2.5, 5: 2.0}
MUTANTS = ("boundary_row", "param0_for_all", "last_family_for_all", "aux_dropped", "const_without_last")

# largest error / bounds(r, 16) seen on the MI355X, per case: (score, hess, energy, loglik), as tests/test_gpu_composite.py prints them
RATIOS = {"cuts": (0.006, 0.004, 0.000, 0.000), "one": (0.004, 0.003, 0.000, 0.000), "same_nodes": (0.004, 0.002, 0.000, 0.000),
          "six": (0.004, 0.004, 0.000, 0.000), "sixteen": (0.005, 0.005, 0.000, 0.000)}


class CompObs:
    """the observations of a composite: family / param per component, rowptr (0-based), y and aux per row (aux None: none; NaN on the
    rows of components that have none). `family` is the object itself: what fisher_design_ref passes on to the pointwise rule."""

    def __init__(self, families, params, rowptr, y, aux, mutant=None):
        self.families, self.params, self.rowptr = list(families), list(params), np.asarray(rowptr, np.int64)
        self.y, self.aux, self.param, self.idx, self.mutant = np.asarray(y, np.float64), aux, None, None, mutant
        self.family = self

    @property
    def ncomp(self):
        return len(self.families)

    def comp_of_row(self):
        return np.repeat(np.arange(self.ncomp), np.diff(self.rowptr))

    def with_mutant(self, m):
        return CompObs(self.families, self.params, self.rowptr, self.y, self.aux, m)

    def rows(self):
        """(family, param, row indices) per component as the (possibly mutated) evaluation sees them"""
        comp = self.comp_of_row()
        fam, par = list(self.families), list(self.params)
        if self.mutant == "boundary_row" and self.ncomp > 1:        # the first row of component 1 goes to component 0
            comp = comp.copy()
            comp[self.rowptr[1]] = 0
        if self.mutant == "param0_for_all":
            par = [par[0]] * self.ncomp
        if self.mutant == "last_family_for_all":
            fam = [fam[-1]] * self.ncomp
        return [(fam[c], par[c], np.flatnonzero(comp == c)) for c in range(self.ncomp)]

    def aux_rows(self, f, i):
        if self.aux is None or f not in READS_AUX or self.mutant == "aux_dropped":
            return np.ones(len(i)) if f == 3 and self.mutant == "aux_dropped" else None
        return np.asarray(self.aux)[i]


def pointwise(obs, eta, dtype=LD):
    eta = np.asarray(eta, dtype)
    out = [np.zeros(len(eta), dtype) for _ in range(4)]
    for f, p, i in obs.rows():
        if len(i):
            for o, v in zip(out, ref.pointwise(f, eta[i], obs.y[i], obs.aux_rows(f, i), p, dtype)):
                o[i] = v
    return tuple(out)


def const_terms(obs):
    """the x-independent terms per component (long double arrays), in component order"""
    rows = obs.rows()
    if obs.mutant == "const_without_last":
        rows = rows[:-1]
    return [ref.loglik_const_terms(f, obs.y[i], obs.aux_rows(f, i), p) if len(i) else np.zeros(0, LD) for f, p, i in rows]


def loglik_const(obs):
    t = const_terms(obs)
    return sum((c.sum(dtype=LD) for c in t), LD(0)), sum((np.abs(c).sum(dtype=LD) for c in t), LD(0))


def pointwise_const(obs):
    """the constant of every observation's log density (gmrfx_obs_pointwise_const), long double"""
    out = np.zeros(len(obs.y), LD)
    for f, p, i in obs.rows():
        t = ref.loglik_const_terms(f, obs.y[i], obs.aux_rows(f, i), p)
        out[i] = t.reshape(-1, len(i)).sum(0) if len(t) else 0
    return out


class _Ref:
    """fisher_ref with the two per-family rules dispatched on a CompObs"""

    def __getattr__(self, name):
        return getattr(ref, name)

    @staticmethod
    def pointwise(family, eta, y, aux, param, dtype=LD):
        return pointwise(family, eta, dtype) if isinstance(family, CompObs) else ref.pointwise(family, eta, y, aux, param, dtype)

    @staticmethod
    def loglik_const(family, y, aux, param):
        return loglik_const(family) if isinstance(family, CompObs) else ref.loglik_const(family, y, aux, param)


@contextlib.contextmanager
def restated():
    """fisher_design_ref reaches fisher_ref through its module attribute `ref` alone (ref.pointwise, ref.loglik_const, ...): the proxy
    stands there for the duration of a call. Should fisher_design_ref ever bind one of the two rules by name instead
    (`from fisher_ref import pointwise`), a CompObs would reach the single-family rule: the assertion says so in plain words."""
    assert dref.ref is ref and not hasattr(dref, "pointwise") and not hasattr(dref, "loglik_const"), \
        "fisher_design_ref no longer reaches fisher_ref.pointwise / loglik_const through its attribute `ref`: restated() cannot dispatch"
    saved, dref.ref = dref.ref, _Ref()
    try:
        yield
    finally:
        dref.ref = saved


def _abs_aux(obs):
    """|aux| where it is read, 0 elsewhere: what eval_ref's ll_abs takes (NaN rows would poison the bound)"""
    a = np.zeros(len(obs.y))
    for f, _, i in obs.rows():
        ax = obs.aux_rows(f, i)
        if ax is not None:
            a[i] = np.abs(ax)
    return a


class _BoundObs:
    """the CompObs as eval_ref reads it: aux replaced by its magnitudes where read (eval_ref only takes |aux| of it beside the calls above)"""

    def __init__(self, obs):
        self.family, self.y, self.param, self.aux = obs, obs.y, None, _abs_aux(obs)


def eval_ref(c, x, mu, tm=None):
    with restated():
        return dref.eval_ref(c, _BoundObs(c["obs"]), x, mu, tm)


def eval_f64(c, x, mu, tm, mutant=None):
    with restated():
        return dref.eval_f64(c, c["obs"].with_mutant(mutant), x, mu, tm)


def exceeds(c, x, mu, tm, r, got, factor):
    return dref.exceeds(c, None, x, mu, tm, r, got, factor)


def newton_loop(c, dtype):
    D = c["Q"].toarray()
    S = np.triu(D) + np.triu(D, 1).T
    with restated():
        return dref.newton_loop(S, None, c["obs"], c["A"].toarray(), b=c["b"], x0=c.get("x0"), A=c.get("C"), dtype=dtype)


# ---- purity: which nodes and Hessian positions belong to one component alone ------------------------------------------------------------
def purity(c, tm=None):
    """(node_comp n, pos_comp cnt): the component whose rows alone touch column j of A / make up position p's term list; -1 mixed,
    -2 untouched"""
    A, obs = sp.csc_matrix(c["A"]), c["obs"]
    comp = obs.comp_of_row()
    tm = dref.hess_map(c["Q"], c["uplo"], c["A"]) if tm is None else tm

    def owner(ptr, rows):
        out = np.full(len(ptr) - 1, -2)
        for s in range(len(ptr) - 1):
            cs = set(comp[rows[ptr[s]:ptr[s + 1]]].tolist())
            if cs:
                out[s] = cs.pop() if len(cs) == 1 else -1
        return out
    return owner(A.indptr, A.indices), owner(tm[1], tm[2])


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _values(families, rowptr, rng, nan_elsewhere=True):
    nobs = int(rowptr[-1])
    y, aux = np.zeros(nobs), np.full(nobs, np.nan if nan_elsewhere else 0.0)
    for c, f in enumerate(families):
        o = ref.make_obs(f, int(rowptr[c + 1] - rowptr[c]), rng)
        y[rowptr[c]:rowptr[c + 1]] = o.y
        if o.aux is not None:
            aux[rowptr[c]:rowptr[c + 1]] = o.aux
    return y, (aux if any(f in READS_AUX for f in families) else None)


def _private_rows(n, families, rowptr, rng, shared0):
    """row i of component c: the component's private pair of nodes (4 c, 4 c + 1) and, on every other row, one of the shared nodes
    shared0 .. n - 1: private nodes and positions are pure, the shared ones mixed (two components at least reach each)"""
    r, cc, v = [], [], []
    for c in range(len(families)):
        for i in range(rowptr[c], rowptr[c + 1]):
            cols = [4 * c, 4 * c + 1] + ([shared0 + (i + c) % (n - shared0)] if (i - rowptr[c]) % 2 == 0 else [])
            r += [i] * len(cols)
            cc += cols
            v += list(rng.uniform(0.3, 1.0, len(cols)))
    return sp.csr_matrix((v, (r, cc)), shape=(int(rowptr[-1]), n))


def _case(Q0, A, storage, families, rowptr, rng, offset, pure, seed_pt):
    Q, u = dref.with_pattern(Q0, A, storage)
    y, aux = _values(families, rowptr, rng)
    obs = CompObs(families, [PARAM[f] for f in families], rowptr, y, aux)
    nobs, n = A.shape
    b = rng.uniform(-0.3, 0.3, nobs) if offset else None
    r2 = np.random.default_rng(seed_pt)
    return dict(Q=Q, uplo=u, A=A, b=b, obs=obs, pure=pure, x=r2.uniform(-0.6, 0.6, n), mu=r2.uniform(-0.2, 0.2, n))


def eval_cases():
    """name -> dict(Q, uplo, A, b, obs, pure, x, mu). ROWS = kDesignRows rows make a workgroup of k_design_eta_comp: the cuts between
    components sit on and beside the workgroups' edges."""
    R = dref.ROWS
    rng = np.random.default_rng(23)
    out = {}
    # one component, Poisson with exposure: the design form itself
    n, nobs = 40, 2 * R + 1
    A = dref._rows_matrix(n, [3] * nobs, rng)
    out["one"] = _case(ref.banded(n, 2, seed=1), A, "U", [1], [0, nobs], rng, True, False, 1)
    # two components on the same nodes: Normal and Poisson on identical selection rows (no pure node: every node has both)
    n, m = 40, R + 1
    nodes = np.sort(rng.choice(n, m, replace=False))
    S = sp.csr_matrix((np.ones(m), (np.arange(m), nodes)), shape=(m, n))
    out["same_nodes"] = _case(ref.banded(n, 2, seed=2), sp.vstack([S, S], format="csr"), "L", [0, 1], [0, m, 2 * m], rng, False, False, 2)
    # cuts at 1, R - 1, R, R + 1, 2 R - 1, 2 R, 2 R + 1 and nobs - 1: one-row components on either side of a workgroup's edge; an
    # empty row of A inside a component (row 20: eta = b); every family, a Binomial component between rows whose aux is NaN
    nobs = 2 * R + 8
    rowptr = np.array([0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, nobs - 1, nobs])
    fam = [0, 3, 2, 1, 5, 4, 0, 3, 1]
    n = 4 * len(fam) + 8
    A = _private_rows(n, fam, rowptr, rng, 4 * len(fam)).tolil()
    A[20, :] = 0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    out["cuts"] = _case(ref.banded(n, 2, seed=3), A, "full", fam, rowptr, rng, True, True, 3)
    # every family once, seven rows each
    fam = [0, 1, 2, 3, 4, 5]
    rowptr = np.arange(7) * 7
    n = 4 * 6 + 16
    out["six"] = _case(ref.banded(n, 3, seed=4), _private_rows(n, fam, rowptr, rng, 24), "U", fam, rowptr, rng, False, True, 4)
    # sixteen components of 1 .. 4 rows
    fam = [c % 6 for c in range(16)]
    rowptr = np.r_[0, np.cumsum([1 + c % 4 for c in range(16)])]
    n = 72
    out["sixteen"] = _case(ref.banded(n, 2, seed=5), _private_rows(n, fam, rowptr, rng, 64), "L", fam, rowptr, rng, True, True, 5)
    return out


def loop_cases():
    """a Normal + Poisson + Bernoulli joint model on a chain of 60 nodes: Normal measurements of every second node, Poisson counts
    through two-node averages, Bernoulli presence on the last 20 nodes; with and without a sum-to-zero constraint"""
    rng = np.random.default_rng(5)
    n = 60
    truth = np.sin(np.arange(n) / 6.0)
    S0 = sp.csr_matrix((np.ones(30), (np.arange(30), np.arange(0, n, 2))), shape=(30, n))
    j = rng.integers(0, n - 1, 24)
    S1 = sp.csr_matrix((np.full(48, 0.5), (np.repeat(np.arange(24), 2), np.c_[j, j + 1].ravel())), shape=(24, n))
    S2 = sp.csr_matrix((np.ones(20), (np.arange(20), np.arange(40, 60))), shape=(20, n))
    A = sp.vstack([S0, S1, S2], format="csr")
    rowptr = np.array([0, 30, 54, 74])
    y = np.r_[S0 @ truth + 0.3 * rng.standard_normal(30), rng.poisson(np.exp(S1 @ truth + 1.0)), rng.uniform(size=20) < 1 / (1 + np.exp(-(S2 @ truth)))]
    aux = np.r_[np.full(30, np.nan), np.full(24, 1.0), np.full(20, np.nan)]
    obs = CompObs([0, 1, 2], [0.3, 0.0, 0.0], rowptr, y.astype(float), aux)
    Q, u = dref.with_pattern(ref.banded(n, 2, seed=9), A, "full")
    base = dict(Q=Q, uplo=u, A=A, b=None, obs=obs, x0=None)
    return {"joint": dict(base, C=None), "joint_sum0": dict(base, C=np.ones((1, n)))}


def stacked(c, index_base=0):
    """the arguments of gmrfx_obs_set_composite for a case, as contiguous arrays"""
    o = c["obs"]
    Ac = sp.csc_matrix(c["A"])
    Ac.sort_indices()
    return dict(family=np.asarray(o.families, np.int32), param=np.asarray(o.params, np.float64), rowptr=np.ascontiguousarray(o.rowptr, np.int64),
                cp=np.ascontiguousarray(Ac.indptr, np.int64) + index_base, rv=np.ascontiguousarray(Ac.indices, np.int64) + index_base,
                nz=np.ascontiguousarray(Ac.data, np.float64), y=np.ascontiguousarray(o.y), aux=None if o.aux is None else np.ascontiguousarray(o.aux),
                b=None if c["b"] is None else np.ascontiguousarray(c["b"]))
