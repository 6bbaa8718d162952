"""The pullback of gaussian_approximation, what needs no device (tests/ga_pullback_ref.py; gmrfx_ga_pullback and gmrfx_obs_design_rows on
symbolic_only handles).

1. Finite differences. objective() = the Laplace marginal likelihood logpdf(prior, x*) + loglik(x*) - logpdf(posterior, x*) plus a
   linear functional of the mode (so that the mean cotangent is not zero), the prior precision scaled by theta, the mode re-solved in
   long double by 40 Newton steps (converged to ~1e-19, far below the steps). The restatement's total derivative by theta and by the
   family's parameter against central differences with relative steps H1 = 1e-3 and H2 = 5e-4.
   MEASURED HERE (CPU, np.longdouble, all six families, node and design form): the relative discrepancy at H2 is at most 1.92e-6
   (the Normal family's sigma, node form; theta: at most 2.3e-7) and H1's is 4.00 times H2's in every case. Asserted: FD_BOUND = 1.92e-5,
   that figure with a tenfold margin, and a ratio between 3 and 5. The precision cotangent is contracted with dQ/dtheta as
   gmrfx_pattern_dot does (one triangle, off-diagonal entries twice). Every named mutant breaks the bound.
2. The float64 control stays inside the per-entry bounds WITHOUT their factor 16; every mutant leaves them with it.
3. The C ABI's refusals, in the header's order, and NO_DEVICE behind them.
4. The plan's transposed term table against a brute-force construction."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fisher_design_ref as dref
import fisher_ref as ref
import ga_pullback_ref as gref
from gmrfx._lib import GmrfxOpts, lib, ptr

LD = gref.LD
INVALID_ARG = 1
H1, H2, FD_BOUND = 1e-3, 5e-4, 1.92e-5


def _fd(f, at, h):
    return (f(at * (1 + LD(h))) - f(at * (1 - LD(h)))) / (2 * at * LD(h))


def _fd_case(family, design):
    S0, mu, A, b, obs, wlin = gref.small_case(family, design=design)
    theta = LD(1.3)
    x0 = gref.mode(theta * S0, mu, A, b, obs, mu)
    return S0, mu, A, b, obs, wlin, theta, x0


@pytest.mark.parametrize("design", [False, True])
@pytest.mark.parametrize("family", range(6))
def test_total_derivative_against_central_differences(family, design):
    S0, mu, A, b, obs, wlin, theta, x0 = _fd_case(family, design)
    dth, dpar = gref.rule_derivatives(S0, theta, mu, A, b, obs, wlin, x0)
    checks = [("theta", dth, lambda t: gref.objective(S0, t, mu, A, b, obs, obs.param, wlin, x0)[0], theta)]
    if family in gref.HAS_PARAM:
        checks.append(("param", dpar, lambda p: gref.objective(S0, theta, mu, A, b, obs, p, wlin, x0)[0], LD(obs.param)))
    for name, rule, f, at in checks:
        e1, e2 = (abs(_fd(f, at, h) - rule) / abs(rule) for h in (H1, H2))
        print(f"family {family} design {design} d/d{name}: rule {float(rule):.12e} rel. discrepancy h1 {float(e1):.3e} h2 {float(e2):.3e} ratio {float(e1 / e2):.2f}")
        assert e2 <= FD_BOUND
        assert e1 < 1e-12 or 3 < e1 / e2 < 5


@pytest.mark.parametrize("mutant", gref.MUTANTS)
def test_every_mutant_breaks_the_finite_difference_bound(mutant):
    S0, mu, A, b, obs, wlin, theta, x0 = _fd_case(4, True)
    Cc = np.ones((1, S0.shape[0]), LD)
    dth, dpar = gref.rule_derivatives(S0, theta, mu, A, b, obs, wlin, x0, mutant=mutant, C=Cc)
    fth = _fd(lambda t: gref.objective(S0, t, mu, A, b, obs, obs.param, wlin, x0)[0], theta, H2)
    fpa = _fd(lambda p: gref.objective(S0, theta, mu, A, b, obs, p, wlin, x0)[0], LD(obs.param), H2)
    worst = max(abs(fth - dth) / abs(fth), abs(fpa - dpar) / abs(fpa))
    print(f"{mutant}: rel. discrepancy {float(worst):.3e}")
    assert worst > FD_BOUND


def _bound_case(family, design, seed=3):
    S0, mu, A, b, obs, wlin = gref.small_case(family, seed=seed, design=design)
    rng = np.random.default_rng(seed)
    n = S0.shape[0]
    x = np.asarray(mu, float) + 0.4 * rng.standard_normal(n)
    G = rng.standard_normal((n, n))
    G = (G + G.T) / 2
    mubar = rng.standard_normal(n)
    return S0, mu, A, b, obs, x, mubar, G


@pytest.mark.parametrize("design", [False, True])
@pytest.mark.parametrize("family", range(6))
def test_float64_control_inside_the_bounds_and_mutants_outside(family, design):
    S0, mu, A, b, obs, x, mubar, G = _bound_case(family, design)
    Cc = np.ones((1, S0.shape[0]))
    full = gref.restate(S0, mu, A, b, obs, x, mubar, G)
    lam64 = np.asarray(full["lam"], np.float64)           # one lam for both: the solve is not what is bounded
    r = gref.restate(S0, mu, A, b, obs, x, mubar, G, lam=lam64)
    bd1 = gref.bounds(S0, A, b, obs, x, mubar, G, r, lam64, factor=1)
    ctl = gref.restate(S0, mu, A, b, obs, x, mubar, G, dtype=np.float64, lam=lam64)
    rat = gref.ratios({k: ctl[k] for k in ("xbar", "Qbar_prior", "mubar_prior", "param", "check")}, r, bd1)
    print(f"family {family} design {design}: control err/bound {rat}")
    assert max(rat.values()) <= 1.0
    bd = gref.bounds(S0, A, b, obs, x, mubar, G, r, lam64)
    for mutant in gref.MUTANTS:
        if mutant == "no_dp" and family not in gref.HAS_PARAM:
            continue
        if mutant == "no_factor_2" and not design:
            continue                    # (a node-form row has no off-diagonal pair)
        if mutant == "d3_sign" and family == 0:
            continue                    # (d3 = 0)
        # a mutant that changes lam is judged on lam' xbar and on what follows from its own lam
        m = gref.restate(S0, mu, A, b, obs, x, mubar, G, mutant=mutant, C=Cc)
        bad = gref.ratios({k: m[k] for k in ("xbar", "Qbar_prior", "mubar_prior", "param")}, full, bd)
        print(f"  {mutant}: err/bound {max(bad.values()):.3e}")
        assert max(bad.values()) > 1.0, mutant


# ---- the C ABI on symbolic_only handles -----------------------------------------------------------------------------------------------------
class _Handle:
    def __init__(self, Q, uplo="U", batched=0):
        self.Q, self.uplo, self.batched = Q, uplo, batched

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        o.uplo = 0 if self.uplo == "U" else 1
        cp, ri = np.ascontiguousarray(self.Q.indptr, np.int64), np.ascontiguousarray(self.Q.indices, np.int64)
        if self.batched:
            rc = lib().gmrfx_create_batched(self.Q.shape[0], ptr(cp), ptr(ri), 0, None, self.batched, C.byref(o), C.byref(self.h))
        else:
            rc = lib().gmrfx_create(self.Q.shape[0], ptr(cp), ptr(ri), 0, None, C.byref(o), C.byref(self.h))
        assert rc == 0 and self.h.value, lib().gmrfx_last_create_error()
        return self.h

    def __exit__(self, *exc):
        lib().gmrfx_destroy(self.h)


def _msg(h):
    return lib().gmrfx_last_error(h).decode()


def _call(h, n, nnz, x=True, mubar=True, Qbar=True, flags=0, outs=(True, True, True), out=True, dev=False):
    a = lambda on, k: np.zeros(k) if on else None
    fn = lib().gmrfx_ga_pullback_dev if dev else lib().gmrfx_ga_pullback
    return fn(h, ptr(a(x, n)), None, ptr(a(mubar, n)), ptr(a(Qbar, nnz)), flags, ptr(a(outs[0], nnz)), ptr(a(outs[1], n)), ptr(a(outs[2], n)),
              ptr(a(out, 2)))


def test_refusals_on_symbolic_only_handles():
    Q = ref.banded(8, 1)
    n, nnz = 8, Q.nnz
    y = np.ones(n)
    with _Handle(Q) as h:
        assert _call(h, n, nnz) == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert lib().gmrfx_obs_set(h, 1, n, None, 0, ptr(y), None, 0.0) == 0
        no_device = lib().gmrfx_fisher_eval(h, ptr(np.zeros(n)), None, None, None, ptr(np.zeros(2)))
        assert no_device not in (0, INVALID_ARG)
        for kw, what in ((dict(x=False), "x is null"), (dict(out=False), "out is null"), (dict(flags=4), "unknown flag bits"),
                         (dict(flags=-1), "unknown flag bits"), (dict(mubar=False, Qbar=False), "both null"),
                         (dict(outs=(False, False, False)), "every output is null"), (dict(flags=1), "needs a constraint")):
            for dev in (False, True):
                assert _call(h, n, nnz, dev=dev, **kw) == INVALID_ARG, kw
                assert what in _msg(h), (kw, _msg(h))
        # behind the argument checks: no device, with or without the refactorisation bit, each nullable argument on its own
        for kw in (dict(), dict(flags=2), dict(mubar=False), dict(Qbar=False), dict(outs=(True, False, False)), dict(outs=(False, False, True))):
            assert _call(h, n, nnz, **kw) == no_device, kw
        # with a constraint bit 0 passes the argument checks
        rp, ci, v, e = np.array([0, n], np.int64), np.arange(n, dtype=np.int64), np.ones(n), np.zeros(1)
        assert lib().gmrfx_constraints_set(h, 1, ptr(rp), ptr(ci), ptr(v), 0, ptr(e)) == 0
        assert _call(h, n, nnz, flags=1) == no_device
        assert lib().gmrfx_ga_pullback(None, None, None, None, None, 0, None, None, None, None) == INVALID_ARG
    with _Handle(Q, batched=2) as h:
        assert _call(h, n, nnz) == INVALID_ARG and "batched" in _msg(h)


@pytest.mark.parametrize("name", ["mesh", "rows", "one"])
def test_transposed_term_table_against_brute_force(name):
    c = dref.eval_cases()[name]
    A = sp.csc_matrix(c["A"])
    A.sort_indices()
    nobs = A.shape[0]
    with _Handle(c["Q"], c["uplo"]) as h:
        cp, rv, nz = (np.ascontiguousarray(a, t) for a, t in ((A.indptr, np.int64), (A.indices, np.int64), (A.data, np.float64)))
        assert lib().gmrfx_obs_set_design(h, 1, nobs, ptr(cp), ptr(rv), ptr(nz), 0, None, ptr(np.ones(nobs)), None, 0.0) == 0, _msg(h)
        terms = C.c_int64(0)
        assert lib().gmrfx_obs_design_info(h, None, None, C.byref(terms)) == 0
        p, pos, w = np.full(nobs + 1, -1, np.int64), np.full(terms.value, -1, np.int64), np.full(terms.value, np.nan)
        assert lib().gmrfx_obs_design_rows(h, ptr(p), ptr(pos), ptr(w)) == 0
    bp, bpos, bw = gref.term_rows_brute(c["Q"], c["uplo"], c["A"])
    assert np.array_equal(p, bp) and np.array_equal(pos, bpos) and np.array_equal(w, bw)
    rows = np.diff(sp.csr_matrix(c["A"]).indptr)
    assert np.array_equal(np.diff(p), rows * (rows + 1) // 2)
    for i in range(nobs):
        assert (np.diff(pos[p[i]:p[i + 1]]) > 0).all()


def test_no_design_rows_without_a_design():
    with _Handle(ref.banded(8, 1)) as h:
        assert lib().gmrfx_obs_design_rows(h, None, None, None) == INVALID_ARG and "no design likelihood" in _msg(h)
