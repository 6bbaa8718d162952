"""The pullback of gaussian_approximation on the device (csrc/ga_pullback.hip, gmrfx_ga_pullback[_dev]).

Reference: tests/ga_pullback_ref.py -- the rule restated in np.longdouble on dense matrices, fed the handle's own lam, and the per-entry
bounds derived there (times the project's factor 16). lam itself: the normwise bound of the one-right-hand-side solve tests,
|Q_post lam - xbar| / |xbar| < 1e-10 (tests/test_gpu_parity.py); xbar, recovered as Q_post lam, is held to its own bound plus that
residual. Shapes: a 13 x 13 Matern grid observed on a strict subset of its nodes (node form) and the cases of
tests/test_gpu_fisher_design.py (fisher_design_ref.eval_cases): rows of 0, 1, 3, 16, 17 and 33 entries (561 pairs: more than a chunk),
a node observed by two rows, nobs > n, columns at every class edge, an intercept column of 1537 entries (four chunks), node counts
that are no multiple of the 16-row tiling. A point x that is not the mode serves: the rule's arithmetic is the same at any x, and
flag bit 1 factorises Q_prior - H(x) there (H is negative semi-definite for all six families)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import constraint_ref as cref
import fisher_design_ref as dref
import fisher_ref as ref
import ga_pullback_ref as gref
import gmrfx
from gmrfx import spde
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
LD = gref.LD
DESIGN = dref.eval_cases()
_BE = {}


def _grid():
    mesh = spde.grid_mesh_2d(13, 13, jitter=0.2, seed=2)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.4))
    Q.sort_indices()
    return Q


GRID = _grid()


def _case(name):
    """(Q, uplo, dense A or None, b)"""
    if name == "grid":
        return GRID, "U", None, None
    c = DESIGN[name]
    return c["Q"], c["uplo"], c["A"], c["b"]


def _backend(name):
    if name not in _BE:
        Q, uplo = _case(name)[:2]
        _BE[name] = gmrfx.MI355XBackend(Q, device=0, uplo=uplo, factorize=False)
    return _BE[name]


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    for be in _BE.values():
        be.close()
    _BE.clear()


def _setup(name, family, seed=0):
    """sets likelihood and prior on the case's handle; returns everything the restatement needs"""
    Q, uplo, A, b = _case(name)
    n = Q.shape[0]
    be = _backend(name)
    rng = np.random.default_rng(1000 * family + seed)
    if A is None:
        obs = ref.make_obs(family, n, rng, "subset")
        be.set_observations(obs.family, obs.y, obs.idx, obs.aux, obs.param)
        be.set_prior(Q.data, diag_positions(Q))
        Ad = np.zeros((len(obs.idx), n))
        Ad[np.arange(len(obs.idx)), obs.idx] = 1.0
    else:
        obs = dref.make_obs(family, A.shape[0], 10 * family + 1 + seed)
        be.set_design_observations(obs.family, obs.y, A, b, obs.aux, obs.param)
        be.set_prior(Q.data, be.observations_hess_map())
        Ad = A.toarray()
    mu = 0.5 * rng.standard_normal(n)
    x = mu + 0.4 * rng.standard_normal(n)
    mubar = rng.standard_normal(n)
    Gv, Gd = gref.random_cotangent(Q, rng)
    S = gref._sym(Q, uplo)
    krow = ref.symmetric_coo(Q, uplo)[3]
    return dict(be=be, Q=Q, S=S, Ad=Ad, b=b, obs=obs, mu=mu, x=x, mubar=mubar, Gv=Gv, Gd=Gd, krow=krow, n=n)


def _check(tag, s, got, mubar=True, G=True, project_C=None):
    """got = (Qbar_prior, mubar_prior, lam, param, check) of the handle against the restatement fed the handle's lam"""
    qp, mp, lam, par, chk = got
    mb, Gd = (s["mubar"] if mubar else None), (s["Gd"] if G else None)
    r = gref.restate(s["S"], s["mu"], s["Ad"], s["b"], s["obs"], s["x"], mb, Gd, lam=lam)
    bd = gref.bounds(s["S"], s["Ad"], s["b"], s["obs"], s["x"], mb, Gd, r, lam, krow=s["krow"])
    assert np.isfinite(lam).all()
    xb = r["xbar"]
    nx = float(np.sqrt((xb * xb).sum()))
    if project_C is None:        # (a projected lam solves another system: its own test)
        resid = r["Qpost"] @ np.asarray(lam, LD) - xb
        rel = float(np.sqrt((resid * resid).sum())) / nx
        assert rel < gref.SOLVE_RESIDUAL, rel
        assert (np.abs(resid) <= bd["xbar"] + gref.SOLVE_RESIDUAL * nx).all()
    got_d = {"param": par, "check": chk}
    if qp is not None:
        got_d["Qbar_prior"] = qp
        r = dict(r, Qbar_prior=gref.to_pattern(s["Q"], r["Qbar_prior"]))
        bd = dict(bd, Qbar_prior=gref.to_pattern(s["Q"], bd["Qbar_prior"]))
    if mp is not None:
        got_d["mubar_prior"] = mp
    rat = gref.ratios(got_d, r, bd)
    print(f"{tag}: err/bound {rat}")
    assert all(np.isfinite(np.asarray(v)).all() for v in got_d.values())
    assert max(rat.values()) <= 1.0, rat
    return r


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("name", ["grid", "mesh", "rows", "cols", "intercept", "one"])
def test_every_output_entry_by_entry(name, family):
    s = _setup(name, family)
    got = s["be"].ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], refactorize=True)
    r = _check(f"{name} family {family}", s, got)
    if name == "grid":          # unobserved nodes contribute exactly 0: xbar = mubar there
        unobs = np.setdiff1d(np.arange(s["n"]), s["obs"].idx)
        assert len(unobs) > 0 and np.array_equal(np.asarray(r["xbar"][unobs], float), s["mubar"][unobs])
    if family not in gref.HAS_PARAM:
        assert got[3] == 0.0
    again = s["be"].ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"])         # on the factor in hand, bit for bit
    assert all(same_bits(a, b) for a, b in zip(got[:3], again[:3])) and got[3:] == again[3:]


@pytest.mark.parametrize("family", [2, 3])
@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_logit_families_are_finite_at_eta_700(name, family):
    s = _setup(name, family)
    x = s["x"].copy()
    x[::2], x[1::2] = 700.0, -700.0
    if name == "mesh":
        s["be"].set_design_observations(s["obs"].family, s["obs"].y, _case(name)[2], None, s["obs"].aux, s["obs"].param)
        s["be"].set_prior(s["Q"].data, s["be"].observations_hess_map())
    qp, mp, lam, par, chk = s["be"].ga_pullback(x, s["mu"], s["mubar"], s["Gv"], refactorize=True)
    assert np.isfinite(qp).all() and np.isfinite(mp).all() and np.isfinite(lam).all() and np.isfinite([par, chk]).all()


@pytest.mark.parametrize("family", range(6))
def test_a_selection_matrix_has_the_bits_of_the_node_form(family):
    s = _setup("grid", family)
    be, obs, n = s["be"], s["obs"], s["n"]
    node = be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], refactorize=True)
    k = len(obs.idx)
    A = sp.csr_matrix((np.ones(k), (np.arange(k), obs.idx)), shape=(k, n))
    be.set_design_observations(obs.family, obs.y, A, None, obs.aux, obs.param)
    m = be.observations_hess_map()
    assert np.array_equal(m, np.sort(diag_positions(s["Q"])[obs.idx]))
    be.set_prior(s["Q"].data, m)
    des = be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], refactorize=True)
    assert all(same_bits(a, b) for a, b in zip(node[:3], des[:3])) and node[4] == des[4]
    _check(f"selection family {family}", s, des)           # (the parameter sum groups its terms by observation: held to its bound)


def _dev(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize("name", ["grid", "mesh", "intercept"])
def test_host_device_and_misaligned_forms_agree_bit_for_bit(name):
    s = _setup(name, 4)
    be, n, nnz = s["be"], s["n"], s["Q"].nnz
    host = be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], refactorize=True)
    dev = torch.device("cuda:0")
    for off in (0, 1, 3):           # doubles: offsets 1 and 3 are 8-byte aligned only
        lens = (n, n, n, nnz, nnz, n, n)
        bufs = [torch.full((k + 8,), float("nan"), dtype=torch.float64, device=dev) for k in lens]
        dx, dm, db, dq, oq, om, ol = (b[off:off + k] for b, k in zip(bufs, lens))
        for t, a in ((dx, s["x"]), (dm, s["mu"]), (db, s["mubar"]), (dq, s["Gv"])):
            t.copy_(torch.from_numpy(a))
        torch.cuda.synchronize()
        par, chk = be.ga_pullback_dev(_dev(dx), _dev(dm), _dev(db), _dev(dq), _dev(oq), _dev(om), _dev(ol))
        torch.cuda.synchronize()
        assert (par, chk) == host[3:]
        for t, a in ((oq, host[0]), (om, host[1]), (ol, host[2])):
            assert same_bits(t.cpu().numpy(), a)
        for b, k in zip(bufs[4:], lens[4:]):        # nothing is written outside the window
            assert bool(torch.isnan(torch.cat([b[:off], b[off + k:]])).all())
        # Qbar_prior written over Qbar
        par2, chk2 = be.ga_pullback_dev(_dev(dx), _dev(dm), _dev(db), _dev(dq), _dev(dq), 0, 0)
        torch.cuda.synchronize()
        assert (par2, chk2) == host[3:] and same_bits(dq.cpu().numpy(), host[0])


@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_each_nullable_argument_on_its_own(name):
    s = _setup(name, 5)
    be = s["be"]
    full = be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], refactorize=True)
    for want in ((True, False, False), (False, True, False), (False, False, True)):
        got = be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], want_Qbar_prior=want[0], want_mubar_prior=want[1], want_lambda=want[2])
        for w, a, b in zip(want, got[:3], full[:3]):
            assert (a is None) if not w else same_bits(a, b)
        assert got[3:] == full[3:]
    _check(f"{name} no Qbar", s, be.ga_pullback(s["x"], s["mu"], s["mubar"], None), G=False)
    _check(f"{name} no mubar", s, be.ga_pullback(s["x"], s["mu"], None, s["Gv"]), mubar=False)
    s0 = dict(s, mu=np.zeros(s["n"]))
    be.ga_pullback(s["x"], None, s["mubar"], s["Gv"], refactorize=True)
    _check(f"{name} no mu", s0, be.ga_pullback(s["x"], None, s["mubar"], s["Gv"]))


def _loop_problem(design):
    """the loop's cases: a Poisson likelihood on the 13 x 13 grid, by node or through three-entry rows"""
    Q = GRID
    n = Q.shape[0]
    rng = np.random.default_rng(5)
    if design:
        nobs = 200
        A = dref._rows_matrix(n, [3] * nobs, rng)
        Qd, uplo = dref.with_pattern(Q, A, "full")
    else:
        A, Qd, uplo = None, Q, "U"
    be = gmrfx.MI355XBackend(Qd, device=0, uplo=uplo, factorize=False)
    if design:
        obs = ref.Obs(1, None, rng.poisson(3.0, nobs).astype(float), None, 0.0)
        be.set_design_observations(1, obs.y, A)
        be.set_prior(Qd.data, be.observations_hess_map())
        Ad = A.toarray()
    else:
        obs = ref.make_obs(1, n, rng, "subset")
        be.set_observations(1, obs.y, obs.idx, obs.aux)
        be.set_prior(Qd.data, diag_positions(Qd))
        Ad = np.zeros((len(obs.idx), n))
        Ad[np.arange(len(obs.idx)), obs.idx] = 1.0
    return be, Qd, uplo, Ad, obs, rng


@pytest.mark.parametrize("design", [False, True])
def test_flag_bit_1_gives_the_bits_of_loop_then_pullback(design):
    be, Q, uplo, Ad, obs, rng = _loop_problem(design)
    try:
        n = Q.shape[0]
        mu = 0.1 * rng.standard_normal(n)
        x, _, info = be.gaussian_approximation(mu, refactorize_final=True)
        assert info["converged"]
        mubar = rng.standard_normal(n)
        Gv, _ = gref.random_cotangent(Q, rng)
        a = be.ga_pullback(x, mu, mubar, Gv)
        b = be.ga_pullback(x, mu, mubar, Gv, refactorize=True)
        assert all(same_bits(u, v) for u, v in zip(a[:3], b[:3])) and a[3:] == b[3:]
    finally:
        be.close()


@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_projection_with_a_sum_to_zero_constraint(name):
    s = _setup(name, 1)
    be, n = s["be"], s["n"]
    Cm = sp.csr_matrix(np.ones((1, n)))
    be.set_constraints(Cm, np.zeros(1))
    try:
        plain = be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], refactorize=True)
        proj = be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"], project=True)
        assert same_bits(plain[2], be.ga_pullback(s["x"], s["mu"], s["mubar"], s["Gv"])[2])       # bit 0 clear: the plain solve
        At, _ = be.constraint_fields()
        c = cref.prepare(Cm, np.zeros(1), At)
        rr = cref.correct(c, plain[2])
        err = np.abs(np.asarray(proj[2], LD) - rr["Xc"][:, 0])
        assert (err <= cref.bound_X(c, rr)[:, 0]).all()
        assert cref.residual_ratio(Cm, np.zeros(1), proj[2]) <= 1.0
        _check(f"{name} projected", s, proj, project_C=Cm)
    finally:
        be.clear_constraints()


def test_end_to_end_gradient_of_the_laplace_objective():
    """gaussian_approximation_dev (flag bit 3) -> logpdf_grad_dev -> ga_pullback_dev -> pattern_dot_dev for theta scaling the prior
    precision: the posterior's -logpdf(posterior, x*) term of the Laplace objective, d/dtheta [-1/2 logdet Q_post(theta)] through the mode.
    Bound: the sum of the stages' -- the loop leaves x* within its tolerance of the mode, so the restatement is evaluated AT the
    handle's x* and fed the handle's Qbar (its own test bounds it: tests/test_gpu_grad.py) and lam; what remains is this call's
    Qbar_prior bound carried through the contraction, sum_e w_e |J_e| b_e, plus the contraction's own (nnz / 4096 + 22) eps sum |terms|."""
    be, Q, uplo, Ad, obs, rng = _loop_problem(True)
    try:
        n, nnz = Q.shape[0], Q.nnz
        dev = torch.device("cuda:0")
        theta = 1.3
        be.set_prior(theta * Q.data, be.observations_hess_map())
        mu = 0.1 * rng.standard_normal(n)
        d_mu, d_x = torch.from_numpy(mu).to(dev), torch.empty(n, dtype=torch.float64, device=dev)
        d_G, d_J = torch.empty(nnz, dtype=torch.float64, device=dev), torch.from_numpy(Q.data.copy()).to(dev)
        info = be.gaussian_approximation_dev(d_x.data_ptr(), d_mu=d_mu.data_ptr(), refactorize_final=True)
        assert info["converged"]
        be.logpdf_grad_dev(d_x.data_ptr(), d_Qbar=d_G.data_ptr(), d_mu=d_x.data_ptr(), ybar=-1.0)      # cotangent of -logpdf(posterior, x*): -(Sigma / 2)
        torch.cuda.synchronize()
        Gv = d_G.cpu().numpy()
        d_lam = torch.empty(n, dtype=torch.float64, device=dev)
        be.ga_pullback_dev(d_x.data_ptr(), d_mu.data_ptr(), 0, d_G.data_ptr(), d_G.data_ptr(), 0, d_lam.data_ptr())
        got = be.pattern_dot_dev(d_G.data_ptr(), d_J.data_ptr(), nnz, 1)[0]
        x, lam = d_x.cpu().numpy(), d_lam.cpu().numpy()
        rows, cols = gref.pattern_rc(Q)
        Gd = np.zeros((n, n))
        Gd[rows, cols] = Gv
        S = LD(theta) * gref._sym(Q, uplo)
        r = gref.restate(S, mu, Ad, None, obs, x, None, Gd, lam=lam)
        bd = gref.bounds(S, Ad, None, obs, x, None, Gd, r, lam, krow=ref.symmetric_coo(Q, uplo)[3])
        wgt = np.where(rows == cols, 1.0, np.where(rows < cols, 2.0, 0.0))
        J = np.asarray(Q.data, LD)
        terms = wgt * gref.to_pattern(Q, r["Qbar_prior"]) * J
        want = terms.sum()
        bound = (wgt * np.abs(J) * gref.to_pattern(Q, bd["Qbar_prior"])).sum() + gref.FACTOR * (nnz // 4096 + 22) * gref.EPS * np.abs(terms).sum()
        print(f"end to end: dL/dtheta {got:.12e} restatement {float(want):.12e} err/bound {float(abs(got - want) / bound):.3f}")
        assert abs(got - want) <= bound
        # and the restatement's own solve agrees with the handle's to the solve bound
        resid = r["Qpost"] @ np.asarray(lam, LD) - r["xbar"]
        assert float(np.sqrt((resid * resid).sum() / (r["xbar"] * r["xbar"]).sum())) < gref.SOLVE_RESIDUAL
    finally:
        be.close()
