"""The evaluation of a Fisher-scoring iterate through a sparse design matrix on the device (csrc/fisher_design.hip,
gmrfx_obs_set_design / gmrfx_fisher_eval[_dev] in design form).

Reference: tests/fisher_design_ref.py, np.longdouble (eps_ld = 2^-63, negligible beside the bounds). eps = 2^-52; first-order bounds
(Higham, Accuracy and Stability, section 3.1: a sum of m terms formed in any order has error <= gamma_m sum |terms|), times the
project's factor 16. With r_i the entries of row i of A, c_j those of column j, T_p the terms of position p:
  eta_i     e_eta_i = (r_i + 1) eps (sum_k |A_ik| |x_k| + |b_i|): r_i fused multiply-adds on any path, one addition of b_i.
  g_i, d_i  e_pt_i = 4 eps (|y_i| + L_i (1 + |eta_i|)) + L_i e_eta_i. The first term is the pointwise term of tests/test_gpu_fisher.py
            (a few operations on y_i and on the mean mu_i = E[y_i], whose argument's ulp moves exp by |eta_i| ulp), the second carries
            the error of eta through: dg/deta = d and |d3 l / deta3| <= |d| for all six families, so both g and d move by at most
            L_i e_eta_i with L_i = max(mu_i, |d_i|) (mu_i itself for Poisson, Bernoulli and binomial, as in the node form's bound).
  (A' g)_j  (c_j + depth + 2) eps sum_i |A_ij| |g_i| + sum_i |A_ij| e_pt_i: at most c_j roundings on a lane's chain, `depth` more in
            the butterfly (4) and, for a chunked column, the chunk's tree (8) and the chain over the chunk sums (ceil(chunks / 16)).
  score_j   the node form's term for (Q x)_j - h_j, (k_j + 4) eps (sum |Q_jk| |x_k| + |h_j|), plus that of (A' g)_j.
  hess[p]   (T_p + depth + 1) eps sum_t |w_t| |d_{i_t}| + sum_t |w_t| e_pt_{i_t}: as a column, one rounding more for w_t = A_ij A_ik.
  energy    as the node form: (k_max + 4 + reduction_depth(n)) eps sum_j |x_j| sum_k |Q_jk| (|x_k| + |mu_k|).
  loglik    (4 + reduction_depth(nobs)) eps (sum_i |l_i| + |y_i| (|eta_i| + |aux_i|) + mu_i (1 + |eta_i|) + sum |constants|)
            + sum_i |g_i| e_eta_i (dl/deta = g).
tests/test_fisher_design_host.py checks on the CPU that a float64 numpy evaluation stays inside these bounds WITHOUT the factor 16 and
that five named wrong evaluations leave them with it, and that the cases below reach the edges they claim.
Bits: the host and _dev forms, two runs, and operands at an 8-byte-only aligned offset agree bit for bit; for a selection matrix
without offset, score, energy and hess at the observed nodes have the bits of the node form."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fisher_design_ref as dref
import fisher_ref as ref
import gmrfx
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
CASES = dref.eval_cases()
_BACKENDS, _TM = {}, {}


def _backend(name):
    """one handle per case, never factorised by the evaluation tests; the prior's values: Q's own"""
    if name not in _BACKENDS:
        c = CASES[name]
        _BACKENDS[name] = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=False)
        _TM[name] = dref.hess_map(c["Q"], c["uplo"], c["A"])
    return _BACKENDS[name]


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    for be in _BACKENDS.values():
        be.close()
    _BACKENDS.clear()


def _point(n, seed):
    rng = np.random.default_rng(seed)
    return 0.8 * rng.standard_normal(n), 0.5 * rng.standard_normal(n)


def _set(be, c, obs):
    be.set_design_observations(obs.family, obs.y, c["A"], c["b"], obs.aux, obs.param)
    m = be.observations_hess_map()
    be.set_prior(c["Q"].data, m)
    return m


def _check(name, be, c, obs, x, mu, tm):
    score, hess, en, ll = be.fisher_eval(x, mu)
    r = dref.eval_ref(c, obs, x, mu, tm)
    bs, bh, b_en, b_ll = dref.bounds(r, 16)[:4]
    es, eh = np.abs(score - r["score"]), np.abs(hess - r["hess"])
    tiny = ref.LD(1e-300)
    print(f"{name} family {obs.family}: score err/bound {float(np.max(es / (bs + tiny))):.3f} hess {float(np.max(eh / (bh + tiny))) if len(eh) else 0.0:.3f} "
          f"energy {float(abs(en - r['energy']) / b_en):.3f} loglik {float(abs(ll - r['loglik']) / b_ll):.3f}")
    assert np.isfinite(score).all() and np.isfinite(hess).all() and len(hess) == len(tm[0])
    assert (es <= bs).all() and (eh <= bh).all()
    assert abs(en - r["energy"]) <= b_en and abs(ll - r["loglik"]) <= b_ll
    return score, hess, en, ll


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("name", list(CASES))
def test_evaluation_entry_by_entry(name, family):
    c = CASES[name]
    be = _backend(name)
    obs = dref.make_obs(family, c["A"].shape[0], 10 * family + 1)
    m = _set(be, c, obs)
    assert np.array_equal(m, _TM[name][0])
    x, mu = _point(c["Q"].shape[0], family)
    score, hess, en, ll = _check(name, be, c, obs, x, mu, _TM[name])
    s2, h2, en2, ll2 = be.fisher_eval(x, mu)
    assert same_bits(score, s2) and same_bits(hess, h2) and (en, ll) == (en2, ll2)
    s3, none, en3, ll3 = be.fisher_eval(x, mu, want_hess=False)
    assert none is None and same_bits(score, s3) and (en, ll) == (en3, ll3)
    none, h4, en4, ll4 = be.fisher_eval(x, mu, want_score=False)
    assert none is None and same_bits(hess, h4) and (en, ll) == (en4, ll4)


@pytest.mark.parametrize("name", ["mesh", "cols", "intercept"])
def test_device_form_and_alignment_give_the_same_bits(name):
    c = CASES[name]
    n = c["Q"].shape[0]
    be = _backend(name)
    obs = dref.make_obs(1, c["A"].shape[0], 3)
    cnt = len(_set(be, c, obs))
    x, mu = _point(n, 11)
    score, hess, en, ll = be.fisher_eval(x, mu)
    dev = torch.device("cuda:0")
    for off in (0, 1, 3):           # doubles: offsets 1 and 3 are 8-byte aligned only
        lens = (n, n, n, cnt)
        bufs = [torch.full((k + 8,), float("nan"), dtype=torch.float64, device=dev) for k in lens]
        dx, dm, ds, dh = (b[off:off + k] for b, k in zip(bufs, lens))
        dx.copy_(torch.from_numpy(x))
        dm.copy_(torch.from_numpy(mu))
        torch.cuda.synchronize()
        e2, l2 = be.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())
        torch.cuda.synchronize()
        assert (e2, l2) == (en, ll)
        assert same_bits(ds.cpu().numpy(), score) and same_bits(dh.cpu().numpy(), hess)
        for b, k in ((bufs[2], n), (bufs[3], cnt)):      # nothing is written outside the window
            assert bool(torch.isnan(torch.cat([b[:off], b[off + k:]])).all())


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("name", ["tri17", "row17", "hub", "storedL"])
def test_a_selection_matrix_has_the_bits_of_the_node_form(name, family):
    Q, uplo = ref.shape_cases()[name]
    n = Q.shape[0]
    rng = np.random.default_rng(family)
    obs = ref.make_obs(family, n, rng, "subset")
    k = len(obs.idx)
    A = sp.csr_matrix((np.ones(k), (np.arange(k), obs.idx)), shape=(k, n))
    x, mu = _point(n, family + 20)
    be = gmrfx.MI355XBackend(Q, device=0, uplo=uplo, factorize=False)
    try:
        dp = diag_positions(Q)
        be.set_observations(obs.family, obs.y, obs.idx, obs.aux, obs.param)
        be.set_prior(Q.data, dp)
        s0, h0, e0, l0 = be.fisher_eval(x, mu)
        be.set_design_observations(obs.family, obs.y, A, None, obs.aux, obs.param)
        m = be.observations_hess_map()
        assert np.array_equal(m, np.sort(dp[obs.idx]))
        with pytest.raises(ValueError, match="not the map of gmrfx_obs_hess_map"):
            be.fisher_eval(x, mu)           # (the diagonal map of the node form is not the design form's)
        be.set_prior(Q.data, m)
        s1, h1, e1, l1 = be.fisher_eval(x, mu)
        node_of = {int(dp[j]): j for j in obs.idx}
        assert same_bits(s1, s0) and e1 == e0
        assert same_bits(h1, h0[[node_of[int(p)] for p in m]])
        r = ref.eval_ref(Q, uplo, x, mu, obs)
        assert abs(l1 - r["loglik"]) <= 16 * (4 + ref.reduction_depth(k)) * ref.EPS * r["ll_abs"]       # (another tree: k rows, not n)
        be.set_observations(obs.family, obs.y, obs.idx, obs.aux, obs.param)       # and back: the node form again, bit for bit
        be.set_prior(Q.data, dp)
        s2, h2, e2, l2 = be.fisher_eval(x, mu)
        assert same_bits(s2, s0) and same_bits(h2, h0) and (e2, l2) == (e0, l0)
    finally:
        be.close()


@pytest.mark.parametrize("family", [2, 3])
def test_extreme_linear_predictors_stay_finite(family):
    name = "mesh"
    c = dict(CASES[name])
    nobs = c["A"].shape[0]
    c["b"] = np.resize(np.array([-700.0, -40.0, 40.0, 700.0]), nobs)
    be = _backend(name)
    obs = dref.make_obs(family, nobs, family)
    obs.aux = None if family == 2 else obs.aux
    _set(be, c, obs)
    x, _ = _point(c["Q"].shape[0], 1)
    _check(name, be, c, obs, x, None, _TM[name])


def test_a_design_matrix_without_entries():
    """eta = b, cnt = 0: an empty Hessian vector, score = Q_p x - h exactly as the node pass forms it, loglik from b alone"""
    c = dict(CASES["mesh"])
    nobs, n = 5, c["Q"].shape[0]
    c["A"], c["b"] = sp.csr_matrix((nobs, n)), np.linspace(-1.0, 1.0, nobs)
    obs = dref.make_obs(1, nobs, 2)
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=False)
    try:
        assert len(_set(be, c, obs)) == 0
        x, mu = _point(n, 4)
        tm = dref.hess_map(c["Q"], c["uplo"], c["A"])
        score, hess, en, ll = _check("empty", be, c, obs, x, mu, tm)
        assert hess.shape == (0,)
        xm, hm, info = be.gaussian_approximation(mean=mu)       # the likelihood does not see x: the mode is the prior mean
        assert hm.shape == (0,) and info["converged"] and np.abs(xm - mu).max() <= 1e-12
    finally:
        be.close()


@pytest.mark.parametrize("name", ["mesh", "intercept"])
def test_the_hessian_values_are_those_of_the_host_route(name):
    """gmrfx_refactorize_update with the returned hess = gmrfx_refactorize of Q_p - A' D A: bit for bit against the values scattered on
    the host (the comparison tests/test_gpu_parity.py makes for gmrfx_refactorize_update), and against a dense host assembly"""
    c = CASES[name]
    Q, uplo, A = c["Q"], c["uplo"], c["A"]
    n = Q.shape[0]
    obs = dref.make_obs(1, A.shape[0], 5)
    be = gmrfx.MI355XBackend(Q, device=0, uplo=uplo, factorize=False)
    other = gmrfx.MI355XBackend(Q, device=0, uplo=uplo, factorize=False)
    try:
        m = _set(be, c, obs)
        x, mu = _point(n, 9)
        score, hess, _, _ = be.fisher_eval(x, mu)
        assert be.refactorize_update(hess) == 0
        nz = Q.data.copy()
        nz[m] -= hess
        other.refactorize_values(nz)
        assert np.array_equal(be.factor_values(), other.factor_values()) and be.compute_logdet() == other.compute_logdet()
        D = Q.toarray()
        S = np.triu(D) + np.triu(D, 1).T if uplo == "U" else np.tril(D) + np.tril(D, -1).T
        eta = A @ x + (0 if c["b"] is None else c["b"])
        d = np.asarray(ref.pointwise(1, eta, obs.y, obs.aux, obs.param, np.float64)[1])
        Ad = A.toarray()
        want = np.linalg.slogdet(S - Ad.T @ (d[:, None] * Ad))[1]
        assert abs(be.compute_logdet() - want) <= 1e-10 * abs(want)
    finally:
        be.close()
        other.close()
