"""The fused evaluation of a Fisher-scoring iterate on the device (csrc/fisher.hip, gmrfx_obs_set / gmrfx_fisher_eval[_dev]).

Reference: tests/fisher_ref.py, np.longdouble (eps_ld = 2^-63, negligible beside the bounds below). eps = 2^-52.

PER-ENTRY BOUND for score_i and hess_i, with k_i the stored entries of row i of Symmetric(Q):
    16 (k_i + 4) eps (sum_j |Q_ij| |x_j| + |h_i| + |y_i| + |mu_i| (1 + |eta_i|))
Derivation. (Q x)_i is a dot product of k_i terms summed by 16 lanes and a 4-step butterfly: at most k_i roundings on any path, so
its error is <= gamma_k sum_j |Q_ij| |x_j| (Higham, Accuracy and Stability, section 3.1); h_i = (Q mu)_i likewise, its absolute sum
is represented by |h_i| for the well-conditioned rows used here. The two subtractions (Qx - h) - g add 2 eps of their results. g_i is
a few operations on y_i, and on mu_i = E[y_i] (exp / logistic of eta_i, times trials or r): the device's exp and log1p are accurate
to a few ulp, and an ulp of the ARGUMENT eta_i (+ aux_i) moves exp by |eta_i| ulp -- hence |mu_i| (1 + |eta_i|). Four more roundings
than k_i, and the project's factor 16 over a first-order bound. hess_i is made of the same mu_i and y_i.
SUMS. energy = sum_i (0.5 x_i (Qx)_i - x_i h_i) and loglik = sum_i l_i + const go through reduction_depth(n) additions on their
longest path (workgroup tree, strided loop, final tree); bounds 16 (k_max + 4 + depth) eps sum_i |x_i| (sum_j |Q_ij| (|x_j| + |mu_j|)) and
16 (4 + depth) eps (sum_i |l_i| + |y_i| (|eta_i| + |aux_i|) + |mu_i| (1 + |eta_i|) + sum |constant terms|).
Nodes without an observation: hess is +0.0 exactly and score has the bits it has under any other family (g = 0 exactly).
Bits: host and _dev forms, two runs, and operands at an 8-byte-only aligned offset of a larger buffer agree bit for bit.
Shapes and observation sets: tests/fisher_ref.py (shape_cases, make_obs); every family on every shape; all nodes / a strict unsorted
subset with 1-based indices alternate over the cases; with and without aux; no observation at all is "no likelihood": INVALID_ARG."""
import numpy as np
import pytest
import torch

import fisher_ref as ref
import gmrfx
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
EPS = ref.EPS
CASES = ref.shape_cases()
_BACKENDS = {}


def _backend(name):
    """one handle per shape case, never factorised (the evaluation needs no factorisation), prior = Q's own values"""
    if name not in _BACKENDS:
        Q, uplo = CASES[name]
        be = gmrfx.MI355XBackend(Q, device=0, uplo=uplo, factorize=False)
        be.set_prior(Q.data, diag_positions(Q))
        _BACKENDS[name] = be
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


def _set(be, obs, base=0):
    be.set_observations(obs.family, obs.y, None if obs.idx is None else obs.idx + base, obs.aux, obs.param, index_base=base)


def _check(name, be, Q, uplo, obs, x, mu):
    n = Q.shape[0]
    score, hess, en, ll = be.fisher_eval(x, mu)
    r = ref.eval_ref(Q, uplo, x, mu, obs)
    b = 16 * (r["k"] + 4) * EPS * (r["absrow"] + np.abs(r["h"]) + r["y"] + r["mean"] * (1 + r["eta"]))
    es, eh = np.abs(score - r["score"]), np.abs(hess - r["hess"])
    depth = ref.reduction_depth(n)
    be_n = 16 * (int(r["k"].max()) + 4 + depth) * EPS * r["en_abs"]
    bl = 16 * (4 + depth) * EPS * r["ll_abs"]
    print(f"{name} family {obs.family} n={n}: score err/bound {float(np.max(es / b)):.3f} hess {float(np.max(eh / b)):.3f} "
          f"energy {float(abs(en - r['energy']) / be_n):.3f} loglik {float(abs(ll - r['loglik']) / bl):.3f}")
    assert np.isfinite(score).all() and np.isfinite(hess).all()
    assert (es <= b).all() and (eh <= b).all()
    assert abs(en - r["energy"]) <= be_n
    assert abs(ll - r["loglik"]) <= bl
    assert same_bits(hess[~r["observed"]], np.zeros(int((~r["observed"]).sum())))
    return score, hess, en, ll, r


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("name", list(CASES))
def test_evaluation_entry_by_entry(name, family):
    Q, uplo = CASES[name]
    n = Q.shape[0]
    be = _backend(name)
    k = list(CASES).index(name) + family
    rng = np.random.default_rng(100 * k + family)
    subset = k % 2 == 1 and n > 1
    obs = ref.make_obs(family, n, rng, "subset" if subset else "all", with_aux=k % 3 != 0)
    _set(be, obs, base=1 if subset else 0)
    x, mu = _point(n, k)
    score, hess, en, ll, r = _check(name, be, Q, uplo, obs, x, mu)
    # two runs; outputs asked for one at a time; zero mean = no mean
    s2, h2, en2, ll2 = be.fisher_eval(x, mu)
    assert same_bits(score, s2) and same_bits(hess, h2) and (en, ll) == (en2, ll2)
    s3, none, en3, ll3 = be.fisher_eval(x, mu, want_hess=False)
    assert none is None and same_bits(score, s3) and (en, ll) == (en3, ll3)
    sz, _, enz, _ = be.fisher_eval(x, np.zeros(n))
    sn, _, enn, _ = be.fisher_eval(x, None)
    assert same_bits(sz, sn) and enz == enn
    # g = 0 exactly where nothing is observed: the same bits under another family on the same nodes
    if subset:
        other = ref.make_obs((family + 1) % 6, n, rng, "all")
        other.idx = obs.idx
        for a in ("y", "aux"):
            v = getattr(other, a)
            setattr(other, a, None if v is None else v[:len(obs.idx)])
        _set(be, other)
        so = be.fisher_eval(x, mu)[0]
        assert same_bits(so[~r["observed"]], score[~r["observed"]])


@pytest.mark.parametrize("name", ["tri17", "row16", "hub", "storedL", f"tri{ref.FINAL * ref.R + 1}"])
def test_device_form_and_alignment_give_the_same_bits(name):
    Q, uplo = CASES[name]
    n = Q.shape[0]
    be = _backend(name)
    obs = ref.make_obs(1, n, np.random.default_rng(3), "subset")
    _set(be, obs)
    x, mu = _point(n, 11)
    score, hess, en, ll = be.fisher_eval(x, mu)
    dev = torch.device("cuda:0")
    for off in (0, 1, 3):           # doubles: offsets 1 and 3 are 8-byte aligned only
        bufs = [torch.full((n + 8,), float("nan"), dtype=torch.float64, device=dev) for _ in range(4)]
        dx, dm, ds, dh = (b[off:off + n] for b in bufs)
        dx.copy_(torch.from_numpy(x))
        dm.copy_(torch.from_numpy(mu))
        torch.cuda.synchronize()
        e2, l2 = be.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())
        torch.cuda.synchronize()
        assert (e2, l2) == (en, ll)
        assert same_bits(ds.cpu().numpy(), score) and same_bits(dh.cpu().numpy(), hess)
        for b in (bufs[2], bufs[3]):     # nothing is written outside the window
            rest = torch.cat([b[:off], b[off + n:]])
            assert bool(torch.isnan(rest).all())


@pytest.mark.parametrize("family", [1, 2, 3])
def test_extreme_linear_predictors_stay_finite(family):
    name = "tri17"
    Q, uplo = CASES[name]
    n = Q.shape[0]
    be = _backend(name)
    ext = np.array([-700.0, -40.0] if family == 1 else [-700.0, -40.0, 40.0, 700.0])
    x = np.resize(ext, n)
    rng = np.random.default_rng(family)
    obs = ref.make_obs(family, n, rng, "all", with_aux=False)
    _set(be, obs)
    _check(name, be, Q, uplo, obs, x, None)


def test_refusals_and_unchanged_solves():
    Q, uplo = CASES["row17"]
    n = Q.shape[0]
    be = gmrfx.MI355XBackend(Q, device=0, uplo=uplo)
    try:
        obs = ref.make_obs(1, n, np.random.default_rng(0), "all")
        x, mu = _point(n, 5)
        _set(be, obs)
        with pytest.raises(ValueError, match="gmrfx_set_prior has not been called"):
            be.fisher_eval(x, mu)
        dp = diag_positions(Q)
        be.set_prior(Q.data, dp[:-1])
        with pytest.raises(ValueError, match="diagonal Hessians only"):
            be.fisher_eval(x, mu)
        wrong = dp.copy()
        wrong[3] = dp[3] + 1
        be.set_prior(Q.data, wrong)
        with pytest.raises(ValueError, match="diagonal Hessians only"):
            be.fisher_eval(x, mu)
        be.set_prior(Q.data, dp)
        be.set_observations(1, np.zeros(0))          # nothing observed = no likelihood
        with pytest.raises(ValueError, match="no observation likelihood"):
            be.fisher_eval(x, mu)
        # the Newton entry point gives the same bits before and after the handle has carried a likelihood
        rhs = np.random.default_rng(1).standard_normal(n)
        hv = -np.random.default_rng(2).uniform(0.1, 1.0, n)
        X0 = be.refactorize_update_solve(hv, rhs)
        _set(be, obs)
        score, hess, en, ll = be.fisher_eval(x, mu)
        X1 = be.refactorize_update_solve(hv, rhs)
        assert same_bits(X0, X1)
        # the evaluation leaves the factorisation alone, and its outputs are the operands of one Newton step
        s2 = be.fisher_eval(x, mu)[0]
        assert same_bits(s2, score)
        step = be.refactorize_update_solve(hess, score)
        S = np.triu(Q.toarray()) + np.triu(Q.toarray(), 1).T
        want = np.linalg.solve(S - np.diag(hess), score)
        assert np.abs(step - want).max() <= 1e-10 * np.abs(want).max()
        # a clone carries the likelihood (not the prior's values)
        cl = be.clone()
        try:
            assert cl.observations_info() == be.observations_info()
            cl.set_prior(Q.data, dp)
            sc, hc, ec, lc = cl.fisher_eval(x, mu)
            assert same_bits(sc, score) and same_bits(hc, hess) and (ec, lc) == (en, ll)
        finally:
            cl.close()
    finally:
        be.close()
