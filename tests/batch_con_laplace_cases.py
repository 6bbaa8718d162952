"""Problems of the constrained batched Laplace tests (gmrfx_batch_constrained_gaussian_approximation), chosen on the CPU with the
restatements of tests/fisher_ref.py and tests/fisher_design_ref.py (newton_loop(..., A=...), which project every step as the reference's
_workspace_constrain_with_matrix does). Members are Q_k = s_k M + c_k I on one pattern; ONE constraint A x = 0 for all members; x0 = 0, so
every iterate satisfies the constraint up to rounding. Each case is the smallest at which its code path can go wrong:

  rw1_B1/2/3   rw1_cycle(12): n = 12, m = 1 (the vector path of k_con_apply, m < 4), B = 1, 2, 3
  besag        besag_torus((9, 7), 1e-6): n = 63, sum to zero, the scalings of batch_laplace_cases.MIXED_SC, counts of zero_mean_counts:
               members stop at iterates 7, 8, 9, 7, 5 with 2 / 3 / 3 / 1 / 0 backtracks, member 2 alone through the frozen finish (the
               masks of the projection differ from iterate to iterate); besag50: B = 50 scalings on a log grid
  m13_m4/m5    matern2d_13x13_a3_structural_zeros: n = 169 (no multiple of 64), m = 4, 5 sparse random rows (MFMA path, MQ = 1, 2), B = 3
  m16_m5/m64   matern2d_16x16_a2: n = 256, m = 5, 64 (MQ = 2, 16), B = 3
  design       the smallest design case of tests/batch_design_cases.py with an intercept (n = 257 nodes with the intercept; its 17 x 17
               relatives do not exist: intercept_far0 is the one there is), sum to zero on the field, the intercept free, B = 3
  equal_rows   rw1_cycle(12) with two equal rows of A: W_k is singular for every member, cinfo = 2
  one_fails    besag with a batch_laplace_cases.fail_shift member between healthy ones (the shift taken RATE - 1 further: H(0) = -RATE I
               with the exposure of zero_mean_counts, so that lambda_min(Q_p - H(0)) = -2 and the first factorisation fails)

The MFMA-path rows are sparse random rows on disjoint column blocks (tests/constraint_edges.py: block_rows) with cond(W_k) <= KAPPA_MAX for
every member at x0, checked on the CPU by tests/test_batch_con_laplace_host.py."""
import numpy as np
import scipy.sparse as sp

import batch_design_cases as bdc
import batch_laplace_cases as bc
import constraint_edges as ce
import fisher_design_ref as dref
import fisher_loop_cases as lc
import fisher_ref as ref
import intrinsic_models as im

KAPPA_MAX = ce.KAPPA_MAX


def block_rows(n, m, seed):
    return sp.csr_matrix(ce.block_rows(n, m, np.random.default_rng(seed)))


def _node(M, sc, obs, A, **kw):
    B = len(sc)
    return dict(M=M, Qs=bdc.members(M, sc), obs=obs, params=np.zeros(B), x0=np.zeros((M.shape[0], B)), A=sp.csr_matrix(A), kw=kw, design=None)


SC3 = [(1.0, 0.0), (30.0, 0.0), (0.05, 50.0)]


RATE = 20.0


def zero_mean_counts(n, seed, sd=2.0, rate=RATE):
    """Poisson counts whose log rate is log(rate) (the exposure, aux) plus a field of mean zero: data a sum-to-zero model can follow, so
    that the steps are of the size of the modes (the residual bound is stated in |x|), and rough enough (sd = 2) for the line search
    to backtrack from x0 = 0"""
    rng = np.random.default_rng(seed)
    z = sd * rng.standard_normal(n)
    z -= z.mean()
    return ref.Obs(1, None, rng.poisson(rate * np.exp(z)).astype(float), np.full(n, np.log(rate)), 0.0)


def cases():
    """name -> dict(M, Qs, obs, params, x0 (n, B), A (m x n CSR, e = 0), kw, design (the base case of dref.loop_cases or None))"""
    out = {}
    R = im.rw1_cycle(12, 1e-6).Q
    pr = ref.Obs(1, None, [2, 1, 3, 0, 4, 1, 2, 3, 5, 0, 1, 2], None, 0.0)
    for B in (1, 2, 3):
        out[f"rw1_B{B}"] = _node(R, SC3[:B], pr, np.ones((1, 12)))
    Bq = im.besag_torus((9, 7), 1e-6).Q
    pois63 = zero_mean_counts(63, 3)
    out["besag"] = _node(Bq, bc.MIXED_SC, pois63, np.ones((1, 63)))
    out["besag50"] = _node(Bq, [(float(s), 0.0) for s in np.logspace(-1, 2, 50)], pois63, np.ones((1, 63)))
    M13, M16 = lc.load("matern2d_13x13_a3_structural_zeros"), lc.load("matern2d_16x16_a2")
    for m in (4, 5):
        out[f"m13_m{m}"] = _node(M13, SC3, lc._poisson(169, 3.0, 2), block_rows(169, m, m))
    for m in (5, 64):
        out[f"m16_m{m}"] = _node(M16, SC3, lc._poisson(256, 3.0, 3), block_rows(256, m, m))
    d = bdc.loop_cases()["intercept_far0"]
    n = d["Qs"][0].shape[0]
    Ad = sp.csr_matrix(np.r_[np.ones(n - 1), 0.0][None, :])
    out["design"] = dict(M=d["base"]["Q"], Qs=d["Qs"], obs=d["obs"], params=d["params"], x0=d["x0"], A=Ad, kw={}, design=d["base"])
    out["equal_rows"] = _node(R, SC3, pr, np.ones((2, 12)))
    out["one_fails"] = dict(_node(Bq, SC3, pois63, np.ones((1, 63))),
                            Qs=[bdc.shifted(Bq, 1.0, 0.0), bdc.shifted(Bq, 1.0, -(bc.fail_shift(Bq) + RATE - 1.0)), bdc.shifted(Bq, 5.0, 0.0)])
    return out


def member_obs(c, k):
    o = c["obs"]
    return ref.Obs(o.family, o.idx, o.y, o.aux, float(c["params"][k]))


def dense(c, k):
    return bdc.sym_dense(c["Qs"][k], c["design"]["uplo"]) if c["design"] else lc.dense(c["Qs"][k])


def restate(c, k, dtype, **kw):
    """member k alone: the reference's loop with every step projected onto A s = 0"""
    kw = {**c["kw"], **kw}
    A = c["A"].toarray()
    if c["design"]:
        b = c["design"]
        return dref.newton_loop(dense(c, k), None, member_obs(c, k), b["A"].toarray(), b=b["b"], x0=c["x0"][:, k], A=A, dtype=dtype, **kw)
    return ref.newton_loop(dense(c, k), None, member_obs(c, k), x0=c["x0"][:, k], A=A, dtype=dtype, **kw)


def post_dense(c, k, x):
    """Q_p,k - H(x), dense (Poisson and its relatives through ref.pointwise)"""
    S = dense(c, k)
    o = member_obs(c, k)
    if c["design"]:
        Ad = c["design"]["A"].toarray()
        b = c["design"]["b"]
        eta = Ad @ x + (0.0 if b is None else b)
        d = ref.pointwise(o.family, eta, o.y, o.aux, o.param, np.float64)[1]
        return S - Ad.T @ (d[:, None] * Ad)
    idx = np.arange(S.shape[0]) if o.idx is None else np.asarray(o.idx)
    d = np.zeros(S.shape[0])
    d[idx] = ref.pointwise(o.family, np.asarray(x, float)[idx], o.y, o.aux, o.param, np.float64)[1]
    return S - np.diag(d)


def cond_W(c, k, x=None):
    """cond_2 of W_k = A (Q_p,k - H(x))^-1 A' (x = x0 by default)"""
    A = c["A"].toarray()
    W = A @ np.linalg.solve(post_dense(c, k, c["x0"][:, k] if x is None else x), A.T)
    return float(np.linalg.cond(W))


def residual_bound(c, x, iters):
    """64 eps (iters + 1) max_r (|A| |x|)_r: every projected step leaves a residual of a few eps |A| |s|, and there are at most
    iters + 1 of them (the frozen finish's three count as its one iterate: their steps are of the size of the last decrement)"""
    return 64 * ref.EPS * (iters + 1) * float((abs(c["A"]) @ np.abs(x)).max())
