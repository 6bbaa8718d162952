"""Problems of the batched Laplace tests (gmrfx_batch_fisher_eval, gmrfx_batch_gaussian_approximation), chosen on the CPU with the
restatement of tests/fisher_ref.py (newton_loop). Members are Q_k = s_k M + c_k I on one pattern.

loop cases: "mixed" (B = 5 on the Matern matrix, Poisson lambda = 200, x0 = 0, max_iter = 7): members that stop at iterates 6, 7 (max_iter,
not converged), 5 (frozen finish), 6 (frozen finish) and 3, with 2 / 1 / 0 / 1 / 0 backtracks in iterate 1; the look-ahead fires for
members 2, 3 and 4 and never for 0 and 1, and member 4's is rejected. "negbin3": B = 3, NegBinomial with r = 0.5, 2.5, 40 on sprand_spd_60.
"one_fails": member 1 is M - c I with lambda_min(Q_p - H(x0)) <= -1, its factorisation fails at iterate 1. tests/test_batch_laplace_host.py
asserts all of this."""
import numpy as np
import scipy.sparse as sp

import fisher_loop_cases as lc
import fisher_ref as ref


def shifted(M, s, c):
    """s M + c I on M's pattern (the diagonal is stored)"""
    Q = sp.csc_matrix(s * M + c * sp.identity(M.shape[0], format="csc"))
    Q.sort_indices()
    assert np.array_equal(Q.indptr, M.indptr) and np.array_equal(Q.indices, M.indices)
    return Q


def arrowhead(n=40):
    """first row and column full (n entries), every other row two"""
    return ref.hub(n)


def tridiag(n):
    return ref.banded(n, 1)


def members(M, sc):
    return [shifted(M, s, c) for s, c in sc]


def values(Qs):
    """(nnz, B): column k = Q_k's values"""
    return np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))


MIXED_SC = [(1.0, 0.0), (30.0, 0.0), (0.05, 50.0), (200.0, 0.0), (1000.0, 50.0)]


def fail_shift(M):
    """c with lambda_min((M - c I) - H(0)) <= -1 for Poisson at x0 = 0 (H = -I): c = lambda_min(M) + 3"""
    return float(np.linalg.eigvalsh(lc.dense(M)).min()) + 3.0


def loop_cases():
    """name -> dict(M, Qs, obs (one data set), params (B), x0 (n, B), kw)"""
    M, P = lc.load("matern2d_16x16_a2"), lc.load("sprand_spd_60")
    pois = lc._poisson(256, 200.0, 1)
    out = {
        "mixed": dict(M=M, Qs=members(M, MIXED_SC), obs=pois, params=np.zeros(5), x0=np.zeros((256, 5)), kw=dict(max_iter=7)),
        "negbin3": dict(M=P, Qs=members(P, [(1.0, 0.0), (3.0, 0.5), (0.5, 2.0)]),
                        obs=ref.Obs(4, None, np.random.default_rng(7).poisson(6.0, 60).astype(float), None, 1.0),
                        params=np.array([0.5, 2.5, 40.0]), x0=np.zeros((60, 3)), kw={}),
        "one_fails": dict(M=M, Qs=[shifted(M, 1.0, 0.0), shifted(M, 1.0, -fail_shift(M)), shifted(M, 5.0, 0.0)], obs=pois, params=np.zeros(3),
                          x0=np.zeros((256, 3)), kw={}),
    }
    return out


def member_obs(c, k):
    o = c["obs"]
    return ref.Obs(o.family, o.idx, o.y, o.aux, float(c["params"][k]))


def restate(c, k, dtype):
    return ref.newton_loop(lc.dense(c["Qs"][k]), None, member_obs(c, k), x0=c["x0"][:, k], dtype=dtype, **c["kw"])


# ---- the evaluation's shapes: the smallest at which the members of fisher.hip can go wrong --------------------------------------------------
def eval_shapes():
    """name -> M: n = 1, 15, 16, 17 (tridiagonal: both sides of a workgroup of 16 rows), 40 (arrowhead: rows of 2 and of 40 entries), 60,
    256, 4097 (tridiagonal, one entry past a chunk of the reductions)"""
    out = {f"tri{n}": tridiag(n) for n in (1, 15, 16, 17, 4097)}
    out["arrow40"] = arrowhead(40)
    out["sprand60"] = lc.load("sprand_spd_60")
    out["matern256"] = lc.load("matern2d_16x16_a2")
    return out


def eval_members(M, B, seed=0):
    rng = np.random.default_rng(seed)
    return members(M, [(float(s), float(c)) for s, c in zip(rng.uniform(0.5, 2.0, B), rng.uniform(0.0, 1.0, B))])


def family_params(family, B):
    """a distinct sigma / r / phi per member (0 where the family has none)"""
    return np.linspace(0.6, 3.1, B) if family in (0, 4, 5) else np.zeros(B)
