"""Problems of the batched pullback tests (gmrfx_batch_ga_pullback; tests/test_batch_ga_pullback_host.py,
tests/test_gpu_batch_ga_pullback.py), built from what exists: the evaluation cases of tests/fisher_design_ref.py, the data sets of
tests/fisher_ref.py / the plain pullback test, the member rules of tests/batch_laplace_cases.py and tests/batch_design_cases.py.
Members are Q_k = s_k Q + c_k I on the case's pattern, B = 3 (SC; a B = 1 batch takes member 1), one data set for all, a distinct
sigma / r / phi per member for families 0, 4, 5 (batch_laplace_cases.family_params).

node form  "grid": a 17 x 17 Matern grid, n = 289 > kGapNode = 256, observed on a strict subset of its nodes: two workgroups per member
           in k_gap_point_node / k_gap_param_node, so a wrong per-member offset of the partial sums or of xbar shows.
design     "mesh", "rows" (rows of 0, 1, 3, 16, 17, 33 entries; nobs = 8, no multiple of 16), "cols", "intercept" (a column of 1537 entries:
           four chunks of k_gap_chunks per member, so the per-member cpart offset is exercised).
A point x_k that is not the mode serves, as in the plain test: the rule's arithmetic is the same at any x and flag bit 1 factorises
Q_p,k - H(x_k) there (H is negative semi-definite for all six families, so Q_post,k >= Q_p,k > 0: MARGIN below).
The failing member: Q - c I in the middle, with batch_laplace_cases.fail_shift fed Q_post(x_1) - I: lambda_min(Q_post,1) = -2 <= -1."""
import numpy as np
import scipy.sparse as sp

import batch_design_cases as dc
import batch_laplace_cases as bc
import fisher_design_ref as dref
import fisher_ref as ref
import ga_pullback_ref as gref
from gmrfx import spde

K_GAP_NODE, CHUNK = 256, 512       # csrc/kernels.h: kGapNode, kDesignChunk
SC = [(1.0, 0.0), (2.5, 0.3), (0.4, 1.0)]
NAMES = ("grid", "mesh", "rows", "cols", "intercept")
MARGIN = 0.05                      # lambda_min(Q_p,k - H(x_k)) of every healthy member of every case is at least this (host test)
_DESIGN = None


def grid():
    mesh = spde.grid_mesh_2d(17, 17, jitter=0.2, seed=2)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.4))
    Q.sort_indices()
    return Q


def case(name):
    """dict(Q, uplo, A (sparse, None in node form), b)"""
    global _DESIGN
    if name == "grid":
        return dict(Q=grid(), uplo="U", A=None, b=None)
    if _DESIGN is None:
        _DESIGN = dref.eval_cases()
    return _DESIGN[name]


def problem(name, family, seed=0):
    """everything of a B = 3 problem: the members, the one data set, the per-member parameters, points, means and cotangents"""
    c = case(name)
    Q, A = c["Q"], c["A"]
    n, B = Q.shape[0], len(SC)
    rng = np.random.default_rng(1000 * family + seed + 17)
    if A is None:
        obs = ref.make_obs(family, n, rng, "subset")
        Ad = np.zeros((len(obs.idx), n))
        Ad[np.arange(len(obs.idx)), obs.idx] = 1.0
    else:
        obs = dref.make_obs(family, A.shape[0], 10 * family + 1 + seed)
        Ad = A.toarray()
    Qs = dc.members(Q, SC)
    params = bc.family_params(family, B)
    mu = np.asfortranarray(0.5 * rng.standard_normal((n, B)))
    X = np.asfortranarray(mu + 0.4 * rng.standard_normal((n, B)))
    mubar = np.asfortranarray(rng.standard_normal((n, B)))
    cot = [gref.random_cotangent(Q, rng) for _ in range(B)]
    Gv = np.asfortranarray(np.stack([g[0] for g in cot], axis=1))
    return dict(name=name, Q=Q, uplo=c["uplo"], A=A, b=c["b"], Ad=Ad, obs=obs, Qs=Qs, params=params, mu=mu, X=X, mubar=mubar, Gv=Gv,
                Gd=[g[1] for g in cot], n=n, B=B)


def member_obs(p, k):
    o = p["obs"]
    return ref.Obs(o.family, o.idx, o.y, o.aux, float(p["params"][k]))


def select(p, ks):
    """the batch of the members ks of p, in that order"""
    ks = list(ks)
    cols = lambda a: np.asfortranarray(a[:, ks])
    return dict(p, Qs=[p["Qs"][k] for k in ks], params=p["params"][ks], mu=cols(p["mu"]), X=cols(p["X"]), mubar=cols(p["mubar"]), Gv=cols(p["Gv"]),
                Gd=[p["Gd"][k] for k in ks], B=len(ks))


def post_dense(p, k, Q=None):
    """dense Q_p,k - H(x_k) = Q_p,k + A' (-D) A in float64 (Q: another precision on the pattern in member k's place)"""
    o = member_obs(p, k)
    S = dc.sym_dense(p["Qs"][k] if Q is None else Q, p["uplo"])
    eta = p["Ad"] @ p["X"][:, k] + (0 if p["b"] is None else p["b"])
    d = np.asarray(ref.pointwise(o.family, eta, o.y, o.aux, o.param)[1], float)
    return S - p["Ad"].T @ (d[:, None] * p["Ad"])


def with_failing_member(p):
    """p with member 1 replaced by Q - c I, c = batch_laplace_cases.fail_shift on Q_post(x_1) - I: lambda_min(Q_post,1) = -2"""
    c = bc.fail_shift(sp.csc_matrix(post_dense(p, 1, Q=p["Q"]) - np.eye(p["n"])))
    Qs = list(p["Qs"])
    Qs[1] = dc.shifted(p["Q"], 1.0, -c)
    return dict(p, Qs=Qs)


def intercept_chunks():
    """chunks of the longest column of the intercept case's A (design_chunks of csrc/kernels.h)"""
    A = sp.csc_matrix(case("intercept")["A"])
    longest = int(np.diff(A.indptr).max())
    return longest, (longest + CHUNK - 1) // CHUNK if longest > CHUNK else 0
