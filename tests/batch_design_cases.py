"""Problems of the batched design-form tests (gmrfx_batch_obs_set_design, gmrfx_batch_fisher_eval and gmrfx_batch_gaussian_approximation through
eta = A x + b), built from what exists: the evaluation and loop cases of tests/fisher_design_ref.py and the member rules of
tests/batch_laplace_cases.py. Members are Q_k = s_k Q + c_k I on the pattern of the case's Q, explicit zeros kept (the positions of
pattern(A'A) must stay stored, so the values are scaled in place instead of going through sparse arithmetic).

Loop cases (chosen on the CPU with the float64 restatement dref.newton_loop; tests/test_batch_design_host.py asserts all of it):
every member of every case satisfies dref.far_from_thresholds. "one_fails": member 1 is Q - c I with
lambda_min(Q_p + A'A) = -2 at x0 = 0 (Poisson: H(0) = -A'A), between two healthy members."""
import numpy as np
import scipy.sparse as sp

import batch_laplace_cases as bc
import fisher_design_ref as dref
import fisher_ref as ref
from layout_buffers import diag_positions


def shifted(Q, s, c):
    """s Q + c I with Q's stored pattern, explicit zeros included (batch_laplace_cases.shifted for a pattern that holds them)"""
    out = sp.csc_matrix((s * Q.data, Q.indices.copy(), Q.indptr.copy()), shape=Q.shape)
    out.data[diag_positions(Q)] += c
    return out


def members(Q, sc):
    return [shifted(Q, s, c) for s, c in sc]


def sym_dense(Q, uplo):
    """the dense symmetric matrix the handle sees: the triangle in use, mirrored"""
    D = Q.toarray()
    return np.triu(D) + np.triu(D, 1).T if uplo == "U" else np.tril(D) + np.tril(D, -1).T


def fail_shift(c):
    """shift with lambda_min((Q - shift I) + A'A) = -2 <= -1: batch_laplace_cases.fail_shift on Q + A'A - I (its rule adds H(0) = -I)"""
    Ad = c["A"].toarray()
    return bc.fail_shift(sp.csc_matrix(sym_dense(c["Q"], c["uplo"]) + Ad.T @ Ad - np.eye(Ad.shape[1])))


# member scalings (s_k, c_k) per loop case of dref.loop_cases(); see test_batch_design_host.py for what they have to show
# mesh_far0: members stop at iterates 6, 6 (frozen finish), 4 (frozen finish, no backtrack) and 8 (frozen finish), with 2 / 1 / 0 / 1
# backtracks; mesh_far8: nobody backtracks, member 0 takes the frozen finish, members 1 and 2 do not; intercept_far0: iterates 7
# (frozen), 5 and 5 (frozen)
LOOP_SC = {
    "mesh_far0": [(1.0, 0.0), (200.0, 0.0), (1000.0, 50.0), (0.05, 50.0)],
    "mesh_far8": [(1.0, 0.0), (0.05, 50.0), (1000.0, 50.0)],
    "intercept_far0": [(1.0, 0.0), (0.05, 50.0), (1000.0, 50.0)],
}


def loop_cases():
    """name -> dict(base (the case of dref.loop_cases), Qs, obs, params (B), x0 (n, B), kw)"""
    base = dref.loop_cases()
    out = {}
    for name, sc in LOOP_SC.items():
        c = base[name]
        n = c["Q"].shape[0]
        x0 = np.zeros(n) if c["x0"] is None else c["x0"]
        out[name] = dict(base=c, Qs=members(c["Q"], sc), obs=c["obs"], params=np.zeros(len(sc)), x0=np.repeat(x0[:, None], len(sc), axis=1), kw={})
    c = base["mesh_far0"]
    n = c["Q"].shape[0]
    out["one_fails"] = dict(base=c, Qs=[shifted(c["Q"], 1.0, 0.0), shifted(c["Q"], 1.0, -fail_shift(c)), shifted(c["Q"], 30.0, 0.0)], obs=c["obs"],
                            params=np.zeros(3), x0=np.zeros((n, 3)), kw={})
    return out


def member_obs(c, k):
    o = c["obs"]
    return ref.Obs(o.family, o.idx, o.y, o.aux, float(c["params"][k]))


def restate(c, k, dtype, **kw):
    b = c["base"]
    return dref.newton_loop(sym_dense(c["Qs"][k], b["uplo"]), None, member_obs(c, k), b["A"].toarray(), b=b["b"], x0=c["x0"][:, k], dtype=dtype,
                            **{**c["kw"], **kw})


def member_case(c, Q):
    """the evaluation / loop case of dref with another member's Q"""
    return dict(c, Q=Q)


# ---- the evaluation -----------------------------------------------------------------------------------------------------------------------
def eval_members(Q, B, seed=0):
    """B members s_k Q + c_k I, s in [0.5, 2], c in [0, 1] (the rule of batch_laplace_cases.eval_members)"""
    rng = np.random.default_rng(seed)
    return members(Q, [(float(s), float(c)) for s, c in zip(rng.uniform(0.5, 2.0, B), rng.uniform(0.0, 1.0, B))])


def selection_case(n=37, seed=3):
    """A = rows of the identity (an observed subset, in scrambled order), no offset, on a banded Q: the design form must give the bits of
    the node form"""
    rng = np.random.default_rng(seed)
    Q = ref.banded(n, 3, seed=5)
    idx = rng.permutation(n)[:n - 9]
    A = sp.csr_matrix((np.ones(len(idx)), (np.arange(len(idx)), idx)), shape=(len(idx), n))
    return Q, idx, A


def empty_case(n=20, nobs=5):
    """a design matrix without a stored entry: cnt = 0, eta = b, Q_post = Q_p"""
    Q = ref.banded(n, 2, seed=2)
    return dict(Q=Q, uplo="U", A=sp.csr_matrix((nobs, n)), b=np.linspace(-0.2, 0.2, nobs))
