"""Dense numpy restatement of the log-density gradients on Q's pattern (include/gmrfx.h "Log-density gradients"), for the tests:

    logpdf(z)      = -r'Qr/2 + logdet(Q)/2 - n log(2 pi)/2,                  r = z - mu
    correction     = (m log(2 pi) + logdet W + s' W^-1 s)/2 - logdet(A A')/2,  s = e - A mu,  W = A Q^-1 A'
    Qbar           = c (Sigma - r r') - c (B B' - u u'),   c = ybar/2,  B = At L_c^-T,  At = Sigma A',  u = B L_c^-1 s
    mubar          = ybar Q r - ybar A' W^-1 s
    out[k]         = sum_e w_e G[e] J[e, k]

The constraint terms are written once for any floating type (`constraint_terms`): with np.longdouble and the hand-written m x m
Cholesky below they are the yardstick the float64 version -- and the device -- is measured against."""
import numpy as np
import scipy.sparse as sp

EPS = np.finfo(np.float64).eps


def weights(Q, mode):
    """w_e of the stored entries of csc Q: 1 on the diagonal; "L" / "U": 2 in that strict triangle, 0 in the other; "full": 1 everywhere
    (both triangles define Q)"""
    Q = sp.csc_matrix(Q)
    cols = np.repeat(np.arange(Q.shape[1]), np.diff(Q.indptr))
    rows = Q.indices
    if mode == "full":
        return np.ones(Q.nnz)
    used = rows > cols if mode == "L" else rows < cols
    return np.where(rows == cols, 1.0, np.where(used, 2.0, 0.0))


def symmetric_dense(Q, mode):
    """the dense matrix the stored values define: Symmetric(Q, mode) for "L" / "U", Q itself for "full" """
    D = sp.csc_matrix(Q).toarray()
    if mode == "full":
        return D
    T = np.tril(D, -1) if mode == "L" else np.triu(D, 1)
    return T + T.T + np.diag(np.diag(D))


def cholesky_lower(W):
    """hand-written Cholesky of a small dense matrix in W's own dtype: L with L L' = W"""
    m = W.shape[0]
    L = np.zeros_like(W)
    for j in range(m):
        d = W[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert d > 0
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            L[i, j] = (W[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def lower_inverse(L):
    m = L.shape[0]
    X = np.zeros_like(L)
    for j in range(m):
        X[j, j] = 1 / L[j, j]
        for i in range(j + 1, m):
            X[i, j] = -(L[i, j:i] * X[j:i, j]).sum() / L[i, i]
    return X


def constraint_terms(At, W, A, e, mu, dtype=np.float64):
    """(BBt - uu' as a dense n x n array, its absolute sum |B||B|' + |u||u|', A' W^-1 s, its absolute sum) in `dtype`, from the
    operands a handle keeps: At = Q^-1 A' (n x m) and W = A At"""
    At = np.asarray(At, dtype=dtype)
    W = np.asarray(W, dtype=dtype)
    Ad = np.asarray(A.toarray() if sp.issparse(A) else A, dtype=dtype)
    s = np.asarray(e, dtype=dtype) - Ad @ np.asarray(mu, dtype=dtype)
    Li = lower_inverse(cholesky_lower(W))
    B = At @ Li.T
    t = Li @ s
    u = B @ t
    w = Li.T @ t
    return B @ B.T - np.outer(u, u), np.abs(B) @ np.abs(B).T + np.outer(np.abs(u), np.abs(u)), Ad.T @ w, np.abs(Ad).T @ np.abs(w)


def logpdf_dense(Qd, z, mu, A=None, e=None):
    n = Qd.shape[0]
    r = z - mu
    val = -0.5 * r @ Qd @ r + 0.5 * np.linalg.slogdet(Qd)[1] - 0.5 * n * np.log(2 * np.pi)
    if A is not None and A.shape[0] > 0:
        Ad = A.toarray() if sp.issparse(A) else np.asarray(A)
        m = Ad.shape[0]
        W = Ad @ np.linalg.solve(Qd, Ad.T)
        s = e - Ad @ mu
        val += 0.5 * (m * np.log(2 * np.pi) + np.linalg.slogdet(W)[1] + s @ np.linalg.solve(W, s)) - 0.5 * np.linalg.slogdet(Ad @ Ad.T)[1]
    return val


def grad_dense(Qd, z, mu, ybar=1.0, A=None, e=None):
    """(Qbar dense n x n, mubar) of logpdf_dense at cotangent ybar"""
    Sigma = np.linalg.inv(Qd)
    r = z - mu
    c = 0.5 * ybar
    Qbar = c * (Sigma - np.outer(r, r))
    mubar = ybar * (Qd @ r)
    if A is not None and A.shape[0] > 0:
        Ad = A.toarray() if sp.issparse(A) else np.asarray(A)
        At = Sigma @ Ad.T
        T, _, av, _ = constraint_terms(At, Ad @ At, Ad, e, mu)
        Qbar = Qbar - c * T
        mubar = mubar - ybar * av
    return Qbar, mubar


def on_pattern(D, Q):
    """the entries of dense D at the stored positions of csc Q, in storage order"""
    Q = sp.csc_matrix(Q)
    cols = np.repeat(np.arange(Q.shape[1]), np.diff(Q.indptr))
    return D[Q.indices, cols]


def pattern_dot(Q, mode, G, J):
    w = weights(Q, mode)
    return (w * G) @ J


def sum_to_zero(n, m):
    """m sum-to-zero rows over disjoint groups of nodes (a well-conditioned W), as a csr matrix, and e"""
    rows, cols = [], []
    edges = np.linspace(0, n, m + 1).astype(int)
    for k in range(m):
        cols += list(range(edges[k], edges[k + 1]))
        rows += [k] * (edges[k + 1] - edges[k])
    A = sp.csr_matrix((np.ones(len(cols)), (rows, cols)), shape=(m, n))
    return A, 0.1 * np.cos(np.arange(m))
