"""Test-only helpers: near-singular (intrinsic) GMRF precisions with closed-form spectra, float64 truth by refinement,
error measures, and exact power-of-two scalings.

The intrinsic models are those of the reference package (src/latent_models/rw.jl, besag.jl, separable.jl): a singular
structure matrix S plus `regularization` on the diagonal. Here they live on periodic lattices (cycles and tori), where S is
a circulant operator: its eigenvectors are the Fourier modes and its eigenvalues have the closed forms below. The lattice is
vertex-transitive, so every diagonal entry of Sigma = Q^-1 is the same, and Sigma between two nodes depends only on their
offset.

The stored matrix is never exactly S + eps I: its diagonal is fl(c + eps). Every closed form here uses the shift that
the stored values actually carry (computed exactly from them), so the spectra are those of the float64 matrix the
kernels see, not of a nearby one that differs by 1e-6 relative in its smallest eigenvalue at eps = 1e-10."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import scipy.sparse as sp


# ---- lattices and closed-form spectra ------------------------------------------------------------------------------

def torus_laplacian(dims) -> sp.csc_matrix:
    """Graph Laplacian D - W of the periodic lattice with side lengths `dims` (every side >= 3; node index in C order,
    the last axis fastest). Integer values, so exact in float64."""
    dims = tuple(int(m) for m in dims)
    assert all(m >= 3 for m in dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims)
    r = np.concatenate([idx.ravel()] * len(dims))
    c = np.concatenate([np.roll(idx, -1, axis=d).ravel() for d in range(len(dims))])
    W = sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    W = (W + W.T).tocsc()
    return sp.csc_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W)


def _sin2(dims):
    """4 sin^2(pi k_d / m_d) on the mode grid, one array per axis (broadcastable). The sin^2 form keeps full relative
    accuracy for small k, where 2 - 2 cos(2 pi k / m) cancels."""
    out = []
    for d, m in enumerate(dims):
        shape = [1] * len(dims)
        shape[d] = m
        out.append((4.0 * np.sin(np.pi * np.arange(m) / m) ** 2).reshape(shape))
    return out


def _canonical(Q) -> sp.csc_matrix:
    Q = sp.csc_matrix(Q)
    Q.sum_duplicates()
    Q.sort_indices()
    return Q


def _diag_shift(c: float, eps: float) -> float:
    """The eps that fl(c + eps) really adds to c (exact: Sterbenz)."""
    return (c + eps) - c


@dataclass
class Model:
    """A precision matrix Q on a periodic lattice of shape `dims`, with Q's eigenvalues `lam` on the mode grid (same
    shape): Q cos(theta_k . i) = lam[k] cos(theta_k . i), theta_k = 2 pi k / dims."""
    name: str
    Q: sp.csc_matrix
    dims: tuple
    lam: np.ndarray
    eps: float

    @property
    def n(self) -> int:
        return self.Q.shape[0]

    def logdet(self) -> float:
        return math.fsum(np.log(self.lam).ravel())

    def sigma_offset(self, offset) -> float:
        """Sigma[i, i + offset] (the same for every i): mean over the modes of cos(theta_k . offset) / lam_k."""
        ph = np.zeros(self.dims)
        for d, (m, o) in enumerate(zip(self.dims, offset)):
            shape = [1] * len(self.dims)
            shape[d] = m
            ph = ph + (2.0 * np.pi * ((np.arange(m) * o) % m) / m).reshape(shape)
        return math.fsum((np.cos(ph) / self.lam).ravel()) / self.n

    def sigma_diag(self) -> float:
        return math.fsum((1.0 / self.lam).ravel()) / self.n

    def offset_pairs(self, offset):
        """(i, j) index arrays of every node i and its partner j = i + offset on the lattice"""
        idx = np.arange(self.n).reshape(self.dims)
        j = idx
        for d, o in enumerate(offset):
            j = np.roll(j, -o, axis=d)
        return idx.ravel(), j.ravel()

    def mode(self, k):
        """(x, lam_k): the Fourier mode x_i = cos(theta_k . i) (float64) and its eigenvalue"""
        grids = np.meshgrid(*[np.arange(m) for m in self.dims], indexing="ij")
        ph = sum(2.0 * np.pi * ((g * kk) % m) / m for g, kk, m in zip(grids, k, self.dims))
        return np.cos(ph).ravel(), float(self.lam[tuple(k)])


def rw1_cycle(m: int, eps: float) -> Model:
    """First-order random walk on a cycle of m nodes + eps I: eigenvalues 4 sin^2(pi k / m) + eps."""
    Q = _canonical(torus_laplacian((m,)) + eps * sp.identity(m))
    (s,) = _sin2((m,))
    return Model(f"rw1_cycle{m}", Q, (m,), s + _diag_shift(2.0, eps), eps)


def rw2_cycle(m: int, eps: float) -> Model:
    """Second-order random walk on a cycle (stencil 1 -4 6 -4 1) + eps I: eigenvalues 16 sin^4(pi k / m) + eps."""
    L = torus_laplacian((m,))
    Q = _canonical(L @ L + eps * sp.identity(m))
    (s,) = _sin2((m,))
    return Model(f"rw2_cycle{m}", Q, (m,), s * s + _diag_shift(6.0, eps), eps)


def besag_torus(dims, eps: float) -> Model:
    """Besag (intrinsic CAR) on a 2-D or 3-D torus + eps I: eigenvalues sum_d 4 sin^2(pi k_d / m_d) + eps."""
    dims = tuple(dims)
    n = int(np.prod(dims))
    Q = _canonical(torus_laplacian(dims) + eps * sp.identity(n))
    lam = sum(_sin2(dims)) + _diag_shift(2.0 * len(dims), eps)
    return Model("besag" + "x".join(map(str, dims)), Q, dims, lam, eps)


def separable_rw1_besag(T: int, m: int, eps: float, rejoin: bool = True) -> Model:
    """RW1 (cycle of T) x Besag (m x m torus), built as separable.jl builds it: kron(Q1 + eps I, Q2 + eps I), where only eps^2
    reaches the joint null space, and, since both components are constrained, + eps I again (rejoin=False leaves the diluted
    eps^2). Eigenvalues (l1 + a)(l2 + b) + g with the shifts a, b, g that the stored values carry."""
    A = torus_laplacian((T,)) + eps * sp.identity(T)
    B = torus_laplacian((m, m)) + eps * sp.identity(m * m)
    Q = sp.kron(sp.csc_matrix(A), sp.csc_matrix(B), format="csc")
    if rejoin:
        Q = Q + eps * sp.identity(T * m * m)
    Q = _canonical(Q)
    a0, b0 = 2.0 + eps, 4.0 + eps
    g = Fraction(float(Q.diagonal()[0])) - Fraction(a0) * Fraction(b0)
    assert np.all(Q.diagonal() == Q.diagonal()[0])
    s1, s2, s3 = _sin2((T, m, m))
    lam = (s1 + (a0 - 2.0)) * ((s2 + s3) + (b0 - 4.0)) + float(g)
    return Model(f"sep_rw1_{T}_besag{m}" + ("" if rejoin else "_diluted"), Q, (T, m, m), lam, eps)


# ---- models without a closed form ----------------------------------------------------------------------------------

def rw2_chain(n: int, eps: float) -> sp.csc_matrix:
    """Second-order random walk on a chain (D2' D2, the non-periodic RW2 of rw.jl) + eps I: null space of dimension 2."""
    D = sp.diags([np.ones(n - 2), -2.0 * np.ones(n - 2), np.ones(n - 2)], [0, 1, 2], shape=(n - 2, n))
    return _canonical(D.T @ D + eps * sp.identity(n))


# ---- truth by refinement, error measures -----------------------------------------------------------------------------

def refined_solve(Q, F, B, iters: int = 6) -> np.ndarray:
    """Q^-1 B for the float64 Q and B, as np.longdouble: residuals in extended precision, corrections from the float64
    factor F (anything with .solve). Accurate to about cond(Q) * 5e-20."""
    Ql = sp.csr_matrix(Q).astype(np.longdouble)
    Bl = np.asarray(B, dtype=np.longdouble)
    X = np.asarray(F.solve(np.asarray(B, dtype=np.float64)), dtype=np.longdouble)
    for _ in range(iters):
        R = Bl - Ql @ X
        dX = np.asarray(F.solve(R.astype(np.float64)), dtype=np.longdouble)
        X = X + dX
        if np.abs(dX).max() <= 1e-22 * np.abs(X).max():
            break
    return X


def rel_fwd(x, truth) -> float:
    """max |x - truth| / max |truth|, in extended precision"""
    t = np.asarray(truth, dtype=np.longdouble)
    return float(np.abs(np.asarray(x, dtype=np.longdouble) - t).max() / np.abs(t).max())


def backward_error(Q, X, B) -> float:
    """Normwise backward error of X as a solution of Q X = B, worst column: ||Q x - b|| / (||Q|| ||x|| + ||b||) in the
    infinity norm, residual in extended precision."""
    Ql = sp.csr_matrix(Q).astype(np.longdouble)
    X = np.asarray(X, dtype=np.longdouble).reshape(Q.shape[0], -1)
    B = np.asarray(B, dtype=np.longdouble).reshape(Q.shape[0], -1)
    R = np.abs(Ql @ X - B).max(axis=0)
    nQ = float(abs(sp.csr_matrix(Q)).sum(axis=1).max())
    return float((R / (nQ * np.abs(X).max(axis=0) + np.abs(B).max(axis=0))).max())


def factor_residual(Q, perm, L) -> float:
    """||P Q P' - L L'||_F / ||Q||_F in extended precision (L: lower factor in elimination order; entries above the
    diagonal are ignored)."""
    perm = np.asarray(perm)
    Ll = sp.csc_matrix(sp.tril(sp.csc_matrix(L))).astype(np.longdouble)
    PQ = sp.csc_matrix(Q)[perm][:, perm].astype(np.longdouble)
    E = (PQ - Ll @ Ll.T.tocsc()).tocsc()
    E.sum_duplicates()
    return float(np.sqrt((E.data ** 2).sum()) / np.sqrt((Q.data.astype(np.longdouble) ** 2).sum()))


# ---- exact power-of-two scalings --------------------------------------------------------------------------------------

def pow2_diag(n: int, rng, lo: int = -30, hi: int = 30) -> np.ndarray:
    """d_i = 2^k_i with k_i uniform in [lo, hi]"""
    return np.ldexp(1.0, rng.integers(lo, hi + 1, n))


def scaled_values(Q, d) -> np.ndarray:
    """The values of D Q D in Q's CSC order (exact: every factor is a power of two)."""
    Q = sp.csc_matrix(Q)
    cols = np.repeat(np.arange(Q.shape[1]), np.diff(Q.indptr))
    return Q.data * d[Q.indices] * d[cols]


def scaled(Q, d) -> sp.csc_matrix:
    """D Q D with Q's pattern and order"""
    Q = sp.csc_matrix(Q)
    return sp.csc_matrix((scaled_values(Q, d), Q.indices.copy(), Q.indptr.copy()), shape=Q.shape)


def scale_rows(M, r) -> sp.csc_matrix:
    """diag(r) M, pattern and order kept"""
    M = sp.csc_matrix(M).copy()
    M.data = M.data * r[M.indices]
    return M


def scale_cols_csr(A, d) -> sp.csr_matrix:
    """A diag(d) for a CSR A, pattern and order kept"""
    A = sp.csr_matrix(A).copy()
    A.data = A.data * d[A.indices]
    return A


def scale_both(M, r) -> sp.csc_matrix:
    """diag(r) M diag(r), pattern and order kept"""
    return scaled(M, r)


def log2_shift(d) -> float:
    """2 sum log d_i, the exact change of log det under Q -> D Q D (d powers of two: log d_i = k_i log 2)"""
    return 2.0 * math.log(2.0) * float(np.sum(np.frexp(d)[1] - 1))
