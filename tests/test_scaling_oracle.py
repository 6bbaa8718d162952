"""Exact metamorphic relations of Q -> D Q D with D = diag(2^k_i) on the float64 CPU oracle (oracle/gmrf_oracle.c).

Multiplying by a power of two is exact, so a scale-equivariant implementation gives, bit for bit: L' = D_p L (D_p = D in
elimination order), solve'(D b) = D^-1 solve(b), backward_solve'(z) = D^-1 backward_solve(z), Sigma' = D^-1 Sigma D^-1,
tr(Sigma' D B D) = tr(Sigma B), diag(A D Sigma' D A') = diag(A Sigma A'), (D^-1 x)' Q' (D^-1 x) = x' Q x, the same failing
pivot; and log det' = log det + 2 sum log d_i up to rounding. This file shows that the relations, and the bookkeeping of D
and the permutation that tests/test_gpu_scaling.py shares, hold for a plain double implementation: a failure there is then
a property of the HIP kernels."""
import numpy as np
import pytest
import scipy.sparse as sp

import orc
import intrinsic_models as im
from gmrfx import spde


def _cases():
    rng = np.random.default_rng(5)
    m = spde.grid_mesh_2d(30, 30, jitter=0.2, seed=3)
    yield "matern30_alpha2", spde.matern_precision(m, 1, 0.4), rng.permutation(900)
    yield "rand120", spde.random_spd_precision(120, 0.05), rng.permutation(120)
    yield "dense40", sp.csc_matrix(np.cov(rng.standard_normal((40, 90))) + np.eye(40)), np.arange(40)
    yield "besag_torus_9x8", im.besag_torus((9, 8), 1e-8).Q, rng.permutation(72)
    yield "matern3d_6", spde.matern_precision(spde.grid_mesh_3d(6, 6, 6), 0, 0.5), rng.permutation(216)


CASES = list(_cases())


def _scalings(n, seed):
    rng = np.random.default_rng(seed)
    yield "diag", im.pow2_diag(n, rng)
    for k in (-150, -20, 20, 150):              # Q' = 4^k Q
        yield f"uniform4^{k}", np.full(n, np.ldexp(1.0, k))


def _logdet_tol(ld, d):
    return 1e-13 * (abs(ld) + np.abs(2.0 * np.log(d)).sum())


@pytest.mark.parametrize("name,Q,perm", CASES, ids=[c[0] for c in CASES])
def test_oracle_is_scale_equivariant(name, Q, perm):
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    n = Q.shape[0]
    F = orc.OracleFactor(Q, perm)
    L, S = F.L(), F.selinv()
    rng = np.random.default_rng(11)
    B = rng.standard_normal((n, 3))
    Z = rng.standard_normal((n, 2))
    X, Y, sd, ld = F.solve(B), F.backward_solve(Z), F.selinv_diag(), F.logdet()
    x, mu = rng.standard_normal(n), rng.standard_normal(n)
    q = orc.sqmahal(Q, x, mu)
    # a design matrix with rows inside pattern(Q) and a matrix on pattern(Q) for the contractions
    C = sp.triu(Q).tocoo()
    pick = rng.choice(len(C.row), size=min(40, len(C.row)), replace=False)
    A = sp.csr_matrix((rng.standard_normal(2 * len(pick)), (np.repeat(np.arange(len(pick)), 2),
                                                           np.stack([C.row[pick], C.col[pick]], 1).ravel())), shape=(len(pick), n))
    A.sum_duplicates()
    Bm = Q.copy()
    Bm.data = rng.standard_normal(Q.nnz)
    rd, dot = orc.row_diag_ASigmaAt(F, A), orc.selinv_dot(F, Bm)
    for tag, d in _scalings(n, 7):
        Qs = im.scaled(Q, d)
        Fs = orc.OracleFactor(Qs, perm)
        Ls = Fs.L()
        want = im.scale_rows(L, d[perm])
        assert np.array_equal(Ls.indptr, want.indptr) and np.array_equal(Ls.indices, want.indices)
        assert np.array_equal(Ls.data, want.data), tag
        assert np.array_equal(Fs.solve(B * d[:, None]), X / d[:, None]), tag
        assert np.array_equal(Fs.backward_solve(Z), Y / d[:, None]), tag
        assert np.array_equal(Fs.selinv_diag(), sd / d / d), tag
        Ss = Fs.selinv()
        assert np.array_equal(Ss.data, im.scale_both(S, 1.0 / d).data), tag
        assert orc.sqmahal(Qs, x / d, mu / d) == q
        assert orc.selinv_dot(Fs, im.scaled(Bm, d)) == dot
        assert np.array_equal(orc.row_diag_ASigmaAt(Fs, im.scale_cols_csr(A, d)), rd)
        shift = im.log2_shift(d)
        assert abs(Fs.logdet() - (ld + shift)) <= _logdet_tol(ld, d), tag


def test_failing_pivot_is_scale_invariant():
    m = spde.grid_mesh_2d(20, 20, jitter=0.2, seed=1)
    Q = sp.csc_matrix(spde.matern_precision(m, 0, 0.3))
    Q.sort_indices()
    n = Q.shape[0]
    perm = np.random.default_rng(2).permutation(n)
    col = n // 3
    k = Q.indptr[col] + int(np.searchsorted(Q.indices[Q.indptr[col]:Q.indptr[col + 1]], col))
    Q.data[k] = -abs(Q.data[k])
    fc = orc.OracleFactor(Q, perm).fail_col
    assert fc >= 0
    for _, d in _scalings(n, 3):
        assert orc.OracleFactor(im.scaled(Q, d), perm).fail_col == fc


def test_scaling_bookkeeping():
    rng = np.random.default_rng(0)
    d = im.pow2_diag(1000, rng)
    k = np.log2(d)
    assert np.all(k == np.round(k)) and k.min() == -30 and k.max() == 30
    Q = sp.csc_matrix(spde.random_spd_precision(50, 0.1))
    d = im.pow2_diag(50, rng)
    assert np.array_equal(im.scaled(Q, d).toarray(), np.diag(d) @ Q.toarray() @ np.diag(d))
    assert abs(im.log2_shift(d) - 2.0 * np.log(d).sum()) <= 1e-12 * np.abs(np.log(d)).sum()
