"""The closed forms of tests/intrinsic_models.py against dense arbitrary-precision arithmetic (mpmath, 50 digits) on the very
float64 matrices the GPU tests factor, at n <= 100: log det, Sigma_ii, Sigma between lattice neighbours and the quadratic
form of a Fourier mode, down to eps = 1e-10. Also checks that the extended-precision refinement reaches the closed-form
solve of a Fourier mode and that the error measures see a planted error."""
import math

import mpmath as mp
import numpy as np
import pytest
import scipy.sparse as sp

import orc
import intrinsic_models as im


def _mp_cholesky(Q):
    """lower Cholesky factor of the dense float64 matrix Q, every value converted exactly"""
    A = Q.toarray()
    n = A.shape[0]
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        s = mp.mpf(A[j, j]) - mp.fsum(L[j][k] ** 2 for k in range(j))
        assert s > 0
        L[j][j] = mp.sqrt(s)
        for i in range(j + 1, n):
            L[i][j] = (mp.mpf(A[i, j]) - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    return L


def _mp_solve(L, b):
    n = len(L)
    y = [mp.mpf(0)] * n
    for i in range(n):
        y[i] = (mp.mpf(b[i]) - mp.fsum(L[i][k] * y[k] for k in range(i))) / L[i][i]
    x = [mp.mpf(0)] * n
    for i in reversed(range(n)):
        x[i] = (y[i] - mp.fsum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
    return x


def _models():
    for eps in (1e-5, 1e-8, 1e-10):
        yield im.rw1_cycle(60, eps), (1,)
        yield im.rw2_cycle(40, eps), (1,)
        yield im.besag_torus((9, 11), eps), (0, 1)
        yield im.besag_torus((4, 5, 4), eps), (1, 0, 0)
    yield im.separable_rw1_besag(4, 5, 1e-5), (1, 0, 0)
    yield im.separable_rw1_besag(3, 5, 1e-3), (0, 0, 1)
    yield im.separable_rw1_besag(4, 5, 1e-5, rejoin=False), (0, 1, 0)


MODELS = list(_models())


@pytest.mark.parametrize("model,offset", MODELS, ids=[f"{m.name}-eps{m.eps:g}" for m, _ in MODELS])
def test_closed_forms_match_dense_multiprecision(model, offset):
    mp.mp.dps = 50
    Q = model.Q
    n = model.n
    assert n <= 100 and (abs(Q - Q.T) > 0).nnz == 0
    L = _mp_cholesky(Q)
    logdet = 2 * mp.fsum(mp.log(L[j][j]) for j in range(n))
    assert abs(model.logdet() - float(logdet)) <= 1e-14 * abs(float(logdet)) + 1e-13
    # a whole column of Sigma: the diagonal entry and the partner at `offset`
    e0 = [0.0] * n
    e0[0] = 1.0
    s0 = _mp_solve(L, e0)
    i, j = model.offset_pairs(offset)
    assert i[0] == 0
    assert abs(model.sigma_diag() - float(s0[0])) <= 1e-13 * abs(float(s0[0]))
    want = float(s0[int(j[0])])
    assert abs(model.sigma_offset(offset) - want) <= 1e-13 * abs(float(s0[0]))
    # the lattice is vertex-transitive: another node has the same diagonal entry
    k = n // 2 + 1
    ek = [0.0] * n
    ek[k] = 1.0
    assert abs(_mp_solve(L, ek)[k] - s0[0]) <= mp.mpf(10) ** -30 * abs(s0[0])
    # a Fourier mode: x' Q x = lam_k ||x||^2 (x exactly as stored)
    kk = tuple(1 if d == 0 else 0 for d in range(len(model.dims)))
    x, lam = model.mode(kk)
    Qd = Q.toarray()
    quad = mp.fsum(mp.mpf(x[a]) * mp.mpf(Qd[a, b]) * mp.mpf(x[b]) for a, b in zip(*np.nonzero(Qd)))
    assert abs(lam * math.fsum(x * x) - float(quad)) <= 1e-14 * abs(float(quad))
    # the smallest eigenvalue is the nominal shift up to the rounding of the stored diagonal: eps, or eps^2 + eps for the
    # separable model (eps^2 when the joint eps I is left out)
    e = model.eps
    nominal = e * e if model.name.endswith("_diluted") else e * e + e if model.name.startswith("sep") else e
    assert abs(model.lam.min() - nominal) <= 2e-15


def test_shift_is_the_stored_one_not_the_nominal_one():
    # at eps = 1e-10 the nominal eps differs from what fl(4 + eps) adds by ~1e-6 relative: the closed forms use the latter
    m = im.besag_torus((6, 6), 1e-10)
    assert m.lam.min() == (4.0 + 1e-10) - 4.0 != 1e-10
    assert abs(m.lam.min() / 1e-10 - 1.0) > 1e-8


@pytest.mark.parametrize("eps", [1e-5, 1e-10])
def test_refinement_reaches_the_closed_form_solve(eps):
    model = im.besag_torus((24, 24), eps)
    Q, n = model.Q, model.n
    F = orc.OracleFactor(Q)
    x1, lam1 = model.mode((1, 0))
    x0, lam0 = model.mode((0, 0))
    b = x1 + x0                                      # the constant mode: Q^-1 b ~ 1 / eps there
    X = im.refined_solve(Q, F, b)
    want = np.asarray(x1, np.longdouble) / np.longdouble(lam1) + np.asarray(x0, np.longdouble) / np.longdouble(lam0)
    # the truth is as good as the extended-precision residual allows (b is exact here: the modes are 1 and cos(2 pi i / 24))
    cond = model.lam.max() / model.lam.min()
    assert im.rel_fwd(X, want) <= 1e-19 * cond + 1e-15
    assert im.backward_error(Q, X, b) <= 1e-18
    # and the float64 oracle's solve is worse than the truth by what its conditioning allows, not by more
    assert im.rel_fwd(F.solve(b), X) <= 1e-15 * model.lam.max() / model.lam.min()


def test_error_measures_see_a_planted_error():
    model = im.rw1_cycle(50, 1e-5)
    Q = model.Q
    F = orc.OracleFactor(Q)
    b = np.random.default_rng(0).standard_normal(model.n)
    x = F.solve(b)
    assert im.backward_error(Q, x, b) < 1e-15
    x2 = x.copy()
    x2[7] *= 1 + 1e-12
    assert im.backward_error(Q, x2, b) > 1e-14
    L = F.L()
    assert im.factor_residual(Q, np.arange(model.n), L) < 1e-15
    L2 = L.copy()
    L2.data[3] *= 1 + 1e-12
    assert im.factor_residual(Q, np.arange(model.n), L2) > 1e-14
