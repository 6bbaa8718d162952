"""Linear equality constraints A x = e computed on the device (include/gmrfx.h: gmrfx_constraints_*, gmrfx_sample; kernels in
csrc/constraint.hip) against the dense kriging formulas (Rue & Held 2005, 2.3.3; restated from
tests/test_seam_a_and_constraints.py::_dense_constrained), against the host mirror of the reference's ConstraintInfo / WorkspaceGMRF
(tests/mirror/workspace_gmrf.py), for bit-reproducibility, over the handle's life cycle, on intrinsic models with closed forms,
and at the benchmark's size. Every case prints its figures (pytest -rP shows them)."""
import math
import time

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import intrinsic_models as im
from gmrfx import spde
from gmrfx._lib import PosDefException
from mirror import GMRFWorkspace
from mirror.workspace_gmrf import WorkspaceGMRF

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def matern(nx, ny, seed=3):
    m = spde.grid_mesh_2d(nx, ny, jitter=0.2, seed=seed)
    return m, sp.csc_matrix(spde.matern_precision(m, 0, 0.4))


def constraint_rows(n, m, seed):
    """One dense sum-to-zero row plus m - 1 sparse random rows, e != 0."""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n))
    A[0] = 1.0
    for r in range(1, m):
        idx = rng.choice(n, size=7, replace=False)
        A[r, idx] = rng.standard_normal(7)
    return A, rng.standard_normal(m)


def _dense_constrained(Qd, mu, A, e):
    Sigma = np.linalg.inv(Qd)
    SAt = Sigma @ A.T
    W = A @ SAt
    mean_c = mu - SAt @ np.linalg.solve(W, A @ mu - e)
    Sigma_c = Sigma - SAt @ np.linalg.solve(W, SAt.T)
    return Sigma, SAt, W, mean_c, Sigma_c


@pytest.mark.parametrize("m", [1, 3, 4, 17, 64])
def test_against_dense_kriging(m):
    mesh, Q = matern(24 + m % 5, 21, seed=8 + m)
    n = Q.shape[0]
    rng = np.random.default_rng(m)
    A, e = constraint_rows(n, m, seed=100 + m)
    mu = rng.standard_normal(n)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    be.set_constraints(sp.csr_matrix(A), e)
    info = be.constraint_info()
    assert info["m"] == m and be.stats()["last_nrhs"] == m            # the one blocked solve
    Sigma, SAt, W, mean_c, Sigma_c = _dense_constrained(Q.toarray(), mu, A, e)
    At, Wd = be.constraint_fields()
    ldW = np.linalg.slogdet(W)[1]
    mc, lcorr = be.constrained_mean(mu)
    resid = e - A @ mu
    lref = 0.5 * (m * np.log(2.0 * np.pi) + ldW + resid @ np.linalg.solve(W, resid)) - 0.5 * np.linalg.slogdet(A @ A.T)[1]
    v = be.constrained_var()
    figs = dict(At=relerr(At, SAt), W=relerr(Wd, W), logdetW=abs(info["logdet_W"] - ldW) / abs(ldW), mean=relerr(mc, mean_c),
                Ax_e=float(np.abs(A @ mc - e).max()), logcorr=abs(lcorr - lref) / abs(lref),
                var=float(np.abs(v - np.diag(Sigma_c)).max()), prep_ms=info["ms"])
    print(f"m={m} n={n}", {k: f"{x:.3g}" for k, x in figs.items()})
    assert figs["At"] < 1e-10 and figs["W"] < 1e-10 and figs["mean"] < 1e-10
    assert figs["logdetW"] < 1e-9 and figs["logcorr"] < 1e-9
    assert figs["Ax_e"] <= 1e-9
    assert np.allclose(v, np.diag(Sigma_c), rtol=1e-7, atol=1e-12) and v.min() >= 0.0
    # mu = None is the zero mean
    mc0, _ = be.constrained_mean()
    assert relerr(mc0, _dense_constrained(Q.toarray(), np.zeros(n), A, e)[3]) < 1e-10


@pytest.mark.parametrize("shape,m", [((23, 21), 1), ((23, 21), 3), ((31, 27), 17), ((26, 24), 4)])
def test_correction_and_sample_against_the_host_mirror(shape, m):
    """constraint_correct / sample against WorkspaceGMRF.rand_from on the same Z, 1e-12 relative; odd n (23 x 21, 31 x 27)."""
    import torch
    mesh, Q = matern(*shape, seed=5)
    n = Q.shape[0]
    rng = np.random.default_rng(7)
    A, e = constraint_rows(n, m, seed=3 * m)
    mu = rng.standard_normal(n)
    ws = GMRFWorkspace(Q, coords=mesh.points)
    d = WorkspaceGMRF(mu, Q, ws, sp.csr_matrix(A), e)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    be.set_constraints(sp.csr_matrix(A), e)
    dev = torch.device("cuda", 0)
    for nvec in (1, 5, 16, 17, 64, 70, 256):
        Z = rng.standard_normal((n, nvec))
        ref = d.rand_from(Z)
        X = be.sample(Z, mean=mu)
        Y = be.backend_backward_solve(Z).reshape(n, nvec) + mu[:, None]
        Xc = be.constraint_correct(Y)
        r1, r2 = relerr(X, ref), relerr(Xc, ref)
        res = float(np.abs(A @ X - e[:, None]).max()), float(np.abs(A @ Xc - e[:, None]).max())
        print(f"n={n} m={m} nvec={nvec}: sample {r1:.2e} correct {r2:.2e} residuals {res[0]:.2e} {res[1]:.2e}")
        assert r1 < 1e-12 and r2 < 1e-12
        assert max(res) <= 1e-9
        # device-pointer forms = host forms, bit for bit; with ldx > n and an unaligned column start (odd offset of 8 bytes)
        for ld, off in ((n, 0), (n + 3, 1)):
            buf = torch.zeros(ld * nvec + off + 1, dtype=torch.float64, device=dev)
            view = buf[off:off + ld * nvec].view(nvec, ld)
            view[:, :n] = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
            torch.cuda.synchronize()
            be.constraint_correct_dev(buf.data_ptr() + 8 * off, ld, nvec)
            got = view[:, :n].cpu().numpy().T
            assert np.array_equal(got, Xc), (nvec, ld, off)
            assert float(buf[off + n:off + ld].abs().max()) == 0.0 if ld > n else True       # the padding is untouched
            dz = torch.from_numpy(np.ascontiguousarray(Z.T)).to(dev)
            dmu = torch.from_numpy(mu).to(dev)
            buf.zero_()
            torch.cuda.synchronize()
            be.sample_dev(dz.data_ptr(), n, nvec, buf.data_ptr() + 8 * off, ld, dmu.data_ptr())
            assert np.array_equal(view[:, :n].cpu().numpy().T, X), (nvec, ld, off)
        # run to run
        assert np.array_equal(be.sample(Z, mean=mu), X) and np.array_equal(be.constraint_correct(Y), Xc)
    if m == 3:
        z = rng.standard_normal(n)
        assert relerr(be.sample(z, mean=mu), d.rand_from(z[:, None])[:, 0]) < 1e-12


def test_reproducible_and_transparent_without_a_constraint():
    mesh, Q = matern(25, 23, seed=2)
    n = Q.shape[0]
    rng = np.random.default_rng(0)
    A, e = constraint_rows(n, 5, seed=9)
    mu = rng.standard_normal(n)
    Z = rng.standard_normal((n, 19))
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    # without a constraint: the existing entry points' bits
    assert be.constraint_info()["m"] == 0
    assert np.array_equal(be.sample(Z), be.backend_backward_solve(Z))
    assert np.array_equal(be.constrained_var(), be.get_selinv_diag())
    assert np.array_equal(be.constraint_correct(Z), Z)
    assert np.array_equal(be.sample(Z, mean=mu), be.backend_backward_solve(Z) + mu[:, None])
    mc, lc = be.constrained_mean(mu)
    assert np.array_equal(mc, mu) and lc == 0.0

    def everything(b):
        At, W = b.constraint_fields()
        i = b.constraint_info()
        mc, lc = b.constrained_mean(mu)
        return [At, W, np.array([i["logdet_W"], i["logdet_AAt"], lc]), mc, b.constrained_var(), b.sample(Z, mean=mu), b.sample(Z),
                b.constraint_correct(Z)]

    be.set_constraints(sp.csr_matrix(A), e)
    first = everything(be)
    be2 = gmrfx.MI355XBackend(Q, coords=mesh.points)
    be2.set_constraints(sp.csr_matrix(A), e)
    for a, b, c, d in zip(first, everything(be), everything(be2), everything(be.clone())):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)       # again, a second handle, a clone


def test_lifecycle():
    mesh, Q = matern(22, 19, seed=4)
    n = Q.shape[0]
    rng = np.random.default_rng(1)
    A, e = constraint_rows(n, 4, seed=6)
    mu = rng.standard_normal(n)
    Z = rng.standard_normal((n, 6))
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    unconstrained = be.sample(Z, mean=mu)
    be.set_constraints(sp.csr_matrix(A), e)
    At1, W1 = be.constraint_fields()
    # refactorisation with scaled values: the cache follows (W scales with 1 / 4)
    be.refactorize_values(4.0 * Q.data)
    At2, W2 = be.constraint_fields()
    Sigma, SAt, W, mean_c, Sigma_c = _dense_constrained(4.0 * Q.toarray(), mu, A, e)
    print("after refactorisation: W", relerr(W2, W), "At", relerr(At2, SAt), "W2 / W1", relerr(4.0 * W2, W1))
    assert relerr(W2, W) < 1e-10 and relerr(At2, SAt) < 1e-10 and relerr(4.0 * W2, W1) < 1e-10
    assert relerr(be.constrained_mean(mu)[0], mean_c) < 1e-10
    assert np.allclose(be.constrained_var(), np.diag(Sigma_c), rtol=1e-7, atol=1e-12)
    assert abs(be.constraint_info()["logdet_W"] - np.linalg.slogdet(W)[1]) < 1e-9 * abs(np.linalg.slogdet(W)[1])
    be.refactorize_values(Q.data)
    assert np.array_equal(be.constraint_fields()[1], W1)
    # rank-deficient A (two equal rows): NOT_POSDEF, and the handle stays usable
    Abad = np.vstack([A[:2], A[1:2]])
    be.set_constraints(sp.csr_matrix(Abad), np.array([0.1, 0.2, 0.2]))
    for call in (be.constraint_fields, be.constraint_info, be.constrained_var, lambda: be.constrained_mean(mu), lambda: be.sample(Z),
                 lambda: be.constraint_correct(Z)):
        with pytest.raises(PosDefException):
            call()
    assert np.array_equal(be.backend_backward_solve(Z) + mu[:, None], unconstrained)
    be.set_constraints(sp.csr_matrix(A), e)
    assert np.array_equal(be.constraint_fields()[1], W1)
    # clearing restores the unconstrained results
    be.clear_constraints()
    assert np.array_equal(be.sample(Z, mean=mu), unconstrained)
    assert np.array_equal(be.constrained_var(), be.get_selinv_diag())
    # before the first factorisation
    raw = gmrfx.MI355XBackend(Q, coords=mesh.points, factorize=False)
    raw.set_constraints(sp.csr_matrix(A), e)
    with pytest.raises(gmrfx._lib.GmrfxError) as ei:
        raw.constrained_var()
    assert ei.value.code == gmrfx._lib.ERR_NOT_FACTORIZED


# ---- intrinsic models under the sum-to-zero row -------------------------------------------------------------------------------
def _ok(e_gpu, e_orc, floor=1e-14):
    return e_gpu <= 10.0 * e_orc + floor


INTRINSIC = [(lambda eps=eps: im.besag_torus((64, 64), eps), f"besag64x64-{eps:g}") for eps in (1e-5, 1e-8)] + \
            [(lambda eps=eps: im.rw1_cycle(100, eps), f"rw1_cycle100-{eps:g}") for eps in (1e-5, 1e-8)]


@pytest.mark.parametrize("make", [c[0] for c in INTRINSIC], ids=[c[1] for c in INTRINSIC])
def test_intrinsic_models_sum_to_zero(make):
    """Constant vectors are eigenvectors of these precisions (eigenvalue lam_0 = the eps really added), so under A = 1' the
    constrained variance is sigma_diag() - 1 / (n lam_0) = (1 / n) sum_{k != 0} 1 / lam_k -- evaluated in that second form, which does
    not cancel -- and the constrained mean of a constant mu is 0. The device's subtraction cancels heavily (1 / (n eps) against a
    difference of order one), so the bar is this project's ratio criterion: the device error may be at most 10 x the error of
    the host float64 restatement (the mirror's arithmetic, fed by the same handle's solve and selinv_diag) + 1e-14."""
    mdl = make()
    n = mdl.n
    inv = (1.0 / mdl.lam).ravel()
    truth = math.fsum(inv[1:]) / n
    A = sp.csr_matrix(np.ones((1, n)))
    e = np.zeros(1)
    be = gmrfx.MI355XBackend(mdl.Q)
    sigma = be.get_selinv_diag().copy()
    At_h = be.backend_solve(np.ones((n, 1)))                     # the mirror's one blocked solve, on the same handle
    L_c = np.linalg.cholesky(np.asarray(A @ At_h))
    B_T = np.linalg.solve(L_c, At_h.T)
    var_h = np.maximum(sigma - (B_T ** 2).sum(axis=0), 0.0)
    c = 3.7
    mu = np.full(n, c)
    mean_h = mu - At_h @ np.linalg.solve(L_c.T, np.linalg.solve(L_c, A @ mu - e))
    be.set_constraints(A, e)
    var_d = be.constrained_var()
    mean_d, _ = be.constrained_mean(mu)
    ev_d, ev_h = float(np.abs(var_d - truth).max() / truth), float(np.abs(var_h - truth).max() / truth)
    em_d, em_h = float(np.abs(mean_d).max() / c), float(np.abs(mean_h).max() / c)
    print(f"{mdl.name} eps={mdl.eps:g}: var err device {ev_d:.3e} host {ev_h:.3e}; mean err device {em_d:.3e} host {em_h:.3e}")
    assert var_d.min() >= 0.0
    assert _ok(ev_d, ev_h), (ev_d, ev_h)
    assert _ok(em_d, em_h), (em_d, em_h)


# ---- one size that matters ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 32])
def test_benchmark_size_resident_samples(m):
    """The 1000 x 1000 Matern grid of the benchmark, 256 samples resident on the device: the correction kernels' GPU time (events on
    the handle's stream), the bytes 8 n (2 k + m) they must move and the fraction of the 6.29 TB/s copy rate that makes, beside the
    host expression it replaces (numpy, on the downloaded arrays). The residual bound is the worst case of the device sum's
    order for a row of n entries: 16 sequential + 8 tree + ceil(n / 4096) chunk additions, each one rounding of the running
    |a|'|x|, plus the same again for the product that is subtracted: 2 (24 + ceil(n / 4096)) eps (|A| |x| + |e|)."""
    import torch
    mesh = spde.grid_mesh_2d(1000, 1000, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.3))
    n, k = Q.shape[0], 256
    A, e = constraint_rows(n, m, seed=11) if m > 1 else (np.ones((1, n)), np.array([0.25]))
    Asp = sp.csr_matrix(A)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0)
    be.set_constraints(Asp, e)
    info = be.constraint_info()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    dZ = torch.randn((k, n), dtype=torch.float64, device=dev, generator=g)
    dX = torch.empty_like(dZ)
    torch.cuda.synchronize()
    be.backward_solve_dev(dZ.data_ptr(), n, k, dX.data_ptr(), n)
    Y = dX.cpu().numpy().T                                      # n x k (column-major view), before the correction
    side = torch.cuda.Stream(device=dev)
    be.set_stream(side.cuda_stream, True, False)               # events on this stream bracket the handle's kernels
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for rep in range(3):
        dW = dX.clone()
        torch.cuda.synchronize()
        ev[0].record(side)
        be.constraint_correct_dev(dW.data_ptr(), n, k)
        ev[1].record(side)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    be.set_stream(0, False, False)
    Xd = dW.cpu().numpy().T
    At, W = be.constraint_fields()
    t0 = time.perf_counter()
    L_c = np.linalg.cholesky(W)
    Xh = Y - At @ np.linalg.solve(L_c.T, np.linalg.solve(L_c, Asp @ Y - e[:, None]))
    host_ms = 1e3 * (time.perf_counter() - t0)
    res = np.abs(Asp @ Xd - e[:, None])
    bound = 2 * (24 + math.ceil(n / 4096)) * np.finfo(float).eps * (abs(Asp) @ np.abs(Xd) + np.abs(e)[:, None])
    nbytes = 8.0 * n * (2 * k + m)
    ms = min(times)
    print(f"n={n} m={m} k={k}: preparation {info['ms']:.2f} ms; correction {ms:.3f} ms (runs {['%.3f' % t for t in times]}), "
          f"{nbytes / 1e9:.3f} GB -> {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms * 1e-3) / 6.29e12:.0f}% of 6.29 TB/s; "
          f"host expression {host_ms:.0f} ms; max residual {res.max():.2e} (bound {bound.min():.2e} .. {bound.max():.2e}); "
          f"device vs host {relerr(Xd, Xh):.2e}")
    assert (res <= bound).all()
    assert relerr(Xd, Xh) < 1e-12
