"""Batched handles on the GPU (gmrfx_create_batched): B members with one pattern factored as diag(Q_1 .. Q_B). Every member is
checked against the oracle with the member's order and against a plain handle of its values alone (bit-identical for B = 1); a
failing member leaves the others' bits alone; the fused batched logpdf call gives the bits of the separate calls; runs and clones
repeat bits."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import orc
from gmrfx import spde

pytestmark = pytest.mark.gpu

_MESHES = {}


def _problem(name):
    if name not in _MESHES:
        if name == "m20":
            m = spde.grid_mesh_2d(20, 20, jitter=0.25, seed=1)          # small fronts only
            Q = spde.matern_precision(m, 0, 0.3)
        elif name == "m100":
            m = spde.grid_mesh_2d(100, 100, jitter=0.25, seed=2)        # big fronts: potrf / trsm / gemm path
            Q = spde.matern_precision(m, 0, 0.2)
        else:
            m = spde.grid_mesh_3d(16, 16, 16)                           # 3-D: the contribution-block SYRK runs
            Q = spde.matern_precision(m, 0, 0.5)
        _MESHES[name] = (sp.csc_matrix(Q), m.points)
    return _MESHES[name]


def _member_values(Q, B, seed=0):
    """NZ[:, k] = tau_k Q + delta_k I on Q's pattern"""
    rng = np.random.default_rng(seed)
    isdiag = np.zeros(Q.nnz)
    for j in range(Q.shape[0]):
        r = Q.indices[Q.indptr[j]:Q.indptr[j + 1]]
        isdiag[Q.indptr[j] + np.flatnonzero(r == j)] = 1.0
    dmax = float(Q.diagonal().max())
    tau = rng.uniform(0.5, 2.0, B)
    delta = rng.uniform(0.0, 0.1, B) * dmax
    return np.asfortranarray(Q.data[:, None] * tau[None, :] + isdiag[:, None] * delta[None, :]), isdiag


def _member(Q, NZ, k):
    return sp.csc_matrix((NZ[:, k].copy(), Q.indices, Q.indptr), shape=Q.shape)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _dev_solve(bb, R, backward=False, pad_in=(3, 5), pad_out=(1, 11)):
    """the _dev entry points with padded leading dimensions and member strides: R (n, r, B) -> X (n, r, B)"""
    import torch
    n, r, B = R.shape
    ldb, ldx = n + pad_in[0], n + pad_out[0]
    sb, sx = ldb * r + pad_in[1], ldx * r + pad_out[1]
    hb = np.zeros(sb * B)
    for k in range(B):
        for j in range(r):
            hb[k * sb + j * ldb: k * sb + j * ldb + n] = R[:, j, k]
    d_B = torch.from_numpy(hb).cuda()
    d_X = torch.full((sx * B,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    (bb.backward_solve_dev if backward else bb.solve_dev)(d_B.data_ptr(), ldb, sb, r, d_X.data_ptr(), ldx, sx)
    hx = d_X.cpu().numpy()
    X = np.empty((n, r, B))
    for k in range(B):
        for j in range(r):
            X[:, j, k] = hx[k * sx + j * ldx: k * sx + j * ldx + n]
        gap = hx[k * sx + r * ldx: (k + 1) * sx] if k + 1 < B else hx[k * sx + r * ldx:]
        assert np.all(gap == 7.0), "the solve wrote outside member blocks"
    return X


_CASES = [("m20", 1), ("m20", 3), ("m20", 17), ("m20", 50), ("m100", 1), ("m100", 3), ("m100", 17), ("m100", 50),
          ("g16", 1), ("g16", 3), ("g16", 17)]


@pytest.mark.parametrize("name,B", _CASES, ids=[f"{a}_B{b}" for a, b in _CASES])
def test_batch_members_match_oracle_and_plain_handles(name, B):
    Q, pts = _problem(name)
    n = Q.shape[0]
    NZ, _ = _member_values(Q, B)
    bb = gmrfx.MI355XBatchBackend(Q, B, coords=pts, device=0)
    perm = bb.ordering_permutation()
    info = bb.refactorize_values(NZ)
    assert np.all(info == 0) and np.all(bb.info() == 0)
    ld = bb.logdet()
    rng = np.random.default_rng(5)
    R = {r: rng.standard_normal((n, r, B)) for r in (1, 5, 64)}
    Xs = {r: bb.solve(R[r]) for r in R}
    Xb = bb.backward_solve(R[5])
    Xv = bb.solve(R[1][:, 0, :])                                      # the (n, B) form
    assert np.array_equal(Xv, Xs[1][:, 0, :])
    for r in (1, 64):                                                 # device arrays, padded ld and stride: the same bits
        assert np.array_equal(_dev_solve(bb, R[r]), Xs[r])
    assert np.array_equal(_dev_solve(bb, R[5], backward=True), Xb)
    Z = rng.standard_normal((n, 2, B))
    mu = rng.standard_normal((n, B))
    quad = bb.sqmahal(Z, mean=mu)
    assert quad.shape == (2, B)
    sd = bb.selinv_diag()
    assert sd.shape == (n, B)
    for k in sorted({0, B // 2, B - 1}):
        Qk = _member(Q, NZ, k)
        F = orc.OracleFactor(Qk, perm)
        assert abs(ld[k] - F.logdet()) <= 1e-12 * abs(F.logdet())
        for r in R:
            assert _rel(Xs[r][:, :, k], F.solve(R[r][:, :, k])) < 1e-10, r
        assert _rel(Xb[:, :, k], F.backward_solve(R[5][:, :, k])) < 1e-9
        for v in range(2):
            q = orc.sqmahal(Qk, Z[:, v, k], mu[:, k])
            assert abs(quad[v, k] - q) <= 1e-12 * abs(q)
        assert _rel(sd[:, k], F.selinv_diag()) < 1e-8
        plain = gmrfx.MI355XBackend(Qk, ordering=perm, device=0)
        assert np.array_equal(plain.ordering_permutation(), perm)
        Xp = plain.backend_solve(R[5][:, :, k])
        Xpb = plain.backend_backward_solve(R[5][:, :, k])
        if B == 1:      # the same analysis, the same kernels: the same bits
            assert np.array_equal(bb.factor_values(), plain.factor_values())
            assert np.array_equal(Xs[5][:, :, 0], Xp) and np.array_equal(Xb[:, :, 0], Xpb)
        else:
            assert _rel(Xs[5][:, :, k], Xp) < 1e-12 and _rel(Xb[:, :, k], Xpb) < 1e-12
            assert abs(ld[k] - plain.compute_logdet()) <= 1e-12 * abs(ld[k])
        plain.close()
    # the plain entry point acts on the block-diagonal matrix: log det = the sum over the members
    tot = ctypes.c_double(0.0)
    assert gmrfx._lib.lib().gmrfx_logdet(bb._h, ctypes.byref(tot)) == 0
    assert abs(tot.value - float(np.sum(ld))) <= 1e-12 * abs(np.sum(ld))
    # two runs, and a clone, give the same bits
    assert np.all(bb.refactorize_values(NZ) == 0)
    assert np.array_equal(bb.logdet(), ld) and np.array_equal(bb.solve(R[5]), Xs[5])
    c = bb.clone()
    assert np.array_equal(c.logdet(), ld) and np.array_equal(c.solve(R[5]), Xs[5]) and np.array_equal(c.backward_solve(R[5]), Xb)
    assert np.array_equal(c.ordering_permutation(), perm)


@pytest.mark.parametrize("name,B", [("m20", 17), ("m100", 3), ("g16", 3)])
def test_fused_logpdf_gives_the_bits_of_the_separate_calls(name, B):
    import torch
    Q, pts = _problem(name)
    n = Q.shape[0]
    NZ, _ = _member_values(Q, B, seed=2)
    bb = gmrfx.MI355XBatchBackend(Q, B, coords=pts, device=0)
    rng = np.random.default_rng(9)
    nvec = 3
    X = rng.standard_normal((n, nvec, B))
    mu = rng.standard_normal((n, B))
    d_nz = torch.from_numpy(np.ascontiguousarray(NZ.T).reshape(-1)).cuda()       # nnz x B column-major
    d_X = torch.from_numpy(np.ascontiguousarray(X.transpose(2, 1, 0)).reshape(-1)).cuda()
    d_mu = torch.from_numpy(np.ascontiguousarray(mu.T).reshape(-1)).cuda()
    torch.cuda.synchronize()
    ld_f, q_f, info_f = bb.refactorize_logpdf_dev(d_nz.data_ptr(), d_X.data_ptr(), n, n * nvec, nvec, d_mu.data_ptr())
    assert np.all(info_f == 0)
    info_s = bb.refactorize_dev(d_nz.data_ptr())
    q_s = bb.quadform_dev(d_nz.data_ptr(), d_X.data_ptr(), n, n * nvec, nvec, d_mu.data_ptr())
    ld_s = bb.logdet()
    assert np.array_equal(info_s, info_f) and np.array_equal(ld_s, ld_f) and np.array_equal(q_s, q_f)
    # the host-array form and the oracle
    ld_h, q_h, info_h = bb.refactorize_logpdf(NZ, X, mean=mu)
    assert np.array_equal(ld_h, ld_f) and np.array_equal(q_h, q_f) and np.all(info_h == 0)
    perm = bb.ordering_permutation()
    for k in (0, B - 1):
        Qk = _member(Q, NZ, k)
        F = orc.OracleFactor(Qk, perm)
        assert abs(ld_f[k] - F.logdet()) <= 1e-12 * abs(F.logdet())
        assert abs(q_f[1, k] - orc.sqmahal(Qk, X[:, 1, k], mu[:, k])) <= 1e-12 * abs(q_f[1, k])
    # a plain handle's fused call on member 0
    if B <= 3:
        plain = gmrfx.MI355XBackend(_member(Q, NZ, 0), ordering=perm, device=0)
        d_nz0 = d_nz[:Q.nnz].clone()
        d_X0 = d_X[:n * nvec].clone()
        d_mu0 = d_mu[:n].clone()
        torch.cuda.synchronize()
        q0, ld0 = plain.refactorize_logpdf_dev(d_nz0.data_ptr(), d_X0.data_ptr(), n, nvec, d_mu0.data_ptr())
        assert np.abs(q0 - q_f[:, 0]).max() <= 1e-13 * np.abs(q0).max()
        assert abs(ld0 - ld_f[0]) <= 1e-12 * abs(ld0)


@pytest.mark.parametrize("name,B,bad", [("m20", 17, 5), ("m100", 3, 1), ("g16", 3, 2)])
def test_failing_member_is_isolated(name, B, bad):
    Q, pts = _problem(name)
    n = Q.shape[0]
    NZ, isdiag = _member_values(Q, B, seed=4)
    NZb = NZ.copy(order="F")
    # member `bad`: an indefinite matrix (a large negative shift on part of the diagonal)
    dpos = np.flatnonzero(isdiag)
    shift = np.zeros(Q.nnz)
    shift[dpos[n // 2:]] = -3.0 * float(np.abs(NZ[:, bad]).max())
    NZb[:, bad] += shift
    bb = gmrfx.MI355XBatchBackend(Q, B, coords=pts, device=0)
    perm = bb.ordering_permutation()
    rng = np.random.default_rng(11)
    R = rng.standard_normal((n, 4, B))
    assert np.all(bb.refactorize_values(NZ) == 0)
    ld_good, X_good = bb.logdet(), bb.solve(R)
    info = bb.refactorize_values(NZb)
    plain = gmrfx.MI355XBackend(_member(Q, NZb, bad), ordering=perm, device=0)
    assert plain.last_info > 0
    assert info[bad] == plain.last_info
    assert all(info[k] == 0 for k in range(B) if k != bad)
    ld_bad, X_bad = bb.logdet(), bb.solve(R)
    others = [k for k in range(B) if k != bad]
    assert np.array_equal(ld_bad[others], ld_good[others])
    assert np.array_equal(X_bad[:, :, others], X_good[:, :, others])
    # check_posdef = 1: NOT_POSDEF, and info is filled in
    bc = gmrfx.MI355XBatchBackend(Q, B, coords=pts, device=0, check_posdef=True)
    with pytest.raises(gmrfx.PosDefException):
        bc.refactorize_values(NZb)
    assert np.array_equal(bc.info(), info)
    assert np.all(bc.refactorize_values(NZ) == 0)
