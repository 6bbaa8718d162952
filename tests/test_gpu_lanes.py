"""Solves of more than 64 right-hand sides run as 64-column passes that alternate between two sweep lanes (a stream and a set of
right-hand-side buffers each); the pipelined factor + solve call runs its first pass's forward sweep on the side stream. Whatever
lane a pass runs on and however often a lane's buffers are reused, a pass gives the bits of a call on its columns alone: 3 and 4
passes (130 / 193 columns, the last pass 2 / 1 columns wide: the narrow kernels once on each lane), full and backward-only
solves, the pipelined call, the solve statistics, and member-strided solves of a batched handle."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
from gmrfx import spde

pytestmark = pytest.mark.gpu

_STATE = {}


def _problem():
    """the mesh of the pipelined parity test: sweep tasks, big fronts (X2 in use), several levels"""
    if "Q" not in _STATE:
        mesh = spde.grid_mesh_2d(150, 140, jitter=0.25, seed=5)
        _STATE["Q"] = sp.csc_matrix(spde.matern_precision(mesh, 0, 0.2))
        _STATE["pts"] = mesh.points
    return _STATE["Q"], _STATE["pts"]


def _handle():
    if "be" not in _STATE:
        Q, pts = _problem()
        _STATE["be"] = gmrfx.MI355XBackend(Q, coords=pts, device=0)
    return _STATE["be"]


def _rhs(nrhs, n, seed):
    """column-major n x nrhs on the device (row j of the tensor = column j)"""
    import torch
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((nrhs, n))).cuda()


def _call(fn, d_B, n):
    import torch
    d_X = torch.zeros_like(d_B)
    torch.cuda.synchronize()
    fn(d_B.data_ptr(), n, d_B.shape[0], d_X.data_ptr(), n)
    torch.cuda.synchronize()
    return d_X


@pytest.mark.parametrize("nrhs", [130, 193])
@pytest.mark.parametrize("which", ["solve_dev", "backward_solve_dev"])
def test_every_pass_gives_the_bits_of_a_call_on_its_block_alone(which, nrhs):
    import torch
    be = _handle()
    n = be.n
    fn = getattr(be, which)
    d_B = _rhs(nrhs, n, 100 + nrhs)
    d_X = _call(fn, d_B, n)
    for j0 in range(0, nrhs, 64):
        d_Xj = _call(fn, d_B[j0:j0 + 64].contiguous(), n)
        assert torch.equal(d_X[j0:j0 + 64], d_Xj), f"{which}, nrhs={nrhs}: columns {j0}.. differ from a call on that block alone"
    assert torch.equal(d_X, _call(fn, d_B, n))                        # and the call repeats its bits


def test_one_pass_solve_is_the_same_before_and_after_a_four_pass_solve():
    import torch
    be = _handle()
    n = be.n
    d_B64, d_B193 = _rhs(64, n, 7), _rhs(193, n, 8)
    before = _call(be.solve_dev, d_B64, n)
    _call(be.solve_dev, d_B193, n)
    after = _call(be.solve_dev, d_B64, n)
    assert torch.equal(before, after)
    resid = np.linalg.norm(_problem()[0] @ after.cpu().numpy().T - d_B64.cpu().numpy().T) / np.linalg.norm(d_B64.cpu().numpy())
    assert resid < 1e-10


def test_statistics_of_a_three_pass_solve():
    be = _handle()
    _call(be.solve_dev, _rhs(130, be.n, 9), be.n)
    st = be.stats()
    assert st["last_nrhs"] == 130
    assert st["ms_solve"] > 0 and st["ms_solve_fwd"] > 0 and st["ms_solve_bwd"] > 0


def test_pipelined_call_of_three_passes_equals_separate_calls():
    import torch
    Q, pts = _problem()
    n, nrhs = Q.shape[0], 130
    a = gmrfx.MI355XBackend(Q, coords=pts, device=0)          # factorised once: the inverse cap is decided, the next call is pipelined
    b = _handle()
    d_nz = torch.from_numpy(np.ascontiguousarray(Q.data * 1.25)).cuda()
    d_B = _rhs(nrhs, n, 10)
    d_Xa = torch.zeros_like(d_B)
    torch.cuda.synchronize()
    assert a.refactorize_solve_dev(d_nz.data_ptr(), d_B.data_ptr(), n, nrhs, d_Xa.data_ptr(), n) == 0
    torch.cuda.synchronize()
    try:
        assert b.refactorize_dev(d_nz.data_ptr()) == 0
        d_Xb = _call(b.solve_dev, d_B, n)
        assert torch.equal(d_Xa, d_Xb)
        assert np.array_equal(a.factor_values(), b.factor_values())
        assert a.compute_logdet() == b.compute_logdet()
        assert a.stats()["last_nrhs"] == nrhs
        assert torch.equal(_call(a.solve_dev, d_B, n), d_Xb)          # a plain solve on the pipelined handle afterwards
    finally:
        d_q = torch.from_numpy(np.ascontiguousarray(Q.data)).cuda()   # the shared handle goes back to Q's own values
        torch.cuda.synchronize()
        assert b.refactorize_dev(d_q.data_ptr()) == 0
    a.close()


def test_batched_member_strided_solve_of_two_passes():
    import torch
    mesh = spde.grid_mesh_2d(40, 36, jitter=0.25, seed=3)
    Q = sp.csc_matrix(spde.matern_precision(mesh, 0, 0.3))
    n, nb, nrhs = Q.shape[0], 3, 70
    tau = np.array([0.75, 1.0, 1.5])
    bb = gmrfx.MI355XBatchBackend(Q, nb, coords=mesh.points, device=0)
    assert np.all(bb.refactorize_values(np.asfortranarray(Q.data[:, None] * tau[None, :])) == 0)
    perm = bb.ordering_permutation()
    ld = n + 3
    stride = ld * nrhs + 13                                           # larger than ld * nrhs
    rng = np.random.default_rng(11)
    hb = rng.standard_normal(stride * nb)
    d_B = torch.from_numpy(hb).cuda()
    d_X = torch.full((stride * nb,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    bb.solve_dev(d_B.data_ptr(), ld, stride, nrhs, d_X.data_ptr(), ld, stride)
    torch.cuda.synchronize()
    for k in range(nb):
        plain = gmrfx.MI355XBackend(sp.csc_matrix((Q.data * tau[k], Q.indices, Q.indptr), shape=Q.shape), ordering=perm, device=0)
        blk_B = d_B[k * stride:k * stride + ld * nrhs].reshape(nrhs, ld)
        blk_X = d_X[k * stride:k * stride + ld * nrhs].reshape(nrhs, ld)
        assert torch.all(blk_X[:, n:] == 7.0) and torch.all(d_X[k * stride + ld * nrhs:(k + 1) * stride] == 7.0)
        for j0 in range(0, nrhs, 64):
            d_Bj = blk_B[j0:j0 + 64, :n].contiguous()
            d_Xj = _call(plain.solve_dev, d_Bj, n)
            diff = float((blk_X[j0:j0 + 64, :n] - d_Xj).abs().max() / d_Xj.abs().max())
            print(f"member {k}, columns {j0}..: relative difference to the plain handle {diff:.3e}")
            assert torch.equal(blk_X[j0:j0 + 64, :n], d_Xj), (k, j0, diff)
        plain.close()
    bb.close()
