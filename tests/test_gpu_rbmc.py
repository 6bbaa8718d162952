"""Rao-Blackwellised Monte Carlo marginal variances on the device (include/gmrfx.h: gmrfx_rbmc_var(_dev); csrc/rbmc.hip) against the
numpy restatement of src/solvers/rbmc.jl in tests/rbmc_ref.py. The restatement is fed the samples X that backend_backward_solve(Z)
returns, so sampling error cancels: the comparison is exact up to rounding, bound max|v - v_ref| <= 1e-8 max|v_ref| (the project's
tolerance for marginal variances). Determinism (host / _dev forms, ldz, alignment, second handle, clone), held / given values, the
reference's own accuracy test against the true variances, a non-grid pattern, a batched handle, and the error paths."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import orc
import rbmc_ref
from gmrfx import _lib, spde

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8
KS = [2, 63, 64, 65, 127, 128, 129, 200]


class Model:
    def __init__(self, smoothness):
        self.mesh = spde.grid_mesh_2d(21, 21)
        self.Q = sp.csc_matrix(spde.matern_precision(self.mesh, smoothness=smoothness, range_=0.2))
        self.n = self.Q.shape[0]
        self.be = gmrfx.MI355XBackend(self.Q, coords=self.mesh.points, device=0)
        self.sq = rbmc_ref.SymQ(self.Q)
        self.Z = np.asfortranarray(np.random.default_rng(11 + smoothness).standard_normal((self.n, max(KS))))
        self._ops, self._X = {}, {}

    def ops(self, enc):
        if enc >= 0 and enc not in self._ops:
            self._ops[enc] = rbmc_ref.block_ops(self.sq, enc)
        return self._ops.get(enc)

    def X(self, k):
        if k not in self._X:
            self._X[k] = self.be.backend_backward_solve(self.Z[:, :k])
        return self._X[k]


@pytest.fixture(scope="module")
def models():
    return {1: Model(1), 0: Model(0)}


def _relerr(v, ref):
    return np.abs(v - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("enclosure_size", [-1, 0, 1, 2])
@pytest.mark.parametrize("smoothness", [1, 0])
def test_against_the_restatement(models, smoothness, enclosure_size, k):
    m = models[smoothness]
    v = m.be.rbmc_var(m.Z[:, :k], enclosure_size)
    ref = rbmc_ref.rbmc_var(m.sq, m.X(k), enclosure_size, m.ops(enclosure_size))
    err = _relerr(v, ref)
    print(f"rbmc smoothness={smoothness} enclosure={enclosure_size} k={k}: max|v - v_ref| / max|v_ref| = {err:.3e}")
    assert np.isfinite(v).all() and err <= TOL
    assert m.be.stats()["ms_rbmc"] > 0.0


def _dev_form(be, Z, enclosure_size, ld=None, off=0, nzval=None):
    import torch
    n, k = Z.shape
    ld = ld or n
    dev = torch.device("cuda", 0)
    buf = torch.full((ld * k + off + 1,), float("nan"), dtype=torch.float64, device=dev)
    view = buf[off:off + ld * k].view(k, ld)
    view[:, :n] = torch.from_numpy(np.ascontiguousarray(Z.T)).to(dev)
    out = torch.empty(n + 1, dtype=torch.float64, device=dev)
    dnz = None if nzval is None else torch.from_numpy(np.ascontiguousarray(nzval)).to(dev)
    torch.cuda.synchronize()
    be.rbmc_var_dev(buf.data_ptr() + 8 * off, ld, k, out.data_ptr() + 8 * (off % 2), enclosure_size, 0 if dnz is None else dnz.data_ptr())
    torch.cuda.synchronize()
    return out[off % 2:off % 2 + n].cpu().numpy()


@pytest.mark.parametrize("enclosure_size", [-1, 1])
def test_bits_do_not_depend_on_form_layout_or_handle(models, enclosure_size):
    m = models[1]
    n, k = m.n, 129
    Z = m.Z[:, :k]
    v = m.be.rbmc_var(Z, enclosure_size)
    assert (m.be.rbmc_var(Z, enclosure_size) == v).all()                                    # run to run
    assert (_dev_form(m.be, Z, enclosure_size) == v).all()                                  # host / _dev
    assert (_dev_form(m.be, Z, enclosure_size, ld=n + 3) == v).all()                        # ldz = n + 3
    assert (_dev_form(m.be, Z, enclosure_size, ld=n + 3, off=1) == v).all()                 # Z at an odd 8-byte offset
    Zpad = np.asfortranarray(np.vstack([Z, np.full((3, k), np.nan)]))                       # host form with ldz = n + 3
    out = np.empty(n)
    _lib.check(_lib.lib().gmrfx_rbmc_var(m.be._h, None, _lib.ptr(Zpad), n + 3, k, enclosure_size, _lib.ptr(out)), m.be._h)
    assert (out == v).all()
    second = gmrfx.MI355XBackend(m.Q, coords=m.mesh.points, device=0)
    assert (second.rbmc_var(Z, enclosure_size) == v).all()                                  # a second handle
    clone = m.be.clone()
    with pytest.raises(ValueError):                                                         # a clone does not hold Q's values
        clone.rbmc_var(Z, enclosure_size)
    assert (clone.rbmc_var(Z, enclosure_size, nzval=m.Q.data) == v).all()                   # a clone
    assert (_dev_form(clone, Z, enclosure_size, nzval=m.Q.data) == v).all()


@pytest.mark.parametrize("enclosure_size", [-1, 0])
def test_values_given_and_held(models, enclosure_size):
    m = models[0]
    Z = m.Z[:, :65]
    be = gmrfx.MI355XBackend(m.Q, coords=m.mesh.points, device=0)
    nz2 = 1.5 * m.Q.data
    be.refactorize_values(nz2)
    held = be.rbmc_var(Z, enclosure_size)
    assert (be.rbmc_var(Z, enclosure_size, nzval=nz2) == held).all()
    X = be.backend_backward_solve(Z)
    assert _relerr(held, rbmc_ref.rbmc_var(rbmc_ref.SymQ(1.5 * m.Q), X, enclosure_size)) <= TOL
    # only the defining triangle is read: garbage in the lower one of a handle whose upper triangle defines Q
    junk = nz2.copy()
    rows, cols = m.Q.indices, np.repeat(np.arange(m.n), np.diff(m.Q.indptr))
    junk[rows > cols] = 1e30
    assert (be.rbmc_var(Z, enclosure_size, nzval=junk) == held).all()


def test_against_the_true_variances(models):
    """the reference's own test (test/solvers/variance/test_rbmc.jl:30-37): 21 x 21, smoothness 1, k = 500"""
    m = models[1]
    Z = np.random.default_rng(854289).standard_normal((m.n, 500))
    truth = m.be.get_selinv_diag()
    plain = m.be.rbmc_var(Z, -1)
    block = m.be.rbmc_var(Z, 2)
    e_plain = np.linalg.norm(plain - truth) / np.linalg.norm(truth)
    e_block = np.linalg.norm(block - truth) / np.linalg.norm(truth)
    print(f"rbmc vs selinv_diag, k = 500: plain {e_plain:.3e}, enclosure_size = 2 {e_block:.3e}")
    assert e_plain < 0.05
    assert e_block < 0.01


def test_non_grid_pattern():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sprand_spd_60.npz"))
    n = int(g["n"])
    Q = sp.csc_matrix((g["nzval"], g["rowval"], g["colptr"]), shape=(n, n))
    be = gmrfx.MI355XBackend(Q, device=0)
    Z = np.random.default_rng(3).standard_normal((n, 70))
    v = be.rbmc_var(Z, 1)
    err = _relerr(v, rbmc_ref.rbmc_var(rbmc_ref.SymQ(Q), be.backend_backward_solve(Z), 1))
    print(f"rbmc sprand_spd_60 enclosure=1: {err:.3e}")
    assert err <= TOL


def test_batched_handle():
    mesh = spde.grid_mesh_2d(9, 8, jitter=0.2, seed=1)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.4))
    n, B, k = Q.shape[0], 3, 70
    bb = gmrfx.MI355XBatchBackend(Q, B, coords=mesh.points, device=0)
    NZ = np.stack([Q.data * s for s in (1.0, 2.0, 0.5)], axis=1)
    assert not bb.refactorize_values(NZ).any()
    Z = np.random.default_rng(4).standard_normal((n * B, k))
    v = bb.rbmc_var(Z, -1)
    assert v.shape == (n, B)
    X = bb.backward_solve(Z.reshape(B, n, k).transpose(1, 2, 0))          # (n, k, B)
    for b, s in enumerate((1.0, 2.0, 0.5)):
        ref = rbmc_ref.plain_var(rbmc_ref.SymQ(Q * s), np.ascontiguousarray(X[:, :, b]))
        assert _relerr(v[:, b], ref) <= TOL, b
    assert (bb.rbmc_var(Z, -1, nzval=NZ) == v).all()


def test_errors_leave_the_handle_usable(models):
    m = models[0]
    Z = m.Z[:, :8]
    raw = gmrfx.MI355XBackend(m.Q, coords=m.mesh.points, device=0, factorize=False)
    with pytest.raises(_lib.GmrfxError) as ei:
        raw.rbmc_var(Z, -1, nzval=m.Q.data)
    assert ei.value.code == _lib.ERR_NOT_FACTORIZED
    be = gmrfx.MI355XBackend(m.Q, coords=m.mesh.points, device=0)
    with pytest.raises(ValueError, match="nsamples"):
        be.rbmc_var(Z[:, :1], -1)
    with pytest.raises(ValueError, match="enclosure_size"):
        be.rbmc_var(Z, -2)
    be.set_constraints(sp.csr_matrix(np.ones((1, m.n))), np.zeros(1))
    with pytest.raises(ValueError, match="constraint"):
        be.rbmc_var(Z, 0)
    be.clear_constraints()
    assert _relerr(be.rbmc_var(Z, 0), rbmc_ref.rbmc_var(m.sq, be.backend_backward_solve(Z), 0)) <= TOL
    B = np.random.default_rng(2).standard_normal((m.n, 3))
    F = orc.OracleFactor(m.Q, be.ordering_permutation())
    X = be.backend_solve(B)
    assert np.abs(X - F.solve(B)).max() / np.abs(X).max() < 1e-10
