"""One constraint A x = e for every member of a batched handle, computed per member on the device (include/gmrfx.h:
gmrfx_batch_constraints_*, gmrfx_batch_sample, gmrfx_batch_constrained_logpdf_dev; kernels in csrc/constraint.hip): against the
dense kriging formulas per member, against plain handles of the members' values, against the host mirror of the reference's
WorkspaceGMRF fed each member's own fields, for member independence, rank-deficient A, the fused call against its pieces, the
life cycle, and on an intrinsic model. Tolerances are those of tests/test_gpu_constraints.py. Every case prints its figures."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg

import gmrfx
import intrinsic_models as im
from gmrfx import _lib, spde
from gmrfx._lib import PosDefException
from mirror.workspace_gmrf import ConstraintInfo, WorkspaceGMRF

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def members(nx, ny, B, seed):
    """B Matern precisions on one nx x ny grid, each with its own tau and range: one pattern, B sets of values (nnz, B)."""
    mesh = spde.grid_mesh_2d(nx, ny, jitter=0.2, seed=seed)
    rng = np.random.default_rng(seed)
    Qs = []
    for k in range(B):
        Qk = sp.csc_matrix(rng.uniform(0.5, 2.0) * spde.matern_precision(mesh, 0, rng.uniform(0.3, 0.6)))
        Qk.sort_indices()
        Qs.append(Qk)
    for Qk in Qs[1:]:
        assert np.array_equal(Qk.indices, Qs[0].indices) and np.array_equal(Qk.indptr, Qs[0].indptr)
    return mesh, Qs, np.asfortranarray(np.stack([Qk.data for Qk in Qs], axis=1))


def constraint_rows(n, m, seed):
    """One dense sum-to-zero row plus m - 1 sparse random rows, e != 0."""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n))
    A[0] = 1.0
    for r in range(1, m):
        idx = rng.choice(n, size=7, replace=False)
        A[r, idx] = rng.standard_normal(7)
    return A, rng.standard_normal(m)


def batch(mesh, Qs, NZ, A=None, e=None):
    bb = gmrfx.MI355XBatchBackend(Qs[0], len(Qs), coords=mesh.points)
    bb.refactorize_values(NZ)
    if A is not None:
        bb.set_constraints(sp.csr_matrix(A), e)
    return bb


def log_correction_ref(A, e, mu, W):
    m = A.shape[0]
    r = e - A @ mu
    return 0.5 * (m * np.log(2.0 * np.pi) + np.linalg.slogdet(W)[1] + r @ np.linalg.solve(W, r)) - 0.5 * np.linalg.slogdet(A @ A.T)[1]


# ---- 1. dense kriging per member -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 5, 64])
def test_dense_kriging_per_member(m):
    B = 3
    mesh, Qs, NZ = members(12, 11, B, seed=10 + m)
    n = Qs[0].shape[0]
    A, e = constraint_rows(n, m, seed=100 + m)
    mu = np.random.default_rng(m).standard_normal((n, B))
    bb = batch(mesh, Qs, NZ, A, e)
    info = bb.constraint_info()
    assert info["m"] == m and np.array_equal(info["cinfo"], np.zeros(B))
    assert bb.stats()["last_nrhs"] == m                                   # the ONE forest solve of m columns
    mc, lc = bb.constrained_mean(mu)
    v = bb.constrained_var()
    for k in range(B):
        Sigma = np.linalg.inv(Qs[k].toarray())
        SAt = Sigma @ A.T
        W = A @ SAt
        mean_c = mu[:, k] - SAt @ np.linalg.solve(W, A @ mu[:, k] - e)
        var_c = np.diag(Sigma - SAt @ np.linalg.solve(W, SAt.T))
        At, Wd = bb.constraint_fields(k)
        ldW, lref = np.linalg.slogdet(W)[1], log_correction_ref(A, e, mu[:, k], W)
        figs = dict(At=relerr(At, SAt), W=relerr(Wd, W), mean=relerr(mc[:, k], mean_c), logdetW=abs(info["logdet_W"][k] - ldW) / abs(ldW),
                    logcorr=abs(lc[k] - lref) / abs(lref), Ax_e=float(np.abs(A @ mc[:, k] - e).max()), var=float(np.abs(v[:, k] - var_c).max()))
        print(f"m={m} member {k}", {a: f"{x:.3g}" for a, x in figs.items()}, f"prep {info['ms']:.3f} ms")
        assert figs["At"] < 1e-10 and figs["W"] < 1e-10 and figs["mean"] < 1e-10
        assert figs["logdetW"] < 1e-9 and figs["logcorr"] < 1e-9
        assert figs["Ax_e"] <= 1e-9
        assert np.allclose(v[:, k], var_c, rtol=1e-7, atol=1e-12) and v[:, k].min() >= 0.0


# ---- 2. against plain handles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 17])
def test_against_plain_handles(m):
    import torch
    B = 5
    mesh, Qs, NZ = members(23, 21, B, seed=20 + m)
    n = Qs[0].shape[0]
    A, e = constraint_rows(n, m, seed=200 + m)
    mu = np.random.default_rng(m).standard_normal((n, B))
    bb = batch(mesh, Qs, NZ, A, e)
    info = bb.constraint_info()
    mc, lc = bb.constrained_mean(mu)
    v = bb.constrained_var()
    # A~'_k = what gmrfx_batch_solve_dev makes of the replicated dense A', bit for bit
    d_R = torch.from_numpy(np.ascontiguousarray(np.tile(A, (B, 1)))).cuda()          # member k's n x m block at k n m, ld n
    d_X = torch.empty_like(d_R)
    torch.cuda.synchronize()
    bb.solve_dev(d_R.data_ptr(), n, n * m, m, d_X.data_ptr(), n, n * m)
    solved = d_X.cpu().numpy().reshape(B, m, n)
    perm = bb.ordering_permutation()
    for k in range(B):
        At, W = bb.constraint_fields(k)
        assert np.array_equal(At, solved[k].T), k
        be = gmrfx.MI355XBackend(Qs[k], ordering=perm)
        be.set_constraints(sp.csr_matrix(A), e)
        pi = be.constraint_info()
        At_p, W_p = be.constraint_fields()
        mc_p, lc_p = be.constrained_mean(mu[:, k])
        v_p = be.constrained_var()
        figs = dict(At=relerr(At, At_p), W=relerr(W, W_p), mean=relerr(mc[:, k], mc_p), logdetW=abs(info["logdet_W"][k] - pi["logdet_W"]) /
                    abs(pi["logdet_W"]), logcorr=abs(lc[k] - lc_p) / abs(lc_p), var=float(np.abs(v[:, k] - v_p).max()))
        print(f"m={m} member {k}", {a: f"{x:.3g}" for a, x in figs.items()})
        assert figs["At"] < 1e-10 and figs["W"] < 1e-10 and figs["mean"] < 1e-10
        assert figs["logdetW"] < 1e-9 and figs["logcorr"] < 1e-9
        assert np.allclose(v[:, k], v_p, rtol=1e-7, atol=1e-12)


# ---- 3. rows longer than one reduction chunk -------------------------------------------------------------------------------------
def test_rows_longer_than_one_chunk():
    B = 2
    mesh, Qs, NZ = members(70, 70, B, seed=3)
    n = Qs[0].shape[0]
    assert n > 4096
    A = sp.lil_matrix((2, n))
    A[0, :] = 1.0
    A[1, [5, 2500, n - 1]] = [1.0, -2.0, 0.5]
    A = sp.csr_matrix(A)
    e = np.array([0.0, 0.3])
    bb = batch(mesh, Qs, NZ, A, e)
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((n, 3, B))
    X = bb.sample(Z)
    for k in range(B):
        lu = sp.linalg.splu(Qs[k])
        W = A @ lu.solve(A.T.toarray())
        Wd = bb.constraint_fields(k)[1]
        res = float(np.abs(A @ X[:, :, k] - e[:, None]).max())
        print(f"member {k}: W {relerr(Wd, W):.3g}, max |A x - e| {res:.3g}")
        assert relerr(Wd, W) < 1e-10
        assert res <= 1e-9


# ---- 4. correction and sample ----------------------------------------------------------------------------------------------------
class _MemberWorkspace:
    """What WorkspaceGMRF.rand_from asks of a workspace, answered by one member of a batched handle"""
    loaded_version = 0

    def __init__(self, bb, k):
        self.bb, self.k = bb, k

    def backward_solve(self, Z):
        Zb = np.zeros(Z.shape + (self.bb.nbatch,))
        Zb[..., self.k] = Z
        return self.bb.backward_solve(Zb)[..., self.k]


def _mirror(bb, k, A, e, mu):
    """the mirror's WorkspaceGMRF with ConstraintInfo's fields taken from member k of the device"""
    At, W = bb.constraint_fields(k)
    ci = object.__new__(ConstraintInfo)
    ci.matrix, ci.vector, ci.A_tilde_T, ci.L_c = sp.csc_matrix(A), e, At, np.linalg.cholesky(W)
    d = object.__new__(WorkspaceGMRF)
    d.mean_, d.workspace, d.version, d.constraints = mu, _MemberWorkspace(bb, k), 0, ci
    return d


@pytest.mark.parametrize("nvec", [1, 9, 65])
def test_correction_and_sample(nvec):
    import torch
    B, m = 3, 5
    mesh, Qs, NZ = members(31, 27, B, seed=5)
    n = Qs[0].shape[0]
    A, e = constraint_rows(n, m, seed=15)
    rng = np.random.default_rng(7)
    mu = rng.standard_normal((n, B))
    Z = rng.standard_normal((n, nvec, B))
    bb = batch(mesh, Qs, NZ, A, e)
    X = bb.sample(Z, mean=mu)
    Y = bb.backward_solve(Z) + mu[:, None, :]
    Xc = bb.constraint_correct(Y)
    for k in range(B):
        ref = _mirror(bb, k, A, e, mu[:, k]).rand_from(Z[:, :, k])
        r1, r2 = relerr(X[:, :, k], ref), relerr(Xc[:, :, k], ref)
        res = float(np.abs(A @ X[:, :, k] - e[:, None]).max())
        print(f"nvec={nvec} member {k}: sample {r1:.2e} correct {r2:.2e} residual {res:.2e}")
        assert r1 < 1e-12 and r2 < 1e-12
        assert res <= 1e-9
    # device-pointer forms = host forms, bit for bit, with ldx > n, a padded member stride and an odd offset of 8 bytes
    ldx = n + 3
    sx = ldx * nvec + 5

    def padded(V, fill):
        h = np.full(sx * B + 1, fill)
        for k in range(B):
            for j in range(nvec):
                h[1 + k * sx + j * ldx: 1 + k * sx + j * ldx + n] = V[:, j, k]
        return torch.from_numpy(h).cuda()

    def unpadded(d, fill):
        h = d.cpu().numpy()
        V = np.empty((n, nvec, B))
        mask = np.ones(h.shape, bool)
        for k in range(B):
            for j in range(nvec):
                V[:, j, k] = h[1 + k * sx + j * ldx: 1 + k * sx + j * ldx + n]
                mask[1 + k * sx + j * ldx: 1 + k * sx + j * ldx + n] = False
        assert np.all(h[mask] == fill), "written outside the members' blocks"
        return V

    d_Y = padded(Y, 7.0)
    torch.cuda.synchronize()
    bb.constraint_correct_dev(d_Y.data_ptr() + 8, ldx, sx, nvec)
    assert np.array_equal(unpadded(d_Y, 7.0), Xc)
    d_Z = torch.from_numpy(np.ascontiguousarray(np.transpose(Z, (2, 1, 0)))).cuda()
    d_mu = torch.from_numpy(np.ascontiguousarray(mu.T)).cuda()
    d_X = padded(np.zeros_like(Z), 3.0)
    torch.cuda.synchronize()
    bb.sample_dev(d_Z.data_ptr(), n, n * nvec, nvec, d_X.data_ptr() + 8, ldx, sx, d_mu.data_ptr())
    assert np.array_equal(unpadded(d_X, 3.0), X)
    # run to run, a second handle, a clone
    for other in (bb, batch(mesh, Qs, NZ, A, e), bb.clone()):
        assert np.array_equal(other.sample(Z, mean=mu), X) and np.array_equal(other.constraint_correct(Y), Xc)


# ---- 5. member independence ------------------------------------------------------------------------------------------------------
def test_member_independence():
    B, m = 3, 4
    mesh, Qs, NZ = members(19, 17, B, seed=6)
    n = Qs[0].shape[0]
    A, e = constraint_rows(n, m, seed=16)
    rng = np.random.default_rng(2)
    mu = rng.standard_normal((n, B))
    Z = rng.standard_normal((n, 2, B))

    def everything(bb):
        i = bb.constraint_info()
        mc, lc = bb.constrained_mean(mu)
        return dict(cinfo=i["cinfo"], logdet_W=i["logdet_W"], mean=mc, logcorr=lc, sample=bb.sample(Z, mean=mu), var=bb.constrained_var(),
                    At=np.stack([bb.constraint_fields(k)[0] for k in range(B)], axis=-1), W=np.stack([bb.constraint_fields(k)[1] for k in range(B)], axis=-1))

    good = everything(batch(mesh, Qs, NZ, A, e))
    bad_nz = NZ.copy(order="F")
    bad_nz[:, 1] = -bad_nz[:, 1]
    bb = gmrfx.MI355XBatchBackend(Qs[0], B, coords=mesh.points)
    finfo = bb.refactorize_values(bad_nz)
    assert finfo[0] == 0 and finfo[1] > 0 and finfo[2] == 0
    bb.set_constraints(sp.csr_matrix(A), e)
    got = everything(bb)           # no exception: a member whose factorisation failed is reported through cinfo only
    assert np.array_equal(got["cinfo"], [0, -1, 0])
    for name in ("logdet_W", "mean", "logcorr", "sample", "var", "At", "W"):
        assert np.all(np.isnan(got[name][..., 1])), name
        for k in (0, 2):
            assert np.array_equal(got[name][..., k], good[name][..., k]), (name, k)
    # the fused call: the members' info says which one failed, cinfo agrees, the others' numbers are the good batch's
    import torch
    d_nz = torch.from_numpy(np.ascontiguousarray(bad_nz.T)).cuda()
    d_x = torch.from_numpy(np.ascontiguousarray(Z[:, 0, :].T)).cuda()
    d_mu = torch.from_numpy(np.ascontiguousarray(mu.T)).cuda()
    torch.cuda.synchronize()
    ld, quad, lc, info, cinfo = bb.constrained_logpdf_dev(d_nz.data_ptr(), d_x.data_ptr(), n, n, 1, d_mu.data_ptr())
    assert np.array_equal(info, finfo) and np.array_equal(cinfo, [0, -1, 0])
    assert np.isnan(lc[1]) and np.array_equal(lc[[0, 2]], good["logcorr"][[0, 2]])


# ---- 6. rank-deficient A ---------------------------------------------------------------------------------------------------------
def test_rank_deficient_constraint():
    B = 3
    mesh, Qs, NZ = members(16, 15, B, seed=7)
    n = Qs[0].shape[0]
    A, e = constraint_rows(n, 3, seed=17)
    Z = np.random.default_rng(3).standard_normal((n, 4, B))
    bb = batch(mesh, Qs, NZ)
    unconstrained = bb.sample(Z)
    Abad = np.vstack([A[1:2], A[1:2]])                      # two equal rows: pivot 1 of every W_k is zero within rounding
    bb.set_constraints(sp.csr_matrix(Abad), np.array([0.2, 0.2]))
    cinfo = np.zeros(B, np.int64)
    code = _lib.lib().gmrfx_batch_constraints_info(bb._h, None, None, None, _lib.ptr(cinfo), None)
    assert code == _lib.ERR_NOT_POSDEF and np.array_equal(cinfo, [2, 2, 2])          # 1 + pivot 1
    assert np.array_equal(bb.constraint_info(check_posdef=False)["cinfo"], [2, 2, 2])
    for call in (lambda: bb.constraint_fields(0), bb.constraint_info, bb.constrained_var, bb.constrained_mean, lambda: bb.sample(Z),
                 lambda: bb.constraint_correct(Z)):
        with pytest.raises(PosDefException):
            call()
    assert np.array_equal(bb.backward_solve(Z), unconstrained)
    bb.clear_constraints()
    assert np.array_equal(bb.sample(Z), unconstrained)
    bb.set_constraints(sp.csr_matrix(A), e)
    assert np.array_equal(bb.constraint_info()["cinfo"], np.zeros(B))


# ---- 7. one call versus the pieces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mu", [True, False])
def test_fused_call_against_the_pieces(with_mu):
    import torch
    B, m, nvec = 4, 6, 3
    mesh, Qs, NZ = members(21, 18, B, seed=8)
    n = Qs[0].shape[0]
    A, e = constraint_rows(n, m, seed=18)
    rng = np.random.default_rng(4)
    mu = rng.standard_normal((n, B)) if with_mu else None
    X = rng.standard_normal((n, nvec, B))
    d_nz = torch.from_numpy(np.ascontiguousarray(NZ.T)).cuda()
    d_x = torch.from_numpy(np.ascontiguousarray(np.transpose(X, (2, 1, 0)))).cuda()
    d_mu = torch.from_numpy(np.ascontiguousarray(mu.T)).cuda() if with_mu else None
    p_mu = d_mu.data_ptr() if with_mu else 0
    torch.cuda.synchronize()
    bb = gmrfx.MI355XBatchBackend(Qs[0], B, coords=mesh.points)
    bb.set_constraints(sp.csr_matrix(A), e)
    ld0, quad0, info0 = bb.refactorize_logpdf_dev(d_nz.data_ptr(), d_x.data_ptr(), n, n * nvec, nvec, p_mu)
    lc0 = bb.constrained_mean(mu)[1]
    for rep in range(2):
        ld, quad, lc, info, cinfo = bb.constrained_logpdf_dev(d_nz.data_ptr(), d_x.data_ptr(), n, n * nvec, nvec, p_mu)
        assert np.array_equal(ld, ld0) and np.array_equal(quad, quad0) and np.array_equal(info, info0) and np.array_equal(lc, lc0)
        assert np.array_equal(cinfo, np.zeros(B))
    # and the numbers are the reference's terms: log_correction per member against numpy
    for k in range(B):
        W = A @ np.linalg.solve(Qs[k].toarray(), A.T)
        lref = log_correction_ref(A, e, mu[:, k] if with_mu else np.zeros(n), W)
        assert abs(lc[k] - lref) < 1e-9 * abs(lref)
    # without a constraint: zeros beside the unconstrained call's bits
    bb.clear_constraints()
    ld, quad, lc, info, cinfo = bb.constrained_logpdf_dev(d_nz.data_ptr(), d_x.data_ptr(), n, n * nvec, nvec, p_mu)
    assert np.array_equal(ld, ld0) and np.array_equal(quad, quad0) and not lc.any() and not cinfo.any()


# ---- 8. life cycle ---------------------------------------------------------------------------------------------------------------
def test_lifecycle():
    B = 3
    mesh, Qs, NZ = members(18, 14, B, seed=9)
    n = Qs[0].shape[0]
    A, e = constraint_rows(n, 4, seed=19)
    Z = np.random.default_rng(5).standard_normal((n, 6, B))
    bb = batch(mesh, Qs, NZ)
    # without a constraint: the existing entry points' bits
    assert bb.constraint_info()["m"] == 0
    assert np.array_equal(bb.sample(Z), bb.backward_solve(Z))
    assert np.array_equal(bb.constrained_var(), bb.selinv_diag())
    assert np.array_equal(bb.constraint_correct(Z), Z)
    bb.set_constraints(sp.csr_matrix(A), e)
    i1 = bb.constraint_info()
    W1 = [bb.constraint_fields(k)[1] for k in range(B)]
    assert i1["ms"] > 0.0
    # a refactorisation drops the cache: W_k scales with 1 / 4, log det W_k moves by -m log 4
    bb.refactorize_values(4.0 * NZ)
    i2 = bb.constraint_info()
    assert i2["ms"] > 0.0 and not np.array_equal(i2["logdet_W"], i1["logdet_W"])
    for k in range(B):
        W = A @ np.linalg.solve(4.0 * Qs[k].toarray(), A.T)
        assert relerr(bb.constraint_fields(k)[1], W) < 1e-10
        assert abs(i2["logdet_W"][k] - (i1["logdet_W"][k] - 4 * np.log(4.0))) < 1e-9 * abs(i1["logdet_W"][k])
    bb.refactorize_values(NZ)
    assert np.array_equal(bb.constraint_info()["logdet_W"], i1["logdet_W"])
    assert all(np.array_equal(bb.constraint_fields(k)[1], W1[k]) for k in range(B))
    bb.clear_constraints()
    assert np.array_equal(bb.sample(Z), bb.backward_solve(Z))
    # before the first factorisation
    raw = gmrfx.MI355XBatchBackend(Qs[0], B, coords=mesh.points)
    raw.set_constraints(sp.csr_matrix(A), e)
    with pytest.raises(_lib.GmrfxError) as ei:
        raw.constrained_var()
    assert ei.value.code == _lib.ERR_NOT_FACTORIZED
    # a plain handle is a batch of one
    be = gmrfx.MI355XBackend(Qs[0], coords=mesh.points)
    rp, ci, va = sp.csr_matrix(A).indptr.astype(np.int64), sp.csr_matrix(A).indices.astype(np.int64), sp.csr_matrix(A).data
    L = _lib.lib()
    assert L.gmrfx_batch_constraints_set(be._h, 4, _lib.ptr(rp), _lib.ptr(ci), _lib.ptr(va), 0, _lib.ptr(e)) == 0
    ldw, c1 = np.zeros(1), np.ones(1, np.int64)
    assert L.gmrfx_batch_constraints_info(be._h, None, _lib.ptr(ldw), None, _lib.ptr(c1), None) == 0 and c1[0] == 0
    assert abs(ldw[0] - i1["logdet_W"][0]) < 1e-9 * abs(ldw[0])


# ---- 9. intrinsic model under the sum-to-zero row --------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 1e-8])
def test_intrinsic_besag_sum_to_zero(eps):
    """The criterion of test_gpu_constraints.py::test_intrinsic_models_sum_to_zero per member: members Q and 2 Q (an exact scaling:
    eigenvalues lam and 2 lam), constrained variance (1 / n) sum_{k != 0} 1 / lam_k and constrained mean 0 of a constant mu; the
    device error may be at most 10 x the error of the host float64 restatement fed by the same handle's solve and selinv_diag,
    + 1e-14."""
    mdl = im.besag_torus((64, 64), eps)
    n, scales = mdl.n, (1.0, 2.0)
    B = len(scales)
    Q = sp.csc_matrix(mdl.Q)
    NZ = np.asfortranarray(np.stack([s * Q.data for s in scales], axis=1))
    A, e = sp.csr_matrix(np.ones((1, n))), np.zeros(1)
    c = 3.7
    mu = np.full((n, B), c)
    bb = gmrfx.MI355XBatchBackend(Q, B)
    bb.refactorize_values(NZ)
    sigma = bb.selinv_diag().copy()
    At_h = bb.solve(np.ones((n, B)))                       # the mirror's one blocked solve, on the same handle
    bb.set_constraints(A, e)
    var_d = bb.constrained_var()
    mean_d, _ = bb.constrained_mean(mu)
    for k, s in enumerate(scales):
        truth = math.fsum((1.0 / (s * mdl.lam)).ravel()[1:]) / n
        a = At_h[:, k:k + 1]
        L_c = np.linalg.cholesky(np.asarray(A @ a))
        B_T = np.linalg.solve(L_c, a.T)
        var_h = np.maximum(sigma[:, k] - (B_T ** 2).sum(axis=0), 0.0)
        mean_h = mu[:, k] - a @ np.linalg.solve(L_c.T, np.linalg.solve(L_c, A @ mu[:, k] - e))
        ev_d, ev_h = float(np.abs(var_d[:, k] - truth).max() / truth), float(np.abs(var_h - truth).max() / truth)
        em_d, em_h = float(np.abs(mean_d[:, k]).max() / c), float(np.abs(mean_h).max() / c)
        print(f"{mdl.name} eps={eps:g} x {s:g}: var err device {ev_d:.3e} host {ev_h:.3e}; mean err device {em_d:.3e} host {em_h:.3e}")
        assert var_d[:, k].min() >= 0.0
        assert ev_d <= 10.0 * ev_h + 1e-14, (ev_d, ev_h)
        assert em_d <= 10.0 * em_h + 1e-14, (em_d, em_h)
