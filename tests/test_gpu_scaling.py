"""Exact metamorphic relations of the HIP path under power-of-two scaling (run with -m gpu on an MI355X).

Q' = D Q D with D = diag(2^k_i): the pattern and the ordering stay, and every product of an exact implementation scales by
a power of two, so a scale-equivariant implementation gives these results BIT FOR BIT (tests/test_scaling_oracle.py shows
that the float64 CPU oracle does): factor_csc' = D_p L (D_p: D in elimination order), solve'(D b) = D^-1 solve(b),
backward_solve'(z) = D^-1 backward_solve(z), Sigma' = D^-1 Sigma D^-1 (diagonal, full CSC, extracted on a pattern),
selinv_dot'(D B D) = selinv_dot(B), row_diag_ASigmaAt'(A D) = row_diag_ASigmaAt(A), sqmahal'(D^-1 x, D^-1 mu) = sqmahal(x, mu)
and the same failing pivot; log det' = log det + 2 sum log d_i to rounding. An absolute threshold anywhere in a kernel (a
cut-off, an epsilon, a flush), or an approximate instruction whose result does not scale with its input, breaks them.

Cases: the CASES of test_gpu_parity.py, a front wider than the inverse cap (default cap and GMRFX_INV_CAP=128), and a 2-D mesh
whose levels hold thousands of fronts (sweep chunk programs, wave and workgroup tasks, and with GMRFX_FWD_FRONT=1 /
GMRFX_BWD_FRONT=1 the one-workgroup sweep steps). Entry points: the plain refactorise, the pipelined refactorise+solve (host
and device), the one-call logpdf, the Newton update (set_prior + refactorize_update[_solve]) and batched handles whose
members carry different D_k; plus Q' = 4^k Q for k = +-20, +-150. The RBMC marginal variances (csrc/rbmc.hip), plain and block form:
rbmc_var'(Z) = D^-2 rbmc_var(Z) -- given backward_solve' = D^-1 backward_solve (asserted above), every product of the estimators scales
by a power of two, the pivots' sqrt included once both of a pivot's d_i factors are counted."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import intrinsic_models as im
import rbmc_patterns
from gmrfx import spde
from test_gpu_parity import CASES as PARITY_CASES

pytestmark = pytest.mark.gpu

_NAMES = ("rand400", "matern64_coords", "cfg1_alpha3_65x65", "matern3d_10", "natural_chain", "dense70", "tall_fronts", "scalar", "diag")


def _cases():
    for name, Q, kw in PARITY_CASES:
        if name in _NAMES:
            yield name, sp.csc_matrix(Q), kw, {}
    wide = sp.csc_matrix(np.cov(np.random.default_rng(128).standard_normal((330, 900))) + np.eye(330))
    yield "wide_front_330", wide, {}, {}
    yield "wide_front_330_cap128", wide, {}, {"GMRFX_INV_CAP": "128"}
    m = spde.grid_mesh_2d(150, 140, jitter=0.25, seed=5)
    mesh = sp.csc_matrix(spde.matern_precision(m, 0, 0.2))
    yield "mesh150x140", mesh, {"coords": m.points}, {}
    yield "mesh150x140_front_steps", mesh, {"coords": m.points}, {"GMRFX_FWD_FRONT": "1", "GMRFX_BWD_FRONT": "1"}


CASES = list(_cases())


def _canon(Q):
    Q = sp.csc_matrix(Q, copy=True)
    Q.sort_indices()
    return Q


def _logdet_ok(ld_s, ld, d):
    return abs(ld_s - (ld + im.log2_shift(d))) <= 1e-13 * (abs(ld) + np.abs(2.0 * np.log(d)).sum())


def _diag_positions(Q):
    return np.array([Q.indptr[j] + np.searchsorted(Q.indices[Q.indptr[j]:Q.indptr[j + 1]], j) for j in range(Q.shape[0])])


def _design(Q, rng):
    """rows with two entries on neighbours in Q (inside the factor pattern) and an empty row"""
    n = Q.shape[0]
    C = sp.triu(Q).tocoo()
    pick = rng.choice(len(C.row), size=min(len(C.row), 200), replace=False)
    A = sp.csr_matrix((rng.standard_normal(2 * len(pick)), (np.repeat(np.arange(len(pick)), 2),
                                                           np.stack([C.row[pick], C.col[pick]], 1).ravel())), shape=(len(pick) + 1, n))
    A.sum_duplicates()
    A.sort_indices()
    return A


def _same_factor(bs, be, d, perm, tag):
    L, Ls = be.factor_csc(), bs.factor_csc()
    want = im.scale_rows(L, d[perm])
    assert np.array_equal(Ls.indptr, want.indptr) and np.array_equal(Ls.indices, want.indices)
    bad = np.flatnonzero(Ls.data != want.data)
    if bad.size:
        cols = np.repeat(np.arange(Ls.shape[1]), np.diff(Ls.indptr))
        pytest.fail(f"{tag}: factor differs in {bad.size} entries, first column (elimination order) {cols[bad].min()}")


def _scalings(n, seed):
    yield "diag", im.pow2_diag(n, np.random.default_rng(seed))
    for k in (-150, -20, 20, 150):
        yield f"uniform4^{k}", np.full(n, np.ldexp(1.0, k))


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    name, Q, kw, env = request.param
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, v)
    Q = _canon(Q)
    be = gmrfx.MI355XBackend(Q, **kw)
    yield name, Q, kw, be
    be.close()
    mp.undo()


def test_plain_handle_relations(case):
    name, Q, kw, be = case
    n = Q.shape[0]
    perm = be.ordering_permutation()
    rng = np.random.default_rng(1)
    B = rng.standard_normal((n, 3))
    Z = rng.standard_normal((n, 2))
    x, mu = rng.standard_normal((n, 2)), rng.standard_normal(n)
    Bm = Q.copy()
    Bm.data = rng.standard_normal(Q.nnz)
    A = _design(Q, rng)
    assert be.last_info == 0
    # well-conditioned fronts keep the default inverse cap (Device::decide_inverse_cap lowers it only for pivot growth > 1e4)
    assert be.stats()["inv_cap"] == (128 if name.endswith("_cap128") else 2048)
    ld = be.compute_logdet()
    X, Y = be.backend_solve(B), be.backend_backward_solve(Z)
    sd, S = be.get_selinv_diag().copy(), be.get_selinv().copy()
    ext = be.selinv_extract_at(Bm)
    dot, dotd = be.selinv_dot(Bm), be.selinv_dot_device(Bm)
    rd = be.row_diag_ASigmaAt(A)
    q = be.sqmahal(x, mu)
    for tag, d in _scalings(n, 2):
        tag = f"{name}/{tag}"
        bs = gmrfx.MI355XBackend(im.scaled(Q, d), **kw)
        assert np.array_equal(bs.ordering_permutation(), perm)
        assert bs.last_info == 0
        assert bs.stats()["inv_cap"] == be.stats()["inv_cap"], tag       # the decision does not see the scaling
        _same_factor(bs, be, d, perm, tag)
        assert _logdet_ok(bs.compute_logdet(), ld, d), tag
        assert np.array_equal(bs.backend_solve(B * d[:, None]), X / d[:, None]), tag
        assert np.array_equal(bs.backend_backward_solve(Z), Y / d[:, None]), tag
        assert np.array_equal(bs.get_selinv_diag(), sd / d / d), tag
        Ss = bs.get_selinv()
        assert np.array_equal(Ss.indptr, S.indptr) and np.array_equal(Ss.indices, S.indices)
        assert np.array_equal(Ss.data, im.scale_both(S, 1.0 / d).data), tag
        Bs = im.scaled(Bm, d)
        assert np.array_equal(bs.selinv_extract_at(Bs).data, im.scale_both(ext, 1.0 / d).data), tag
        assert bs.selinv_dot(Bs) == dot and bs.selinv_dot_device(Bs) == dotd, tag
        assert np.array_equal(bs.row_diag_ASigmaAt(im.scale_cols_csr(A, d)), rd), tag
        assert np.array_equal(bs.sqmahal(x / d[:, None], mu / d), q), tag
        bs.close()


def test_pipelined_and_device_entry_points(case):
    import torch
    name, Q, kw, be = case
    n = Q.shape[0]
    rng = np.random.default_rng(3)
    dev = torch.device("cuda", 0)
    nz = 1.5 * Q.data                                        # new values: Q2 = 1.5 Q
    Q2 = sp.csc_matrix((nz, Q.indices, Q.indptr), shape=Q.shape)
    d = im.pow2_diag(n, rng)
    nzs = im.scaled_values(Q2, d)
    a = gmrfx.MI355XBackend(Q, **kw, factorize=False)
    b = gmrfx.MI355XBackend(im.scaled(Q, d), **kw, factorize=False)
    perm = a.ordering_permutation()
    # host pipelined call
    B = rng.standard_normal((n, 5))
    X = a.refactorize_solve(nz, B)
    Xs = b.refactorize_solve(nzs, B * d[:, None])
    assert a.last_info == 0 and b.last_info == 0
    assert np.array_equal(Xs, X / d[:, None]), name
    _same_factor(b, a, d, perm, name + "/pipelined")
    # device pipelined call, rows of right-hand sides (ld = n)
    for nrhs in (1, 64):
        Bh = rng.standard_normal((nrhs, n))
        d_nz, d_nzs = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (nz, nzs))
        d_B, d_Bs = torch.from_numpy(Bh).to(dev), torch.from_numpy(Bh * d[None, :]).to(dev)
        d_X, d_Xs = torch.zeros_like(d_B), torch.zeros_like(d_B)
        torch.cuda.synchronize()
        assert a.refactorize_solve_dev(d_nz.data_ptr(), d_B.data_ptr(), n, nrhs, d_X.data_ptr(), n) == 0
        assert b.refactorize_solve_dev(d_nzs.data_ptr(), d_Bs.data_ptr(), n, nrhs, d_Xs.data_ptr(), n) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_Xs.cpu().numpy(), d_X.cpu().numpy() / d[None, :]), f"{name} nrhs={nrhs}"
    # one-call logpdf: quadratic forms bit for bit, log det to rounding
    Zh = rng.standard_normal((3, n))
    mu = rng.standard_normal(n)
    d_Z, d_Zs = torch.from_numpy(Zh).to(dev), torch.from_numpy(Zh / d[None, :]).to(dev)
    d_mu, d_mus = torch.from_numpy(mu).to(dev), torch.from_numpy(mu / d).to(dev)
    torch.cuda.synchronize()
    for use_mu in (False, True):
        q, ld = a.refactorize_logpdf_dev(d_nz.data_ptr(), d_Z.data_ptr(), n, 3, d_mu.data_ptr() if use_mu else 0)
        qs, lds = b.refactorize_logpdf_dev(d_nzs.data_ptr(), d_Zs.data_ptr(), n, 3, d_mus.data_ptr() if use_mu else 0)
        assert a.last_info == 0 and b.last_info == 0
        assert np.array_equal(qs, q), name
        assert _logdet_ok(lds, ld, d), name
    _same_factor(b, a, d, perm, name + "/logpdf")
    a.close(); b.close()


def test_newton_update_relations(case):
    name, Q, kw, be = case
    n = Q.shape[0]
    rng = np.random.default_rng(4)
    d = im.pow2_diag(n, rng)
    a = gmrfx.MI355XBackend(Q, **kw)
    b = gmrfx.MI355XBackend(im.scaled(Q, d), **kw)
    perm = a.ordering_permutation()
    diag = _diag_positions(Q)
    # Q_prior' = D Q D, H' = D H D on the diagonal
    a.set_prior(Q.data, diag)
    b.set_prior(im.scaled_values(Q, d), diag)
    h = -rng.uniform(0.1, 2.0, n) * np.abs(Q.diagonal())
    assert a.refactorize_update(h) == 0 and b.refactorize_update(h * d * d) == 0
    _same_factor(b, a, d, perm, name + "/update")
    B = rng.standard_normal((n, 4))
    X = a.refactorize_update_solve(0.5 * h, B)
    Xs = b.refactorize_update_solve(0.5 * h * d * d, B * d[:, None])
    assert np.array_equal(Xs, X / d[:, None]), name
    a.close(); b.close()


def test_failing_pivot_is_scale_invariant(case):
    import torch
    name, Q, kw, be = case
    n = Q.shape[0]
    rng = np.random.default_rng(6)
    bad = Q.copy()
    col = n // 2
    bad.data[_diag_positions(Q)[col]] = -abs(bad.data[_diag_positions(Q)[col]])
    be.refactorize_values(bad.data)
    info = be.last_info
    assert info > 0
    dev = torch.device("cuda", 0)
    for tag, d in _scalings(n, 8):
        nzs = im.scaled_values(bad, d)
        bs = gmrfx.MI355XBackend(Q, **kw, factorize=False)
        bs.refactorize_values(nzs)
        assert bs.last_info == info, tag
        d_nz = torch.from_numpy(np.ascontiguousarray(nzs)).to(dev)
        d_B = torch.from_numpy(rng.standard_normal((2, n))).to(dev)
        d_X = torch.zeros_like(d_B)
        torch.cuda.synchronize()
        assert bs.refactorize_solve_dev(d_nz.data_ptr(), d_B.data_ptr(), n, 2, d_X.data_ptr(), n) == info, tag
        bs.close()
    be.refactorize_values(Q.data)
    assert be.last_info == 0


@pytest.mark.parametrize("nbatch", [1, 5])
def test_batched_members_with_their_own_scalings(nbatch):
    """Members Q_k = tau_k Q + delta_k I, scaled by their own D_k: every member of the scaled batch gives the bits of the
    unscaled batch's member, scaled, on every batch entry point, the fused logpdf included. With one member the batch is
    the plain handle's analysis and kernels: its factor and solves are the bits of the plain handle of D Q D (its log det
    is summed by the batch's own kernel, so it agrees to rounding)."""
    import torch
    m = spde.grid_mesh_2d(60, 60, jitter=0.25, seed=2)
    Q = _canon(spde.matern_precision(m, 0, 0.2))
    n = Q.shape[0]
    rng = np.random.default_rng(9)
    tau, delta = rng.uniform(0.5, 2.0, nbatch), rng.uniform(0.0, 0.1, nbatch) * Q.diagonal().max()
    isdiag = np.zeros(Q.nnz)
    isdiag[_diag_positions(Q)] = 1.0
    NZ = np.asfortranarray(Q.data[:, None] * tau[None, :] + isdiag[:, None] * delta[None, :])
    Dk = np.stack([im.pow2_diag(n, rng) for _ in range(nbatch)], axis=1)        # (n, B)
    NZs = np.asfortranarray(np.stack([im.scaled_values(sp.csc_matrix((NZ[:, k], Q.indices, Q.indptr), shape=Q.shape), Dk[:, k])
                                      for k in range(nbatch)], axis=1))
    a = gmrfx.MI355XBatchBackend(Q, nbatch, coords=m.points)
    b = gmrfx.MI355XBatchBackend(Q, nbatch, coords=m.points)
    assert np.all(a.refactorize_values(NZ) == 0) and np.all(b.refactorize_values(NZs) == 0)
    R = rng.standard_normal((n, 3, nbatch))
    X, Xs = a.solve(R), b.solve(R * Dk[:, None, :])
    assert np.array_equal(Xs, X / Dk[:, None, :])
    Y, Ys = a.backward_solve(R), b.backward_solve(R)
    assert np.array_equal(Ys, Y / Dk[:, None, :])
    assert np.array_equal(b.selinv_diag(), a.selinv_diag() / Dk / Dk)
    V, mu = rng.standard_normal((n, 2, nbatch)), rng.standard_normal((n, nbatch))
    q, qs = a.sqmahal(V, mu), b.sqmahal(V / Dk[:, None, :], mu / Dk)
    assert np.array_equal(qs, q)
    ld, lds = a.logdet(), b.logdet()
    for k in range(nbatch):
        assert _logdet_ok(lds[k], ld[k], Dk[:, k]), k
    # the fused batch logpdf (one call) on the device
    dev = torch.device("cuda", 0)
    d_nz, d_nzs = torch.from_numpy(NZ.T.copy()).to(dev), torch.from_numpy(NZs.T.copy()).to(dev)
    Vh = np.ascontiguousarray(np.transpose(V, (2, 1, 0)))                        # (B, nvec, n): member stride 2 n
    Vhs = np.ascontiguousarray(np.transpose(V / Dk[:, None, :], (2, 1, 0)))
    mh, mhs = np.ascontiguousarray(mu.T), np.ascontiguousarray((mu / Dk).T)
    d_V, d_Vs, d_m, d_ms = (torch.from_numpy(v).to(dev) for v in (Vh, Vhs, mh, mhs))
    torch.cuda.synchronize()
    l1, q1, i1 = a.refactorize_logpdf_dev(d_nz.data_ptr(), d_V.data_ptr(), n, 2 * n, 2, d_m.data_ptr())
    l2, q2, i2 = b.refactorize_logpdf_dev(d_nzs.data_ptr(), d_Vs.data_ptr(), n, 2 * n, 2, d_ms.data_ptr())
    assert np.all(i1 == 0) and np.all(i2 == 0)
    assert np.array_equal(q2, q1) and np.array_equal(q1, q)
    assert np.array_equal(l1, ld) and np.array_equal(l2, lds)
    if nbatch == 1:
        p = gmrfx.MI355XBackend(sp.csc_matrix((NZs[:, 0], Q.indices, Q.indptr), shape=Q.shape), coords=m.points)
        assert np.array_equal(p.factor_values(), b.factor_values())
        assert np.array_equal(p.backend_solve(R[:, :, 0] * Dk[:, :1]), Xs[:, :, 0])
        assert abs(p.compute_logdet() - lds[0]) <= 4 * np.spacing(abs(lds[0]))      # (reduced by another kernel: batch.hip)
        p.close()
    a.close(); b.close()


def _rbmc_cases():
    name, Q, kw = next(c for c in PARITY_CASES if c[0] == "matern64_coords")
    yield name, sp.csc_matrix(Q), kw
    yield "banded400_32", rbmc_patterns.banded(400, 32), {}


@pytest.mark.parametrize("name,Q,kw", list(_rbmc_cases()), ids=["matern64_coords", "banded400_32"])
def test_rbmc_variances_scale_exactly(name, Q, kw):
    """Two handles, Q and D Q D, the same Z: the variances of the scaled handle are those of the plain one divided by d_i^2, bit for
    bit, for the plain estimator and the block estimator (enclosure_size 0 and 2; k = 70: two sample blocks and a Chan merge).
    D = diag(2^k_i) with k_i of this file's range, and D = 2^p I (Q' = 4^p Q, factor 4^-p) for p = +-20."""
    Q = _canon(Q)
    n = Q.shape[0]
    Z = np.random.default_rng(12).standard_normal((n, 70))
    be = gmrfx.MI355XBackend(Q, **kw)
    want = {enc: be.rbmc_var(Z, enc) for enc in (-1, 0, 2)}
    for enc, v in want.items():
        assert np.isfinite(v).all() and (v > 0).all(), enc
    scalings = [("diag", im.pow2_diag(n, np.random.default_rng(13)))] + [(f"uniform4^{p}", np.full(n, np.ldexp(1.0, p))) for p in (-20, 20)]
    for tag, d in scalings:
        bs = gmrfx.MI355XBackend(im.scaled(Q, d), **kw)
        assert np.array_equal(bs.ordering_permutation(), be.ordering_permutation())
        for enc, v in want.items():
            got = bs.rbmc_var(Z, enc)
            bad = np.flatnonzero(got != v / d / d)
            assert bad.size == 0, f"{name}/{tag} enclosure_size={enc}: {bad.size} of {n} variances differ, first row {bad[:1]}"
        bs.close()
    be.close()
