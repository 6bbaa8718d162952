"""Batched handles (gmrfx_create_batched) at their edges: levels wider than 65535 fronts (grid y / z of the per-level launches),
right-hand-side widths around the permute kernels' switch points and the 64-column passes, members of 1 to 1025 nodes that make
permute tiles and diagonal blocks straddle members, the stored triangle, pivot failures of every kind, and the batch entry points
on a plain handle.

Every member is checked. Member values come from P prototypes (tau from 1e-3 to 1e3, so a member that read a neighbour's values
cannot pass by accident); member k takes prototype (7919 k) % P. The first member of each prototype is compared with the float64
oracle (and dense numpy for small members); every other member must give the bits of the first member of its prototype: the same
values and the same kernels give the same bits wherever the member sits."""

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import orc
from gmrfx import spde

pytestmark = pytest.mark.gpu

SENTINEL = -1.25e300


# ---- members ---------------------------------------------------------------------------------------------------------------

def _grid(nx, ny, rng_=0.3, seed=1):
    m = spde.grid_mesh_2d(nx, ny, jitter=0.25, seed=seed)
    return _csc(spde.matern_precision(m, 0, rng_)), m.points


def _csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


def _chain(n, phi=0.9):
    """AR(1) precision: tridiagonal, 1 + phi^2 inside, 1 at the ends"""
    d = np.full(n, 1.0 + phi * phi)
    d[0] = d[-1] = 1.0
    if n == 1:
        return _csc(np.array([[1.0]]))
    return _csc(sp.diags([d, np.full(n - 1, -phi), np.full(n - 1, -phi)], [0, -1, 1]))


def _dense(n, seed=3):
    G = np.random.default_rng(seed).standard_normal((n, n))
    return _csc(G @ G.T / n + np.eye(n))


def _arrow(K, S=128):
    """K leaves, each coupled to the same S separator nodes (the last S), diagonally dominant: with the natural order one level
    holds the K leaves, each a front of 1 column and S + 1 rows"""
    n = K + S
    r = np.repeat(np.arange(K), S)
    c = K + np.tile(np.arange(S), K)
    v = -0.01 * (1.0 + np.random.default_rng(K).random(K * S))
    A = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsc()
    A = A + A.T
    return _csc(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0))


def _isdiag(Q):
    out = np.zeros(Q.nnz)
    for j in range(Q.shape[0]):
        r = Q.indices[Q.indptr[j]:Q.indptr[j + 1]]
        out[Q.indptr[j] + np.flatnonzero(r == j)] = 1.0
    return out


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


class Protos:
    """P value vectors on Q's pattern (tau_p (Q + delta_p I), tau from 1e-3 to 1e3), each with its right-hand sides, quadratic-form
    vectors and mean; member k of a batch of B takes prototype (7919 k) % P"""

    def __init__(self, Q, P=4, seed=0, nrhs=(1, 17), nq=2):
        self.Q = Q
        assert sp.isspmatrix_csc(Q) and Q.has_sorted_indices      # NZ follows the handle's CSC order
        n, nnz = self.Q.shape[0], self.Q.nnz
        rng = np.random.default_rng(seed)
        self.isdiag = _isdiag(self.Q)
        dmax = float(np.abs(self.Q.diagonal()).max())
        self.tau = np.logspace(-3, 3, P)
        delta = rng.uniform(0.01, 0.2, P) * dmax
        self.NZ = np.asfortranarray(self.Q.data[:, None] * self.tau[None, :] + self.isdiag[:, None] * (self.tau * delta)[None, :])
        self.P, self.n = P, n
        self.R = {r: rng.standard_normal((n, r, P)) for r in nrhs}
        self.Xq = rng.standard_normal((n, nq, P))
        self.mu = rng.standard_normal((n, P))

    @staticmethod
    def assign(B, P):
        return (np.arange(B) * 7919) % P

    def member(self, p, nz=None):
        return sp.csc_matrix((self.NZ[:, p].copy() if nz is None else nz, self.Q.indices, self.Q.indptr), shape=self.Q.shape)


def _firsts(assign):
    """first member of each prototype, and for every member the first member of its prototype"""
    first = {int(p): int(np.flatnonzero(assign == p)[0]) for p in np.unique(assign)}
    return first, np.array([first[int(p)] for p in assign])


def _member_factor(bb, B, n):
    """the member-k slices of factor_values(): for every member the lower trapezoids of its panels, located through
    gmrfx_symbolic_get on the batched handle. Returns (L, idx(k) -> index array)"""
    sy = gmrfx.MI355XBackend.symbolic(bb)
    ns_all = len(sy.super_parent)
    assert ns_all % B == 0
    ns = ns_all // B
    first = sy.super_first[:ns_all].reshape(B, ns)
    assert np.array_equal(first - first[:, :1], np.tile(first[0] - first[0, 0], (B, 1)))     # the member's supernodes, repeated
    assert np.array_equal(first[:, 0], np.arange(B) * n)
    nrow = np.diff(sy.row_ptr).reshape(B, ns)
    ld = sy.panel_ld.reshape(B, ns)
    assert np.all(nrow == nrow[0]) and np.all(ld == ld[0])
    ncol = np.diff(sy.super_first)[:ns]
    sup, rel = [], []
    for s in range(ns):
        for c in range(ncol[s]):
            i = np.arange(c, nrow[0, s])
            rel.append(c * ld[0, s] + i)
            sup.append(np.full(len(i), s))
    sup, rel = np.concatenate(sup), np.concatenate(rel)
    pp = sy.panel_ptr[:ns_all].reshape(B, ns)
    L = bb.factor_values()
    return L, (lambda ks: pp[np.asarray(ks)][:, sup] + rel[None, :])


def _check_factor_bits(bb, B, n, ref, chunk=256):
    L, idx = _member_factor(bb, B, n)
    for k0 in range(0, B, chunk):
        ks = np.arange(k0, min(B, k0 + chunk))
        assert np.array_equal(L[idx(ks)], L[idx(ref[ks])]), "a member's factor differs from its prototype's first member"


def _dev_solve(bb, R, backward=False, pad_in=(3, 5), pad_out=(2, 7)):
    """the _dev entry points with padded leading dimensions and member strides: R (n, r, B) -> X (n, r, B). Every padding element
    of the output (rows n..ld-1 of each column, the gap after each member) keeps its sentinel; the input is left alone"""
    import torch
    n, r, B = R.shape
    ldb, ldx = n + pad_in[0], n + pad_out[0]
    sb, sx = ldb * r + pad_in[1], ldx * r + pad_out[1]
    hb = np.full((B, sb), SENTINEL)
    hb[:, :ldb * r].reshape(B, r, ldb)[:, :, :n] = R.transpose(2, 1, 0)
    d_B = torch.from_numpy(hb.reshape(-1)).cuda()
    d_X = torch.full((sx * B,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    (bb.backward_solve_dev if backward else bb.solve_dev)(d_B.data_ptr(), ldb, sb, r, d_X.data_ptr(), ldx, sx)
    hx = d_X.cpu().numpy().reshape(B, sx)
    assert np.array_equal(d_B.cpu().numpy().reshape(B, sb), hb), "the solve wrote into its input"
    body = hx[:, :ldx * r].reshape(B, r, ldx)
    assert np.all(body[:, :, n:] == SENTINEL), "the solve wrote into the padding rows n..ld-1"
    assert np.all(hx[:, ldx * r:] == SENTINEL), "the solve wrote into the gap between members"
    return np.ascontiguousarray(body[:, :, :n].transpose(2, 1, 0))


def _check_batch(bb, pr, assign, nrhs=(1, 17), selinv=True, factor=True, dev=(), dense_max=200):
    """refactorise with the prototypes' values, then every quantity of every member: the oracle for the first member of each
    prototype, the first member's bits for the others. dev: widths also run through the _dev form (same bits as the host form)"""
    B, n = len(assign), pr.n
    first, ref = _firsts(assign)
    NZ = np.asfortranarray(pr.NZ[:, assign])
    info = bb.refactorize_values(NZ)
    assert np.all(info == 0) and np.all(bb.info() == 0)
    ld = bb.logdet()
    X = {r: bb.solve(pr.R[r][:, :, assign]) for r in nrhs}
    r0 = max(nrhs)
    Xb = bb.backward_solve(pr.R[r0][:, :, assign])
    q = bb.sqmahal(pr.Xq[:, :, assign], mean=pr.mu[:, assign])
    sd = bb.selinv_diag() if selinv else None
    for r in dev:
        assert np.array_equal(_dev_solve(bb, pr.R[r][:, :, assign]), X[r]), r
    if r0 in dev:
        assert np.array_equal(_dev_solve(bb, pr.R[r0][:, :, assign], backward=True), Xb)
    perm = bb.ordering_permutation()
    for p, k in first.items():
        Qk = pr.member(p)
        F = orc.OracleFactor(Qk, perm)
        assert F.fail_col == -1
        assert abs(ld[k] - F.logdet()) <= 1e-12 * max(abs(F.logdet()), 1.0), (p, ld[k], F.logdet())
        for r in nrhs:
            assert _rel(X[r][:, :, k], F.solve(pr.R[r][:, :, p])) < 1e-10, (p, r)
        assert _rel(Xb[:, :, k], F.backward_solve(pr.R[r0][:, :, p])) < 1e-9, p
        for v in range(pr.Xq.shape[1]):
            qo = orc.sqmahal(Qk, pr.Xq[:, v, p], pr.mu[:, p])
            assert abs(q[v, k] - qo) <= 1e-12 * abs(qo), (p, v)
        if selinv:
            assert _rel(sd[:, k], F.selinv_diag()) < 1e-8, p
        if n <= dense_max:
            D = Qk.toarray()
            D = np.triu(D) + np.triu(D, 1).T
            assert abs(ld[k] - np.linalg.slogdet(D)[1]) <= 1e-11 * max(abs(ld[k]), 1.0)
            assert _rel(X[r0][:, :, k], np.linalg.solve(D, pr.R[r0][:, :, p])) < 1e-9
            if selinv:
                assert _rel(sd[:, k], np.diag(np.linalg.inv(D))) < 1e-8
    # every member: the bits of the first member of its prototype
    assert np.array_equal(ld, ld[ref])
    for r in nrhs:
        assert np.array_equal(X[r], X[r][:, :, ref]), r
    assert np.array_equal(Xb, Xb[:, :, ref])
    assert np.array_equal(q, q[:, ref])
    if selinv:
        assert np.array_equal(sd, sd[:, ref])
    if factor:
        _check_factor_bits(bb, B, n, ref)
    return dict(ld=ld, X=X, Xb=Xb, q=q, sd=sd, NZ=NZ)


def _host_quad(pr, assign, X, mu):
    """(x_vk - mu_k)' Q_k (x_vk - mu_k) for all pairs, vectorised per prototype in float64, and the sum of the absolute terms
    (the scale of the rounding error)"""
    n, nvec, B = X.shape
    q, qa = np.empty((nvec, B)), np.empty((nvec, B))
    for p in np.unique(assign):
        ks = np.flatnonzero(assign == p)
        Qp = pr.member(p)
        D = (X[:, :, ks] - mu[:, None, ks]).reshape(n, -1)
        q[:, ks] = np.einsum("ij,ij->j", D, Qp @ D).reshape(nvec, len(ks))
        qa[:, ks] = np.einsum("ij,ij->j", np.abs(D), abs(Qp) @ np.abs(D)).reshape(nvec, len(ks))
    return q, qa


def _widest_level(be, min_rows=0):
    s = gmrfx.MI355XBackend.symbolic(be)
    lv = s.level[np.diff(s.row_ptr) > min_rows]
    return int(np.bincount(lv).max()) if len(lv) else 0


# ---- 1. levels wider than 65535 fronts, batched ----------------------------------------------------------------------------

@pytest.mark.parametrize("knobs", [False, True], ids=["default", "per_level"])
def test_wide_levels_batched(knobs, monkeypatch):
    if knobs:       # every factor and sweep launch per level: no subtree tasks, no sweep tasks
        monkeypatch.setenv("GMRFX_SUBTREE_MAX", "0")
        monkeypatch.setenv("GMRFX_SWEEP_TASK_ROWS", "0")
    Q, pts = _grid(20, 20)
    B = 6000
    one = gmrfx.MI355XBackend(Q, coords=pts, symbolic_only=True)
    assert _widest_level(one) * B > 65535
    pr = Protos(Q, P=5, seed=1)
    assign = Protos.assign(B, pr.P)
    bb = gmrfx.MI355XBatchBackend(Q, B, coords=pts, device=0)
    assert _widest_level(bb) == _widest_level(one) * B
    _check_batch(bb, pr, assign, nrhs=(1, 17))
    # quadratic forms of 11 vectors per member: 66000 (vector, member) pairs, more than one grid y of k_batch_quadform
    nvec = 11
    rng = np.random.default_rng(7)
    X = rng.standard_normal((Q.shape[0], nvec, B))
    mu = rng.standard_normal((Q.shape[0], B))
    assert nvec * B > 65535
    q = bb.sqmahal(X, mean=mu)
    want, scale = _host_quad(pr, assign, X, mu)
    assert np.all(np.abs(q - want) <= 1e-12 * scale)


# ---- 2. levels wider than 65535 fronts on the generic front path ----------------------------------------------------------

def test_wide_levels_generic_fronts_plain_handle():
    K = 70000
    Q = _arrow(K)
    n = Q.shape[0]
    be = gmrfx.MI355XBackend(Q, ordering="natural", device=0)
    assert _widest_level(be, min_rows=128) > 65535
    perm = be.ordering_permutation()
    assert np.array_equal(perm, np.arange(n))
    assert be.last_info == 0
    F = orc.OracleFactor(Q, perm)
    Lo = F.L().tocsc()
    Lg = be.factor_csc()
    assert abs(Lg - Lo).max() <= 1e-12 * abs(Lo).max()
    rng = np.random.default_rng(3)
    for r in (1, 16, 64, 65):
        R = rng.standard_normal((n, r))
        assert _rel(be.backend_solve(R), F.solve(R)) < 1e-10, r
    Z = rng.standard_normal((n, 5))
    assert _rel(be.backend_backward_solve(Z), F.backward_solve(Z)) < 1e-9
    assert abs(be.compute_logdet() - F.logdet()) <= 1e-12 * abs(F.logdet())
    assert _rel(be.get_selinv_diag(), F.selinv_diag()) < 1e-8
    # Sigma on a sample of Q's upper triangle: leaf-separator couplings spread over the whole wide level, and diagonal entries
    Sig = F.selinv().tocsc()
    T = sp.triu(Q).tocoo()
    pick = rng.choice(T.nnz, 20000, replace=False)
    Bm = sp.csc_matrix((rng.standard_normal(len(pick)), (T.row[pick], T.col[pick])), shape=(n, n))
    got = be.selinv_extract_at(Bm)
    want = Sig.multiply(Bm != 0).tocsc()
    assert abs(got - want).max() <= 1e-8 * abs(want).max()
    ref = float(Sig.multiply(Bm).sum())
    assert abs(be.selinv_dot(Bm) - ref) <= 1e-8 * float(abs(Sig).multiply(abs(Bm)).sum())


def test_wide_levels_generic_fronts_batched():
    K, B = 1100, 64
    Q = _arrow(K)
    one = gmrfx.MI355XBackend(Q, ordering="natural", symbolic_only=True)
    assert _widest_level(one, min_rows=128) * B > 65535
    pr = Protos(Q, P=3, seed=2, nrhs=(1, 65))
    bb = gmrfx.MI355XBatchBackend(Q, B, ordering="natural", device=0)
    assert _widest_level(bb, min_rows=128) > 65535
    _check_batch(bb, pr, Protos.assign(B, pr.P), nrhs=(1, 65), dev=(65,))


# ---- 3. right-hand-side widths ---------------------------------------------------------------------------------------------

_WIDTHS = (1, 2, 8, 9, 16, 17, 33, 63, 64, 65, 128, 129)


def test_rhs_widths_host_and_dev_forms():
    Q, pts = _grid(20, 20)
    B = 7
    pr = Protos(Q, P=4, seed=3, nrhs=_WIDTHS)
    assign = Protos.assign(B, pr.P)
    bb = gmrfx.MI355XBatchBackend(Q, B, coords=pts, device=0)
    _check_batch(bb, pr, assign, nrhs=_WIDTHS, dev=_WIDTHS)
    first, ref = _firsts(assign)
    perm = bb.ordering_permutation()
    for r in _WIDTHS:       # backward solves at every width: host form, _dev form, oracle, prototype bits
        Z = pr.R[r][:, :, assign]
        Xb = bb.backward_solve(Z)
        assert np.array_equal(_dev_solve(bb, Z, backward=True), Xb), r
        assert np.array_equal(Xb, Xb[:, :, ref]), r
        for p, k in first.items():
            assert _rel(Xb[:, :, k], orc.OracleFactor(pr.member(p), perm).backward_solve(pr.R[r][:, :, p])) < 1e-9, (p, r)


# ---- 4. member sizes -------------------------------------------------------------------------------------------------------

def _member_case(name):
    if name == "1x1":
        return _csc(np.array([[2.0]]))
    if name in ("dense2", "dense3", "dense150"):
        return _dense(int(name[5:]))
    if name in ("grid63", "grid64", "grid65"):
        nx, ny = {"grid63": (7, 9), "grid64": (8, 8), "grid65": (5, 13)}[name]
        return _grid(nx, ny, 0.4)[0]
    if name.startswith("chain"):
        return _chain(int(name[5:]))
    if name == "disconnected":     # the member itself is a forest: 1, 7 and 40 nodes
        return _csc(sp.block_diag([sp.csc_matrix(np.array([[3.0]])), _dense(7, seed=5), _grid(5, 8, 0.4)[0]]))
    raise KeyError(name)


_SIZES = ["1x1", "dense2", "dense3", "grid63", "grid64", "grid65", "chain1023", "chain1024", "chain1025", "disconnected",
          "dense150"]


@pytest.mark.parametrize("B", [3, 65, 200])
@pytest.mark.parametrize("name", _SIZES)
def test_member_sizes(name, B):
    Q = _member_case(name)
    n = Q.shape[0]
    pr = Protos(Q, P=5 if B > 3 else 3, seed=4, nrhs=(1, 9, 65))
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    assert bb.batch_size() == (B, n)
    _check_batch(bb, pr, Protos.assign(B, pr.P), nrhs=(1, 9, 65), dev=(1, 9, 65))


# ---- 5. the stored triangle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["garbage_lower_U", "garbage_upper_L", "triu", "tril"])
def test_stored_triangle(form):
    import torch
    Q, pts = _grid(20, 20)
    n, B = Q.shape[0], 5
    pr = Protos(Q, P=3, seed=5, nrhs=(1, 9))
    assign = Protos.assign(B, pr.P)
    full = gmrfx.MI355XBatchBackend(Q, B, coords=pts, device=0)
    perm = full.ordering_permutation()
    want = _check_batch(full, pr, assign, nrhs=(1, 9), selinv=False, factor=False)
    NZf = want["NZ"]
    # the batch in the form under test: its pattern and every member's values on it
    cols, rws = np.repeat(np.arange(n), np.diff(Q.indptr)), Q.indices      # column and row of each stored entry
    rng = np.random.default_rng(6)
    if form in ("garbage_lower_U", "garbage_upper_L"):
        other = (rws > cols) if form == "garbage_lower_U" else (rws < cols)
        Qf, NZ = Q, NZf.copy(order="F")
        NZ[other, :] = 7.0 * np.abs(NZ[other, :]) + rng.uniform(1.0, 2.0, (int(other.sum()), B))
    else:
        keep = (rws <= cols) if form == "triu" else (rws >= cols)
        Qf = _csc(sp.triu(Q) if form == "triu" else sp.tril(Q))
        assert Qf.nnz == int(keep.sum())
        NZ = np.asfortranarray(NZf[keep, :])
    uplo = "L" if form in ("garbage_upper_L", "tril") else "U"
    bb = gmrfx.MI355XBatchBackend(Qf, B, ordering=perm, device=0, uplo=uplo)
    assert np.array_equal(bb.ordering_permutation(), perm)
    assert np.all(bb.refactorize_values(NZ) == 0)
    assert np.abs(bb.logdet() - want["ld"]).max() <= 1e-12 * np.abs(want["ld"]).max()
    for r in (1, 9):
        R = pr.R[r][:, :, assign]
        assert _rel(bb.solve(R), want["X"][r]) < 1e-12, r
        assert _rel(_dev_solve(bb, R), want["X"][r]) < 1e-12, r
    Xq, mu = pr.Xq[:, :, assign], pr.mu[:, assign]
    q = bb.sqmahal(Xq, mean=mu)
    assert np.all(np.abs(q - want["q"]) <= 1e-12 * np.abs(want["q"]))
    q2 = bb.sqmahal(Xq, mean=mu, nzval=2.0 * NZ)         # explicit values: twice the handle's
    assert np.all(np.abs(q2 - 2.0 * want["q"]) <= 2e-12 * np.abs(want["q"]))
    # device-pointer form with explicit values; a handle refactorised from a caller's device buffer does not hold the values
    nq = Xq.shape[1]
    d_nz = torch.from_numpy(np.ascontiguousarray(NZ.T).reshape(-1)).cuda()
    d_X = torch.from_numpy(np.ascontiguousarray(Xq.transpose(2, 1, 0)).reshape(-1)).cuda()
    d_mu = torch.from_numpy(np.ascontiguousarray(mu.T).reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert np.all(bb.refactorize_dev(d_nz.data_ptr()) == 0)
    qd = bb.quadform_dev(d_nz.data_ptr(), d_X.data_ptr(), n, n * nq, nq, d_mu.data_ptr())
    assert np.array_equal(qd, q)
    with pytest.raises(ValueError):
        bb.quadform_dev(0, d_X.data_ptr(), n, n * nq, nq, d_mu.data_ptr())


# ---- 6. pivot failures -----------------------------------------------------------------------------------------------------

def _pivot_problem():
    """a 20 x 20 Matern member plus an isolated node (a zero pivot when its value is 0)"""
    Qg, _ = _grid(20, 20)
    return _csc(sp.block_diag([Qg, sp.csc_matrix(np.array([[1.0]]))]))


def _diag_pos(Q, i):
    r = Q.indices[Q.indptr[i]:Q.indptr[i + 1]]
    return Q.indptr[i] + int(np.flatnonzero(r == i)[0])


def _break(Q, perm, nz, how):
    nz = nz.copy()
    n = Q.shape[0]
    if how == "first":
        nz[_diag_pos(Q, perm[0])] = -abs(nz[_diag_pos(Q, perm[0])])
    elif how == "last":
        nz[_diag_pos(Q, perm[n - 1])] = -1e6 * np.abs(nz).max()
    elif how == "zero":
        nz[_diag_pos(Q, n - 1)] = 0.0
    elif how == "nan":
        j = perm[n // 3]
        nz[_diag_pos(Q, j)] = np.nan
    return nz


_FAILS = {"first": {2: "first"}, "last": {4: "last"}, "zero": {1: "zero"}, "nan": {3: "nan"},
          "several": {0: "zero", 3: "first", 5: "nan", 8: "last"}}


@pytest.mark.parametrize("path", ["values", "dev", "fused"])
@pytest.mark.parametrize("case", list(_FAILS))
def test_pivot_failures(case, path):
    import torch
    Q = _pivot_problem()
    n, B = Q.shape[0], 9
    pr = Protos(Q, P=3, seed=6, nrhs=(1, 9))
    assign = Protos.assign(B, pr.P)
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    perm = bb.ordering_permutation()
    NZg = np.asfortranarray(pr.NZ[:, assign])
    NZb = NZg.copy(order="F")
    expect = np.zeros(B, np.int64)
    for k, how in _FAILS[case].items():
        NZb[:, k] = _break(Q, perm, NZg[:, k], how)
        F = orc.OracleFactor(pr.member(0, NZb[:, k]), perm)
        plain = gmrfx.MI355XBackend(pr.member(0, NZb[:, k]), ordering=perm, device=0)
        assert F.fail_col >= 0 and plain.last_info == F.fail_col + 1, (how, plain.last_info, F.fail_col)
        expect[k] = plain.last_info
        plain.close()
    if case == "first":
        assert expect[2] == 1
    if case == "last":
        assert expect[4] == n
    good = [k for k in range(B) if k not in _FAILS[case]]
    Xq, mu = pr.Xq[:, :, assign], pr.mu[:, assign]
    nq = Xq.shape[1]
    R = pr.R[9][:, :, assign]
    d_X = torch.from_numpy(np.ascontiguousarray(Xq.transpose(2, 1, 0)).reshape(-1)).cuda()
    d_mu = torch.from_numpy(np.ascontiguousarray(mu.T).reshape(-1)).cuda()

    def run(h, NZ):
        d_nz = torch.from_numpy(np.ascontiguousarray(NZ.T).reshape(-1)).cuda()
        torch.cuda.synchronize()
        if path == "values":
            info = h.refactorize_values(NZ)
            q = h.sqmahal(Xq, mean=mu)
        elif path == "dev":
            info = h.refactorize_dev(d_nz.data_ptr())
            q = h.quadform_dev(d_nz.data_ptr(), d_X.data_ptr(), n, n * nq, nq, d_mu.data_ptr())
        else:
            ld_f, q, info = h.refactorize_logpdf_dev(d_nz.data_ptr(), d_X.data_ptr(), n, n * nq, nq, d_mu.data_ptr())
            assert np.array_equal(ld_f, h.logdet(), equal_nan=True)
        return info, h.logdet(), h.solve(R), h.backward_solve(R), q

    g = run(bb, NZg)
    assert np.all(g[0] == 0)
    b = run(bb, NZb)
    assert np.array_equal(b[0], expect) and np.array_equal(bb.info(), expect)
    for want, got in zip(g[1:], b[1:]):
        assert np.array_equal(got[..., good], want[..., good])
    for k in _FAILS[case]:
        assert not np.isfinite(b[1][k])            # a flagged pivot: L_jj <= 0 or NaN
    # check_posdef: NOT_POSDEF, and info is still filled in
    bc = gmrfx.MI355XBatchBackend(Q, B, device=0, check_posdef=True)
    with pytest.raises(gmrfx.PosDefException):
        run(bc, NZb)
    assert np.array_equal(bc.info(), expect)
    # a good refactorisation restores everything, on both handles
    for h in (bb, bc):
        r = run(h, NZg)
        assert np.all(r[0] == 0)
        for want, got in zip(g[1:], r[1:]):
            assert np.array_equal(got, want)


# ---- 7. the batch entry points on a plain handle: a batch of one ------------------------------------------------------------

class _BatchOfOne(gmrfx.MI355XBatchBackend):
    """the batch entry points of a plain handle (its own handle pointer, not owned)"""

    def __init__(self, plain):
        self.n, self.nbatch, self._nnz, self._h = plain.n, 1, plain._nnz, plain._h
        self._info = np.zeros(1, np.int64)

    def close(self):
        self._h = None


_PLAIN = {"m20": lambda: _grid(20, 20),
          "m100": lambda: _grid(100, 100, 0.2, seed=2),
          "g16": lambda: (_csc(spde.matern_precision(spde.grid_mesh_3d(16, 16, 16), 0, 0.5)), spde.grid_mesh_3d(16, 16, 16).points)}


@pytest.mark.parametrize("name", list(_PLAIN))
def test_batch_entry_points_on_a_plain_handle(name):
    import torch
    Q, pts = _PLAIN[name]()
    n = Q.shape[0]
    NZ = 1.5 * Q.data + _isdiag(Q) * 0.01 * float(Q.diagonal().max())
    plain = gmrfx.MI355XBackend(Q, coords=pts, device=0)
    plain.refactorize_values(NZ)
    rng = np.random.default_rng(8)
    R = rng.standard_normal((n, 9))
    Xq = rng.standard_normal((n, 3))
    mu = rng.standard_normal(n)
    L0 = plain.factor_values()
    ld0 = plain.compute_logdet()
    X0, Xb0 = plain.backend_solve(R), plain.backend_backward_solve(R)
    q0 = plain.sqmahal(Xq, mean=mu)

    one = _BatchOfOne(plain)
    assert one.batch_size() == (1, n)
    assert np.all(one.refactorize_values(NZ[:, None]) == 0)
    assert np.array_equal(plain.factor_values(), L0)
    ld1 = one.logdet()
    assert abs(ld1[0] - ld0) <= 1e-13 * abs(ld0)           # another reduction tree than gmrfx_logdet
    assert np.array_equal(one.solve(R[:, :, None])[:, :, 0], X0)
    assert np.array_equal(one.backward_solve(R[:, :, None])[:, :, 0], Xb0)
    q1 = one.sqmahal(Xq[:, :, None], mean=mu[:, None])[:, 0]
    assert np.array_equal(q1, q0)
    d_nz = torch.from_numpy(np.ascontiguousarray(NZ)).cuda()
    d_X = torch.from_numpy(np.ascontiguousarray(Xq.T).reshape(-1)).cuda()
    d_mu = torch.from_numpy(mu.copy()).cuda()
    torch.cuda.synchronize()
    ld_f, q_f, info_f = one.refactorize_logpdf_dev(d_nz.data_ptr(), d_X.data_ptr(), n, 3 * n, 3, d_mu.data_ptr())
    assert np.all(info_f == 0) and np.array_equal(ld_f, ld1) and np.array_equal(q_f[:, 0], q0)
    # the plain entry points still give their bits
    assert np.array_equal(plain.factor_values(), L0)
    assert plain.compute_logdet() == ld0
    assert np.array_equal(plain.backend_solve(R), X0) and np.array_equal(plain.backend_backward_solve(R), Xb0)
    plain.refactorize_values(NZ)
    assert plain.last_info == 0 and np.array_equal(plain.factor_values(), L0) and plain.compute_logdet() == ld0
    assert np.array_equal(plain.sqmahal(Xq, mean=mu), q0)
    # and a clone taken afterwards
    c = plain.clone()
    assert np.array_equal(c.backend_solve(R), X0) and c.compute_logdet() == ld0
    c.close()
    one.close()
