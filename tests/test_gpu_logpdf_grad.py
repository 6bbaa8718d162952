"""Log-density gradients on Q's own pattern (csrc/grad.hip, gmrfx_logpdf_grad / gmrfx_pattern_dot and their batch forms) on the device.

Bit-exact pins (no tolerance): z = mu, ybar = 2 gives Sigma on pattern(Q) exactly as selinv_extract_at does; host and _dev forms,
two runs, any alignment / member stride of z, a batch of one and the plain call, member k of a batch and a plain handle on Q_k all
agree bit for bit; pattern_dot with one-hot columns returns w_e G[e].

Accuracy, each bound derived from the arithmetic it covers (eps = 2^-52):
  * unconstrained Qbar[e] against c (Sigma_e - r_i r_j) formed in numpy from the handle's own extracted Sigma: one subtraction and
    two products, 4 eps |ybar|/2 (|Sigma_e| + |r_i r_j|);
  * against the dense inverse: the project's tolerance for the full selected inverse, 1e-6 relative;
  * mubar_i against scipy's product: (nnz(row i) + 2) eps |ybar| sum_j |Q_ij| |r_j|;
  * the constraint terms against the long-double restatement fed the handle's OWN At and W (tests/logpdf_grad_ref.py): per entry
    max(64 E_e, 16 eps S_e), E_e = the error the float64 restatement itself shows against the long-double one at that entry, S_e
    the term's absolute sum. The Qbar term is recovered as (unconstrained Qbar of the same handle) - (constrained Qbar): the final
    subtraction of the documented formula rounds once more, eps |Qbar_e|, which is added to the bound; likewise eps |mubar_i|;
  * pattern_dot: chunk-length eps sum |w G J| (4096 entries per chunk, then at most 4096 chunk sums).
Shapes: n = 1, 2, 3; n at the pattern kernel's workgroup (64 columns) and the mean kernel's (16 rows) and one more / less; an arrowhead
whose hub column has more entries than a 16-lane group takes in a pass; nnz at the contraction's chunk (4096) and one more / less;
p = 1 and 5 with ldj > nnz; index_base 1; uplo L / U with 1e30 in the other triangle; explicit stored zeros; a 40 x 40 grid (small
fronts, sweep-task fronts, multi-block fronts); m = 1, 2, 63, 64; B = 1, 2, 3 with a member that is not positive definite and,
separately, one whose W alone is rank deficient (rows a1 and a1 + e_d of A, Q_dd = 1e20 in that member): NaN and info > 0 for that
member only, the others bit-equal to the run without it; two equal rows of A (every W_k singular); refactorisation with new values; a
clone."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import logpdf_grad_ref as ref
from gmrfx._lib import GmrfxOpts, lib, ptr
from layout_buffers import same_bits

pytestmark = pytest.mark.gpu
EPS = ref.EPS


# ---- patterns ----------------------------------------------------------------------------------------------------------------------
def _csc(D):
    Q = sp.csc_matrix(D)
    Q.sort_indices()
    return Q


def tridiag(n, extra_pairs=0):
    """diagonally dominant tridiagonal matrix, both triangles, plus `extra_pairs` symmetric long-range pairs: nnz = 3n - 2 + 2 pairs"""
    rng = np.random.default_rng(n + 7 * extra_pairs)
    i = np.arange(n - 1)
    off = -rng.uniform(0.2, 1.0, max(n - 1, 0))
    T = sp.coo_matrix((np.r_[off, off], (np.r_[i, i + 1], np.r_[i + 1, i])), shape=(n, n)).tolil()
    for k in range(extra_pairs):
        T[5 * k, 5 * k + 3] = T[5 * k + 3, 5 * k] = -0.1
    T = sp.csc_matrix(T)
    d = np.asarray(abs(T).sum(1)).ravel() + rng.uniform(0.5, 1.5, n)
    return _csc(T + sp.diags(d))


def grid(nx, ny):
    ex, ey = np.ones(nx), np.ones(ny)
    Lx = sp.diags([-ex[:-1], 2 * ex, -ex[:-1]], [-1, 0, 1])
    Ly = sp.diags([-ey[:-1], 2 * ey, -ey[:-1]], [-1, 0, 1])
    return _csc(sp.kron(sp.eye(ny), Lx) + sp.kron(Ly, sp.eye(nx)) + 0.3 * sp.eye(nx * ny))


def arrowhead(n):
    D = np.diag(np.full(n, 3.0 + n / 8))
    D[0, 1:] = D[1:, 0] = -0.1
    return _csc(D)


def _vectors(n, seed=0):
    rng = np.random.default_rng(seed + n)
    return rng.standard_normal(n), 0.5 * rng.standard_normal(n)


def _cols(Q):
    return np.repeat(np.arange(Q.shape[1]), np.diff(Q.indptr))


# ---- the checks every pattern goes through -----------------------------------------------------------------------------------------
def _check_unconstrained(Q, uplo="U", be=None):
    n = Q.shape[0]
    own = be is None
    be = be or gmrfx.MI355XBackend(Q, device=0, uplo=uplo)
    try:
        z, mu = _vectors(n)
        rows, cols = Q.indices, _cols(Q)
        sig = be.selinv_extract_at(Q).data
        # bit pin: r = 0 and c = 1 leave Sigma itself
        Q0, m0 = be.logpdf_grad(mu, mean=mu, ybar=2.0)
        assert same_bits(Q0.data, sig)
        assert np.array_equal(m0, np.zeros(n))
        ybar = -1.3
        Qb, mb = be.logpdf_grad(z, mean=mu, ybar=ybar)
        Qb2, mb2 = be.logpdf_grad(z, mean=mu, ybar=ybar)
        assert same_bits(Qb.data, Qb2.data) and same_bits(mb, mb2)
        r = z - mu
        rr = r[rows] * r[cols]
        want = 0.5 * ybar * (sig - rr)
        bound = 4 * EPS * abs(ybar) / 2 * (np.abs(sig) + np.abs(rr))
        err = np.abs(Qb.data - want)
        print(f"n={n} nnz={Q.nnz}: Qbar max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
        S = ref.symmetric_dense(Q, "L" if uplo == "L" else "U")
        Qd, md = ref.grad_dense(S, z, mu, ybar)
        assert np.abs(Qb.data - ref.on_pattern(Qd, Q)).max() <= 1e-6 * np.abs(Qd).max()
        Ss = sp.csr_matrix(S)
        Sa = abs(Ss)
        mbound = (np.diff(Ss.indptr) + 2) * EPS * abs(ybar) * (Sa @ np.abs(r))
        merr = np.abs(mb - ybar * (Ss @ r))
        print(f"n={n}: mubar max err / bound {np.max(merr / np.maximum(mbound, 1e-300)):.3f}")
        assert (merr <= mbound).all()
        # zero mean as None
        Qn, mn = be.logpdf_grad(z, ybar=ybar)
        Qz, mz = be.logpdf_grad(z, mean=np.zeros(n), ybar=ybar)
        assert same_bits(Qn.data, Qz.data) and same_bits(mn, mz)
        return Qb.data.copy(), mb.copy()
    finally:
        if own:
            be.close()


@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 63, 64, 65, 129])
def test_tridiagonal_sizes_at_the_workgroup_edges(n):
    _check_unconstrained(tridiag(n))


def test_arrowhead_hub_column_takes_several_passes():
    _check_unconstrained(arrowhead(70))       # the hub column and row: 70 entries, 5 passes of 16 lanes


def test_grid_40x40_fronts_of_every_kind():
    Q = grid(40, 40)
    _check_unconstrained(Q)


@pytest.mark.parametrize("uplo", ["L", "U"])
def test_unused_triangle_is_never_read(uplo):
    Q = grid(9, 7)
    clean, mclean = _check_unconstrained(Q, uplo)
    junk = Q.copy()
    cols = _cols(Q)
    junk.data[(Q.indices < cols) if uplo == "L" else (Q.indices > cols)] = 1e30
    be = gmrfx.MI355XBackend(junk, device=0, uplo=uplo)
    try:
        z, mu = _vectors(Q.shape[0])
        Qb, mb = be.logpdf_grad(z, mean=mu, ybar=-1.3)
        assert same_bits(Qb.data, clean) and same_bits(mb, mclean)      # every entry gets its value, whichever triangle it lies in
    finally:
        be.close()


def test_explicit_stored_zeros_are_entries():
    Q = tridiag(40)
    D = Q.tolil()
    pairs = [(0, 2), (10, 12), (30, 33)]
    for i, j in pairs:
        D[i, j] = D[j, i] = 7.0
    P = _csc(sp.csc_matrix(D))
    for i, j in pairs:          # stored, value zero
        for a, b in ((i, j), (j, i)):
            k = P.indptr[b] + int(np.flatnonzero(P.indices[P.indptr[b]:P.indptr[b + 1]] == a)[0])
            P.data[k] = 0.0
    assert P.nnz == Q.nnz + 6
    _check_unconstrained(P)


def test_index_base_one_gives_the_same_bits():
    Q = grid(6, 5)
    n, nnz = Q.shape[0], Q.nnz
    z, mu = _vectors(n)
    be = gmrfx.MI355XBackend(Q, device=0)
    want_q, want_m = be.logpdf_grad(z, mean=mu, ybar=0.7)
    perm = be.ordering_permutation()
    be.close()
    o = GmrfxOpts()
    o.struct_size = C.sizeof(GmrfxOpts)
    o.device = 0
    h = C.c_void_p()
    cp, ri = (Q.indptr + 1).astype(np.int64), (Q.indices + 1).astype(np.int64)
    p1 = np.ascontiguousarray(perm + 1, dtype=np.int64)
    assert lib().gmrfx_create(n, ptr(cp), ptr(ri), 1, ptr(p1), C.byref(o), C.byref(h)) == 0
    try:
        info = C.c_int64(0)
        assert lib().gmrfx_refactorize(h, ptr(np.ascontiguousarray(Q.data)), C.byref(info)) == 0
        qb, mb = np.empty(nnz), np.empty(n)
        assert lib().gmrfx_logpdf_grad(h, None, ptr(z), ptr(mu), 0.7, ptr(qb), ptr(mb)) == 0
        assert same_bits(qb, want_q.data) and same_bits(mb, want_m)
    finally:
        lib().gmrfx_destroy(h)


def test_refactorize_drops_the_caches_and_a_clone_gives_the_same_bits():
    Q = grid(12, 11)
    n = Q.shape[0]
    z, mu = _vectors(n)
    A, e = ref.sum_to_zero(n, 2)
    be = gmrfx.MI355XBackend(Q, device=0)
    fresh = None
    try:
        be.set_constraints(A, e)
        first = be.logpdf_grad(z, mean=mu)
        Q2 = Q.copy()
        Q2.data = Q.data * 1.5
        be.refactorize_values(Q2.data)
        second = be.logpdf_grad(z, mean=mu)
        fresh = gmrfx.MI355XBackend(Q2, device=0)
        fresh.set_constraints(A, e)
        want = fresh.logpdf_grad(z, mean=mu)
        assert same_bits(second[0].data, want[0].data) and same_bits(second[1], want[1])
        assert not same_bits(second[0].data, first[0].data)
        cl = be.clone()
        try:
            got = cl.logpdf_grad(z, mean=mu, nzval=Q2.data)        # (a clone does not hold Q's values)
            assert same_bits(got[0].data, want[0].data) and same_bits(got[1], want[1])
        finally:
            cl.close()
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


# ---- device-pointer forms ------------------------------------------------------------------------------------------------------------
def test_dev_forms_alignment_and_stride():
    import torch
    Q = grid(10, 9)
    n, nnz = Q.shape[0], Q.nnz
    z, mu = _vectors(n)
    be = gmrfx.MI355XBackend(Q, device=0)
    bb = gmrfx.MI355XBatchBackend(Q, 2, device=0)
    try:
        want_q, want_m = be.logpdf_grad(z, mean=mu, ybar=0.9)
        for off in (0, 1, 3):       # 16-byte aligned, then 8-byte aligned only
            dz = torch.full((n + 8,), float("nan"), dtype=torch.float64, device="cuda")
            dz[off:off + n] = torch.from_numpy(z).cuda()
            dm = torch.from_numpy(mu).cuda()
            dq = torch.zeros(nnz + 4, dtype=torch.float64, device="cuda")
            do = torch.zeros(n + 4, dtype=torch.float64, device="cuda")
            dn = torch.from_numpy(Q.data.copy()).cuda()
            torch.cuda.synchronize()
            be.logpdf_grad_dev(dz.data_ptr() + 8 * off, dq.data_ptr() + 8 * (off % 2), do.data_ptr() + 8 * (off % 2), dm.data_ptr(), 0.9, dn.data_ptr())
            torch.cuda.synchronize()
            o2 = off % 2
            assert same_bits(dq.cpu().numpy()[o2:o2 + nnz], want_q.data) and same_bits(do.cpu().numpy()[o2:o2 + n], want_m)
            assert (dq.cpu().numpy()[o2 + nnz:] == 0).all() and (do.cpu().numpy()[o2 + n:] == 0).all()
        # members with a stride: z of member k at + k sz
        NZ = np.stack([Q.data, 1.7 * Q.data], axis=1)
        bb.refactorize_values(NZ)
        Z = np.stack([z, mu + 1.0], axis=1)
        hq, hm, hinfo = bb.logpdf_grad(Z, mean=mu, ybar=[0.9, -0.4])
        assert (hinfo == 0).all()
        for sz, off in ((n, 0), (n + 3, 1), (2 * n + 1, 0)):
            dz = torch.full((off + 2 * sz + 4,), float("nan"), dtype=torch.float64, device="cuda")
            for k in range(2):
                dz[off + k * sz: off + k * sz + n] = torch.from_numpy(Z[:, k].copy()).cuda()
            dm = torch.from_numpy(np.concatenate([mu, mu])).cuda()
            dq = torch.zeros(2 * nnz, dtype=torch.float64, device="cuda")
            do = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            info = bb.logpdf_grad_dev(dz.data_ptr() + 8 * off, sz, [0.9, -0.4], dq.data_ptr(), do.data_ptr(), dm.data_ptr())
            torch.cuda.synchronize()
            assert (info == 0).all()
            assert same_bits(dq.cpu().numpy(), hq.ravel(order="F")) and same_bits(do.cpu().numpy(), hm.ravel(order="F"))
        # the contraction, host against device operands
        J = np.asfortranarray(np.random.default_rng(3).standard_normal((nnz, 5)))
        hd = be.pattern_dot(want_q, J)
        ld = nnz + 3
        dJ = torch.full((ld * 5 + 1,), float("nan"), dtype=torch.float64, device="cuda")
        for k in range(5):
            dJ[1 + k * ld: 1 + k * ld + nnz] = torch.from_numpy(J[:, k].copy()).cuda()
        dG = torch.from_numpy(want_q.data.copy()).cuda()
        torch.cuda.synchronize()
        assert same_bits(be.pattern_dot_dev(dG.data_ptr(), dJ.data_ptr() + 8, ld, 5), hd)
        assert same_bits(be.pattern_dot_dev(dG.data_ptr(), dJ.data_ptr() + 8, ld, 1), hd[:1])
    finally:
        be.close()
        bb.close()


# ---- the contraction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pairs,nnz", [(1365, 1, 4095), (1366, 0, 4096), (1365, 2, 4097), (5, 0, 13)])
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_pattern_dot_at_the_chunk_edges(n, pairs, nnz, uplo):
    Q = tridiag(n, pairs)
    assert Q.nnz == nnz
    rng = np.random.default_rng(nnz)
    be = gmrfx.MI355XBackend(Q, device=0, uplo=uplo, factorize=False)
    try:
        w = ref.weights(Q, uplo)
        G = rng.standard_normal(nnz)
        for p in (1, 5):
            J = rng.standard_normal((nnz, p))
            got = be.pattern_dot(G, J)
            bound = 4096 * EPS * (np.abs(w * G) @ np.abs(J))
            assert (np.abs(got - (w * G) @ J) <= bound).all()
            # the host form with ldj > nnz (the stager packs the columns), plain and as a batch of one with a member stride
            ld = nnz + 3
            Jp = np.full(ld * p + 2, np.nan)
            for k in range(p):
                Jp[k * ld: k * ld + nnz] = J[:, k]
            out = np.empty(p)
            assert lib().gmrfx_pattern_dot(be._h, ptr(G), ptr(Jp), ld, p, ptr(out)) == 0
            assert same_bits(out, got)
            assert lib().gmrfx_batch_pattern_dot(be._h, ptr(G), ptr(Jp), ld, ld * p + 2, p, ptr(out)) == 0
            assert same_bits(out, got)
        # one-hot columns pick w_e G[e] exactly: the first and last entry, the chunk's last and the next chunk's first
        picks = sorted({0, nnz - 1, min(4095, nnz - 1), min(4096, nnz - 1), nnz // 2})
        J = np.zeros((nnz, len(picks)))
        J[picks, np.arange(len(picks))] = 1.0
        assert np.array_equal(be.pattern_dot(G, J), w[picks] * G[picks])
    finally:
        be.close()


# ---- constraints ---------------------------------------------------------------------------------------------------------------------
def _check_constrained(be, Q, A, e, z, mu, ybar):
    """be holds Q's factorisation; returns the largest ratio error / bound over both constraint terms"""
    n = Q.shape[0]
    be.clear_constraints()
    Q0, m0 = be.logpdf_grad(z, mean=mu, ybar=ybar)
    be.set_constraints(A, e)
    Q1, m1 = be.logpdf_grad(z, mean=mu, ybar=ybar)
    Q2, m2 = be.logpdf_grad(z, mean=mu, ybar=ybar)
    assert same_bits(Q1.data, Q2.data) and same_bits(m1, m2)
    At, W = be.constraint_fields()
    T64, S, a64, aS = ref.constraint_terms(At, W, A, e, mu)
    Tld, _, ald, _ = ref.constraint_terms(At, W, A, e, mu, np.longdouble)
    c = 0.5 * ybar
    E_q = np.abs((ref.on_pattern(T64, Q) - ref.on_pattern(Tld, Q)).astype(np.float64)) * abs(c)        # per entry
    E_m = np.abs((a64 - ald).astype(np.float64)) * abs(ybar)
    term_q = Q0.data - Q1.data
    want_q = (c * ref.on_pattern(Tld, Q)).astype(np.float64)
    bound_q = np.maximum(64 * E_q, 16 * EPS * abs(c) * ref.on_pattern(S, Q)) + EPS * np.abs(Q1.data)
    term_m = m0 - m1
    want_m = (ybar * ald).astype(np.float64)
    bound_m = np.maximum(64 * E_m, 16 * EPS * abs(ybar) * aS) + EPS * np.abs(m1)
    rq = np.max(np.abs(term_q - want_q) / bound_q)
    rm = np.max(np.abs(term_m - want_m) / bound_m)
    print(f"n={n} m={A.shape[0]}: constraint terms, largest error / bound: Qbar {rq:.3f} mubar {rm:.3f} (largest E_q {E_q.max():.2e} E_m {E_m.max():.2e})")
    assert rq <= 1 and rm <= 1
    # and the whole gradient against the dense restatement
    Qd, md = ref.grad_dense(ref.symmetric_dense(Q, "U"), z, mu, ybar, A, e)
    assert np.abs(Q1.data - ref.on_pattern(Qd, Q)).max() <= 1e-6 * np.abs(Qd).max()
    assert np.abs(m1 - md).max() <= 1e-6 * np.abs(md).max()
    return max(rq, rm)


@pytest.mark.parametrize("m", [1, 2, 63, 64])
def test_constraint_terms_on_the_grid(m):
    Q = grid(40, 40) if m >= 63 else grid(13, 11)
    n = Q.shape[0]
    z, mu = _vectors(n, 1)
    A, e = ref.sum_to_zero(n, m)
    be = gmrfx.MI355XBackend(Q, device=0)
    try:
        _check_constrained(be, Q, A, e, z, mu, 1.4)
        # z = mu + constrained residual zero is nothing special; a zero mean passed as None
        be.set_constraints(A, e)
        a = be.logpdf_grad(z, ybar=1.4)
        b = be.logpdf_grad(z, mean=np.zeros(n), ybar=1.4)
        assert same_bits(a[0].data, b[0].data) and same_bits(a[1], b[1])
    finally:
        be.close()


@pytest.mark.parametrize("n,m", [(1, 1), (3, 2), (65, 3)])
def test_constraint_terms_on_tiny_and_edge_sizes(n, m):
    Q = tridiag(n)
    z, mu = _vectors(n, 2)
    A, e = ref.sum_to_zero(n, m)
    be = gmrfx.MI355XBackend(Q, device=0)
    try:
        _check_constrained(be, Q, A, e, z, mu, -0.8)
    finally:
        be.close()


def test_rank_deficient_w_is_not_posdef_for_a_plain_handle():
    Q = tridiag(20)
    A = sp.csr_matrix(np.vstack([np.ones(20), np.ones(20)]))
    be = gmrfx.MI355XBackend(Q, device=0)
    try:
        be.set_constraints(A, np.zeros(2))
        with pytest.raises(gmrfx._lib.PosDefException):
            be.logpdf_grad(np.zeros(20))
    finally:
        be.close()


def test_not_factorized_is_reported():
    Q = tridiag(20)
    be = gmrfx.MI355XBackend(Q, device=0, factorize=False)
    try:
        with pytest.raises(gmrfx._lib.GmrfxError) as ei:
            be.logpdf_grad(np.zeros(20))
        assert ei.value.code == 4
    finally:
        be.close()


# ---- batched handles -----------------------------------------------------------------------------------------------------------------
def _member_values(Q, B):
    return np.stack([(1.0 + 0.35 * k) * Q.data for k in range(B)], axis=1)


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("m", [0, 2])
def test_members_equal_plain_handles(B, m):
    Q = grid(9, 8)
    n, nnz = Q.shape[0], Q.nnz
    NZ = _member_values(Q, B)
    rng = np.random.default_rng(B)
    Z, MU = rng.standard_normal((n, B)), rng.standard_normal((n, B))
    yb = np.array([1.0, -0.6, 2.5])[:B]
    A, e = ref.sum_to_zero(n, 2)
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    try:
        bb.refactorize_values(NZ)
        if m:
            bb.set_constraints(A, e)
        qb, mb, info = bb.logpdf_grad(Z, mean=MU, ybar=yb)
        assert (info == 0).all()
        J = rng.standard_normal((nnz, 5, B))
        dots = bb.pattern_dot(qb, J)
        for k in range(B):
            Qk = sp.csc_matrix((NZ[:, k], Q.indices, Q.indptr), shape=Q.shape)
            be = gmrfx.MI355XBackend(Qk, device=0)
            try:
                if m:
                    be.set_constraints(A, e)
                pq, pm = be.logpdf_grad(Z[:, k], mean=MU[:, k], ybar=yb[k])
                assert same_bits(qb[:, k], pq.data) and same_bits(mb[:, k], pm), f"member {k}"
                assert same_bits(dots[:, k], be.pattern_dot(pq, J[:, :, k]))
            finally:
                be.close()
    finally:
        bb.close()


def test_a_plain_handle_is_a_batch_of_one():
    Q = grid(7, 6)
    n, nnz = Q.shape[0], Q.nnz
    z, mu = _vectors(n)
    be = gmrfx.MI355XBackend(Q, device=0)
    try:
        A, e = ref.sum_to_zero(n, 3)
        for con in (False, True):
            if con:
                be.set_constraints(A, e)
            pq, pm = be.logpdf_grad(z, mean=mu, ybar=0.3)
            qb, mb, info, yb = np.empty(nnz), np.empty(n), np.zeros(1, np.int64), np.array([0.3])
            rc = lib().gmrfx_batch_logpdf_grad(be._h, None, ptr(z), n, ptr(mu), ptr(yb), ptr(qb), ptr(mb), ptr(info))
            assert rc == 0 and info[0] == 0
            assert same_bits(qb, pq.data) and same_bits(mb, pm)
            J = np.asfortranarray(np.random.default_rng(1).standard_normal((nnz, 2)))
            out = np.empty(2)
            assert lib().gmrfx_batch_pattern_dot(be._h, ptr(qb), ptr(J), nnz, 2 * nnz, 2, ptr(out)) == 0
            assert same_bits(out, be.pattern_dot(pq, J))
    finally:
        be.close()


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("fault", ["not_posdef", "rank_deficient_w", "equal_rows"])
def test_a_failed_member_gets_nan_and_disturbs_nobody(B, fault):
    """not_posdef: member `bad` has a negative diagonal. rank_deficient_w: the rows of A are a1 and a2 = a1 + e_d, and member `bad` alone
    has Q_dd = 1e20 (still positive definite): its Sigma(d, .) is about 1e-20, the two rows of its W agree to rounding and the relative
    pivot test of the preparation fails for that member only, while the others keep a well-conditioned W. equal_rows: two equal rows of A
    make W_k singular for every member."""
    Q = grid(8, 7)
    n, nnz = Q.shape[0], Q.nnz
    NZ = _member_values(Q, B)
    rng = np.random.default_rng(10 + B)
    Z, MU = rng.standard_normal((n, B)), rng.standard_normal((n, B))
    bad = B - 2
    d = 20
    if fault == "rank_deficient_w":
        a1 = np.ones(n)
        a2 = a1.copy()
        a2[d] += 1.0
        A, e = sp.csr_matrix(np.vstack([a1, a2])), np.array([0.1, -0.2])
    else:
        A, e = ref.sum_to_zero(n, 2)
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    try:
        bb.refactorize_values(NZ)
        bb.set_constraints(A, e)
        want_q, want_m, info = bb.logpdf_grad(Z, mean=MU, ybar=1.1)       # every member with ordinary values: all fine
        assert (info == 0).all() and np.isfinite(want_q).all() and np.isfinite(want_m).all()
        if fault in ("not_posdef", "rank_deficient_w"):
            NZb = NZ.copy()
            diag = Q.indices == _cols(Q)
            if fault == "not_posdef":
                NZb[diag, bad] = -NZb[diag, bad]
            else:
                NZb[np.flatnonzero(diag)[d], bad] = 1e20
            finfo = bb.refactorize_values(NZb)
            qb, mb, info = bb.logpdf_grad(Z, mean=MU, ybar=1.1, nzval=NZb)
            if fault == "not_posdef":
                assert info[bad] == -1
            else:
                assert (finfo == 0).all() and info[bad] > 0        # the factorisation is fine; 1 + the failing pivot of W_k
            assert (np.delete(info, bad) == 0).all()
            assert np.isnan(qb[:, bad]).all() and np.isnan(mb[:, bad]).all()
            for k in range(B):
                if k != bad:
                    assert same_bits(qb[:, k], want_q[:, k]) and same_bits(mb[:, k], want_m[:, k])
        else:
            bb.set_constraints(sp.csr_matrix(np.vstack([np.ones(n), np.ones(n)])), np.zeros(2))
            qb, mb, info = bb.logpdf_grad(Z, mean=MU, ybar=1.1)
            assert (info > 0).all()           # 1 + the failing pivot of W_k
            assert np.isnan(qb).all() and np.isnan(mb).all()
            bb.clear_constraints()
            q0, m0, info = bb.logpdf_grad(Z, mean=MU, ybar=1.1)
            assert (info == 0).all() and np.isfinite(q0).all() and np.isfinite(m0).all()
    finally:
        bb.close()
