"""The read-out kernels -- log det (csrc/util_kernels.hip, csrc/batch.hip), quadratic forms (csrc/quadform.hip, csrc/batch.hip), the
gathers and segment sums over the selected inverse (csrc/util_kernels.hip), the dense operator and the transpose (csrc/dense.hip) --
at every launch edge.

Cases: tests/readout_edges.py (each names its edge; tests/test_readout_edges_host.py checks without a device that it is reached).
Reference: tests/readout_ref.py in np.longdouble, FED the handle's own inputs (the diagonal of factor_values(), selinv_extract_at of
the same handle), so that these kernels are judged on their own arithmetic. Bounds: the first-order bounds derived in the docstring of
tests/readout_ref.py, times the project's factor 16; the control of the host test holds them without that factor on the CPU.

Every call is issued twice and must return the same bits; the exact pins (gathers, masked entries, the unused triangle, mu absent
against mu = 0, fused against separate calls, batched against plain handles, padded and offset device buffers) compare raw words.
Every test prints its largest error / bound ratio (pytest -rP)."""
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gmrfx
import layout_buffers as lb
import readout_edges as re_
import readout_ref as rr
from layout_buffers import same_bits

pytestmark = pytest.mark.gpu
LD = rr.LD


def _device(a):
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert d.data_ptr() % 16 == 0
    return d


def _report(tag, ratios):
    print(f"{tag}: error/bound " + " ".join(f"{k} {v:.3g}" for k, v in sorted(ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _add(ratios, key, got, ref):
    ratios[key] = max(ratios.get(key, 0.0), rr.ratio(got, ref["value"], rr.bound_sum(ref)))


def factor_diag(be):
    """diag L in elimination order from factor_values(): column f + j of supernode s sits at panel_ptr[s] + j (ld[s] + 1)"""
    sy = gmrfx.MI355XBackend.symbolic(be)
    ncol = np.diff(sy.super_first)
    s = np.repeat(np.arange(len(ncol)), ncol)
    j = np.arange(int(ncol.sum())) - sy.super_first[s]
    return be.factor_values()[sy.panel_ptr[s] + j * (sy.panel_ld[s] + 1)]


# ---- log det -----------------------------------------------------------------------------------------------------------------------------
def _check_logdet(be, Q, tag):
    d = factor_diag(be)
    assert len(d) == Q.shape[0] and (d > 0).all()
    ref = rr.logdet(d, LD)
    got = be.compute_logdet()
    ratios = {}
    _add(ratios, "logdet", got, ref)
    # a second evaluation (the value is kept per factorisation: factor again), and the fused call
    be.refactorize_values(Q.data)
    assert same_bits(factor_diag(be), d) and same_bits(np.float64(be.compute_logdet()), np.float64(got)), tag
    d_nz = _device(Q.data)
    torch.cuda.synchronize()
    _, ld = be.refactorize_logpdf_dev(d_nz.data_ptr(), 0, Q.shape[0], 0)
    assert same_bits(np.float64(ld), np.float64(got)), tag
    _report(tag, ratios)


@pytest.mark.parametrize("kind", ["plain", "spread"])
@pytest.mark.parametrize("n", re_.LOGDET_CHAINS)
def test_logdet_chain(n, kind):
    Q = re_.chain(n, kind)
    be = gmrfx.MI355XBackend(Q, ordering="natural", device=0)
    assert be.last_info == 0
    _check_logdet(be, Q, f"logdet n={n} {kind}")
    be.close()


@pytest.fixture(scope="module")
def big_chains():
    """the two handles of n = 262144 and 262145: the only sizes at which per reaches 256 / exceeds it; built once"""
    out = {}
    for n, kind in re_.LOGDET_BIG:
        Q = re_.chain(n, kind)
        t0 = time.perf_counter()
        be = gmrfx.MI355XBackend(Q, device=0)
        print(f"chain n={n} {kind}: handle built in {time.perf_counter() - t0:.2f} s")
        assert be.last_info == 0
        out[n] = (Q, be)
    yield out
    for _, be in out.values():
        be.close()


@pytest.mark.parametrize("n,kind", re_.LOGDET_BIG)
def test_logdet_big_chain(big_chains, n, kind):
    Q, be = big_chains[n]
    t0 = time.perf_counter()
    _check_logdet(be, Q, f"logdet n={n} {kind}")
    print(f"checked in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("B", re_.BATCH_B)
@pytest.mark.parametrize("nm", re_.BATCH_NM)
def test_batched_logdet_per_member(nm, B):
    Q = re_.chain(nm, "spread" if nm > 1 else "plain")
    NZ = re_.member_values(Q, B)
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    info = bb.refactorize_values(NZ)
    assert not info.any()
    ld = bb.logdet()
    assert same_bits(bb.logdet(), ld)
    diag = factor_diag(bb).reshape(B, nm)
    ratios = {}
    for k in range(B):
        assert rr.batch_info(diag[k]) == 0
        _add(ratios, "logdet", ld[k], rr.batch_logdet(diag[k], LD))
    if B == 3 and nm in (1025, 2049):
        # two failing pivots of member 1 in different parts and threads: info is the smaller column + 1, the others keep their bits
        ca, cb = re_.failing_columns(nm)
        perm = bb.ordering_permutation()
        NZb = NZ.copy(order="F")
        for c in (ca, cb):
            node = int(perm[c])
            p = int(Q.indptr[node] + np.flatnonzero(Q.indices[Q.indptr[node]:Q.indptr[node + 1]] == node)[0])
            NZb[p, 1] = -1e3 * abs(NZb[p, 1])
        info = bb.refactorize_values(NZb)
        db = factor_diag(bb).reshape(B, nm)
        assert not (db[1, ca] > 0) and not (db[1, cb] > 0) and (db[1, :ca] > 0).all()
        assert list(info) == [0, ca + 1, 0] and list(bb.info()) == [0, ca + 1, 0] and rr.batch_info(db[1]) == ca + 1
        ldb = bb.logdet()
        assert same_bits(ldb[[0, 2]], ld[[0, 2]]) and not np.isfinite(ldb[1])
        assert not bb.refactorize_values(NZ).any() and same_bits(bb.logdet(), ld)
    _report(f"batchdiag nm={nm} B={B}", ratios)
    bb.close()


# ---- quadratic forms -------------------------------------------------------------------------------------------------------------------------
def _quad_matrices():
    out = [(f"chain{n}", n) for n in re_.QUAD_N]
    return out + [(f"hub{k}_at{hub}", (k, hub)) for k in re_.HUB_ENTRIES for hub in (0, re_.HUB_N - 1)]


def _quad_Q(spec):
    return re_.chain(spec) if isinstance(spec, int) else re_.arrowhead(*spec)


@pytest.mark.parametrize("uplo", ["U", "L"])
@pytest.mark.parametrize("name,spec", _quad_matrices(), ids=[m[0] for m in _quad_matrices()])
def test_quadform_plain_and_batched(name, spec, uplo):
    Q = _quad_Q(spec)
    n, B, use_lower = Q.shape[0], 3, uplo == "L"
    be = gmrfx.MI355XBackend(Q, uplo=uplo, device=0)
    bb = gmrfx.MI355XBatchBackend(Q, B, uplo=uplo, device=0)
    NZ = re_.member_values(Q, B)
    assert not bb.refactorize_values(NZ).any()
    ratios = {}
    for nvec in re_.QUAD_NVEC:
        X, mu = re_.quad_operands(n, nvec)
        got, got0 = be.sqmahal(X, mean=mu), be.sqmahal(X)
        _add(ratios, "plain", got, rr.quadform(Q.indptr, Q.indices, Q.data, X, mu, use_lower, LD))
        _add(ratios, "plain_nomu", got0, rr.quadform(Q.indptr, Q.indices, Q.data, X, None, use_lower, LD))
        assert same_bits(be.sqmahal(X, mean=mu), got) and same_bits(be.sqmahal(X, mean=mu, nzval=Q.data), got)
        assert same_bits(be.sqmahal(X, mean=np.zeros(n)), got0), "mu = 0 is not mu absent"
        Xb = np.stack([np.roll(X, k, axis=0) for k in range(B)], axis=-1)
        mub = np.stack([mu + 0.125 * k for k in range(B)], axis=-1)
        gb, gb0 = bb.sqmahal(Xb, mean=mub), bb.sqmahal(Xb)
        assert same_bits(bb.sqmahal(Xb, mean=mub), gb) and same_bits(bb.sqmahal(Xb, mean=np.zeros((n, B))), gb0)
        for k in range(B):
            _add(ratios, "batched", gb[:, k], rr.quadform(Q.indptr, Q.indices, NZ[:, k], Xb[:, :, k], mub[:, k], use_lower, LD))
            _add(ratios, "batched_nomu", gb0[:, k], rr.quadform(Q.indptr, Q.indices, NZ[:, k], Xb[:, :, k], None, use_lower, LD))
            assert same_bits(be.sqmahal(Xb[:, :, k], mean=mub[:, k], nzval=NZ[:, k]), gb[:, k]), "a member differs from the plain handle"
    _report(f"quad {name} {uplo}", ratios)
    be.close()
    bb.close()


@pytest.mark.parametrize("uplo", ["U", "L"])
def test_quadform_pins(uplo):
    n, nvec, use_lower = 129, 7, uplo == "L"
    Q = re_.chain(n)
    be = gmrfx.MI355XBackend(Q, uplo=uplo, device=0)
    X, mu = re_.quad_operands(n, nvec)
    want = be.sqmahal(X, mean=mu)
    ratios = {}
    # 1e30 in the triangle that does not define Q: the same bits, not a tolerance
    dirty = Q.data.copy()
    dirty[re_.unused_triangle(Q, use_lower)] = 1e30
    assert same_bits(be.sqmahal(X, mean=mu, nzval=dirty), want) and same_bits(be.sqmahal(X, nzval=dirty), be.sqmahal(X))
    # explicit stored zeros; x - mu of order 1e-8 |x|
    z = re_.with_stored_zeros(Q)
    _add(ratios, "stored_zeros", be.sqmahal(X, mean=mu, nzval=z), rr.quadform(Q.indptr, Q.indices, z, X, mu, use_lower, LD))
    Xn = mu[:, None] * (1 + 1e-8 * X)
    _add(ratios, "near_mean", be.sqmahal(Xn, mean=mu), rr.quadform(Q.indptr, Q.indices, Q.data, Xn, mu, use_lower, LD))
    _add(ratios, "near_mean_zeros", be.sqmahal(Xn, mean=mu, nzval=z), rr.quadform(Q.indptr, Q.indices, z, Xn, mu, use_lower, LD))
    # device buffers: ldx > n with NaN in the padding, base aligned to 8 bytes only
    d_nz, d_mu = _device(Q.data), _device(mu)
    for pad, off in ((0, 0), (3, 0), (3, 1), (4, 1)):
        buf = _device(lb.input_buffer(X, n + pad, off))
        torch.cuda.synchronize()
        for nz in (0, d_nz.data_ptr()):
            assert same_bits(be.quadform_dev(nz, buf.data_ptr() + 8 * off, n + pad, nvec, d_mu.data_ptr()), want), (pad, off)
        assert same_bits(be.quadform_dev(0, buf.data_ptr() + 8 * off, n + pad, nvec), be.sqmahal(X)), (pad, off)
    # the fused call: every column and the log det have the bits of the separate calls
    ld = be.compute_logdet()
    buf = _device(lb.input_buffer(X, n + 3, 1))
    torch.cuda.synchronize()
    q, ld2 = be.refactorize_logpdf_dev(d_nz.data_ptr(), buf.data_ptr() + 8, n + 3, nvec, d_mu.data_ptr())
    assert same_bits(q, want) and same_bits(np.float64(ld2), np.float64(ld))
    # the batched fused call: every member has the bits of the separate calls
    B = 3
    bb = gmrfx.MI355XBatchBackend(Q, B, uplo=uplo, device=0)
    NZ = re_.member_values(Q, B)
    assert not bb.refactorize_values(NZ).any()
    Xb = np.stack([np.roll(X, k, axis=0) for k in range(B)], axis=-1)
    mub = np.stack([mu + 0.125 * k for k in range(B)], axis=-1)
    qb, ldb = bb.sqmahal(Xb, mean=mub), bb.logdet()
    ldx, sx = n + 3, (n + 3) * nvec + 5
    idx = 1 + np.arange(n)[:, None, None] + ldx * np.arange(nvec)[None, :, None] + sx * np.arange(B)[None, None, :]
    host = np.full(1 + sx * B + ldx, np.nan)
    host[idx] = Xb
    dX, dNZ, dMU = _device(host), _device(NZ.T), _device(mub.T)
    torch.cuda.synchronize()
    assert same_bits(bb.quadform_dev(dNZ.data_ptr(), dX.data_ptr() + 8, ldx, sx, nvec, dMU.data_ptr()), qb)
    ldf, qf, info = bb.refactorize_logpdf_dev(dNZ.data_ptr(), dX.data_ptr() + 8, ldx, sx, nvec, dMU.data_ptr())
    assert same_bits(qf, qb) and same_bits(ldf, ldb) and not info.any()
    _report(f"quad pins {uplo}", ratios)
    bb.close()
    be.close()


def test_quadform_vector_count_limits():
    """nvec = 65535 (the grid's y extent) at n = 3, 65536 refused; batched: nvec B = 65538 pairs, the grid-y walk runs twice"""
    n = 3
    Q = re_.chain(n)
    be = gmrfx.MI355XBackend(Q, device=0)
    X, mu = re_.quad_operands(n, rr.NVEC_MAX)
    got = be.sqmahal(X, mean=mu)
    ratios = {}
    _add(ratios, "nvec65535", got, rr.quadform(Q.indptr, Q.indices, Q.data, X, mu, False, LD))
    assert same_bits(be.sqmahal(X, mean=mu), got)
    with pytest.raises(ValueError):
        be.sqmahal(np.zeros((n, rr.NVEC_MAX + 1)))
    B, nvec = 3, 21846
    assert nvec * B > rr.NVEC_MAX
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    NZ = re_.member_values(Q, B)
    assert not bb.refactorize_values(NZ).any()
    Xb = re_.quad_operands(n, nvec * B)[0].reshape(n, nvec, B)
    gb = bb.sqmahal(Xb, mean=mu)
    assert same_bits(bb.sqmahal(Xb, mean=mu), gb)
    for k in range(B):
        _add(ratios, "batched65538", gb[:, k], rr.quadform(Q.indptr, Q.indices, NZ[:, k], Xb[:, :, k], mu, False, LD))
    _report("quad limits", ratios)
    bb.close()
    be.close()


# ---- Sigma read-outs ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(re_.SIGMA_Q))
def sigma(request):
    Q = re_.SIGMA_Q[request.param]()
    be = gmrfx.MI355XBackend(Q, device=0)
    S = be.get_selinv()
    inpat = re_.dense_pattern(S)
    assert np.array_equal(inpat, re_.factor_pattern(be))
    yield request.param, Q, be, S, inpat
    be.close()


def test_gathers_are_exact(sigma):
    name, Q, be, S, inpat = sigma
    n = Q.shape[0]
    Sd = S.toarray()
    assert same_bits(be.get_selinv_diag(), Sd.diagonal()) and not np.signbit(Sd[~inpat]).any()
    be._selinv_cache = be._selinv_diag_cache = None                    # a second gather of both
    assert same_bits(be.get_selinv().data, S.data) and same_bits(be.get_selinv_diag(), Sd.diagonal())
    for cnt in re_.DOT_COUNTS:
        if cnt > n * n:
            continue
        B = re_.dot_pattern(Q, inpat, cnt)
        E = be.selinv_extract_at(B)
        r, c = B.indices, np.repeat(np.arange(n), np.diff(B.indptr))
        assert np.array_equal(E.indices, B.indices) and np.array_equal(E.indptr, B.indptr)
        assert same_bits(E.data, np.where(inpat[r, c], Sd[r, c], 0.0)), (name, cnt)       # +0.0 outside the factor pattern
        assert same_bits(be.selinv_extract_at(B).data, E.data)


def test_trace_of_sigma_b(sigma):
    name, Q, be, S, inpat = sigma
    n = Q.shape[0]
    ratios = {}
    for cnt in re_.DOT_COUNTS:
        if cnt > n * n:
            continue
        B = re_.dot_pattern(Q, inpat, cnt)
        r, c = B.indices, np.repeat(np.arange(n), np.diff(B.indptr))
        E = be.selinv_extract_at(B)
        got = be.selinv_dot_device(B)
        ref = rr.selinv_dot(B.data, E.data, inpat[r, c], LD)
        _add(ratios, "dot", got, ref)
        assert same_bits(np.float64(be.selinv_dot_device(B)), np.float64(got))
        if cnt == 0:
            assert got == 0.0
        # entries outside the factor pattern contribute exactly nothing, whatever their value
        for keep in (B.data != re_.HUGE, inpat[r, c]):
            B0 = sp.csc_matrix((np.where(keep, B.data, 0.0), B.indices, B.indptr), shape=B.shape)
            assert same_bits(np.float64(be.selinv_dot_device(B0)), np.float64(got)), (name, cnt)
    _report(f"sigma {name}", ratios)


def test_row_diag_of_a_sigma_at(sigma):
    name, Q, be, S, inpat = sigma
    n = Q.shape[0]
    A = re_.design(n)
    Ac = rr.csr(A)
    P = sp.csc_matrix(abs(Ac).T @ abs(Ac))
    P.sort_indices()
    Sig = be.selinv_extract_at(P).toarray()                            # Sigma on pattern(A'A), 0 outside the factor pattern
    ratios = {}
    be.__dict__.pop("_rd_plans", None)
    kept, once = be.row_diag_ASigmaAt(A), be.row_diag_ASigmaAt_once(A)
    _add(ratios, "kept", kept, rr.row_diag(A, Sig, inpat, LD, 3))
    _add(ratios, "once", once, rr.row_diag(A, Sig, inpat, LD, 2))
    assert kept[0] == 0.0 and once[0] == 0.0                           # the row without entries
    assert same_bits(be.row_diag_ASigmaAt(A), kept) and same_bits(be.row_diag_ASigmaAt_once(A), once)
    # new values on the kept plan
    A2 = sp.coo_matrix((A.data * (1.0 + 0.25 * (np.arange(A.nnz) % 5)) * np.where(np.arange(A.nnz) % 3, 1.0, -1.0), (A.row, A.col)), shape=A.shape)
    got2 = be.row_diag_ASigmaAt(A2)
    assert len(be._rd_plans) == 1
    _add(ratios, "kept_new_values", got2, rr.row_diag(A2, Sig, inpat, LD, 3))
    _add(ratios, "once_new_values", be.row_diag_ASigmaAt_once(A2), rr.row_diag(A2, Sig, inpat, LD, 2))
    # the fifth plan evicts the first; planned again, it gives the same bits
    first = next(iter(be._rd_plans))
    for k, Ak in enumerate(re_.other_designs(n)):
        Pk = sp.csc_matrix(abs(Ak).T @ abs(Ak))
        Pk.sort_indices()
        _add(ratios, f"other{k}", be.row_diag_ASigmaAt(Ak), rr.row_diag(Ak, be.selinv_extract_at(Pk).toarray(), inpat, LD, 3))
    assert len(be._rd_plans) == 4 and first not in be._rd_plans
    assert same_bits(be.row_diag_ASigmaAt(A), kept) and first in be._rd_plans and len(be._rd_plans) == 4
    assert same_bits(be.row_diag_ASigmaAt(A2), got2)
    _report(f"row_diag {name}", ratios)


@pytest.mark.parametrize("nm", re_.SELDIAG_NM)
def test_batched_selinv_diag_straddles_blocks(nm):
    B = 3
    Q = re_.chain(nm)
    NZ = re_.member_values(Q, B)
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    assert not bb.refactorize_values(NZ).any() and (nm * 1) % 256 and (nm * 2) % 256
    sd = bb.selinv_diag()
    assert same_bits(bb.selinv_diag(), sd)
    perm = bb.ordering_permutation()
    for k in range(B):
        plain = gmrfx.MI355XBackend(sp.csc_matrix((NZ[:, k], Q.indices, Q.indptr), shape=Q.shape), ordering=perm, device=0)
        assert same_bits(plain.get_selinv_diag(), sd[:, k]), (nm, k)
        plain.close()
    bb.close()


# ---- dense operator -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def any_handle():
    be = gmrfx.MI355XBackend(sp.identity(4, format="csc"), device=0)
    yield be
    be.close()


def _framed(a, pad):
    """`a` inside a NaN-filled device buffer with `pad` NaNs directly before and behind it: (buffer, pointer to the view)"""
    buf = _device(np.concatenate([np.full(pad, np.nan), np.asarray(a, np.float64).ravel(), np.full(pad, np.nan)]))
    return buf, buf.data_ptr() + 8 * pad


def _unframe(buf, pad, shape):
    h = buf.cpu().numpy()
    size = int(np.prod(shape))
    assert np.isnan(h[:pad]).all() and np.isnan(h[pad + size:]).all(), "written outside the view"
    return h[pad:pad + size].reshape(shape)


@pytest.mark.parametrize("n1,n2", re_.DENSE_SHAPES)
def test_dense_apply_entry_by_entry(any_handle, n1, n2):
    be = any_handle
    D, T = re_.dense_operands(n1, n2)
    ref = rr.dense_apply(D, T, LD)
    ratios, first = {}, None
    for pad in (8, 7):                                                  # views aligned to 16 bytes and to 8 bytes only
        bD, pD = _framed(D, pad)
        bT, pT = _framed(T, pad)
        bR, pR = _framed(np.full((n1, n2), np.nan), pad)
        torch.cuda.synchronize()
        be.dense_apply_dev(pD, n1, pT, n2, pR)
        R = _unframe(bR, pad, (n1, n2))
        _add(ratios, f"pad{pad}", R, ref)
        be.dense_apply_dev(pD, n1, pT, n2, pR)
        assert same_bits(_unframe(bR, pad, (n1, n2)), R)
        first = R if first is None else first
        assert same_bits(R, first), "the result depends on the operands' alignment"
        assert same_bits(_unframe(bD, pad, (n1, n1)), D) and same_bits(_unframe(bT, pad, (n1, n2)), T)
    _report(f"dense {n1}x{n2}", ratios)


@pytest.mark.parametrize("rows,cols", re_.TRANSPOSE_SHAPES)
def test_transpose_is_exact(any_handle, rows, cols):
    be = any_handle
    _, T = re_.dense_operands(rows, cols)
    for pad in (8, 7):
        bS, pS = _framed(T, pad)
        bO, pO = _framed(np.full((cols, rows), np.nan), pad)
        torch.cuda.synchronize()
        for _ in range(2):
            be.transpose_dev(pS, rows, cols, pO)
            assert same_bits(_unframe(bO, pad, (cols, rows)), rr.transpose(T)), (rows, cols, pad)
        assert same_bits(_unframe(bS, pad, (rows, cols)), T)
