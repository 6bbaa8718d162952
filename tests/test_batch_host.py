"""CPU tests of batched handles (gmrfx_create_batched): B members with one pattern analysed as the block-diagonal forest
diag(Q_1 .. Q_B). Symbolic-only handles: the forest's statistics are B times the member's, its trees sit on the member's levels,
its elimination order is the member's replicated; invalid arguments are refused with a message before anything is allocated; the
Python binding checks shapes before it calls the library."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
from gmrfx import _lib, spde
from gmrfx._lib import GmrfxOpts, lib, ptr


def _matern30():
    m = spde.grid_mesh_2d(30, 30, jitter=0.25, seed=3)
    return spde.matern_precision(m, 0, 0.3), m.points


@pytest.mark.parametrize("B", [1, 4, 13])
@pytest.mark.parametrize("use_coords", [True, False], ids=["coords", "graph"])
def test_symbolic_batch_is_b_copies_of_the_member(B, use_coords):
    Q, pts = _matern30()
    n = Q.shape[0]
    kw = {"coords": pts} if use_coords else {}
    one = gmrfx.MI355XBackend(Q, symbolic_only=True, **kw)
    bb = gmrfx.MI355XBatchBackend(Q, B, symbolic_only=True, **kw)
    s1, sb = one.stats(), bb.stats()
    for k in ("n", "nnz_l", "nnz_l_stored", "nsuper", "nnz_q_tri"):
        assert sb[k] == B * s1[k], k
    assert sb["factor_flops"] == B * s1["factor_flops"]
    assert sb["bytes_factor"] == B * s1["bytes_factor"]
    assert sb["bytes_cb_arena"] >= s1["bytes_cb_arena"]        # reported for symbolic-only handles: callers size B with it
    assert sb["nlevels"] == s1["nlevels"]                     # the copies of the tree are aligned on the member's levels
    p1 = one.ordering_permutation()
    assert np.array_equal(bb.ordering_permutation(), p1)
    want = np.concatenate([k * n + p1 for k in range(B)])
    assert np.array_equal(bb.forest_permutation(), want)
    assert bb.batch_size() == (B, n)


def test_user_perm_is_replicated_and_plain_handles_report_a_batch_of_one():
    Q, _ = _matern30()
    n = Q.shape[0]
    perm = np.random.default_rng(0).permutation(n)
    one = gmrfx.MI355XBackend(Q, ordering=perm, symbolic_only=True)
    bb = gmrfx.MI355XBatchBackend(Q, 3, ordering=perm, symbolic_only=True)
    p1 = one.ordering_permutation()
    assert np.array_equal(bb.forest_permutation(), np.concatenate([k * n + p1 for k in range(3)]))
    nb, nm = C.c_int64(0), C.c_int64(0)
    assert lib().gmrfx_batch_size(one._h, C.byref(nb), C.byref(nm)) == 0
    assert (nb.value, nm.value) == (1, n)


def _create(n, colptr, rowval, nbatch, **opt):
    o = GmrfxOpts()
    o.struct_size = C.sizeof(GmrfxOpts)
    o.symbolic_only = 1
    for k, v in opt.items():
        setattr(o, k, v)
    h = C.c_void_p()
    code = lib().gmrfx_create_batched(n, ptr(colptr), ptr(rowval), 0, None, nbatch, C.byref(o), C.byref(h))
    msg = lib().gmrfx_last_create_error().decode()
    if h.value:
        lib().gmrfx_destroy(h)
    return code, msg, h.value


@pytest.mark.parametrize("nbatch", [0, -1])
def test_invalid_nbatch_is_refused(nbatch):
    Q, _ = _matern30()
    code, msg, h = _create(Q.shape[0], Q.indptr.astype(np.int64), Q.indices.astype(np.int64), nbatch)
    assert code == _lib.ERR_INVALID_ARG and h is None and "nbatch" in msg


def test_forest_beyond_int32_is_refused_before_allocation():
    n, B = 1 << 20, 1 << 12                  # 2^32 forest nodes: would need ~100 GB of host arrays if it were built
    colptr = np.arange(n + 1, dtype=np.int64)
    rowval = np.arange(n, dtype=np.int64)
    code, msg, h = _create(n, colptr, rowval, B)
    assert code == _lib.ERR_INVALID_ARG and h is None and "INT32_MAX" in msg


@pytest.mark.parametrize("opt", [{"shard_world": 2, "shard_rank": 0}, {"shard_min_top": 1}], ids=["world2", "min_top"])
def test_sharded_batches_are_refused(opt):
    Q, _ = _matern30()
    code, msg, h = _create(Q.shape[0], Q.indptr.astype(np.int64), Q.indices.astype(np.int64), 2, **opt)
    assert code == _lib.ERR_INVALID_ARG and h is None and "shard" in msg


def test_python_binding_rejects_misshaped_operands():
    Q = sp.csc_matrix(spde.matern_precision(spde.grid_mesh_2d(8, 8), 0, 0.4))
    n, nnz, B = Q.shape[0], Q.nnz, 3
    bb = gmrfx.MI355XBatchBackend(Q, B, symbolic_only=True)
    for NZ in (np.zeros((nnz, B + 1)), np.zeros((nnz + 1, B)), np.zeros(nnz * B), np.zeros((B, nnz))):
        with pytest.raises(ValueError):
            bb.refactorize_values(NZ)
    for R in (np.zeros((n, B + 1)), np.zeros((n - 1, B)), np.zeros(n), np.zeros((n, 2, B - 1)), np.zeros((B, n))):
        with pytest.raises(ValueError):
            bb.solve(R)
        with pytest.raises(ValueError):
            bb.backward_solve(R)
        with pytest.raises(ValueError):
            bb.sqmahal(R)
    with pytest.raises(ValueError):
        bb.sqmahal(np.zeros((n, B)), mean=np.zeros(n + 1))
    with pytest.raises(ValueError):
        bb.refactorize_logpdf(np.zeros((nnz, B)), np.zeros((n, B + 2)))
    with pytest.raises(ValueError):
        gmrfx.MI355XBatchBackend(Q, 0, symbolic_only=True)
    # well-shaped operands reach the library, which reports the missing device state (symbolic_only) instead
    with pytest.raises(gmrfx.NoDeviceError):
        bb.solve(np.zeros((n, B)))


# ---- level widths: the preconditions of the wide-level GPU tests (tests/test_gpu_batch_edges.py) ------------------------------

def _level_counts(be, min_rows=0):
    s = gmrfx.MI355XBackend.symbolic(be)
    return np.bincount(s.level[np.diff(s.row_ptr) > min_rows], minlength=int(s.level.max()) + 1)


@pytest.mark.parametrize("B", [2, 7, 64])
def test_forest_level_counts_are_b_times_the_members(B):
    from test_gpu_batch_edges import _arrow
    for Q, kw in ((_matern30()[0], {}), (_arrow(300), {"ordering": "natural"})):
        one = gmrfx.MI355XBackend(Q, symbolic_only=True, **kw)
        bb = gmrfx.MI355XBatchBackend(Q, B, symbolic_only=True, **kw)
        for m in (0, 128):
            assert np.array_equal(_level_counts(bb, m), B * _level_counts(one, m))


def test_wide_level_preconditions():
    """the GPU tests' batches and the arrow-star matrix really have a level of more than 65535 fronts (grid y > 65535), and the
    arrow's fronts are taller than 128 rows (the generic front path, not the small-front kernels)"""
    from test_gpu_batch_edges import _arrow, _grid
    Q, pts = _grid(20, 20)
    one = gmrfx.MI355XBackend(Q, coords=pts, symbolic_only=True)
    assert _level_counts(one).max() * 6000 > 65535
    assert _level_counts(one).max() * 6000 < 2 * 65535            # wide, not needlessly big
    bb = gmrfx.MI355XBatchBackend(_arrow(1100), 64, ordering="natural", symbolic_only=True)
    assert _level_counts(bb, 128).max() > 65535
    plain = gmrfx.MI355XBackend(_arrow(70000), ordering="natural", symbolic_only=True)
    assert _level_counts(plain, 128).max() > 65535
    assert np.array_equal(plain.ordering_permutation(), np.arange(70128))


# ---- argument checks of the batch entry points: refused before any device state is needed ------------------------------------

def _code(h, name, *args):
    code = getattr(lib(), name)(h, *args)
    return code, (lib().gmrfx_last_error(h) or b"").decode()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("backward", [False, True], ids=["solve", "backward"])
def test_batch_solve_layout_is_checked(dev, backward):
    Q, _ = _matern30()
    n, B, r = Q.shape[0], 3, 4
    bb = gmrfx.MI355XBatchBackend(Q, B, symbolic_only=True)
    name = "gmrfx_batch_" + ("backward_solve" if backward else "solve") + ("_dev" if dev else "")
    buf = np.zeros((n + 8) * r * B + 64)
    p = buf.ctypes.data
    good = (n, n * r)
    bad = {"ld < n": ((n - 1, n * r), "leading dimension"),
           "stride < ld * nrhs": ((n, n * r - 1), "member stride"),
           "negative stride": ((n, -n * r), "member stride"),
           "padded ld, stride too small": ((n + 8, n * r), "member stride")}
    for label, ((ld, s), msg) in bad.items():
        for side in ("B", "X"):
            a = (ld, s) if side == "B" else good
            x = good if side == "B" else (ld, s)
            code, err = _code(bb._h, name, p, a[0], a[1], r, p, x[0], x[1])
            assert code == _lib.ERR_INVALID_ARG and msg in err and err.startswith(side), (label, side, err)
    code, err = _code(bb._h, name, p, n, n * r, -1, p, n, n * r)
    assert code == _lib.ERR_INVALID_ARG and "nrhs" in err
    code, err = _code(bb._h, name, None, n, n * r, r, p, n, n * r)
    assert code == _lib.ERR_INVALID_ARG and "null" in err
    # a well-formed layout (padded ld, a gap between members) reaches the missing device state
    assert _code(bb._h, name, p, n + 3, (n + 3) * r + 5, r, p, n + 1, (n + 1) * r)[0] == _lib.ERR_NO_DEVICE
    # a plain handle is a batch of one: ld < n is refused, the member stride is not used
    one = gmrfx.MI355XBackend(Q, symbolic_only=True)
    assert _code(one._h, name, p, n - 1, 0, r, p, n, 0)[0] == _lib.ERR_INVALID_ARG
    assert _code(one._h, name, p, n, 0, r, p, n, 0)[0] == _lib.ERR_NO_DEVICE


@pytest.mark.parametrize("name", ["gmrfx_batch_quadform", "gmrfx_batch_quadform_dev", "gmrfx_batch_refactorize_logpdf_dev"])
def test_batch_quadform_arguments_are_checked(name):
    Q, _ = _matern30()
    n, B = Q.shape[0], 3
    bb = gmrfx.MI355XBatchBackend(Q, B, symbolic_only=True)
    buf = np.zeros(4 * n * B + 64)
    p = buf.ctypes.data
    fused = name.endswith("logpdf_dev")

    def call(ldx, sx, nvec, X=p, quad=p):
        args = (p, X, ldx, sx, nvec, None, quad) + ((p, None) if fused else ())
        return _code(bb._h, name, *args)

    big = (2**31 - 1) // B + 1                   # nvec * nbatch > INT32_MAX: the pair index of k_batch_quadform is 32-bit
    code, err = call(n, n * big, big)
    assert code == _lib.ERR_INVALID_ARG and "INT32_MAX" in err
    assert call(n, n * (big - 1), big - 1)[0] == _lib.ERR_NO_DEVICE
    for (ldx, sx, nvec), msg in (((n - 1, 2 * n, 2), "leading dimension"), ((n, 2 * n - 1, 2), "member stride"),
                                 ((n, 2 * n, -1), "nvec")):
        code, err = call(ldx, sx, nvec)
        assert code == _lib.ERR_INVALID_ARG and msg in err, err
    code, err = call(n, 2 * n, 2, X=None)
    assert code == _lib.ERR_INVALID_ARG and "null" in err
    code, err = call(n, 2 * n, 2, quad=None)
    assert code == _lib.ERR_INVALID_ARG and "null" in err
    assert call(n, 2 * n, 2)[0] == _lib.ERR_NO_DEVICE
