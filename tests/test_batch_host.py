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
