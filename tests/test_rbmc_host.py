"""Host analysis of the Rao-Blackwellised Monte Carlo variance estimators (include/gmrfx.h: gmrfx_rbmc_plan; csrc/rbmc_plan.cpp) on
symbolic_only handles, against the numpy restatement of src/solvers/rbmc.jl in tests/rbmc_ref.py: blocks (as sets, S first),
n_interior and owner masks for enclosure_size 0, 1, 2; the used triangle only; index bases; a batched handle; argument errors; and
the plans of tests/rbmc_patterns.py, pinned to the (ns, nb) pairs and per-class block counts that tests/test_gpu_rbmc_edges.py relies on."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import rbmc_patterns as rp
import rbmc_ref
from gmrfx import _lib, spde

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = int(g["n"])
    return sp.csc_matrix((g["nzval"], g["rowval"], g["colptr"]), shape=(n, n))


def _matern21(smoothness):
    return sp.csc_matrix(spde.matern_precision(spde.grid_mesh_2d(21, 21), smoothness=smoothness, range_=0.2))


MODELS = {
    "matern21_s1": lambda: _matern21(1),
    "matern21_s0": lambda: _matern21(0),
    "structural_zeros": lambda: _golden("matern2d_13x13_a3_structural_zeros"),
    "sprand_spd_60": lambda: _golden("sprand_spd_60"),
}


@pytest.fixture(scope="module", params=sorted(MODELS))
def model(request):
    Q = MODELS[request.param]()
    return request.param, Q, gmrfx.MI355XBackend(Q, symbolic_only=True), rbmc_ref.SymQ(Q)


def test_the_three_names_are_exported():
    L = _lib.lib()
    for name in ("gmrfx_rbmc_var", "gmrfx_rbmc_var_dev", "gmrfx_rbmc_plan"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).restype is C.c_int32
    assert _lib.GmrfxStats._fields_[-1][0] == "ms_rbmc"
    for cls in (gmrfx.MI355XBackend, gmrfx.MI355XBatchBackend):
        for m in ("rbmc_var", "rbmc_var_dev", "rbmc_plan"):
            assert callable(getattr(cls, m))


@pytest.mark.parametrize("enclosure_size", [0, 1, 2])
def test_plan_equals_the_restatement(model, enclosure_size):
    name, Q, be, sq = model
    ref = rbmc_ref.check_plan(be.rbmc_plan(enclosure_size), sq, enclosure_size)
    if name == "matern21_s1":          # the sizes the reference's own test model reaches: the <= 64, <= 128 and <= 512-row classes
        assert max(len(S) + len(E) for S, E in ref) == {0: 37, 1: 127, 2: 252}[enclosure_size]
        multi = np.zeros(sq.n, int)
        for S, _ in ref:
            multi[S] += 1
        assert (multi > 1).sum() == 405        # "disjoint" subsets overlap: most nodes lie in more than one
    if name == "matern21_s0" and enclosure_size == 0:
        assert max(len(S) + len(E) for S, E in ref) <= 32          # the <= 32-row class


@pytest.mark.parametrize("name,enclosure_size", [(e.name, enc) for e in rp.EDGES for enc in sorted(e.plans)])
def test_edge_patterns_keep_their_edges(name, enclosure_size):
    """the library's plan equals the restatement's on every pattern of tests/rbmc_patterns.py, and holds the blocks the device
    tests are there for: every size-class boundary, ns > 64, s0 > 0, and more blocks of a class than one launch takes"""
    edge = rp.EDGE[name]
    Q = edge.build()
    plan = gmrfx.MI355XBackend(Q, symbolic_only=True).rbmc_plan(enclosure_size)
    ref = rbmc_ref.check_plan(plan, rbmc_ref.SymQ(Q), enclosure_size)
    sizes = rp.plan_sizes(plan)
    assert sizes == rp.plan_sizes(ref)
    rp.check_sizes(sizes, edge.plans[enclosure_size])
    counts = rp.class_counts(sizes)
    if (name, enclosure_size) == ("star200_hub_last", 1):
        assert counts[3] == 200 > rp.CLASS_CHUNK[3] and Q.shape[0] == 201           # a second launch of the <= 512 class at b0 = 128
        hub = 200                                                                   # held by all 200 subsets, owned by the last
        bp, rows, ni, ow = plan["block_ptr"], plan["rows"], plan["n_interior"], plan["owner"]
        held = [b for b in range(200) if hub in rows[bp[b]:bp[b] + ni[b]]]
        owned = [b for b in range(200) if any(r == hub and o for r, o in zip(rows[bp[b]:bp[b] + ni[b]], ow[bp[b]:bp[b] + ni[b]]))]
        assert held == list(range(200)) and owned == [199]
    if name == "star_forest11x100":
        assert counts[2] == 1100 > rp.CLASS_CHUNK[2] and Q.shape[0] == 1111         # a second launch of the <= 128 class at b0 = 1024
    if name == "cliques":
        assert Q.shape[0] == 1187 and plan["max_block"] == 512
        assert [-(-s // 64) for s in (65, 128, 129, 512)] == [2, 2, 3, 8]           # passes of 64 unit vectors
    if name == "banded1200_85":
        assert (171, 511) in sizes and 511 - 171 == 340 and -(-171 // 64) == 3      # s0 = 340, three passes


def test_structural_zeros_are_neighbours():
    Q = _golden("matern2d_13x13_a3_structural_zeros")
    assert (Q.data == 0.0).any()
    dropped = Q.copy()
    dropped.eliminate_zeros()
    assert rbmc_ref.build_blocks(rbmc_ref.SymQ(Q), 0) != rbmc_ref.build_blocks(rbmc_ref.SymQ(dropped), 0)


@pytest.mark.parametrize("enclosure_size", [0, 1, 2])
def test_only_the_defining_triangle_is_read(enclosure_size):
    Q = _matern21(1)
    sq = rbmc_ref.SymQ(Q)
    up = sp.csc_matrix(sp.triu(Q))
    rbmc_ref.check_plan(gmrfx.MI355XBackend(up, symbolic_only=True).rbmc_plan(enclosure_size), sq, enclosure_size)
    # both triangles stored, the LOWER one defines Q; the upper one holds garbage on a different pattern
    # (assembled from index arrays: the matrix holds explicit zeros, which sparse addition would drop)
    n = Q.shape[0]
    lo, junk = sp.coo_matrix(sp.tril(Q)), sp.coo_matrix(sp.triu(sp.random(n, n, density=0.01, random_state=7), 1))
    assert lo.nnz == sp.coo_matrix(sp.triu(Q)).nnz and junk.nnz > 0
    both = sp.csc_matrix((np.r_[lo.data, junk.data + 1.0], (np.r_[lo.row, junk.row], np.r_[lo.col, junk.col])), shape=(n, n))
    assert both.nnz == lo.nnz + junk.nnz
    be = gmrfx.MI355XBackend(both, symbolic_only=True, uplo="L")
    rbmc_ref.check_plan(be.rbmc_plan(enclosure_size), sq, enclosure_size)
    rbmc_ref.check_plan(be.rbmc_plan(enclosure_size), rbmc_ref.SymQ(both, "L"), enclosure_size)


def test_index_base(model):
    _, _, be, sq = model
    p0, p1 = be.rbmc_plan(1, 0), be.rbmc_plan(1, 1)
    rbmc_ref.check_plan(p1, sq, 1, index_base=1)
    assert (p1["rows"] == p0["rows"] + 1).all()
    for k in ("block_ptr", "n_interior", "owner"):
        assert (p0[k] == p1[k]).all()


@pytest.mark.parametrize("enclosure_size", [0, 1])
def test_batched_handle_blocks_never_cross_members(enclosure_size):
    Q = sp.csc_matrix(spde.matern_precision(spde.grid_mesh_2d(9, 8, jitter=0.2, seed=1), smoothness=0, range_=0.4))
    n, B = Q.shape[0], 3
    bb = gmrfx.MI355XBatchBackend(Q, B, symbolic_only=True)
    plan = bb.rbmc_plan(enclosure_size)
    forest = sp.block_diag([Q] * B, format="csc")
    rbmc_ref.check_plan(plan, rbmc_ref.SymQ(forest), enclosure_size)
    bp, rows = plan["block_ptr"], plan["rows"]
    for b in range(len(bp) - 1):
        assert len(set((rows[bp[b]:bp[b + 1]] // n).tolist())) == 1


def _call(be, enclosure_size, index_base, counts=True):
    c = np.full(3, -7, np.int64)
    code = _lib.lib().gmrfx_rbmc_plan(be._h, enclosure_size, index_base, _lib.ptr(c) if counts else None, None, None, None, None)
    return code, _lib.lib().gmrfx_last_error(be._h).decode(), c


def test_argument_errors_have_messages_and_change_nothing():
    Q = _matern21(0)
    be = gmrfx.MI355XBackend(Q, symbolic_only=True)
    before = be.rbmc_plan(1)
    for args in ((-1, 0), (-2, 0), (1, 2), (1, -1)):
        code, msg, c = _call(be, *args)
        assert code == _lib.ERR_INVALID_ARG and msg and (c == -7).all(), args
    code, msg, _ = _call(be, 1, 0, counts=False)
    assert code == _lib.ERR_INVALID_ARG and "counts" in msg
    after = be.rbmc_plan(1)
    for k in ("block_ptr", "rows", "n_interior", "owner"):
        assert (before[k] == after[k]).all()
    # numeric use of a symbolic-only handle
    Z = np.zeros((be.n, 4))
    with pytest.raises(_lib.NoDeviceError):
        be.rbmc_var(Z, 0, nzval=Q.data)
    for bad in (dict(enclosure_size=-2), dict(enclosure_size=0, k=1)):
        with pytest.raises(ValueError):
            be.rbmc_var(Z[:, :bad.get("k", 4)], bad["enclosure_size"], nzval=Q.data)


def test_a_block_over_512_rows_is_refused():
    n = 600
    Q = sp.csc_matrix(np.ones((n, n)) + n * np.eye(n))
    be = gmrfx.MI355XBackend(Q, symbolic_only=True, ordering="natural")
    code, msg, c = _call(be, 0, 0)
    assert code == _lib.ERR_INVALID_ARG and "block 0" in msg and "600" in msg and "512" in msg and (c == -7).all()
    # a grid whose enclosure outgrows the limit: the subsets are fine (enclosure_size = 0 stays available), the rings are not
    big = sp.csc_matrix(spde.matern_precision(spde.grid_mesh_2d(40, 40), smoothness=1, range_=0.2))
    G = gmrfx.MI355XBackend(big, symbolic_only=True)
    small = G.rbmc_plan(0)
    assert small["max_block"] == 37
    code, msg, _ = _call(G, 6, 0)
    assert code == _lib.ERR_INVALID_ARG and "block" in msg and "512" in msg
    again = G.rbmc_plan(0)
    assert again["max_block"] == 37 and (again["rows"] == small["rows"]).all()
