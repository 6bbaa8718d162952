"""One constraint A x = e for every member of a batched handle (include/gmrfx.h: gmrfx_batch_constraints_*, gmrfx_batch_sample,
gmrfx_batch_constrained_logpdf_dev): what can be checked without a GPU, on symbolic_only handles -- the exported symbols against
the header, argument validation that changes nothing, summed duplicates and log det(A A'), clearing and cloning,
GMRFX_ERR_NO_DEVICE from the numeric entry points, the two kinds of constraint excluding each other, sharded handles refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
from gmrfx import _lib, spde

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {
    "gmrfx_batch_constraints_set": "gmrfx_handle*, int64_t, const int64_t*, const int64_t*, const double*, int32_t, const double*",
    "gmrfx_batch_constraints_info": "gmrfx_handle*, int64_t*, double*, double*, int64_t*, double*",
    "gmrfx_batch_constraints_get": "gmrfx_handle*, int64_t, double*, int64_t, double*",
    "gmrfx_batch_constraints_mean": "gmrfx_handle*, const double*, double*, double*",
    "gmrfx_batch_constraints_correct": "gmrfx_handle*, double*, int64_t, int64_t, int64_t",
    "gmrfx_batch_constraints_correct_dev": "gmrfx_handle*, double*, int64_t, int64_t, int64_t",
    "gmrfx_batch_constraints_var": "gmrfx_handle*, double*",
    "gmrfx_batch_sample": "gmrfx_handle*, const double*, int64_t, int64_t, int64_t, const double*, double*, int64_t, int64_t",
    "gmrfx_batch_sample_dev": "gmrfx_handle*, const double*, int64_t, int64_t, int64_t, const double*, double*, int64_t, int64_t",
    "gmrfx_batch_constrained_logpdf_dev": "gmrfx_handle*, const double*, const double*, int64_t, int64_t, int64_t, const double*, double*, "
                                          "double*, double*, int64_t*, int64_t*",
}
POINTERS = (C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64))
CTYPE = {"gmrfx_handle*": (C.c_void_p,), "int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "const int64_t*": POINTERS,
         "const double*": POINTERS, "double*": POINTERS, "int64_t*": POINTERS}
B = 3


def _header_args(name):
    h = open(os.path.join(ROOT, "include", "gmrfx.h")).read()
    h = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", h)
    assert m, f"{name} is not declared in include/gmrfx.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        a = re.sub(r"\s*\b\w+$", "", a) if not a.endswith("*") else a        # drop the parameter name
        out.append(a.replace(" *", "*"))
    return out


@pytest.mark.parametrize("name", sorted(NEW))
def test_symbol_is_exported_with_the_headers_signature(name):
    fn = getattr(_lib.lib(), name)             # AttributeError: not exported
    assert name in _lib.EXPORTS
    want = [a.strip() for a in NEW[name].split(",")]
    assert _header_args(name) == want
    assert fn.restype is C.c_int32
    assert len(fn.argtypes) == len(want)
    for got, w in zip(fn.argtypes, want):
        assert got in CTYPE[w], (name, w, got)


def test_batch_backend_has_the_new_methods():
    for name in ("set_constraints", "clear_constraints", "constraint_info", "constraint_fields", "constrained_mean", "constrained_var",
                 "constraint_correct", "constraint_correct_dev", "sample", "sample_dev", "constrained_logpdf", "constrained_logpdf_dev"):
        assert callable(getattr(gmrfx.MI355XBatchBackend, name)), name


@pytest.fixture(scope="module")
def problem():
    mesh = spde.grid_mesh_2d(9, 8, jitter=0.2, seed=1)
    return sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.4)), mesh.points


def _symbolic(problem, nbatch=B):
    Q, pts = problem
    return gmrfx.MI355XBatchBackend(Q, nbatch, coords=pts, symbolic_only=True), Q.shape[0]


def _set(bb, m, rp, ci, va, e, base=0):
    a = [np.ascontiguousarray(rp, np.int64), np.ascontiguousarray(ci, np.int64), np.ascontiguousarray(va, np.float64),
         np.ascontiguousarray(e, np.float64)]
    code = _lib.lib().gmrfx_batch_constraints_set(bb._h, m, *[_lib.ptr(x) for x in a[:3]], base, _lib.ptr(a[3]))
    return code, _lib.lib().gmrfx_last_error(bb._h)


def _valid(n, m=3, seed=0):
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n))
    A[0] = 1.0
    for r in range(1, m):
        A[r, rng.choice(n, 5, replace=False)] = rng.standard_normal(5)
    return sp.csr_matrix(A), rng.standard_normal(m)


def test_valid_input_duplicates_and_logdet(problem):
    bb, n = _symbolic(problem)
    assert bb.constraint_info() == {"m": 0, "logdet_AAt": 0.0}
    A, e = _valid(n)
    bb.set_constraints(A, e)
    info = bb.constraint_info()
    want = np.linalg.slogdet((A @ A.T).toarray())[1]
    assert info["m"] == 3 and abs(info["logdet_AAt"] - want) <= 1e-12 * abs(want)
    # duplicates are summed, columns in any order, 1-based input: the row [2, 0, .., 0, 3] given as 0.5 + 1.5 and 3
    code, _ = _set(bb, 1, [1, 4], [1, n, 1], [0.5, 3.0, 1.5], [0.25], base=1)
    assert code == 0
    info = bb.constraint_info()
    assert info["m"] == 1 and abs(info["logdet_AAt"] - np.log(13.0)) <= 1e-12 * np.log(13.0)
    bb.clear_constraints()
    assert bb.constraint_info() == {"m": 0, "logdet_AAt": 0.0}


def test_invalid_input_is_refused_and_changes_nothing(problem):
    bb, n = _symbolic(problem)
    A, e = _valid(n, seed=4)
    bb.set_constraints(A, e)
    before = bb.constraint_info()
    ones = np.ones(n)
    cols = np.arange(n)
    bad = {
        "m = 65": (65, np.arange(66), np.arange(65) % n, np.ones(65), np.zeros(65)),
        "column = n_member": (1, [0, 2], [0, n], [1.0, 1.0], [0.0]),
        "negative column": (1, [0, 2], [-1, 3], [1.0, 1.0], [0.0]),
        "empty row": (2, [0, 0, n], cols, ones, [0.0, 0.0]),
        "non-monotone rowptr": (2, [0, 5, 3], cols, ones, [0.0, 0.0]),
    }
    for what, args in bad.items():
        code, msg = _set(bb, *args)
        assert code == _lib.ERR_INVALID_ARG and msg, what
        assert bb.constraint_info() == before, what
    # columns are the MEMBER's: the forest has B n columns, n .. B n - 1 are still out of range
    code, msg = _set(bb, 1, [0, 1], [B * n - 1], [1.0], [0.0])
    assert code == _lib.ERR_INVALID_ARG and b"out of range" in msg
    assert bb.constraint_info() == before


def test_clone_carries_the_constraint(problem):
    bb, n = _symbolic(problem)
    A, e = _valid(n, seed=2)
    bb.set_constraints(A, e)
    c = bb.clone()
    assert c.constraint_info() == bb.constraint_info()
    bb.clear_constraints()
    assert c.constraint_info()["m"] == 3 and bb.constraint_info()["m"] == 0


def test_numeric_entry_points_need_a_device(problem):
    bb, n = _symbolic(problem)
    A, e = _valid(n, seed=3)
    bb.set_constraints(A, e)
    L = _lib.lib()
    x = np.zeros((n, B), order="F")
    out = np.zeros((n, B), order="F")
    w = np.zeros(9)
    q = np.zeros(B)
    ii = np.zeros(B, np.int64)
    m = C.c_int64(0)
    p = _lib.ptr
    calls = {
        "info": lambda: L.gmrfx_batch_constraints_info(bb._h, C.byref(m), p(q), None, None, None),
        "info/cinfo": lambda: L.gmrfx_batch_constraints_info(bb._h, None, None, None, p(ii), None),
        "get": lambda: L.gmrfx_batch_constraints_get(bb._h, 0, p(out), n, p(w)),
        "mean": lambda: L.gmrfx_batch_constraints_mean(bb._h, p(x), p(out), p(q)),
        "correct": lambda: L.gmrfx_batch_constraints_correct(bb._h, p(x), n, n, 1),
        "correct_dev": lambda: L.gmrfx_batch_constraints_correct_dev(bb._h, p(x), n, n, 1),
        "var": lambda: L.gmrfx_batch_constraints_var(bb._h, p(out)),
        "sample": lambda: L.gmrfx_batch_sample(bb._h, p(x), n, n, 1, None, p(out), n, n),
        "sample_dev": lambda: L.gmrfx_batch_sample_dev(bb._h, p(x), n, n, 1, None, p(out), n, n),
        "logpdf": lambda: L.gmrfx_batch_constrained_logpdf_dev(bb._h, p(x), p(x), n, n, 1, None, p(q), p(q), p(q), p(ii), p(ii)),
    }
    for what, call in calls.items():
        assert call() == _lib.ERR_NO_DEVICE, what
    with pytest.raises(_lib.NoDeviceError):
        bb.constrained_var()
    # a handle without a constraint answers the same way
    bb.clear_constraints()
    assert calls["sample"]() == _lib.ERR_NO_DEVICE and calls["var"]() == _lib.ERR_NO_DEVICE


def test_plain_and_batch_constraints_exclude_each_other(problem):
    Q, pts = problem
    n = Q.shape[0]
    A, e = _valid(n, seed=5)
    be = gmrfx.MI355XBackend(Q, coords=pts, symbolic_only=True)          # a plain handle: a batch of one
    rp, ci, va = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    L = _lib.lib()
    m = C.c_int64(-1)
    # batch constraint first: the plain one is refused, and the other way round
    assert _set(be, 3, rp, ci, va, e)[0] == 0
    assert L.gmrfx_batch_constraints_info(be._h, C.byref(m), None, None, None, None) == 0 and m.value == 3
    with pytest.raises(ValueError, match="batch constraint"):
        be.set_constraints(A, e)
    assert be.constraint_info()["m"] == 0
    assert _set(be, 0, [0], [], [], [])[0] == 0
    be.set_constraints(A, e)
    code, msg = _set(be, 3, rp, ci, va, e)
    assert code == _lib.ERR_INVALID_ARG and b"plain constraint" in msg
    assert L.gmrfx_batch_constraints_info(be._h, C.byref(m), None, None, None, None) == 0 and m.value == 0
    assert be.constraint_info()["m"] == 3
    # clearing the kind that is not set is always allowed
    assert _set(be, 0, [0], [], [], [])[0] == 0 and be.constraint_info()["m"] == 3
    # a clone of a plain handle carries its batch constraint too
    be.clear_constraints()
    assert _set(be, 3, rp, ci, va, e)[0] == 0
    c = be.clone()
    assert L.gmrfx_batch_constraints_info(c._h, C.byref(m), None, None, None, None) == 0 and m.value == 3


def test_sharded_symbolic_handle_is_refused(problem):
    Q, pts = problem
    n = Q.shape[0]
    be = gmrfx.MI355XBackend(Q, coords=pts, symbolic_only=True, shard_rank=0, shard_world=2)
    code, msg = _set(be, 1, [0, n], np.arange(n), np.ones(n), [0.0])
    assert code == _lib.ERR_INVALID_ARG and b"sharded" in msg
