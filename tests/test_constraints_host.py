"""Linear equality constraints A x = e as state of a handle (include/gmrfx.h: gmrfx_constraints_*, gmrfx_sample): everything that
can be checked without a GPU -- the exported symbols against the header, the binding's methods, and on symbolic_only handles the
argument validation, log det(A A'), GMRFX_ERR_NO_DEVICE from every numeric entry point, clearing and cloning."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
from gmrfx import _lib, spde
from gmrfx._lib import NoDeviceError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {
    "gmrfx_constraints_set": "gmrfx_handle*, int64_t, const int64_t*, const int64_t*, const double*, int32_t, const double*",
    "gmrfx_constraints_info": "gmrfx_handle*, int64_t*, double*, double*, double*",
    "gmrfx_constraints_get": "gmrfx_handle*, double*, int64_t, double*",
    "gmrfx_constraints_mean": "gmrfx_handle*, const double*, double*, double*",
    "gmrfx_constraints_correct": "gmrfx_handle*, double*, int64_t, int64_t",
    "gmrfx_constraints_correct_dev": "gmrfx_handle*, double*, int64_t, int64_t",
    "gmrfx_constraints_var": "gmrfx_handle*, double*",
    "gmrfx_sample": "gmrfx_handle*, const double*, int64_t, int64_t, const double*, double*, int64_t",
    "gmrfx_sample_dev": "gmrfx_handle*, const double*, int64_t, int64_t, const double*, double*, int64_t",
}
CTYPE = {"gmrfx_handle*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "const int64_t*": C.c_void_p,
         "const double*": C.c_void_p, "double*": (C.c_void_p, C.POINTER(C.c_double)), "int64_t*": (C.c_void_p, C.POINTER(C.c_int64))}


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
    L = _lib.lib()
    fn = getattr(L, name)                      # AttributeError: not exported
    assert name in _lib.EXPORTS
    want = [a.strip() for a in NEW[name].split(",")]
    assert _header_args(name) == want
    assert fn.restype is C.c_int32
    assert len(fn.argtypes) == len(want)
    for got, w in zip(fn.argtypes, want):
        ok = CTYPE[w] if isinstance(CTYPE[w], tuple) else (CTYPE[w],)
        assert got in ok, (name, w, got)


def test_backend_has_the_new_methods():
    for meth in ("set_constraints", "clear_constraints", "constraint_info", "constraint_fields", "constrained_mean", "constrained_var",
                 "constraint_correct", "constraint_correct_dev", "sample", "sample_dev"):
        assert callable(getattr(gmrfx.MI355XBackend, meth)), meth


def _symbolic(nx=12, ny=11):
    mesh = spde.grid_mesh_2d(nx, ny, jitter=0.2, seed=3)
    Q = spde.matern_precision(mesh, smoothness=0, range_=0.4)
    return gmrfx.MI355XBackend(Q, coords=mesh.points, symbolic_only=True), Q


def _rows(n, m, seed=0):
    rng = np.random.default_rng(seed)
    rows = [np.ones(n)]
    for _ in range(m - 1):
        r = np.zeros(n)
        idx = rng.choice(n, size=5, replace=False)
        r[idx] = rng.standard_normal(5)
        rows.append(r)
    return sp.csr_matrix(np.array(rows)), rng.standard_normal(m)


def _invalid(be, m, rowptr, colind, values, e):
    before = be.constraint_info()
    with pytest.raises(ValueError) as ei:
        be.set_constraints_csr(m, rowptr, colind, values, e)
    assert len(str(ei.value)) > len("gmrfx: ")        # GMRFX_ERR_INVALID_ARG with a message
    code = _lib.lib().gmrfx_constraints_set(be._h, m, _lib.ptr(np.asarray(rowptr, np.int64)), _lib.ptr(np.asarray(colind, np.int64)),
                                            _lib.ptr(np.asarray(values, np.float64)), 0, _lib.ptr(np.asarray(e, np.float64)))
    assert code == _lib.ERR_INVALID_ARG
    assert _lib.lib().gmrfx_last_error(be._h)
    assert be.constraint_info() == before              # nothing changed


def test_symbolic_handle_accepts_validates_and_reports():
    be, Q = _symbolic()
    n = be.n
    assert be.constraint_info() == {"m": 0, "logdet_AAt": 0.0}
    for m in (1, 3, 17, 64):
        A, e = _rows(n, m, seed=m)
        be.set_constraints(A, e)
        info = be.constraint_info()
        assert info["m"] == m
        ref = np.linalg.slogdet((A @ A.T).toarray())[1]
        assert abs(info["logdet_AAt"] - ref) <= 1e-12 * abs(ref), (m, info["logdet_AAt"], ref)
    # duplicates within a row are summed: [1, 1] twice on column 0 = 2 on column 0
    be.set_constraints_csr(1, [0, 3], [0, 0, 5], [1.0, 1.0, 3.0], [0.5])
    assert abs(be.constraint_info()["logdet_AAt"] - np.log(2.0 ** 2 + 3.0 ** 2)) < 1e-14
    A, e = _rows(n, 3, seed=1)
    be.set_constraints(A, e)
    # each invalid form: INVALID_ARG, a message, the constraint of before untouched
    A65, e65 = _rows(n, 65, seed=2)
    _invalid(be, 65, A65.indptr, A65.indices, A65.data, e65)                 # m = 65
    _invalid(be, 1, [0, 2], [0, n], [1.0, 1.0], [0.0])                       # column = n
    _invalid(be, 1, [0, 2], [-1, 3], [1.0, 1.0], [0.0])                      # column < 0
    _invalid(be, 2, [0, 2, 2], [0, 1], [1.0, 1.0], [0.0, 0.0])               # an empty row
    _invalid(be, 2, [0, 2, 1], [0, 1], [1.0, 1.0], [0.0, 0.0])               # non-monotone rowptr
    assert be.constraint_info()["m"] == 3
    # a clone carries the constraint
    cl = be.clone()
    assert cl.constraint_info() == be.constraint_info()
    # m = 0 clears (the clone keeps its own)
    be.clear_constraints()
    assert be.constraint_info() == {"m": 0, "logdet_AAt": 0.0}
    assert cl.constraint_info()["m"] == 3


def test_batched_symbolic_handle_is_rejected():
    mesh = spde.grid_mesh_2d(8, 8, jitter=0.2, seed=1)
    Q = spde.matern_precision(mesh, smoothness=0, range_=0.4)
    bb = gmrfx.MI355XBatchBackend(Q, 3, coords=mesh.points, symbolic_only=True)
    n = Q.shape[0]
    rp, ci, va, e = (np.array([0, n], np.int64), np.arange(n, dtype=np.int64), np.ones(n), np.zeros(1))
    code = _lib.lib().gmrfx_constraints_set(bb._h, 1, _lib.ptr(rp), _lib.ptr(ci), _lib.ptr(va), 0, _lib.ptr(e))
    assert code == _lib.ERR_INVALID_ARG
    assert b"batched" in _lib.lib().gmrfx_last_error(bb._h)
    m = C.c_int64(-1)
    assert _lib.lib().gmrfx_constraints_info(bb._h, C.byref(m), None, None, None) == 0 and m.value == 0


def test_numeric_entry_points_need_a_device():
    be, Q = _symbolic()
    n = be.n
    A, e = _rows(n, 3, seed=4)
    be.set_constraints(A, e)
    L = _lib.lib()
    X = np.zeros((n, 2), order="F")
    out = np.zeros(n)
    d, i = C.c_double(0.0), C.c_int64(0)
    calls = [
        lambda: L.gmrfx_constraints_info(be._h, C.byref(i), C.byref(d), None, None),
        lambda: L.gmrfx_constraints_get(be._h, None, n, None),
        lambda: L.gmrfx_constraints_mean(be._h, None, _lib.ptr(out), C.byref(d)),
        lambda: L.gmrfx_constraints_correct(be._h, _lib.ptr(X), n, 2),
        lambda: L.gmrfx_constraints_correct_dev(be._h, _lib.ptr(X), n, 2),
        lambda: L.gmrfx_constraints_var(be._h, _lib.ptr(out)),
        lambda: L.gmrfx_sample(be._h, _lib.ptr(X), n, 2, None, _lib.ptr(X), n),
        lambda: L.gmrfx_sample_dev(be._h, _lib.ptr(X), n, 2, None, _lib.ptr(X), n),
    ]
    for k, f in enumerate(calls):
        assert f() == _lib.ERR_NO_DEVICE, k
    for f in (lambda: be.constraint_fields(), lambda: be.constrained_mean(), lambda: be.constrained_var(), lambda: be.constraint_correct(X),
              lambda: be.sample(X)):
        with pytest.raises(NoDeviceError):
            f()


def test_shape_checks_raise_before_any_call():
    be, Q = _symbolic()
    n = be.n
    with pytest.raises(ValueError):
        be.set_constraints(sp.csr_matrix(np.ones((1, n + 1))), [0.0])
    with pytest.raises(ValueError):
        be.set_constraints(sp.csr_matrix(np.ones((2, n))), [0.0])
    with pytest.raises(ValueError):
        be.constraint_correct(np.zeros((n + 1, 2)))
    with pytest.raises(ValueError):
        be.sample(np.zeros((n, 2)), mean=np.zeros(n - 1))
    with pytest.raises(ValueError):
        be.constrained_mean(np.zeros(n + 2))
    with pytest.raises(ValueError):
        be.constraint_correct_dev(0, n, 2)
    with pytest.raises(ValueError):
        be.sample_dev(1, n - 1, 2, 1, n)
