"""The C ABI's refusals, host only: the (return code, message) pair of every refusing call below is pinned as a literal, recorded
from the library before its boundary file was split by subject. Symbolic-only handles and null or ill-formed arguments only: no
device is touched, nothing numeric runs. A refusal keeps its code, its text byte for byte, and its place in the order of checks
(the last case has two wrong arguments and pins which one is reported)."""
import ctypes as C

import numpy as np
import pytest

from gmrfx._lib import GmrfxOpts, lib, ptr

INVALID_ARG, NO_DEVICE = 1, 2
N = 6           # a tridiagonal pattern of six nodes, both triangles, 0-based
NO_DEVICE_MSG = "handle has no device state (symbolic_only or no HIP device): numeric entry points are GPU-only"


def _pattern():
    cp, ri = [0], []
    for j in range(N):
        ri += [i for i in (j - 1, j, j + 1) if 0 <= i < N]
        cp.append(len(ri))
    return np.array(cp, dtype=np.int64), np.array(ri, dtype=np.int64)


COLPTR, ROWVAL = _pattern()
NNZ = int(COLPTR[-1])


def _opts(**kw):
    o = GmrfxOpts()
    o.struct_size = C.sizeof(GmrfxOpts)
    o.symbolic_only = 1
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _f64(*v):
    return np.array(v, dtype=np.float64)


class _Handle:
    """A symbolic-only handle (nbatch = 0: plain) for the duration of a `with` block."""

    def __init__(self, nbatch=0):
        self.nbatch = nbatch

    def __enter__(self):
        self.h = C.c_void_p()
        o = _opts()
        if self.nbatch:
            rc = lib().gmrfx_create_batched(N, ptr(COLPTR), ptr(ROWVAL), 0, None, self.nbatch, C.byref(o), C.byref(self.h))
        else:
            rc = lib().gmrfx_create(N, ptr(COLPTR), ptr(ROWVAL), 0, None, C.byref(o), C.byref(self.h))
        assert rc == 0 and self.h.value, lib().gmrfx_last_create_error()
        return self.h

    def __exit__(self, *exc):
        lib().gmrfx_destroy(self.h)


def _created(rc, h):
    msg = lib().gmrfx_last_create_error().decode()
    if h.value:
        lib().gmrfx_destroy(h)
    return rc, msg


def _create(out=True, colptr=COLPTR, opts=None):
    h = C.c_void_p()
    o = opts if opts is not None else _opts()
    return _created(lib().gmrfx_create(N, ptr(colptr), ptr(ROWVAL), 0, None, C.byref(o), C.byref(h) if out else None), h)


def _create_batched(n, nbatch, colptr=COLPTR, rowval=ROWVAL, **kw):
    h = C.c_void_p()
    o = _opts(**kw)
    return _created(lib().gmrfx_create_batched(n, ptr(colptr), ptr(rowval), 0, None, nbatch, C.byref(o), C.byref(h)), h)


def _create_coord_dim_4():
    xy = np.zeros((N, 4))
    return _create(opts=_opts(coords=xy.ctypes.data, coord_dim=4))


def _on(call, nbatch=0):
    """(code, message) of call(L, h) on a fresh symbolic-only handle"""
    with _Handle(nbatch) as h:
        rc = call(lib(), h)
        return rc, lib().gmrfx_last_error(h).decode()


X = np.zeros((N, 2), order="F")
X2 = np.zeros(2 * N * 2)          # two members' N x 2 blocks, packed
OUT = np.zeros(2 * N)
A_ROW = dict(rowptr=_i64(0, 2), colind=_i64(0, 3), values=_f64(1.0, 1.0), e=_f64(0.0))


def _con_set(L, h, m=1, rowptr=A_ROW["rowptr"], colind=A_ROW["colind"], values=A_ROW["values"], e=A_ROW["e"], batch=False):
    f = L.gmrfx_batch_constraints_set if batch else L.gmrfx_constraints_set
    return f(h, m, ptr(rowptr), ptr(colind), ptr(values), 0, ptr(e))


def _con_set_while_batch_constraint_held(L, h):
    assert _con_set(L, h, batch=True) == 0
    return _con_set(L, h)


def _kl(ldt=N, task_rows=None, l_colptr=None):
    # L = the identity's pattern (one entry per column); one task of two rows (0, 1) with the columns 0 and 1
    theta = np.eye(N, order="F")
    l_colptr = np.arange(N + 1, dtype=np.int64) if l_colptr is None else l_colptr
    task_rows = _i64(0, 1) if task_rows is None else task_rows
    nz = np.zeros(int(l_colptr[-1]) + 8)
    info = C.c_int64(0)
    rc = lib().gmrfx_kl_cholesky(N, ptr(theta), ldt, 0, ptr(l_colptr), 1, ptr(_i64(0, 2)), ptr(task_rows), ptr(_i64(0, 2)),
                                 ptr(_i64(0, 1)), 0, 0.0, -1, ptr(nz), C.byref(info))
    return rc, lib().gmrfx_last_create_error().decode()


BIG = (1 << 30) + 1         # nvec with nvec * 2 members over INT32_MAX

CASES = {
    # ---- create calls --------------------------------------------------------------------------------------------------------------
    "create_out_null": lambda: _create(out=False),
    "create_colptr_null": lambda: _create(colptr=None),
    "create_struct_size_0": lambda: _create(opts=_opts(struct_size=0)),
    "create_coord_dim_4": _create_coord_dim_4,
    "create_shard_rank_out_of_range": lambda: _create(opts=_opts(shard_world=2, shard_rank=5)),
    "create_batched_nbatch_0": lambda: _create_batched(N, 0),
    "create_batched_forest_over_int32": lambda: _create_batched(1 << 20, 1 << 12, np.arange((1 << 20) + 1, dtype=np.int64),
                                                                np.arange(1 << 20, dtype=np.int64)),
    "create_batched_shard_world_2": lambda: _create_batched(N, 2, shard_world=2),
    # ---- numeric entry points on a symbolic-only handle, one per file of the boundary --------------------------------------------------
    "no_device_core_refactorize": lambda: _on(lambda L, h: L.gmrfx_refactorize(h, ptr(np.ones(NNZ)), None)),
    "no_device_shard_logdet_partial": lambda: _on(lambda L, h: L.gmrfx_logdet_partial(h, C.byref(C.c_double()))),
    "no_device_selinv_diag": lambda: _on(lambda L, h: L.gmrfx_selinv_diag(h, ptr(OUT))),
    "no_device_batch_logdet": lambda: _on(lambda L, h: L.gmrfx_batch_logdet(h, ptr(OUT))),
    "no_device_constraints_var": lambda: _on(lambda L, h: L.gmrfx_constraints_var(h, ptr(OUT))),
    "no_device_rbmc_var": lambda: _on(lambda L, h: L.gmrfx_rbmc_var(h, None, ptr(X), N, 2, -1, ptr(OUT))),
    # ---- checks that fire before the handle is asked for its device ------------------------------------------------------------------
    "batch_solve_ldb_small": lambda: _on(lambda L, h: L.gmrfx_batch_solve(h, ptr(X), N - 1, 0, 2, ptr(X), N, 0)),
    "batch_solve_member_stride_small": lambda: _on(lambda L, h: L.gmrfx_batch_solve(h, ptr(X2), N, 2 * N - 1, 2, ptr(X2), N, 2 * N), nbatch=2),
    "batch_quadform_nvec_nbatch_over_int32": lambda: _on(lambda L, h: L.gmrfx_batch_quadform(h, None, ptr(X2), N, N * BIG, BIG, None, ptr(OUT)),
                                                         nbatch=2),
    "constraints_correct_nvec_negative": lambda: _on(lambda L, h: L.gmrfx_constraints_correct(h, ptr(X), N, -1)),
    "rbmc_var_nsamples_1": lambda: _on(lambda L, h: L.gmrfx_rbmc_var(h, None, ptr(X), N, 1, -1, ptr(OUT))),
    "rbmc_var_enclosure_minus_2": lambda: _on(lambda L, h: L.gmrfx_rbmc_var(h, None, ptr(X), N, 2, -2, ptr(OUT))),
    "rbmc_plan_index_base_2": lambda: _on(lambda L, h: L.gmrfx_rbmc_plan(h, 1, 2, ptr(_i64(0, 0, 0)), None, None, None, None)),
    "constraints_set_m_65": lambda: _on(lambda L, h: _con_set(L, h, m=65)),
    "constraints_set_empty_row": lambda: _on(lambda L, h: _con_set(L, h, m=2, rowptr=_i64(0, 2, 2), e=_f64(0.0, 0.0))),
    "constraints_set_column_out_of_range": lambda: _on(lambda L, h: _con_set(L, h, colind=_i64(0, N))),
    "constraints_set_rowptr_not_monotone": lambda: _on(lambda L, h: _con_set(L, h, m=2, rowptr=_i64(0, 2, 1), e=_f64(0.0, 0.0))),
    "constraints_set_batched_handle": lambda: _on(_con_set, nbatch=2),
    "constraints_set_batch_constraint_held": lambda: _on(_con_set_while_batch_constraint_held),
    "kl_cholesky_ldt_small": lambda: _kl(ldt=N - 1),
    "kl_cholesky_task_rows_out_of_range": lambda: _kl(task_rows=_i64(0, N)),
    "kl_cholesky_column_longer_than_task": lambda: _kl(l_colptr=_i64(0, 3, 4, 5, 6, 7, 8)),
    # ---- two wrong arguments at once: which refusal wins -------------------------------------------------------------------------------
    "batch_solve_nrhs_negative_and_B_null": lambda: _on(lambda L, h: L.gmrfx_batch_solve(h, None, N, 0, -1, ptr(X), N, 0)),
}

EXPECTED = {
    'create_out_null': (INVALID_ARG, 'out is null'),
    'create_colptr_null': (INVALID_ARG, 'colptr/rowval is null'),
    'create_struct_size_0': (INVALID_ARG, 'opts.struct_size not set'),
    'create_coord_dim_4': (INVALID_ARG, 'coord_dim must be 2 or 3'),
    'create_shard_rank_out_of_range': (INVALID_ARG, 'shard_rank out of range'),
    'create_batched_nbatch_0': (INVALID_ARG, 'nbatch must be >= 1'),
    'create_batched_forest_over_int32': (INVALID_ARG, 'nbatch * n exceeds INT32_MAX (32-bit node indices of the forest)'),
    'create_batched_shard_world_2': (INVALID_ARG, 'batched handles cannot be sharded (shard_world > 1 / shard_min_top > 0)'),
    'no_device_core_refactorize': (NO_DEVICE, NO_DEVICE_MSG),
    'no_device_shard_logdet_partial': (NO_DEVICE, NO_DEVICE_MSG),
    'no_device_selinv_diag': (NO_DEVICE, NO_DEVICE_MSG),
    'no_device_batch_logdet': (NO_DEVICE, NO_DEVICE_MSG),
    'no_device_constraints_var': (NO_DEVICE, NO_DEVICE_MSG),
    'no_device_rbmc_var': (NO_DEVICE, NO_DEVICE_MSG),
    'batch_solve_ldb_small': (INVALID_ARG, 'B: leading dimension smaller than n'),
    'batch_solve_member_stride_small': (INVALID_ARG, 'B: member stride smaller than ld * columns'),
    'batch_quadform_nvec_nbatch_over_int32': (INVALID_ARG, 'nvec * nbatch exceeds INT32_MAX'),
    'constraints_correct_nvec_negative': (INVALID_ARG, 'nvec < 0'),
    'rbmc_var_nsamples_1': (INVALID_ARG, 'rbmc_var: nsamples < 2 (the corrected sample variance needs two samples)'),
    'rbmc_var_enclosure_minus_2': (INVALID_ARG, 'rbmc_var: enclosure_size < -1'),
    'rbmc_plan_index_base_2': (INVALID_ARG, 'rbmc_plan: index_base must be 0 or 1'),
    'constraints_set_m_65': (INVALID_ARG, 'constraints: more than 64 rows (the limit of the device path: one sweep pass, m x m operands in LDS)'),
    'constraints_set_empty_row': (INVALID_ARG, 'constraints: row 1 of A is empty'),
    'constraints_set_column_out_of_range': (INVALID_ARG, 'constraints: column index out of range'),
    'constraints_set_rowptr_not_monotone': (INVALID_ARG, 'rowptr not monotone'),
    'constraints_set_batched_handle': (INVALID_ARG, 'constraints: batched handles are not supported (their members take gmrfx_batch_constraints_set)'),
    'constraints_set_batch_constraint_held': (INVALID_ARG, 'constraints: the handle holds a batch constraint (gmrfx_batch_constraints_set); clear it first'),
    'kl_cholesky_ldt_small': (INVALID_ARG, 'kl_cholesky: null argument / ldt < n'),
    'kl_cholesky_task_rows_out_of_range': (INVALID_ARG, 'task_rows out of range'),
    'kl_cholesky_column_longer_than_task': (INVALID_ARG, 'kl_cholesky: a column has more entries than its task has rows'),
    'batch_solve_nrhs_negative_and_B_null': (INVALID_ARG, 'nrhs < 0'),
}


def test_every_case_has_an_expectation():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal_code_and_message(name):
    got = CASES[name]()
    print(name, got)
    assert got == EXPECTED[name]
