"""The handle's replaceable device memory over its life: constraint state (plain and batched), RBMC plan tables, regrown scratch
and row-diag plans are set, grown, replaced and dropped round after round. What is pinned: stats()["bytes_device_total"] comes back
to the same value after every round (exact equality: sums of integers far below 2^53), and the same inputs give the same bits in
every round. Rounds are compared with each other, never with a number written here: one-time lazy growth (right-hand-side panels,
selected-inverse storage, the pattern upload of sqmahal) lands before or in round 1. Every case prints its figures."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gmrfx
from gmrfx._lib import check, lib, ptr
from test_gpu_batch_constraints import constraint_rows, members
from test_gpu_constraints import matern

pytestmark = pytest.mark.gpu

NX, NY = 19, 17          # 323 nodes: odd, several levels of fronts


def total(be):
    return be.stats()["bytes_device_total"]


def _warm_up_plain(be, rng):
    """Factorised handle; both sweep lanes (64 and 65 columns on the device) and the quadratic form's buffers exist."""
    n = be.n
    dev = torch.device("cuda", 0)
    for nrhs in (64, 65):
        B = torch.from_numpy(rng.standard_normal((nrhs, n))).to(dev)                # = column-major n x nrhs
        X = torch.empty_like(B)
        be.solve_dev(B.data_ptr(), n, nrhs, X.data_ptr(), n)
        torch.cuda.synchronize()
    be.sqmahal(rng.standard_normal(n))


def test_plain_constraints_three_rounds():
    mesh, Q = matern(NX, NY)
    n = Q.shape[0]
    rng = np.random.default_rng(11)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    _warm_up_plain(be, rng)
    A, e = constraint_rows(n, 3, seed=5)
    Z1, Z1100, Y1, Y1100 = (rng.standard_normal((n, k)) for k in (1, 1100, 1, 1100))
    mu = rng.standard_normal(n)
    rounds = []
    for r in range(3):
        be.set_constraints(sp.csr_matrix(A), e)
        got = [be.sample(Z1, mean=mu), be.constraint_correct(Y1),
               be.sample(Z1100, mean=mu), be.constraint_correct(Y1100),         # R / part regrow from 64 to 1024 columns
               be.constrained_var()]
        with_con = total(be)
        be.clear_constraints()
        rounds.append((total(be), with_con, got))
        print(f"round {r + 1}: bytes_device_total {rounds[-1][0]:.0f} (with constraints {with_con:.0f})")
    assert rounds[0][1] > rounds[0][0]                  # the constraint state is on the books while it exists
    for after, with_con, got in rounds[1:]:
        assert after == rounds[0][0] and with_con == rounds[0][1]
    for a, b in zip(rounds[0][2], rounds[2][2]):
        assert np.array_equal(a, b)


def _warm_up_batch(bb, rng):
    n, nb = bb.n, bb.nbatch
    dev = torch.device("cuda", 0)
    for nrhs in (64, 65):
        B = torch.from_numpy(rng.standard_normal((nb, nrhs, n))).to(dev)           # member-strided, column-major n x nrhs blocks
        X = torch.empty_like(B)
        bb.solve_dev(B.data_ptr(), n, n * nrhs, nrhs, X.data_ptr(), n, n * nrhs)
        torch.cuda.synchronize()
    bb.sqmahal(rng.standard_normal((n, nb)))


def test_batch_constraints_three_rounds_and_replacement():
    B = 3
    mesh, Qs, NZ = members(NX, NY, B, seed=4)
    n = Qs[0].shape[0]
    rng = np.random.default_rng(12)
    bb = gmrfx.MI355XBatchBackend(Qs[0], B, coords=mesh.points)
    bb.refactorize_values(NZ)
    _warm_up_batch(bb, rng)
    A, e = constraint_rows(n, 3, seed=6)
    Z1, Z1100, Y1, Y1100 = (rng.standard_normal((n, k, B)) for k in (1, 1100, 1, 1100))
    mu = rng.standard_normal((n, B))
    rounds = []
    for r in range(3):
        bb.set_constraints(sp.csr_matrix(A), e)
        got = [bb.sample(Z1, mean=mu), bb.constraint_correct(Y1),
               bb.sample(Z1100, mean=mu), bb.constraint_correct(Y1100),         # R / part regrow from 64 to 1024 columns
               bb.constrained_var()]
        with_con = total(bb)
        bb.clear_constraints()
        rounds.append((total(bb), with_con, got))
        print(f"round {r + 1}: bytes_device_total {rounds[-1][0]:.0f} (with constraints {with_con:.0f})")
    assert rounds[0][1] > rounds[0][0]
    for after, with_con, got in rounds[1:]:
        assert after == rounds[0][0] and with_con == rounds[0][1]
    for a, b in zip(rounds[0][2], rounds[2][2]):
        assert np.array_equal(a, b)
    # replace without clearing: m = 2, 5, 2
    states = []
    for m in (2, 5, 2):
        Am, em = constraint_rows(n, m, seed=40 + m)
        bb.set_constraints(sp.csr_matrix(Am), em)
        info = bb.constraint_info()
        states.append((total(bb), info))
        print(f"m={m}: bytes_device_total {states[-1][0]:.0f} logdet_W {info['logdet_W']}")
    assert states[1][0] > states[0][0]
    assert states[2][0] == states[0][0]
    first, third = states[0][1], states[2][1]
    assert first["m"] == third["m"] == 2 and first["logdet_AAt"] == third["logdet_AAt"]
    assert np.array_equal(first["logdet_W"], third["logdet_W"]) and np.array_equal(first["cinfo"], third["cinfo"])
    bb.clear_constraints()
    assert total(bb) == rounds[0][0]


def test_rbmc_plan_swaps():
    mesh, Q = matern(NX, NY)
    n = Q.shape[0]
    rng = np.random.default_rng(13)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    Z = rng.standard_normal((n, 40))
    start = total(be)
    be.rbmc_var(Z, -1)                                   # no plan: the row structure and the work arrays, once
    without_plan = total(be)
    visits = [(enc, be.rbmc_var(Z, enc), total(be)) for enc in (0, 2, 0, 2)]
    for enc, _, bytes_ in visits:
        print(f"enclosure {enc}: bytes_device_total {bytes_:.0f} (no plan {without_plan:.0f}, before {start:.0f})")
    assert without_plan > start and all(b > without_plan for _, _, b in visits)
    assert visits[2][2] == visits[0][2] and visits[3][2] == visits[1][2]
    assert np.array_equal(visits[2][1], visits[0][1]) and np.array_equal(visits[3][1], visits[1][1])
    assert not np.array_equal(visits[0][1], visits[1][1])


def test_regrown_scratch():
    mesh, Q = matern(NX, NY)
    n = Q.shape[0]
    rng = np.random.default_rng(14)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    for what, call, widths in (("sqmahal", be.sqmahal, (1, 40, 1, 40)), ("solve", be.backend_solve, (1, 70, 1, 70))):
        X = {k: rng.standard_normal((n, k)) for k in set(widths)}
        seen = [(k, call(X[k]), total(be)) for k in widths]
        print(what, [(k, f"{b:.0f}") for k, _, b in seen])
        assert seen[1][2] >= seen[0][2]
        assert seen[2][2] == seen[1][2] and seen[3][2] == seen[1][2]          # constant from the first wide call on
        assert np.array_equal(seen[2][1], seen[0][1]) and np.array_equal(seen[3][1], seen[1][1])


def test_rowdiag_plans_are_not_on_the_books():
    mesh, Q = matern(NX, NY)
    n = Q.shape[0]
    rng = np.random.default_rng(15)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points)
    be.get_selinv_diag()                                 # the selected inverse and its storage exist
    A = sp.csr_matrix(Q[:7] != 0, dtype=np.float64)      # rows inside the factor pattern
    A.data = rng.standard_normal(A.nnz)
    rowptr, colind = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    vals = np.ascontiguousarray(A.data)

    def create():
        pid = C.c_int64(-1)
        check(lib().gmrfx_selinv_row_diag_plan(be._h, A.shape[0], ptr(rowptr), ptr(colind), 0, C.byref(pid)), be._h)
        return pid.value

    def apply(pid):
        out = np.empty(A.shape[0])
        check(lib().gmrfx_selinv_row_diag_apply(be._h, pid, ptr(vals), ptr(out)), be._h)
        return out

    before = total(be)
    first = create()
    v1 = apply(first)
    during = total(be)
    check(lib().gmrfx_selinv_row_diag_free(be._h, first), be._h)
    freed = total(be)
    second = create()
    v2 = apply(second)
    print(f"plan ids {first} {second}; bytes_device_total before {before:.0f} during {during:.0f} after {freed:.0f} again {total(be):.0f}")
    assert second == first
    assert np.array_equal(v1, v2) and np.isfinite(v1).all()
    assert before == during == freed == total(be)
