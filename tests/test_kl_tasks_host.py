"""The task sets of tests/kl_tasks.py without a device: their size classes and edges pinned as literals (what
tests/test_gpu_klchol_edges.py relies on), the 0- and 1-based C-ABI arrays, the long-double reference against the scipy
restatements of oracle/orc.py, and e_ref -- the error of LAPACK's double-precision answer measured against the long-double
one, from which the device test's tolerance is derived."""
import numpy as np
import pytest

import kl_tasks as kt
import orc
from gmrfx import _lib, klchol

SETS = {
    "edges": (kt.edge_set, kt.REG_COLUMN),
    "supernodes": (kt.supernodal_set, kt.REG_SUPERNODAL),
    "chunk": (kt.chunk_set, kt.REG_COLUMN),
    "mixed": (kt.mixed_set, kt.REG_COLUMN),
}


@pytest.fixture(scope="module")
def theta():
    return kt.theta_well(kt.N_THETA, 0)


@pytest.fixture(scope="module")
def reference(theta):
    return kt.Reference(theta)


def test_theta_well_is_well_conditioned(theta):
    assert theta.shape == (640, 640) and (theta == theta.T).all() and theta.flags.f_contiguous
    w = np.linalg.eigvalsh(theta)
    assert w[0] > 1.0 and w[-1] / w[0] < 150.0


def test_class_counts_and_edges_are_pinned():
    """tasks with N <= 32, 33..64, 65..128, > 128"""
    e, s, c, m = kt.edge_set(), kt.supernodal_set(), kt.chunk_set(), kt.mixed_set()
    assert e.sizes() == [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 320, 511, 512]
    assert e.class_counts() == [4, 3, 3, 7]
    assert e.columns() == list(range(17)) and all(e.nk[c] == N for c, N in zip(e.columns(), e.sizes()))
    assert s.sizes() == [32, 64, 65, 128, 129, 200, 512] and s.class_counts() == [1, 1, 2, 3]
    assert sorted(len(cols) for _, cols in s.tasks) == [1, 3, 4, 5, 9, 9, 17]
    nks = {N: sorted(s.nk[c] for c in cols) for (rows, cols), N in zip(s.tasks, s.sizes())}
    assert nks == {N: sorted(k) for N, k in kt.SUPERNODES}
    assert nks[128] == [64] and nks[512] == [1, 64, 65, 128, 129, 192, 193, 511, 512]
    for want in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193):
        assert any(want in v for v in nks.values())
    assert all(N in nks[N] for N in (32, 64, 65, 129, 200, 512)) and all(N - 1 in nks[N] for N in (32, 64, 65, 129, 200, 512))
    # the member columns are listed out of N_k order: wave q % 4 and the column's length are unrelated
    assert any([s.nk[c] for c in cols] != sorted(s.nk[c] for c in cols) for _, cols in s.tasks)
    assert c.sizes() == [129] * 257 and c.class_counts() == [0, 0, 0, 257] and 257 == kt.BIG_CHUNK + 1
    assert m.class_counts() == [3, 0, 3, 258] and m.sizes()[257:] == [65, 100, 128, 5, 32, 17, 512]
    assert m.tasks[:257] == c.tasks
    order3 = [t for t, N in enumerate(m.sizes()) if N > 128]            # launch order of the big class
    assert order3[kt.BIG_CHUNK:] == [256, 263]                          # the second launch
    assert kt.MIXED_BAD == (256, 258, 261, 263) and [m.sizes()[t] for t in kt.MIXED_BAD] == [129, 100, 32, 512]
    assert [kt.private_index(m, t) for t in kt.MIXED_BAD] == [257, 259, 262, 0]
    assert [kt.private_index(e, t) for t in range(17)] == list(range(17))


def test_base0_and_base1_arrays_describe_the_same_problem():
    for build, _ in SETS.values():
        ts = build()
        a0, a1 = ts.arrays(0), ts.arrays(1)
        assert len(a0) == 5
        for x0, x1 in zip(a0, a1):
            assert x0.dtype == np.int64 and x1.dtype == np.int64 and (x1 == x0 + 1).all()
        colptr, rowptr, rows, tcolptr, cols = a0
        assert colptr[0] == rowptr[0] == tcolptr[0] == 0 and len(colptr) == ts.n + 1
        assert rowptr[-1] == len(rows) and tcolptr[-1] == len(cols) and len(rowptr) == len(tcolptr) == len(ts.tasks) + 1
        for t, (R, Cs) in enumerate(ts.tasks):
            assert rows[rowptr[t]:rowptr[t + 1]].tolist() == R and cols[tcolptr[t]:tcolptr[t + 1]].tolist() == Cs
            for c in Cs:                                # N_k = entries of column c = position of c in R, plus one
                assert colptr[c + 1] - colptr[c] == R.index(c) + 1
        P = ts.pattern()
        assert (P.indptr == colptr).all() and P.nnz == colptr[-1]
        ci, ri = ts.lists()
        Q = klchol.supernodal_pattern(ci, ri, ts.n)
        assert (P.indices == Q.indices).all() and (P.indptr == Q.indptr).all()


@pytest.mark.parametrize("base", [0, 1])
def test_both_index_bases_pass_the_argument_checks(theta, base):
    """gmrfx_kl_cholesky shifts every pointer and index by index_base before it checks them (rows in range, every member
    column no longer than its task): a pointer left unshifted pairs tasks with their neighbours' columns and is refused
    there. Without a device the call then ends with a HIP error, with one it computes."""
    sets = [build() for build, _ in SETS.values()] + [kt.edge_set().per_column()]
    for ts in sets:
        for alias in ([False, True] if len(ts.tasks) == ts.n else [False]):
            code, info, _ = ts.run(theta, kt.N_THETA, base=base, alias=alias)
            assert code in (_lib.GMRFX_OK, _lib.ERR_NO_DEVICE, _lib.ERR_HIP) and info == 0, (ts.name, base, alias, code)


def test_per_column_form_aliases_colptr_and_rowptr():
    e = kt.edge_set()
    pc = e.per_column()
    colptr, rowptr, rows, tcolptr, cols = pc.arrays(1)
    assert len(pc.tasks) == pc.n and (colptr == rowptr).all()
    assert (tcolptr == np.arange(1, pc.n + 2)).all() and (cols == np.arange(1, pc.n + 1)).all()
    assert pc.tasks[:17] == e.tasks and pc.class_counts() == [4 + 623, 3, 3, 7]


def test_read_mask_is_the_upper_triangle_of_the_row_blocks():
    e = kt.edge_set()
    A = e.read_mask()
    assert not np.tril(A, -1).any() and A.sum() < A.size // 2
    rows = e.tasks[4][0]
    assert A[rows[-1], rows[0]] and not A[rows[0], rows[-1]]
    assert not A[0, 1] and A[0, 0]                     # columns 0 and 1 are private to tasks 0 and 1


@pytest.mark.parametrize("name", sorted(SETS))
def test_longdouble_reference_agrees_with_the_oracle(name, theta, reference):
    build, reg = SETS[name]
    ts = build()
    ref = reference.columns(ts, reg)
    assert sorted(ref) == sorted(ts.columns()) and all(v.dtype == np.longdouble and len(v) == ts.nk[c] for c, v in ref.items())
    if all(len(cols) == 1 for _, cols in ts.tasks):
        Lo = orc.kl_cholesky_inplace(theta, ts.per_column().pattern(), reg=reg)
    else:
        Lo = orc.kl_cholesky_supernodal(theta, *ts.lists(), reg=reg)
        P = ts.pattern()
        assert (P.indices == Lo.indices).all() and (P.indptr == Lo.indptr).all()
    e_ref = 0.0
    for c, x_ld in ref.items():
        x = Lo.data[Lo.indptr[c]:Lo.indptr[c + 1]]
        assert (Lo.indices[Lo.indptr[c]:Lo.indptr[c + 1]] == ts.column_rows(c)[::-1]).all()
        e_ref = max(e_ref, kt.column_ratio(x, x_ld))
    print(f"kl tasks {name}: e_ref = max_k max|x_lapack - x_ld| / max|x_ld| = {e_ref:.3e}")
    # measured: 1.2e-15 (edges, N = N_k = 512), 9.4e-16 (supernodes), 8.0e-16 (chunk, mixed)
    assert e_ref <= 1e-14


def test_reference_restates_the_contract_on_a_small_task(theta):
    """against the closed form through the dense inverse (double precision): x = M[:nk, :nk]^-1 e_nk * C(nk, nk), reversed"""
    rows, nk, reg = [40, 30, 22, 9, 3], 4, 1e-6
    x = kt.ref_longdouble(theta, rows, nk, reg)
    M = theta[np.ix_(rows, rows)][:nk, :nk] + reg * np.eye(nk)
    y = np.linalg.solve(M, np.eye(nk)[:, -1])          # M^-1 e_nk = C^-T C^-1 e_nk = C^-T e_nk / C(nk, nk)
    want = (y / np.sqrt(y[-1]))[::-1]
    assert np.abs(x - want).max() <= 1e-14 * np.abs(want).max()
    assert kt.ref_longdouble(theta, [7], 1, 0.0)[0] == 1 / np.sqrt(np.longdouble(theta[7, 7]))


def test_a_task_of_513_rows_is_refused_before_any_device_work(theta):
    ts = kt.TaskSet(kt.N_THETA, [(list(range(512, -1, -1)), [0])])
    code, info, _ = ts.run(theta, kt.N_THETA)
    assert code == _lib.ERR_INVALID_ARG and info == 0
    with pytest.raises(ValueError, match="more than 512 rows"):
        _lib.check(code)


def test_wrapper_takes_the_host_arrays_own_leading_dimension():
    """argument handling only (the numeric call needs a device): a column-major window keeps its leading dimension, a
    contradicting ldt is refused"""
    buf = np.zeros((7, 4), order="F")
    with pytest.raises(ValueError, match="leading dimension 7"):
        klchol._run(buf[:4], [0, 1, 2, 3, 4], [0, 1], [0], [0, 1], [0], 1e-6, -1, ldt=4)
    with pytest.raises(ValueError, match="square"):
        klchol._run(buf, [0, 1, 2, 3, 4], [0, 1], [0], [0, 1], [0], 1e-6, -1)
