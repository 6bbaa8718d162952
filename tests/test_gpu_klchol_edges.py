"""The KL (Vecchia) sparse approximate Cholesky kernels (csrc/klchol.hip: k_kl_chol<32|64|128>, k_kl_chol_big, kl_cholesky_run)
column by column on the task sets of tests/kl_tasks.py (tests/test_kl_tasks_host.py pins their size classes): one task at every
class edge, supernodes with 1..17 member columns and N_k on every 64-boundary of the register slots, a 257th task of the big
class (second launch), task order, leading dimensions / device-resident Theta / index_base 1 with the Julia plug-in's aliasing,
the entries of Theta that may be read, and the reported task of a block that is not positive definite.

Comparison rule. Theta = kl_tasks.theta_well(640, 0) has a condition number of about 1e2, and the bound holds for every member
column k on its own, against the long-double restatement of the contract (kl_tasks.ref_longdouble), never against LAPACK:

    max_i |x_gpu - x_ld| <= TOL * max_i |x_ld|,    TOL = 64 * e_ref = 64 * 1.2e-15 = 7.7e-14.

e_ref = 1.2e-15 is what LAPACK's double-precision potrf + trtrs lose against the same long-double reference on these task sets
(measured by tests/test_kl_tasks_host.py: 1.175e-15 at N = N_k = 512, below 9.5e-16 on every other column). The factor 64 is the
allowance for what the kernel does differently from LAPACK while being just as correct: a right-looking update order (each
entry is a different sum of the same N products), inv = 1 / sqrt(d) followed by a multiplication where LAPACK divides by
sqrt(d) (one more rounding per entry), and fused multiply-adds where the compiler contracts. 64 eps-sized allowances still leave
the bound eight orders of magnitude below the 1e-3-of-a-column errors that a whole-matrix bound of 1e-8 * max|L| lets through,
and a column left at zero, reversed, or solved with the wrong right-hand side misses it by twelve.

Largest ratios observed on an MI355X (each case prints its own): 2.1e-15 on the supernodal set (N = 512, N_k = 511), 1.3e-15 on the
edge set (N = N_k = 512), 8.6e-16 over the 257 tasks of 129 rows -- the kernels are as accurate as LAPACK here, 36 times inside TOL."""
import numpy as np
import pytest

import gmrfx
import kl_tasks as kt
from gmrfx import _lib, klchol

pytestmark = pytest.mark.gpu

E_REF = 1.2e-15
TOL = 64 * E_REF
N = kt.N_THETA


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Ctx:
    """Theta, the long-double reference and the task sets, built once; the clean result of a set is computed once and every
    column of it is held to the bound at that moment"""

    def __init__(self):
        self.theta = kt.theta_well(N, 0)
        self.ref = kt.Reference(self.theta)
        self.sets = {"edges": (kt.edge_set(), kt.REG_COLUMN), "supernodes": (kt.supernodal_set(), kt.REG_SUPERNODAL),
                     "chunk": (kt.chunk_set(), kt.REG_COLUMN), "mixed": (kt.mixed_set(), kt.REG_COLUMN)}
        self._clean = {}

    def check_columns(self, ts, nz, reg, label):
        """every member column within TOL of the long-double reference; returns (and prints) the largest ratio"""
        ref = self.ref.columns(ts, reg)
        assert np.isfinite(nz).all(), label
        ratio = {c: kt.column_ratio(ts.column(nz, c), x_ld) for c, x_ld in ref.items()}
        describe = lambda c: (len(ts.tasks[ts.task_of[c]][0]), ts.nk[c], c, ratio[c])
        at = max(ratio, key=ratio.get)
        worst = ratio[at]
        print(f"kl edges {label}: max_k max_i|x - x_ld| / max_i|x_ld| = {worst:.3e} at (N, N_k, column, ratio) = {describe(at)}; TOL = {TOL:.2e}")
        bad = [describe(c) for c in ratio if not ratio[c] <= TOL]
        assert not bad, f"{label}: {len(bad)} columns (N, N_k, column, ratio) over TOL: {bad[:8]}"
        return worst

    def clean(self, name):
        if name not in self._clean:
            ts, reg = self.sets[name]
            code, info, nz = ts.run(self.theta, N, reg=reg)
            assert code == _lib.GMRFX_OK and info == 0
            self.check_columns(ts, nz, reg, name)
            self._clean[name] = nz
        return self._clean[name]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


# ---- 1. one task per class edge ---------------------------------------------------------------------------------------------

def test_one_task_per_class_edge(ctx):
    ts, reg = ctx.sets["edges"]
    nz = ctx.clean("edges")
    for t, (rows, cols) in enumerate(ts.tasks):            # the same task alone: same bits, whatever its neighbours were
        one = ts.subset([t])
        code, info, z = one.run(ctx.theta, N, reg=reg)
        assert code == _lib.GMRFX_OK and info == 0
        assert len(z) == len(rows) and same_bits(z, ts.column(nz, cols[0])), f"task of {len(rows)} rows differs when run alone"
    # and through the wrapper (one task per column of a pattern with a full diagonal)
    pc = ts.per_column()
    L = klchol.sparse_approximate_cholesky_inplace(ctx.theta, pc.pattern())
    for c in ts.columns():
        assert same_bits(L.data[L.indptr[c]:L.indptr[c + 1]], ts.column(nz, c))
        assert (L.indices[L.indptr[c]:L.indptr[c + 1]] == ts.column_rows(c)[::-1]).all()


# ---- 2. supernodal form in every class --------------------------------------------------------------------------------------

def test_supernodes_in_every_class(ctx):
    ts, reg = ctx.sets["supernodes"]
    nz = ctx.clean("supernodes")
    ci, ri = ts.lists()
    P, Q = ts.pattern(), klchol.supernodal_pattern(ci, ri, N)
    assert (P.indices == Q.indices).all() and (P.indptr == Q.indptr).all()
    L = klchol.sparse_approximate_cholesky_supernodal(ctx.theta, ci, ri)
    assert (L.indices == P.indices).all() and (L.indptr == P.indptr).all() and same_bits(L.data, nz)
    for t in range(len(ts.tasks)):                          # each supernode alone: same bits
        one = ts.subset([t])
        code, info, z = one.run(ctx.theta, N, reg=reg)
        assert code == _lib.GMRFX_OK
        for c in one.columns():
            assert same_bits(one.column(z, c), ts.column(nz, c)), (len(ts.tasks[t][0]), ts.nk[c])


# ---- 3. chunked big class ---------------------------------------------------------------------------------------------------

def test_a_257th_task_of_the_big_class(ctx):
    ts, reg = ctx.sets["chunk"]
    nz = ctx.clean("chunk")
    last = len(ts.tasks) - 1
    assert last == kt.BIG_CHUNK
    one = ts.subset([last])
    code, info, z = one.run(ctx.theta, N, reg=reg)
    assert code == _lib.GMRFX_OK and same_bits(z, ts.column(nz, ts.tasks[last][1][0]))


# ---- 4. task order ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edges", "supernodes", "mixed"])
def test_task_order_does_not_change_a_bit(ctx, name):
    ts, reg = ctx.sets[name]
    nz = ctx.clean(name)
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(ts.tasks))
    shuffled = kt.TaskSet(N, [(ts.tasks[t][0], [int(c) for c in rng.permutation(ts.tasks[t][1])]) for t in perm])
    assert shuffled.sizes() != ts.sizes() and sorted(shuffled.sizes()) == sorted(ts.sizes())
    assert (shuffled.colptr == ts.colptr).all()             # nzval is laid out by column: the same array is expected
    code, info, z = shuffled.run(ctx.theta, N, reg=reg)
    assert code == _lib.GMRFX_OK and info == 0 and same_bits(z, nz)
    code, info, again = ts.run(ctx.theta, N, reg=reg)       # two identical calls
    assert code == _lib.GMRFX_OK and same_bits(again, nz)


# ---- 5. layouts and index base ----------------------------------------------------------------------------------------------

def _padded(theta, pad):
    buf = np.full((N + pad, N), np.nan, order="F")
    buf[:N] = theta
    return buf


def test_host_theta_with_a_padded_leading_dimension(ctx):
    ts, reg = ctx.sets["edges"]
    nz = ctx.clean("edges")
    buf = _padded(ctx.theta, 3)
    before = buf.copy(order="F")
    code, info, z = ts.run(buf, N + 3, reg=reg)
    assert code == _lib.GMRFX_OK and info == 0 and same_bits(z, nz) and same_bits(buf, before)
    # the wrapper takes the window's own leading dimension (no copy is needed, none is visible)
    L = klchol.sparse_approximate_cholesky_inplace(buf[:N], ts.per_column().pattern())
    for c in ts.columns():
        assert same_bits(L.data[L.indptr[c]:L.indptr[c + 1]], ts.column(nz, c))
    assert same_bits(buf, before)


@pytest.mark.parametrize("pad", [0, 3])
def test_device_resident_theta(ctx, pad):
    import torch
    ts, reg = ctx.sets["edges"]
    nz = ctx.clean("edges")
    buf = _padded(ctx.theta, pad)                           # column-major (N + pad) x N == row-major N x (N + pad)
    d = torch.from_numpy(np.ascontiguousarray(buf.T)).cuda()
    torch.cuda.synchronize()
    code, info, z = ts.run(int(d.data_ptr()), N + pad, reg=reg)
    assert code == _lib.GMRFX_OK and info == 0 and same_bits(z, nz)
    pc = ts.per_column()
    L = klchol.sparse_approximate_cholesky_inplace(None, pc.pattern(), theta_device_ptr=int(d.data_ptr()), ldt=N + pad)
    for c in ts.columns():
        assert same_bits(L.data[L.indptr[c]:L.indptr[c + 1]], ts.column(nz, c))
    if pad == 0:                                            # ldt defaults to n
        L0 = klchol.sparse_approximate_cholesky_inplace(None, pc.pattern(), theta_device_ptr=int(d.data_ptr()))
        assert same_bits(L0.data, L.data)
    torch.cuda.synchronize()
    assert same_bits(d.cpu().numpy().T, buf)                # Theta and its padding are unchanged


def test_index_base_1_with_colptr_aliased_as_rowptr(ctx):
    """the Julia plug-in's call: one task per column, L.colptr passed as L_colptr and as task_rowptr, everything 1-based"""
    ts, reg = ctx.sets["edges"]
    nz = ctx.clean("edges")
    pc = ts.per_column()
    code, info, z0 = pc.run(ctx.theta, N, base=0, reg=reg)
    assert code == _lib.GMRFX_OK and info == 0
    ctx.check_columns(pc, z0, reg, "edges, one task per column")
    before = ctx.theta.copy(order="F")
    code, info, z1 = pc.run(ctx.theta, N, base=1, reg=reg, alias=True)
    assert code == _lib.GMRFX_OK and info == 0 and same_bits(z1, z0) and same_bits(ctx.theta, before)
    for c in ts.columns():
        assert same_bits(pc.column(z1, c), ts.column(nz, c))


def test_index_base_1_on_the_supernodal_set(ctx):
    ts, reg = ctx.sets["supernodes"]
    nz = ctx.clean("supernodes")
    code, info, z = ts.run(ctx.theta, N, base=1, reg=reg)
    assert code == _lib.GMRFX_OK and info == 0 and same_bits(z, nz)


# ---- 6. only the defining entries are read ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edges", "supernodes"])
def test_only_the_defining_entries_of_theta_are_read(ctx, name):
    """theta[R[i] + R[j] * ldt] for local i >= j: with descending rows the global upper triangle of each R x R. Everything else
    -- the lower triangle, and pairs that share no task -- holds 1e30."""
    ts, reg = ctx.sets[name]
    nz = ctx.clean(name)
    mask = ts.read_mask()
    assert not mask[np.tril_indices(N, -1)].any() and 0 < mask.sum() < N * (N + 1) // 2
    poisoned = np.asfortranarray(np.where(mask, ctx.theta, 1e30))
    code, info, z = ts.run(poisoned, N, reg=reg)
    assert code == _lib.GMRFX_OK and info == 0 and same_bits(z, nz)


# ---- 7. failures ------------------------------------------------------------------------------------------------------------

def _expect_not_posdef(ts, theta, reg, t):
    code, info, _ = ts.run(theta, N, reg=reg)
    msg = _lib.lib().gmrfx_last_create_error().decode()
    assert code == _lib.ERR_NOT_POSDEF and info == 1 + t, (code, info, t, msg)
    assert f"task {t} is not positive definite" in msg, msg


def _clean_again(ctx, name):
    ts, reg = ctx.sets[name]
    code, info, z = ts.run(ctx.theta, N, reg=reg)
    assert code == _lib.GMRFX_OK and info == 0 and same_bits(z, ctx.clean(name))     # (whose columns met the bound)


def _negate(ctx, ts, bad):
    th = ctx.theta.copy(order="F")
    for t in bad:
        k = kt.private_index(ts, t)
        th[k, k] = -th[k, k]
    return th


def _nan(ctx, ts, bad):
    """NaN in one off-diagonal entry that only task t reads: (its private column, its largest row)"""
    th = ctx.theta.copy(order="F")
    for t in bad:
        k, top = kt.private_index(ts, t), ts.tasks[t][0][0]
        assert k < top and ts.read_mask()[k, top]
        th[k, top] = np.nan
    return th


BAD = [(256,), (258,), (261,), (256, 258, 261), (261, 258), (263,)]     # (263,): the LAST pivot of the 512-row task


@pytest.mark.parametrize("defect", ["negated diagonal", "nan"])
@pytest.mark.parametrize("bad", BAD, ids=lambda b: "t" + "_".join(map(str, b)))
def test_the_first_bad_task_is_reported(ctx, bad, defect):
    ts, reg = ctx.sets["mixed"]
    ctx.clean("mixed")
    th = (_negate if defect == "negated diagonal" else _nan)(ctx, ts, bad)
    _expect_not_posdef(ts, th, reg, min(bad))
    _clean_again(ctx, "mixed")


def test_the_wrapper_raises_posdef_with_the_task_number(ctx):
    ts, reg = ctx.sets["mixed"]
    ci, ri = ts.lists()
    for bad in ((258,), (256, 261)):
        with pytest.raises(gmrfx.PosDefException) as ei:
            klchol.sparse_approximate_cholesky_supernodal(_negate(ctx, ts, bad), ci, ri, reg=reg)
        assert ei.value.info == 1 + min(bad) and ei.value.code == _lib.ERR_NOT_POSDEF
        assert f"task {min(bad)} " in str(ei.value)
    L = klchol.sparse_approximate_cholesky_supernodal(ctx.theta, ci, ri, reg=reg)
    assert same_bits(L.data, ctx.clean("mixed"))
    # the one-column wrapper numbers tasks by column
    e, _ = ctx.sets["edges"]
    pc = e.per_column()
    th = ctx.theta.copy(order="F")
    th[9, 9] = -th[9, 9]                                    # column 9: the task of 128 rows
    with pytest.raises(gmrfx.PosDefException) as ei:
        klchol.sparse_approximate_cholesky_inplace(th, pc.pattern())
    assert ei.value.info == 10


def test_a_task_of_513_rows_is_an_argument_error(ctx):
    ts = kt.TaskSet(N, [(list(range(512, -1, -1)), [0])])
    code, info, _ = ts.run(ctx.theta, N)
    assert code == _lib.ERR_INVALID_ARG and info == 0
    with pytest.raises(ValueError, match="more than 512 rows"):
        _lib.check(code)
    with pytest.raises(ValueError, match="more than 512 rows"):
        klchol.sparse_approximate_cholesky_supernodal(ctx.theta, [[0]], [list(range(512, -1, -1))])
    _clean_again(ctx, "edges")
