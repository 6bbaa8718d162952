"""Task sets for the KL (Vecchia) sparse approximate Cholesky kernels (csrc/klchol.hip) and a long-double reference of the
contract in include/gmrfx.h (gmrfx_kl_cholesky). No GPU is needed to build them: tests/test_kl_tasks_host.py pins their
size classes and the reference; tests/test_gpu_klchol_edges.py runs them.

A task is a list of local rows R (distinct indices, DESCENDING) and the member columns it fills. A member column k that
sits at local position p of R has N_k = p + 1 entries, the rows R[0..p] (all >= k: the pattern is lower triangular), so a
task of N rows with member columns at chosen N_k is written down directly. Member columns are disjoint between tasks;
rows may be shared."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

N_THETA = 640
CLASS_EDGES = (32, 64, 128)            # k_kl_chol<32|64|128>; above: k_kl_chol_big (up to KL_MAX rows)
KL_MAX = 512
BIG_CHUNK = 256                        # tasks of the big class per launch (kl_cholesky_run)
REG_COLUMN, REG_SUPERNODAL = 1e-6, 1e-8


def theta_well(n, seed):
    """diag(U(1, 2)) + G G' / 8, G n x 8 standard normal: symmetric positive definite with a condition number of about 1e2
    (about 94 for n = 640), so that a tight per-column bound means something"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 2.0, n)
    G = rng.standard_normal((n, 8))
    return np.asfortranarray(np.diag(d) + G @ G.T / 8.0)


def ref_factor(Theta, rows, reg):
    """C (lower, long double) with C C' = Theta[R, R] + reg I, left-looking, column by column"""
    R = np.asarray(rows, dtype=np.int64)
    N = len(R)
    M = np.asarray(Theta, dtype=np.float64)[np.ix_(R, R)].astype(np.longdouble)
    M[np.arange(N), np.arange(N)] += np.longdouble(reg)
    Cf = np.zeros((N, N), dtype=np.longdouble)
    for j in range(N):
        col = M[j:, j] - Cf[j:, :j] @ Cf[j, :j]          # long-double products: numpy's own loops, no BLAS
        if not col[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        Cf[j, j] = np.sqrt(col[0])
        Cf[j + 1:, j] = col[1:] / Cf[j, j]
    return Cf


def ref_longdouble(Theta, rows, nk, reg, Cf=None):
    """x[N_k-1::-1] (long double) with C' x = e_{N_k} on the leading N_k x N_k block of the factor of Theta[R, R] + reg I:
    the values of member column k in L's storage order (ascending row). Plain loops, no LAPACK."""
    if Cf is None:
        Cf = ref_factor(Theta, rows, reg)
    x = np.zeros(nk, dtype=np.longdouble)
    x[nk - 1] = np.longdouble(1) / Cf[nk - 1, nk - 1]
    for j in range(nk - 2, -1, -1):
        x[j] = -(Cf[j + 1:nk, j] @ x[j + 1:nk]) / Cf[j, j]
    return x[::-1].copy()


class TaskSet:
    """explicit (rows, member columns) lists over n indices; the C-ABI arrays for index_base 0 or 1, the scipy pattern, and the
    direct call of gmrfx_kl_cholesky"""

    def __init__(self, n, tasks, name=""):
        self.n, self.name = int(n), name
        self.tasks = [([int(r) for r in rows], [int(c) for c in cols]) for rows, cols in tasks]
        self.nk = {}                                   # member column -> N_k
        self.task_of = {}                              # member column -> task index
        for t, (rows, cols) in enumerate(self.tasks):
            assert len(rows) >= 1 and all(0 <= r < n for r in rows)
            assert all(a > b for a, b in zip(rows, rows[1:])), "rows must be distinct and descending"
            pos = {r: p for p, r in enumerate(rows)}
            for c in cols:
                assert c in pos and c not in self.nk, "member columns are rows of their task and disjoint between tasks"
                self.nk[c] = pos[c] + 1
                self.task_of[c] = t
        counts = np.zeros(self.n, dtype=np.int64)
        for c, k in self.nk.items():
            counts[c] = k
        self.colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    # ---- description ------------------------------------------------------------------------------------------------------
    def sizes(self):
        return [len(rows) for rows, _ in self.tasks]

    def class_counts(self):
        """tasks with N <= 32, 33..64, 65..128, > 128: the four launches of kl_cholesky_run"""
        s = np.asarray(self.sizes())
        e = CLASS_EDGES
        return [int((s <= e[0]).sum()), int(((s > e[0]) & (s <= e[1])).sum()), int(((s > e[1]) & (s <= e[2])).sum()), int((s > e[2]).sum())]

    def columns(self):
        """member columns in task order"""
        return [c for _, cols in self.tasks for c in cols]

    def column_rows(self, c):
        rows, _ = self.tasks[self.task_of[c]]
        return rows[:self.nk[c]]

    def arrays(self, base=0):
        """L_colptr, task_rowptr, task_rows, task_colptr, task_cols (int64, every index and pointer shifted by base)"""
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r, _ in self.tasks])])
        tcolptr = np.concatenate([[0], np.cumsum([len(c) for _, c in self.tasks])])
        rows = np.concatenate([np.asarray(r, dtype=np.int64) for r, _ in self.tasks])
        cols = np.concatenate([np.asarray(c, dtype=np.int64) for _, c in self.tasks])
        return tuple(np.ascontiguousarray(a, dtype=np.int64) + base for a in (self.colptr, rowptr, rows, tcolptr, cols))

    def pattern(self):
        """the lower-triangular pattern of L (scipy CSC, sorted): column k holds the rows R[0..N_k-1] of its task"""
        indices = np.concatenate([np.asarray(self.column_rows(c)[::-1], dtype=np.int64) if c in self.nk else np.zeros(0, np.int64)
                                  for c in range(self.n)])
        P = sp.csc_matrix((np.ones(len(indices)), indices, self.colptr.copy()), shape=(self.n, self.n))
        assert P.has_sorted_indices
        return P

    def lists(self):
        """(column_indices, row_indices) as klchol.sparse_approximate_cholesky_supernodal and the oracle take them"""
        return [list(c) for _, c in self.tasks], [list(r) for r, _ in self.tasks]

    def column(self, nzval, c):
        return nzval[self.colptr[c]:self.colptr[c + 1]]

    def read_mask(self):
        """the entries of Theta the contract lets a task read: (R[i], R[j]) for local i >= j, i.e. row <= column"""
        A = np.zeros((self.n, self.n), dtype=bool)
        for rows, _ in self.tasks:
            A[np.ix_(rows, rows)] = True
        return np.triu(A)

    # ---- derived sets -----------------------------------------------------------------------------------------------------
    def subset(self, idx):
        return TaskSet(self.n, [self.tasks[t] for t in idx], self.name + "[subset]")

    def per_column(self):
        """one task per column 0..n-1 in column order, as sparse_approximate_cholesky! builds them (task_rowptr == L_colptr):
        this set's tasks (one member column each, the last of its rows) plus a 1-row task for every other column"""
        by_col = {}
        for rows, cols in self.tasks:
            assert len(cols) == 1 and cols[0] == rows[-1]
            by_col[cols[0]] = (rows, cols)
        return TaskSet(self.n, [by_col.get(c, ([c], [c])) for c in range(self.n)], self.name + "[per column]")

    # ---- the call ---------------------------------------------------------------------------------------------------------
    def run(self, theta, ldt, base=0, reg=REG_COLUMN, alias=False, device=-1):
        """gmrfx_kl_cholesky called directly. theta: a host array whose memory is column-major with leading dimension ldt, or an
        int = device pointer. alias: pass ONE array as L_colptr and task_rowptr (the Julia plug-in's call). -> (code, info, nzval)"""
        from gmrfx import _lib
        colptr, rowptr, rows, tcolptr, cols = self.arrays(base)
        if alias:
            assert (colptr == rowptr).all()
            rowptr = colptr
        on_dev = isinstance(theta, int)
        th = C.c_void_p(theta) if on_dev else C.c_void_p(theta.ctypes.data)
        nz = np.full(int(self.colptr[-1]), np.nan)
        info = C.c_int64(-99)
        code = _lib.lib().gmrfx_kl_cholesky(self.n, th, int(ldt), int(on_dev), _lib.ptr(colptr), len(self.tasks), _lib.ptr(rowptr),
                                            _lib.ptr(rows), _lib.ptr(tcolptr), _lib.ptr(cols), base, float(reg), device,
                                            _lib.ptr(nz), C.byref(info))
        return code, int(info.value), nz


def make_task(rng, n, N, nks, taken, low=0):
    """N distinct indices of [low, n), descending, whose positions nk - 1 (nk in nks) hold indices not in `taken`"""
    assert all(1 <= k <= N for k in nks) and len(set(nks)) == len(nks)
    for _ in range(1000):
        rows = np.sort(rng.choice(np.arange(low, n), size=N, replace=False))[::-1].tolist()
        cols = [rows[k - 1] for k in nks]
        if not taken.intersection(cols):
            taken.update(cols)
            return rows, cols
    raise RuntimeError("no free member columns")


def one_column_task(rng, N, col, pool):
    """a one-column task of N rows (N_k = N): N - 1 random indices of `pool` above `col` and, last, its member column `col`"""
    pool = np.asarray(pool)
    rows = np.sort(rng.choice(pool[pool > col], size=N - 1, replace=False))[::-1].tolist() + [col]
    return rows, [col]


EDGE_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 320, 511, 512)


def edge_set(n=N_THETA, seed=1):
    """one one-column task per size-class edge; task i fills column i, its other rows lie in [17, n): Theta[i, :] is read by
    task i alone"""
    rng = np.random.default_rng(seed)
    pool = np.arange(len(EDGE_SIZES), n)
    return TaskSet(n, [one_column_task(rng, N, i, pool) for i, N in enumerate(EDGE_SIZES)], "edges")


# N -> the N_k of its member columns; 1, 3, 4, 5, 9 and 17 member columns
SUPERNODES = (
    (32, (1, 2, 31, 32)),
    (64, (1, 63, 64)),
    (65, (2, 33, 63, 64, 65)),
    (128, (64,)),
    (129, (1, 2, 3, 64, 65, 100, 127, 128, 129)),
    (200, (1, 2, 63, 64, 65, 100, 127, 128, 129, 150, 190, 191, 192, 193, 198, 199, 200)),
    (512, (1, 64, 65, 128, 129, 192, 193, 511, 512)),
)


def supernodal_set(n=N_THETA, seed=2):
    """tasks in every size class with several member columns; the member columns are listed in a shuffled order, so the
    wave that takes a column and the column's N_k are unrelated"""
    rng = np.random.default_rng(seed)
    taken, tasks = set(), []
    for N, nks in SUPERNODES:
        nks = [int(k) for k in rng.permutation(nks)]
        tasks.append(make_task(rng, n, N, nks, taken))
    return TaskSet(n, tasks, "supernodes")


MIXED_TAIL = (65, 100, 128, 5, 32, 17)
_SHARED_LOW = 1 + BIG_CHUNK + 1 + len(MIXED_TAIL)      # 264: the other rows of every task but the 512-row one lie in [264, n)


def chunk_set(n=N_THETA, seed=3):
    """257 one-column tasks of 129 rows, one more than a launch of the big class takes; task t fills column t + 1 (column 0 and
    columns 258..263 are mixed_set's)"""
    rng = np.random.default_rng(seed)
    pool = np.arange(_SHARED_LOW, n)
    return TaskSet(n, [one_column_task(rng, 129, t + 1, pool) for t in range(BIG_CHUNK + 1)], "chunk")


MIXED_BAD = (256, 258, 261, 263)       # second launch of the big class, <= 128 class, <= 32 class, the 512-row task


def mixed_set(n=N_THETA, seed=3):
    """the 257 tasks of chunk_set (t = 0..256: t = 256 alone in the second launch of the big class), three tasks of the <= 128
    class (t = 257..259), three of the <= 32 class (t = 260..262) and one of 512 rows (t = 263, column 0; second launch too).
    The classes launch in the order <= 32, <= 64, <= 128, big, so the task order is the reverse of the launch order. The member
    columns of the tasks MIXED_BAD are rows of no other task (private_index checks it)."""
    tasks = list(chunk_set(n, seed).tasks)
    rng = np.random.default_rng(seed + 100)
    pool = np.arange(_SHARED_LOW, n)
    tasks += [one_column_task(rng, N, BIG_CHUNK + 2 + i, pool) for i, N in enumerate(MIXED_TAIL)]
    keep_out = [tasks[t][1][0] for t in MIXED_BAD[:3]]
    tasks.append(one_column_task(rng, 512, 0, np.setdiff1d(np.arange(1, n), keep_out)))
    return TaskSet(n, tasks, "mixed")


def private_index(ts, t):
    """the member column of one-column task t, after checking that no other task of ts has it among its rows"""
    rows, cols = ts.tasks[t]
    assert len(cols) == 1 and cols[0] == rows[-1]
    assert all(cols[0] not in r for u, (r, _) in enumerate(ts.tasks) if u != t)
    return cols[0]


class Reference:
    """long-double columns of a task set on one Theta, each local factor computed once (tasks are shared between sets)"""

    def __init__(self, Theta):
        self.Theta = Theta
        self._factor = {}
        self._col = {}

    def factor(self, rows, reg):
        key = (tuple(rows), reg)
        if key not in self._factor:
            self._factor[key] = ref_factor(self.Theta, rows, reg)
        return self._factor[key]

    def columns(self, ts, reg):
        """{member column: long-double values in storage order}"""
        out = {}
        for rows, cols in ts.tasks:
            for c in cols:
                key = (tuple(rows), reg, ts.nk[c])
                if key not in self._col:
                    self._col[key] = ref_longdouble(self.Theta, rows, ts.nk[c], reg, self.factor(rows, reg))
                out[c] = self._col[key]
        return out


def column_ratio(x, x_ld):
    """max_i |x_i - x_ld_i| / max_i |x_ld_i|, in long double"""
    x_ld = np.asarray(x_ld, dtype=np.longdouble)
    return float(np.abs(np.asarray(x, dtype=np.longdouble) - x_ld).max() / np.abs(x_ld).max())
