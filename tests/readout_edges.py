"""The cases of tests/test_gpu_readout_edges.py: every launch edge of the read-out kernels (log det, quadratic forms, the Sigma
read-outs, the dense operator), each by the smallest input that reaches it. tests/test_readout_edges_host.py checks WITHOUT a device
that every case reaches the edge it names; tests/readout_ref.py has the restatements, the bounds and the mutants.

GROUPS (group -> what the cases pin)
  logdet    chains (tridiagonal, fisher_ref.banded(n, 1)) in the natural order at n = 1, 255, 256, 257, 511, 513: one thread, a block
            short of / exactly / one over 256 columns (n = 257: 2 blocks of 129 and 128), 2 and 3 blocks; each "plain" and "spread"
            (Q = S Q S with S log-uniform over 1e-3 .. 1e3: L_kk = s_k L_kk spreads likewise, sum log cancels and the bound is about
            sum |log|). n = 262144 (plain) and 262145 (spread), default order: per = 256 and the first per = 257, where a thread
            loops. BLOCKS PAST THE END: for n <= 262144, nparts = ceil(n / 256) and per <= 256 give ceil(n / per) >= nparts, so no
            block is ever empty; the edge first exists at n = 262145 (nparts per = 263168: blocks 1021 .. 1023 start past n and run
            with k1 < k0, block 1020 holds 5 columns), which is why no smaller case names it.
  batchdiag members of nm = 1, 1023, 1024, 1025, 2049 columns, B = 1, 3: parts of 1024, 4 columns per thread. nm = 1025 and 2049 with
            B = 3: member 1 with two failing pivots in different parts and threads. (One failing pivot per member, the first and the
            last column, zero and NaN pivots at nm = 401: tests/test_gpu_batch_edges.py::test_pivot_failures, not repeated.)
  quad      chains at n = 1, 15, 16, 17, 127, 128, 129, 257, 32768, 32769 (lane groups of 16 columns, workgroups of 128, nblk = 256
            and 257), nvec = 1, 2, 7, both uplo, plain and batched (B = 3); arrowheads of n = 40 whose hub column (first or last) has
            1, 16, 17, 33 entries. On n = 129: nvec = 65535 at n = 3 and 65536 refused, ldx > n with NaN padding and a base aligned
            to 8 bytes only, mu absent against mu = 0, 1e30 in the unused triangle, explicit stored zeros, x - mu of order 1e-8 |x|,
            refactorize_logpdf_dev against the separate calls.
  sigma     a 12 x 11 grid (5-point, default order) and a chain of n = 70 (default order): B patterns of 0, 1, 63, 64, 65, 4095, 4096,
            4097 and (grid) 8193 stored entries -- Q's pattern first, then further positions, most of them outside the factor pattern,
            signed values, stored zeros, 1e300 at some entries outside the factor pattern; a design matrix with rows of 0, 1, 2, 10,
            11, 16, 33 entries (0, 1, 3, 55, 66, 136, 561 pairs), signed, one more row that repeats a column.
  dense     n1 = 1 .. 9 with n2 = 3 and 66; (31, 63), (32, 64), (33, 65), (63, 1), (64, 2), (65, 511), (64, 512), (65, 513),
            (130, 1025); transposes at the same shapes and (1, 1), (1, 65), (65, 1). Mixed sign and scale; views inside NaN-padded
            buffers.
  seldiag   batched selected-inverse diagonal at nm = 255, 257 (B = 3): members straddle the 256-thread blocks of k_gather_diag.

MEASURED error / bound ratios (largest over the cases of a group; bounds of tests/readout_ref.py).
Control, F = 1 (float64 restatement, numpy's summation order, against long double; tests/test_readout_edges_host.py prints them):
  logdet 0.028   batchdiag 0.0043   quad 0.15 (x near mu: 0.075)   selinv_dot 0.038   row_diag 0.11   dense 0.19
Device, F = 16 (MI355X; tests/test_gpu_readout_edges.py prints them):
  logdet 0.0017   batchdiag 0.0024   quad 0.0028 (x near mu, stored zeros: 0.0022; 65535 vectors and 65538 batched pairs: 0.0044)   selinv_dot 0.0024
  row_diag 0.0058 (kept plan 0.0052, one-shot 0.0058)   dense 0.012   gathers, transpose, every bit-for-bit pin: exact
The handle of the n = 262145 chain took 0.09 s to build and its test 0.02 s; the whole GPU file 5 s (128 tests), no single test above 0.4 s.
"""
import numpy as np
import scipy.sparse as sp

from fisher_ref import banded

LOGDET_CHAINS = (1, 255, 256, 257, 511, 513)
LOGDET_BIG = ((262144, "plain"), (262145, "spread"))
BATCH_NM = (1, 1023, 1024, 1025, 2049)
BATCH_B = (1, 3)
QUAD_N = (1, 15, 16, 17, 127, 128, 129, 257, 32768, 32769)
QUAD_NVEC = (1, 2, 7)
HUB_N, HUB_ENTRIES = 40, (1, 16, 17, 33)
DOT_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193)
ROW_ENTRIES = (0, 1, 2, 10, 11, 16, 33)
ROW_PAIRS = (0, 1, 3, 55, 66, 136, 561)
DENSE_SMALL = tuple((n1, n2) for n2 in (3, 66) for n1 in range(1, 10))
DENSE_EDGE = ((31, 63), (32, 64), (33, 65), (63, 1), (64, 2), (65, 511), (64, 512), (65, 513), (130, 1025))
DENSE_SHAPES = DENSE_SMALL + DENSE_EDGE
TRANSPOSE_SHAPES = DENSE_SHAPES + ((1, 1), (1, 65), (65, 1))
SELDIAG_NM = (255, 257)
HUGE = 1e300


def _csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


# ---- precisions --------------------------------------------------------------------------------------------------------------------------
def chain(n, kind="plain", seed=0):
    """tridiagonal, diagonally dominant; "spread": S Q S with s_k = 2^e_k, e_k uniform in -10 .. 10 (1e-3 .. 1e3, exact scaling)"""
    Q = banded(n, 1, seed=seed)
    if kind == "spread":
        s = sp.diags(2.0 ** np.random.default_rng(5 + n).integers(-10, 11, n).astype(np.float64))
        Q = _csc(s @ Q @ s)
    return _csc(Q)


def chain_factor_diag(Q):
    """diag L of a symmetric tridiagonal Q in the natural order (the host test's stand-in for factor_values())"""
    d, a = Q.diagonal(), (Q.diagonal(1) if Q.shape[0] > 1 else np.zeros(0))
    out = np.empty(len(d))
    piv = d[0]
    out[0] = piv
    for k in range(1, len(d)):
        piv = d[k] - a[k - 1] * a[k - 1] / piv
        out[k] = piv
    return np.sqrt(out)


def arrowhead(k, hub):
    """n = HUB_N nodes; the hub's column has k stored entries (itself and k - 1 neighbours, the nearest indices)"""
    n = HUB_N
    others = [i for i in range(n) if i != hub]
    nb = others[:k - 1] if hub == 0 else others[len(others) - (k - 1):]
    rng = np.random.default_rng(100 * k + hub)
    v = -rng.uniform(0.1, 1.0, len(nb))
    T = sp.coo_matrix((np.r_[v, v], (np.r_[nb, [hub] * len(nb)], np.r_[[hub] * len(nb), nb])), shape=(n, n))
    T = sp.csc_matrix(T, dtype=np.float64)
    d = np.asarray(abs(T).sum(1)).ravel() + rng.uniform(0.5, 1.5, n)
    return _csc(T + sp.diags(d))


def grid(nx=12, ny=11, seed=2):
    """5-point lattice, diagonally dominant"""
    rng = np.random.default_rng(seed)
    idx = np.arange(nx * ny).reshape(nx, ny)
    e = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()]), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()])], axis=1)
    v = -rng.uniform(0.1, 1.0, e.shape[1])
    T = sp.csc_matrix(sp.coo_matrix((np.r_[v, v], (np.r_[e[0], e[1]], np.r_[e[1], e[0]])), shape=(nx * ny, nx * ny)))
    d = np.asarray(abs(T).sum(1)).ravel() + rng.uniform(0.5, 1.5, nx * ny)
    return _csc(T + sp.diags(d))


SIGMA_Q = {"grid": grid, "chain70": lambda: chain(70)}


def member_values(Q, B):
    """(nnz, B): member k has Q's pattern and the values of (1 + k / 4) Q + (k / 2) I: every value differs between the members"""
    col = np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))
    return np.asfortranarray(np.stack([Q.data * (1 + 0.25 * k) + 0.5 * k * (Q.indices == col) for k in range(B)], axis=1))


def failing_columns(nm):
    """two elimination columns of a member whose pivots are made to fail: different parts of 1024, different threads"""
    return {1025: (300, 1024), 2049: (700, 1500)}[nm]


# ---- quadratic-form operands -----------------------------------------------------------------------------------------------------------------
def quad_operands(n, nvec, seed=0):
    """(X, mu): signed, O(1)"""
    rng = np.random.default_rng(9 + 3 * n + nvec + seed)
    return rng.standard_normal((n, nvec)), rng.standard_normal(n)


def unused_triangle(Q, use_lower):
    """positions in Q's value array of the triangle that does NOT define Q"""
    col = np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))
    return np.flatnonzero(Q.indices < col if use_lower else Q.indices > col)


def with_stored_zeros(Q, every=3):
    """Q's values with the off-diagonal pairs (i, j), (i + j) % every == 0, set to an explicit 0.0 (symmetric)"""
    col = np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))
    lo, hi = np.minimum(Q.indices, col), np.maximum(Q.indices, col)
    return np.where((lo != hi) & ((lo + hi) % every == 0), 0.0, Q.data)


# ---- Sigma read-outs ---------------------------------------------------------------------------------------------------------------------
def dense_pattern(S):
    """dense bool array of the STORED positions of a sparse matrix (explicit zeros included)"""
    S = sp.csc_matrix(S)
    out = np.zeros(S.shape, bool)
    out[S.indices, np.repeat(np.arange(S.shape[1]), np.diff(S.indptr))] = True
    return out


def factor_pattern(be):
    """the factor pattern in original indices, both triangles, from the handle's symbolic structure (no numeric state needed)"""
    sy, perm = be.symbolic(), be.ordering_permutation()
    out = np.zeros((len(perm), len(perm)), bool)
    for s in range(len(sy.super_parent)):
        f, l1 = int(sy.super_first[s]), int(sy.super_first[s + 1])
        rows = sy.rows[sy.row_ptr[s]:sy.row_ptr[s + 1]]
        for j in range(l1 - f):
            a, b = perm[rows[j:]], perm[f + j]
            out[a, b] = out[b, a] = True
    return out


def dot_pattern(Q, inpat, cnt, seed=0):
    """B (CSC, n x n) with exactly cnt stored entries: Q's stored positions first (column-major), then further positions drawn at
    random; signed values, every seventh an explicit zero, HUGE at every fifth entry outside the factor pattern `inpat` (dense bool)"""
    n = Q.shape[0]
    rng = np.random.default_rng(40 + cnt + seed)
    C = sp.coo_matrix(Q)
    own = C.col.astype(np.int64) * n + C.row
    rest = np.setdiff1d(np.arange(n * n, dtype=np.int64), own)
    rng.shuffle(rest)
    flat = np.sort(np.concatenate([np.sort(own), rest])[:cnt])
    r, c = flat % n, flat // n
    v = rng.standard_normal(cnt) * 10.0 ** rng.integers(-2, 3, cnt)
    v[np.arange(cnt) % 7 == 6] = 0.0
    out = np.flatnonzero(~inpat[r, c])
    v[out[::5]] = HUGE
    B = sp.csc_matrix((v, (r, c)), shape=(n, n))
    B.sort_indices()
    assert B.nnz == cnt and len(B.data) == cnt
    return B


def design(n, seed=0, scale=1.0):
    """(A with one row per ROW_ENTRIES at random columns plus a row given with a repeated column, as COO triplets so that the
    duplicate survives until the library's wrapper sums it)"""
    rng = np.random.default_rng(60 + n + seed)
    ri, ci, va = [], [], []
    for r, k in enumerate(ROW_ENTRIES):
        cols = np.sort(rng.choice(n, k, replace=False))
        ri += [r] * k
        ci += list(cols)
        va += list(scale * rng.standard_normal(k) * 10.0 ** rng.integers(-1, 2, k))
    r = len(ROW_ENTRIES)
    ri += [r] * 4
    ci += [3, 9, 3, n - 1]                                         # column 3 twice
    va += [0.75, -1.5, 0.5, 2.0]
    return sp.coo_matrix((np.array(va), (np.array(ri), np.array(ci))), shape=(r + 1, n))


def other_designs(n):
    """four more patterns (for the plan cache of four): rows of 3 entries at shifted columns"""
    out = []
    for s in range(4):
        ri = np.repeat(np.arange(5), 3)
        ci = (np.arange(15) * 4 + s) % n
        out.append(sp.csr_matrix((np.linspace(0.5, 1.5, 15), (ri, ci)), shape=(5, n)))
    return out


# ---- dense operator -------------------------------------------------------------------------------------------------------------------------
def dense_operands(n1, n2):
    """(D, T): signed, scales over 1e-2 .. 1e2"""
    rng = np.random.default_rng(1000 * n1 + n2)
    D = rng.standard_normal((n1, n1)) * 10.0 ** rng.integers(-2, 3, (n1, n1))
    T = rng.standard_normal((n1, n2)) * 10.0 ** rng.integers(-2, 3, (n1, n2))
    return D, T


# the case each mutant of readout_ref.MUTANTS must exceed the device bound on
MUTANT_CASE = {"skip_col_262144": ("logdet", 262145, "spread"), "last_block_twice": ("logdet", 257, "plain"),
               "offdiag_weight1_from_col128": ("quad", 257), "drop_17th_entry": ("hub", 17), "other_triangle": ("quad", 17),
               "mu_ignored_at_row": ("quad", 16), "skip_block_257": ("quad", 32769),
               "drop_elem_64": ("dot", "grid", 65), "masked_counts_sigma0": ("dot", "grid", 4097), "pair_weight1": ("rows", "grid"),
               "drop_chunk_2": ("dot", "grid", 8193),
               "drop_last_k_odd_n2": ("dense", 33, 65), "swap_pair": ("dense", 5, 66), "transpose_clamp": ("transpose", 65, 513)}
