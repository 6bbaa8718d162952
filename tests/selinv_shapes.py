"""Precision matrices whose fronts have PRESCRIBED (columns c, trailing rows m), the dense reference inverse and the
entrywise error measure of the selected-inversion shape tests (test_selinv_shapes_host.py on symbolic-only handles,
test_gpu_selinv_shapes.py on the device).

A matrix is a tree of dense blocks under ordering="natural", relax_cols=1, relax_zeros=1e-9. A node is
(c, m[, where[, kids]]): a dense c x c block coupled densely to m scattered rows of its PARENT's front, kids its own
children, laid out before it. The last block is the root (m = 0). where says which rows of the parent's front:
  "cols"  : all m among the parent's own columns (k_sel_gather reads the parent's Z panel only),
  "trail" : ONE row in the parent's columns -- the first trailing row of a front always is a column of its parent, that is
            what makes it the parent -- and m - 1 among the parent's trailing rows (the parent's trailing block),
  "both"  : (default) half and half where the parent has the rows for it, scattered,
  "first" : the parent's FIRST m columns: such a child is the one that ends right before its parent (the amalgamation's only
            candidate), a "sacrificial" child that the case lists make too sparse to be absorbed.
Children of one node never touch each other. The library postorders and amalgamates, so nothing here trusts positions:
fronts_of() finds every block's front in be.symbolic() by its SET of columns and reports (c, m, level); a block that was
split or absorbed is reported as None.

Two rules of csrc/symbolic.cpp decide whether a block stays whole: a trailing set's first row lies within the first 120
columns of its parent (a run of >= 128 columns that ends at a column with two etree children starts a new supernode
there: _subset sees to it), and the block right before its parent is absorbed when the merge adds <= 2 % zeros or gives
<= 4 columns (absorbed() restates it; the case lists avoid it with a "sacrificial" last child or a parent chosen for it).

Values: off-diagonal entries are multiples of 2^-10 in [-1, 1], the diagonal is the row's absolute sum + 1 (strictly
diagonally dominant, cond(Q) of order 10 and below). The coarse grid is what makes the large-n reference affordable:
with Q = D + A the residual I - Q X is evaluated EXACTLY from float64 BLAS products of A with 24-bit slices of X
(every partial sum is an integer multiple of the slice's unit below 2^53) and summed in extended precision."""
import numpy as np
import scipy.sparse as sp

KW = {"ordering": "natural", "relax_cols": 1, "relax_zeros": 1e-9}


def _subset(rng, size, k):
    """k scattered indices of range(size), sorted, the first one below 120 (see the module docstring) and, where the
    parent has more than one column, not 0: the etree postorder puts the child that reaches its parent's FIRST column
    right before the parent, and that place is kept for where="first" nodes."""
    lo = 1 if size > k else 0
    sub = lo + np.sort(rng.choice(size - lo, k, replace=False))
    if k and sub[0] >= 120:
        sub[0] = rng.integers(lo, 120)
    return sub


def absorbed(cd, md, cp, mp):
    """Would the amalgamation merge a (cd, md) front into its (cp, mp) parent if it ends right before it (and is not a
    wide child among siblings)? symbolic.cpp's rule at relax_cols = 1, relax_zeros = 1e-9."""
    c, r = cd + cp, cd + cp + mp
    total = r * c - c * (c - 1) // 2
    nnz = cd * (cd + md) - cd * (cd - 1) // 2 + cp * (cp + mp) - cp * (cp - 1) // 2
    return c <= 4 or (total - nnz) / total <= 0.02


def _node(spec):
    c, m = spec[0], spec[1]
    where = spec[2] if len(spec) > 2 and spec[2] else "both"
    return c, m, where, list(spec[3]) if len(spec) > 3 else []


def _size(spec):
    return spec[0] + sum(_size(k) for k in _node(spec)[3])


def build(root, children, seed=0):
    """-> (Q csc, blocks): blocks[name] = (first column in the ORIGINAL numbering, c, m, parent's name); names "root",
    its children "0", "1", .., their children "0.0", "0.1", ... and so on."""
    rng = np.random.default_rng(seed)
    n = root + sum(_size(ch) for ch in children)
    A = np.zeros((n, n))
    blocks = {}

    def val(*shape):            # never 0: a zero would be a hole in the pattern
        v = np.round(rng.uniform(-1, 1, shape) * 1024.0) / 1024.0
        v[v == 0.0] = 2.0 ** -10
        return v


    def place(name, spec, at, pcols, ptrail):
        c, m, where, kids = _node(spec)
        c0 = at + sum(_size(k) for k in kids)
        cols = np.arange(c0, c0 + c)
        if where == "cols":
            k = m
        elif where == "trail":
            k = min(m, 1)
        else:
            k = min(max((m + 1) // 2, m - len(ptrail), min(m, 1)), len(pcols))
        head = pcols[:m] if where == "first" else pcols[_subset(rng, len(pcols), k)]
        rows = np.concatenate([head, np.sort(rng.choice(ptrail, m - len(head), replace=False))]).astype(np.int64)
        for j, kid in enumerate(kids):
            place(f"{name}.{j}", kid, at, cols, rows)
            at += _size(kid)
        A[c0:c0 + c, c0:c0 + c] = val(c, c)
        A[np.ix_(rows, cols)] = val(m, c)
        blocks[name] = (c0, c, m, name.rpartition(".")[0] or "root")

    r0 = n - root
    A[r0:, r0:] = val(root, root)
    blocks["root"] = (r0, root, 0, None)
    at = 0
    for i, ch in enumerate(children):
        place(str(i), ch, at, np.arange(r0, n), np.zeros(0, np.int64))
        at += _size(ch)
    assert at == r0
    A = np.tril(A, -1)
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + 1.0
    return _csc(A), blocks


def _csc(A):
    Q = sp.csc_matrix(A)
    Q.sort_indices()
    Q.indices = Q.indices.astype(np.int64)
    Q.indptr = Q.indptr.astype(np.int64)
    return Q


def block_diag(parts):
    """Several build() results side by side (independent trees): blocks renamed "<k>:<name>"."""
    Q = _csc(sp.block_diag([q for q, _ in parts], format="csc"))
    blocks, at = {}, 0
    for k, (q, bl) in enumerate(parts):
        blocks.update({f"{k}:{name}": (b0 + at, cnt, m, par and f"{k}:{par}") for name, (b0, cnt, m, par) in bl.items()})
        at += q.shape[0]
    return Q, blocks


def with_values(Q, seed):
    """The same pattern with other values of the same kind (batched members)."""
    rng = np.random.default_rng(seed)
    A = sp.tril(Q, -1).tocoo()
    v = np.round(rng.uniform(-1, 1, A.nnz) * 1024.0) / 1024.0
    v[v == 0.0] = 2.0 ** -10
    L = sp.coo_matrix((v, (A.row, A.col)), shape=Q.shape)
    M = (L + L.T).tocsc()
    Q2 = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 1.0)).tocsc()
    Q2.sort_indices()
    assert np.array_equal(Q2.indptr, Q.indptr) and np.array_equal(Q2.indices, Q.indices)
    return Q2


def fronts_of(be, blocks):
    """{name: (c, m, level, s)} of every block that is exactly one front of be.symbolic(), None for the others."""
    sym = be.symbolic()
    perm = be.ordering_permutation()
    sf = sym.super_first
    first_of = {int(perm[sf[s]:sf[s + 1]].min()): s for s in range(len(sf) - 1)}
    out = {}
    for name, (b0, cnt, _, _) in blocks.items():
        s = first_of.get(b0)
        out[name] = None
        if s is not None:
            cols = np.sort(perm[sf[s]:sf[s + 1]])
            if len(cols) == cnt and cols[-1] == b0 + cnt - 1:
                out[name] = (cnt, int(sym.row_ptr[s + 1] - sym.row_ptr[s]) - cnt, int(sym.level[s]), s)
    return out


def check_shapes(be, blocks):
    """Every block is one front with exactly the (c, m) it was built for, one level below its parent's, and the matrix has
    no other front. -> {name: (c, m, level, s)}"""
    got = fronts_of(be, blocks)
    for name, (_, c, m, par) in blocks.items():
        assert got[name] is not None and got[name][:2] == (c, m), f"block {name}: wanted a front (c={c}, m={m}), got {got[name]}"
    for name, (_, c, m, par) in blocks.items():
        assert par is None or got[name][2] == got[par][2] - 1, f"block {name}: level {got[name][2]} under a parent on level {got[par][2]}"
    assert len(be.symbolic().level) == len(blocks)
    return got


def level_shapes(be):
    """[(level, c, m)] of ALL fronts: what the launch geometry of a level is computed from."""
    sym = be.symbolic()
    c = np.diff(sym.super_first)
    m = np.diff(sym.row_ptr) - c
    return [(int(l), int(a), int(b)) for l, a, b in zip(sym.level, c, m)]


def dense_class(c, m):
    """The k_sel_dense code class of a front (csrc/selinv.hip): (c mod 4, m mod 4, c > 64, m < 8) -- 64 classes; m = 0
    (phases 0 and 1 return) is the m mod 4 = 0 member of m < 8."""
    return (c % 4, m % 4, c > 64, m < 8)


def is_small(c, m, small_rows):
    """Symbolic's `cls` lambda: the fused one-block path takes fronts of <= 64 columns and <= min(128, small_rows) rows."""
    return c <= 64 and c + m <= min(128, small_rows)


# ---- reference -------------------------------------------------------------------------------------------------------

def _exact_residual(Q, X, dX=None):
    """I - Q (X + dX) in extended precision, the products with X exact (module docstring). Q dense float64."""
    n = Q.shape[0]
    d = np.diag(Q).copy()
    A = Q - np.diag(d)
    assert np.array_equal(A * 1024.0, np.round(A * 1024.0)) and np.abs(A).max() <= 1.0 and n <= 8192
    R = -(d.astype(np.longdouble)[:, None] * X.astype(np.longdouble))
    R[np.diag_indices(n)] += 1.0
    unit = 2.0 ** np.ceil(np.log2(np.abs(X).max(axis=0)))
    rem = X.copy()
    for p in (1, 2, 3):
        g = unit * 2.0 ** (-24 * p)
        piece = np.round(rem / g) * g
        rem -= piece
        R -= A @ piece
    assert np.abs(rem / unit).max() <= 2.0 ** -72
    if dX is not None:
        R -= d.astype(np.longdouble)[:, None] * dX.astype(np.longdouble) + (A @ dX)
    return R


def reference_inverse(Q):
    """-> (X, dX, res): Sigma = X + dX with X float64 and dX the (tiny) Newton correction X (I - Q X), kept apart so that
    nothing is lost to float64; res = max |I - Q (X + dX)|.
    n <= 600: LAPACK's inverse and one Newton step in np.longdouble throughout. Larger: LAPACK's inverse and the same step
    with the residual evaluated exactly through float64 BLAS (_exact_residual)."""
    Qd = Q.toarray() if sp.issparse(Q) else np.asarray(Q)
    n = Qd.shape[0]
    X = np.linalg.inv(Qd)
    X = 0.5 * (X + X.T)
    if n <= 600:
        Ql, Xl = Qd.astype(np.longdouble), X.astype(np.longdouble)
        R = -(Ql @ Xl)
        R[np.diag_indices(n)] += 1.0
        dXl = Xl @ R
        dX = np.asarray(dXl, dtype=np.float64)
        R2 = R - Ql @ dXl
        return X, dX, float(np.abs(R2).max())
    R = _exact_residual(Qd, X)
    dX = X @ np.asarray(R, dtype=np.float64)
    return X, dX, float(np.abs(_exact_residual(Qd, X, dX)).max())


def entry_errors(Z, X, dX):
    """err[k] = |Z[i,j] - Sigma[i,j]| / sqrt(Sigma[i,i] Sigma[j,j]) for every STORED entry k of the sparse Z (coo order)."""
    coo = Z.tocoo()
    sd = np.sqrt(np.diag(X))
    e = np.abs((coo.data - X[coo.row, coo.col]) - dX[coo.row, coo.col]) / (sd[coo.row] * sd[coo.col])
    return coo.row, coo.col, e


def per_front_errors(be, Z, X, dX):
    """[(err, s, c, m, level, i_in_front, j_in_front)] per front, worst entry of each: the entries of front s are the stored
    (row, column) pairs whose column (in elimination order) is one of its columns."""
    sym = be.symbolic()
    perm = be.ordering_permutation()
    n = len(perm)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    row, col, e = entry_errors(Z, X, dX)
    pr, pc = inv[row], inv[col]
    lo = pr >= pc                                   # lower triangle in elimination order: panel entries
    col2s = np.repeat(np.arange(len(sym.super_first) - 1), np.diff(sym.super_first))
    s_of = col2s[pc[lo]]
    el, prl, pcl = e[lo], pr[lo], pc[lo]
    out = []
    for s in range(len(sym.super_first) - 1):
        k = np.nonzero(s_of == s)[0]
        c = int(sym.super_first[s + 1] - sym.super_first[s])
        rows = sym.rows[sym.row_ptr[s]:sym.row_ptr[s + 1]]
        assert len(k) == c * len(rows) - c * (c - 1) // 2, "get_selinv() must return every stored entry of the front"
        w = k[np.argmax(el[k])]
        out.append((float(el[w]), s, c, len(rows) - c, int(sym.level[s]), int(np.searchsorted(rows, prl[w])), int(pcl[w] - sym.super_first[s])))
    return out


def worst(per_front):
    e = max(per_front)
    return e[0], f"front {e[1]} (c={e[2]}, m={e[3]}, level {e[4]}): entry (row {e[5]}, column {e[6]}) of the front, err {e[0]:.3e}"


# ---- the case lists (shared by the host test, which checks the shapes, and the device test, which checks the numbers) ----
C_LIST = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 66, 67, 95, 127, 128, 129, 130, 131, 191, 257]
M_LIST = [1, 2, 3, 5, 6, 7, 8, 9, 31, 32, 33, 63, 64, 65, 66, 67, 127, 129, 130, 131]       # and m = 0: lone fronts / roots
HELPER, HELPER_ROOT = (20, 260), 360      # a tall front under every chain's root: below it no listed pair is absorbed


def chain_cases():
    """(a): every (c, m) of C_LIST x M_LIST ALONE on its level -- chains root <- helper <- front <- front <- ..., one front
    per level, each front's trailing rows scattered over its parent's columns and trailing rows. The order inside a chain
    is chosen so that no front is absorbed by its parent (absorbed()) and fits its rows; pairs that every listed parent
    would absorb (one to three columns over many rows) sit right under the helper."""
    pairs = [(c, m) for c in C_LIST for m in M_LIST]
    hard = {e for e in pairs if all(e[1] > sum(p) or absorbed(*e, *p) for p in pairs)}
    pool = list(pairs)
    np.random.default_rng(5).shuffle(pool)
    pool = [tuple(int(v) for v in e) for e in pool]
    out = []
    while pool:
        chain, par, cols = [], HELPER, 0
        while cols < 1400:
            ok = [e for e in pool if e[1] <= sum(par) and not absorbed(*e, *par)]
            if not ok:
                break
            e = max(ok, key=lambda e: (e in hard, sum(e))) if not chain else max(ok, key=lambda e: (e[1] > 8, pool.index(e) * -1))
            pool.remove(e)
            chain.append(e)
            par, cols = e, cols + e[0]
        assert chain, pool
        spec = None
        for e in reversed(chain):
            spec = (e[0], e[1], "both", [spec] if spec else [])
        out.append({"name": f"chain{len(out)}", "root": HELPER_ROOT, "children": [(HELPER[0], HELPER[1], "cols", [spec])],
                    "seed": 100 + len(out), "alone": True})
    return out


def lone_cases():
    """(a), m = 0: each c of C_LIST as the only front of its matrix."""
    return [{"name": f"lone{c}", "root": c, "children": [], "seed": c, "alone": True} for c in C_LIST]


def small_path_cases():
    """(a), the fused one-block path: every c in 1..64 at m = 0 (64 lone fronts side by side) and at c + m in
    {63, 64, 65, 127, 128} (siblings under one root; a sparse 40-column child takes the place before the root)."""
    out = [{"name": "small_m0", "parts": [(c, [], 300 + c) for c in range(1, 65)]}]
    for r in (63, 64, 65, 127, 128):
        kids = [(c, r - c, "cols") for c in range(1, 65) if r - c >= 1]
        for h, part in enumerate((kids[:32], kids[32:])):
            out.append({"name": f"small_r{r}_{h}", "root": 140, "children": part + [(40, 3, "first")], "seed": 400 + 2 * r + h})
    return out


SACRIFICE = (40, 3, "first")      # never absorbed by a root of >= 140 columns (absorbed()), and the one child that could be


def mixed_cases():
    """(b): levels that mix fronts. narrow: <= 64 columns only (the level's k_sel_dense runs its one-wave form), small-path
    and dense-path fronts side by side; joined: the same with a 65-column front (the four-wave form for all, the narrow
    ones leave through the early returns); spread: no m = 0, very different m (the grid is sized by the largest)."""
    narrow = [(64, 64, "cols"), (33, 5, "cols"), (31, 67, "cols"), (5, 131, "cols"), (63, 9, "cols"), (2, 127, "cols"), (1, 63, "cols")]
    spread = [(66, 1, "cols"), (70, 131, "cols"), (129, 7, "cols"), (95, 64, "cols"), (67, 2, "cols"), (3, 130, "cols")]
    return [{"name": "mixed_narrow", "root": 150, "children": narrow + [SACRIFICE], "seed": 21},
            {"name": "mixed_joined", "root": 150, "children": narrow + [(65, 1, "cols"), SACRIFICE], "seed": 22},
            {"name": "mixed_spread", "root": 150, "children": spread + [(130, 3, "first")], "seed": 23}]


GATHER_TRAILS = {64: (63, 64), 128: (65, 127, 128), 256: (129,)}      # by the thread count of launch_sel_gather


def gather_cases():
    """(c): grandchildren of 7 columns under a (140, 135) child, their trailing rows all in the child's columns / all but
    the first in the child's trailing rows / both; one matrix per thread count of launch_sel_gather, chosen by the
    level's largest trailing count."""
    out = []
    for nthr, trails in GATHER_TRAILS.items():
        gcs = [(7, t, where) for t in trails for where in ("cols", "trail", "both")]
        assert not any(absorbed(g[0], g[1], 140, 135) for g in gcs)
        out.append({"name": f"gather{nthr}", "root": 200, "children": [(140, 135, "cols", gcs), SACRIFICE], "seed": 30 + nthr})
    return out


INV_C = [127, 129, 255, 257, 511, 513, 1023, 1025, 2047, 2049, 2115]


def inverse_cases():
    """(d): the doubling inverse between and beyond its powers of two: a root of c columns (m = 0) over one child of
    c columns and 33 trailing rows."""
    assert not any(absorbed(c, 33, c, 0) for c in INV_C)
    return [{"name": f"inv{c}", "root": c, "children": [(c, 33, "cols")], "seed": 50 + c, "solves": True} for c in INV_C]


def big_cases():
    """(e): k_sel_z21_big (levels with >= 1024 columns and >= 1024 trailing rows) off its 128-grid, and on it."""
    return [{"name": "z21_offgrid", "root": 1200, "children": [(1027, 1030, "cols"), (1025, 1101, "cols")], "seed": 61},
            {"name": "z21_1024_4100", "root": 4100, "children": [(1024, 4100, "cols"), (1024, 4100, "cols")], "seed": 62}]


def all_cases():
    return chain_cases() + lone_cases() + small_path_cases() + mixed_cases() + gather_cases() + inverse_cases() + big_cases()


def make(case):
    if "parts" in case:
        return block_diag([build(c, kids, seed) for c, kids, seed in case["parts"]])
    return build(case["root"], case["children"], case["seed"])
