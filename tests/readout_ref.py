"""What the read-out kernels compute -- the kernels that turn a factor or a selected inverse into the numbers the user reads -- restated
in plain numpy, generic in its dtype: np.longdouble is the reference of tests/test_gpu_readout_edges.py (eps_ld = 2^-63, negligible
beside the bounds), np.float64 with numpy's own summation order is the CONTROL of tests/test_readout_edges_host.py. No device.

    k_logdet_partial / k_logdet_final (csrc/util_kernels.hip)      log det Q = 2 sum_k log L_kk
    k_batch_diag_partial / k_batch_diag_final (csrc/batch.hip)     the same per member + the first column with !(L_kk > 0)
    k_quadform / k_quadform_final (csrc/quadform.hip), k_batch_quadform[_final] (csrc/batch.hip)
                                                                   q = sum_j r_j sum_i w_ij Q_ij r_i,  r = x - mu
    k_gather, k_gather_diag (csrc/util_kernels.hip)                copies: exact, no restatement
    k_seg_wsum, k_seg_wsum_pairs (csrc/util_kernels.hip)           tr(Sigma B), diag(A Sigma A')
    k_dense_apply, k_transpose (csrc/dense.hip)                    R = D T, dst = src'

Each restatement is FED the handle's own inputs (the diagonal of factor_values(), the Sigma entries of selinv_extract_at of the same
handle), so that the factorisation's and the selected inversion's errors, which have their own suites, do not blur these bounds.

BOUNDS: first order, per output, (depth of the addition chain + roundings per term) eps (sum of the absolute terms), eps = 2^-52,
times F = 16, the project's factor over a first-order bound (tests/constraint_ref.py, tests/fisher_ref.py); F = 1 in the control.
The chains, read off the kernels:
  log det   a thread of k_logdet_partial adds log L_kk for k = k0 + tid, + 256, .. < k1 of its block of per = ceil(n / nparts)
            columns, nparts = min(1024, max(1, ceil(n / 256))): ceil(per / 256) additions; 256 thread sums meet in an 8-level LDS
            tree; a thread of k_logdet_final adds part[tid], part[tid + 256], ..: ceil(nparts / 256) additions, and 8 more levels.
            The doubling is exact. The device log of a double is documented to 1 ulp: one more eps per term.
                d = ceil(per / 256) + 8 + ceil(nparts / 256) + 8 + 1,      |d logdet| <= F d eps 2 sum_k |log L_kk|
  batched   k_batch_diag_partial: BD_COLS = 1024 columns per part, a thread adds its 4 (columns past the member read 1.0, log 1 = 0
            exactly), 8 levels; k_batch_diag_final: ceil(parts / 256) additions, 8 levels:
                d = 4 + 8 + ceil(parts / 256) + 8 + 1.      info = 1 + the first member column with !(L_kk > 0), 0 if none: exact
  quadratic form   lane l of a 16-lane group adds entries p0 + l, p0 + l + 16, .. of column j: ceil(len_j / 16) additions; the
            column's lane sum times r_j is added to the THREAD's accumulator over the 8 columns t * 16 + g of the group (8
            additions; the 16 lane sums of a column are NOT combined before the tree: they sit in 16 threads); the 256 threads meet
            in an 8-level tree; k_quadform_final: ceil(nblk / 256) additions and 8 levels, nblk = ceil(n / 128). Per term the
            roundings of x_i - mu_i, x_j - mu_j and of the two products (w_ij is 0, 1 or 2: exact):
                d = ceil(max_j len_j / 16) + 8 + 8 + ceil(nblk / 256) + 8 + 4,      |dq| <= F d eps sum_j |r_j| sum_i w_ij |Q_ij| |r_i|
            with r rounded once from x and mu: the bound is on ABSOLUTE sums and holds whatever cancels in x - mu or in the sum.
  segment sums   one 64-lane wave per segment: lane l adds entries t0 + l, + 64, ..: ceil(len / 64) additions, then a 6-level
            butterfly. Products: w_t Sigma_t (the mask factor 1.0 / 0.0 is exact): 1 in k_seg_wsum fed B's values (selinv_dot); 2 in the
            one-shot row_diag (the host forms c A_p A_q, the device multiplies by Sigma); 3 in k_seg_wsum_pairs (c A_p, A_q, Sigma;
            the first is a doubling and exact, counted all the same):
                d_g = ceil(len_g / 64) + 6 + products,      |d out_g| <= F d_g eps sum_t |w_t| |Sigma_t|
            selinv_dot: segments are fixed chunks of 4096 entries, their sums are added IN ORDER on the host: nchunks more:
                |d tr| <= F (max_g d_g + nchunks) eps sum_e |B_e| |Sigma_e|
            An entry outside the factor pattern (off < 0) reads src[0] times 0.0: it adds +-0 and changes no bit.
  dense     R_ij = sum_k D_ik T_kj, n1 terms in the MFMA path's order (batches of 8 k through the pair loads, the remainder and, for
            odd n2, the last row of T through the masked path; padded k-steps add exact zeros):
                |dR_ij| <= F (n1 + 2) eps sum_k |D_ik| |T_kj|      covers any order (Higham, Accuracy and Stability, 3.1)
  gathers, transpose   exact.

MUTANTS (mutant=...): named wrong restatements, each one plausible kernel slip; tests/test_readout_edges_host.py checks that each
exceeds these bounds with F = 16 on the case of tests/readout_edges.py that names it.

The constants restate csrc/quadform.hip, csrc/batch.hip, csrc/util_kernels.hip, csrc/device.cpp, csrc/api_selinv.cpp and
csrc/dense.hip; the host test checks them against the source."""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -52
LD = np.longdouble
FACTOR = 16
THREADS = 256                   # every reduction kernel's workgroup
LOGDET_MAXPARTS = 1024
QF_COLS, QF_LANES = 128, 16
BD_COLS = 1024
SEG_LANES, DOT_CHUNK = 64, 4096
TILE, XCDS = 64, 8
NVEC_MAX = 65535

LOGDET_MUTANTS = ("skip_col_262144", "last_block_twice")
QUAD_MUTANTS = ("offdiag_weight1_from_col128", "drop_17th_entry", "other_triangle", "mu_ignored_at_row", "skip_block_257")
SEG_MUTANTS = ("drop_elem_64", "masked_counts_sigma0", "pair_weight1", "drop_chunk_2")
DENSE_MUTANTS = ("drop_last_k_odd_n2", "swap_pair", "transpose_clamp")
MUTANTS = LOGDET_MUTANTS + QUAD_MUTANTS + SEG_MUTANTS + DENSE_MUTANTS


def cdiv(a, b):
    return -(-int(a) // int(b))


def ratio(got, ref, bound):
    """the largest error / bound over the entries (0 / 0 counts as 0); inf where `got` is not finite"""
    got = np.asarray(got)
    err = np.abs(np.asarray(got, LD) - np.asarray(ref, LD))
    bound = np.broadcast_to(np.asarray(bound, LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0, err / bound)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.max(q)) if q.size else 0.0


# ---- log det -----------------------------------------------------------------------------------------------------------------------------
def logdet_launch(n):
    """(nparts, per) of Device::enqueue_logdet and k_logdet_partial"""
    nparts = min(LOGDET_MAXPARTS, max(1, cdiv(n, THREADS)))
    return nparts, cdiv(n, nparts)


def logdet_blocks(n):
    """(k0, k1) per block: k1 < k0 in a block past the end"""
    nparts, per = logdet_launch(n)
    k0 = np.arange(nparts, dtype=np.int64) * per
    return k0, np.minimum(n, k0 + per)


def logdet_depth(n):
    nparts, per = logdet_launch(n)
    return cdiv(per, THREADS) + 8 + cdiv(nparts, THREADS) + 8 + 1


def logdet(diag, dtype=LD, mutant=None):
    """2 sum log L_kk through the block sums; {"value", "abs", "depth"}"""
    lg = np.log(np.asarray(diag, dtype))
    n = len(lg)
    if mutant == "skip_col_262144" and n > 262144:
        lg = lg.copy()
        lg[262144] = 0                                              # the second pass of a thread stops at k < 262144
    k0, k1 = logdet_blocks(n)
    part = np.array([lg[a:b].sum() for a, b in zip(k0, k1)], dtype)  # lg[a:b] is empty for b <= a
    if mutant == "last_block_twice":
        last = int(np.flatnonzero(k1 > k0)[-1])
        part[last] = 2 * part[last]                                 # a block past the end re-reads the last one
    return {"value": 2 * part.sum(), "abs": 2 * np.abs(lg).sum(), "depth": logdet_depth(n)}


def batch_parts(nm):
    return cdiv(nm, BD_COLS)


def batch_logdet(diag, dtype=LD):
    """one member: its nm diagonal entries in the member's elimination order"""
    lg = np.log(np.asarray(diag, dtype))
    nm, parts = len(lg), batch_parts(len(lg))
    part = np.array([lg[p * BD_COLS:(p + 1) * BD_COLS].sum() for p in range(parts)], dtype)
    return {"value": 2 * part.sum(), "abs": 2 * np.abs(lg).sum(), "depth": BD_COLS // THREADS + 8 + cdiv(parts, THREADS) + 8 + 1}


def batch_info(diag):
    bad = np.flatnonzero(~(np.asarray(diag, np.float64) > 0))
    return int(bad[0]) + 1 if len(bad) else 0


def bound_sum(r, factor=FACTOR):
    """the bound of a restated scalar or vector of sums: F depth eps (absolute sum)"""
    return factor * EPS * np.asarray(r["depth"], LD) * np.asarray(r["abs"], LD)


# ---- quadratic form ------------------------------------------------------------------------------------------------------------------------
def quadform_blocks(n):
    return cdiv(n, QF_COLS)


def quadform(colptr, row, val, X, mu, use_lower, dtype=LD, mutant=None):
    """q_v for the columns of X (n x nvec) on the stored pattern (colptr, row, val); {"value", "abs", "depth"} (nvec each)"""
    colptr, row = np.asarray(colptr, np.int64), np.asarray(row, np.int64)
    n = len(colptr) - 1
    lens = np.diff(colptr)
    col = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos = np.arange(len(row), dtype=np.int64) - np.repeat(colptr[:-1], lens)
    X = np.asarray(X, dtype).reshape(n, -1)
    R = X if mu is None else X - np.asarray(mu, dtype).reshape(n, 1)
    tri = (row > col) if use_lower else (row < col)
    w = np.where(row == col, 1.0, np.where(tri, 2.0, 0.0))
    if mutant == "offdiag_weight1_from_col128":
        w = np.where((col >= QF_COLS) & (row != col) & tri, 1.0, w)   # the weight formed once per workgroup, from its first one
    if mutant == "drop_17th_entry":
        w = np.where(pos == QF_LANES, 0.0, w)                       # a lane's second pass does not run
    if mutant == "other_triangle":
        w = np.where(row == col, 1.0, 2.0)
    wv = np.asarray(w, dtype) * np.asarray(val, dtype)
    Ri = (X if mutant == "mu_ignored_at_row" else R)[row]
    a, aa = np.zeros(R.shape, dtype), np.zeros(R.shape, dtype)
    np.add.at(a, col, wv[:, None] * Ri)
    np.add.at(aa, col, np.abs(wv)[:, None] * np.abs(R[row]))
    c = a * R
    nblk = quadform_blocks(n)
    blk = np.array([c[b * QF_COLS:(b + 1) * QF_COLS].sum(axis=0) for b in range(nblk)], dtype).reshape(nblk, -1)
    if mutant == "skip_block_257" and nblk > THREADS:
        blk[THREADS] = 0                                            # the strided loop of the final kernel runs once
    depth = cdiv(lens.max() if n else 0, QF_LANES) + 8 + 8 + cdiv(nblk, THREADS) + 8 + 4
    return {"value": blk.sum(axis=0), "abs": (aa * np.abs(R)).sum(axis=0), "depth": depth}


# ---- segment sums over the selected inverse ------------------------------------------------------------------------------------------------
def seg_wsum(w, sig, inpat, segptr, dtype=LD, products=1, mutant=None, sigma0=0.0):
    """out[g] = sum_{t in segment g} w_t Sigma_t [t in the factor pattern]; sigma0: the first word of the panels, what a masked
    entry's clamped read returns"""
    w, sig, inpat = np.asarray(w, dtype), np.asarray(sig, dtype), np.asarray(inpat, bool)
    fill = dtype(sigma0) if mutant == "masked_counts_sigma0" else dtype(0)
    term = w * np.where(inpat, sig, fill)
    nseg = len(segptr) - 1
    out, ab, depth = np.zeros(nseg, dtype), np.zeros(nseg, dtype), np.zeros(nseg, np.int64)
    for g in range(nseg):
        t = term[int(segptr[g]):int(segptr[g + 1])]
        depth[g] = cdiv(len(t), SEG_LANES) + 6 + products
        if mutant == "drop_elem_64" and len(t) > SEG_LANES:
            t = np.delete(t, SEG_LANES)                              # lane 0 never starts its second pass
        out[g], ab[g] = t.sum(), np.abs(t).sum()
    return {"value": out, "abs": ab, "depth": depth}


def dot_chunks(nz):
    """segment pointer of gmrfx_selinv_dot: fixed chunks of 4096 entries"""
    nseg = cdiv(nz, DOT_CHUNK)
    return np.minimum(np.arange(nseg + 1, dtype=np.int64) * DOT_CHUNK, nz)


def selinv_dot(bval, sig, inpat, dtype=LD, mutant=None, sigma0=0.0):
    """tr(Sigma B) = sum_e B_e Sigma_e over B's stored entries in CSC order: chunk sums, added in order"""
    seg = dot_chunks(len(bval))
    r = seg_wsum(bval, sig, inpat, seg, dtype, 1, mutant, sigma0)
    acc = dtype(0)
    for g, v in enumerate(r["value"]):
        if mutant == "drop_chunk_2" and g == 2:
            continue
        acc = acc + v
    nseg = len(seg) - 1
    return {"value": acc, "abs": r["abs"].sum() if nseg else dtype(0), "depth": (int(r["depth"].max()) if nseg else 0) + nseg}


def csr(A):
    A = sp.csr_matrix(A, dtype=np.float64, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    return A


def row_pairs(A):
    """(segptr, p, q) of plan_row_pairs: the pairs (p, q <= p) of the stored entries of every row, p outer, q inner"""
    seg, pi, qi = [0], [], []
    for i in range(A.shape[0]):
        p0, k = int(A.indptr[i]), int(A.indptr[i + 1] - A.indptr[i])
        P, Q = np.tril_indices(k)
        pi.append(p0 + P)
        qi.append(p0 + Q)
        seg.append(seg[-1] + k * (k + 1) // 2)
    cat = (lambda v: np.concatenate(v).astype(np.int64)) if pi else (lambda v: np.zeros(0, np.int64))
    return np.array(seg, np.int64), cat(pi), cat(qi)


def row_diag(A, Sig, inpat, dtype=LD, products=3, mutant=None, sigma0=0.0):
    """diag(A Sigma A') per row; Sig, inpat: dense n x n, Sigma's entries and the factor pattern (both triangles)"""
    A = csr(A)
    seg, pi, qi = row_pairs(A)
    v = np.asarray(A.data, dtype)
    c = np.where(pi == qi, 1.0, 1.0 if mutant == "pair_weight1" else 2.0)
    jp, jq = A.indices[pi], A.indices[qi]
    return seg_wsum(np.asarray(c, dtype) * v[pi] * v[qi], np.asarray(Sig)[jp, jq], np.asarray(inpat)[jp, jq], seg, dtype, products,
                    mutant, sigma0)


# ---- dense operator -----------------------------------------------------------------------------------------------------------------------
def dense_tiles(n1, n2):
    """(mt, nt, workgroups launched, workgroups that return at once) of launch_dense_apply"""
    mt, nt = cdiv(n1, TILE), cdiv(n2, TILE)
    launched = cdiv(nt, XCDS) * mt * XCDS
    return mt, nt, launched, launched - mt * nt


def dense_k_split(n1, n2):
    """(k done by the pair path, k left to the masked path) of k_dense_apply"""
    qpair = n1 - 1 if n2 % 2 else n1
    qd = 8 * (qpair // 8)
    return qd, n1 - qd


def dense_apply(D, T, dtype=LD, mutant=None):
    D, T = np.asarray(D, dtype), np.asarray(T, dtype)
    n1, n2 = T.shape
    if mutant == "drop_last_k_odd_n2" and n2 % 2:
        R = D[:, :n1 - 1] @ T[:n1 - 1]                               # the masked path starts at qd but stops at qpair
    else:
        R = D @ T
    if mutant == "swap_pair":
        R = R.copy()
        ev = np.arange(0, n2 - 1, 2)
        R[:, ev], R[:, ev + 1] = R[:, ev + 1].copy(), R[:, ev].copy()
    return {"value": R, "abs": np.abs(D) @ np.abs(T), "depth": n1 + 2}


def transpose(src, mutant=None):
    src = np.asarray(src)
    dst = np.ascontiguousarray(src.T)
    rows, cols = src.shape
    if mutant == "transpose_clamp" and cols % TILE:
        # the store's `j < cols` replaced by a clamp of j, with the tile filled by unclamped reads (element (i, j >= cols) of a
        # row-major array is the next row's): row cols - 1 of dst is overwritten by what the last tile column read
        flat = src.reshape(-1)
        j = cdiv(cols, TILE) * TILE - 1
        dst[cols - 1] = flat[np.minimum(np.arange(rows) * cols + j, flat.size - 1)]
    return dst
