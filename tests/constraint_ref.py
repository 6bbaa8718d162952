"""What the linear-constraint kernels compute (csrc/constraint.hip, drivers in csrc/device_constraint.cpp), restated in plain numpy,
generic in its dtype: np.longdouble is the reference of tests/test_gpu_constraint_edges.py (eps_ld = 2^-63, negligible beside the
bounds), np.float64 with numpy's own summation order is the CONTROL of tests/test_constraint_edges_host.py. No device.

The restatement is FED the handle's own A~' = Q^-1 A' (constraint_fields()), its own selinv diagonal and, for samples, its own
backward solve: the sweeps' and the selected inversion's errors have their own tests and do not blur these bounds. From A (CSR,
sorted, m <= 64 rows), e, A~', X, mu, sigma it forms, the way the kernels do (chunk sums of CHUNK entries per row, added in chunk
order; lower triangle of W; explicit L_c^-1):
    W = A A~'    L_c L_c' = W    L_c^-1    log det W = 2 sum_j log L_jj
    R = A X (+ (A mu - e) | - e)    T = L_c^-1 R    B = A~' L_c^-T    X_c = X (+ mu) - B T    var = max(sigma - rowsum(B^2), 0)

BOUNDS (bound_W, bound_logdet, bound_X, bound_var: per entry; eps = 2^-52; F = 16 is the project's factor over a first-order bound, F = 1 in the control).
Summation order of (A X)[r, j] for a row of len_r entries: a thread of k_con_ax_part takes at most CHUNK / 256 = 16 entries of its
chunk by FMA (16 roundings), the 256 thread sums meet in an 8-level tree (8), k_con_ax_final adds the ceil(len_r / CHUNK) chunk sums
in order: d_r = 24 + ceil(len_r / CHUNK) roundings on the longest path, each of a partial sum of |a|'|x| (Higham, Accuracy and
Stability, 3.1).
  W      |dW_rj| <= F d_r eps (|A| |A~'|)_rj.
  L_c^-1 is made from the LOWER triangle of the computed W: by a host loop (plain handle) or one wave (k_batch_con_chol), both the
         textbook column Cholesky and forward substitution. With W + DW = L^ L^', |DW| <= dW + (m + 1) eps |L| |L'| (Higham 10.3,
         || |L| |L'| ||_2 <= m ||W||_2) and the computed inverse X^ = L^-1 (I + E), |E| <= m eps |L| |X^| (Higham 8.5, norm <= m
         sqrt(kappa)), every quantity below that is a form u' (L_c^-T L_c^-1) v = b_u' t_v moves by at most
             kappa g_W ||b_u||_2 ||t_v||_2,    g_W = (d_max c_W + 3 m (m + 1)) eps,    c_W = || |A| |A~'| ||_F / ||W||_2,
         because L' (M^ - M) L = -L^-1 DW L^-T to first order (norm <= ||W^-1|| ||DW|| = kappa ||DW|| / ||W||) and the inverse's
         own error adds kappa m^2 eps on each side. kappa = cond_2(W) of the handle's own W (symmetrised from its lower triangle).
  logdet |d log det W| <= F eps (m kappa (d_max c_W + m (m + 1)) + (m + 2) sum_j |2 log L_jj|): tr(W^-1 DW) <= m ||W^-1|| ||DW||
         for the factor, one rounding of each logarithm, of each doubling and m of the running sum for the sum itself.
  X_c    R_rj carries (d_r + 2) roundings of rbar = |A| |X| (+ |A| |mu|) + |e| (the chunk sums, the mean's own sum, - e), T = L_c^-1 R
         is m FMAs per entry, B = A~' L_c^-T is m FMAs per entry, the product is m FMAs (MFMA k-steps; padded steps add exact
         zeros) after one addition of mu:
             |dX_ij| <= F eps ( (m + 1) S_ij + (|B| |L_c^-1| ((d + 2) rbar + m |R|))_ij + m (H |T|)_ij + kappa (g_W / eps) ||b_i|| ||t_j|| )
         with S = |x| + |mu| + sum_l |B_il| |T_lj| and H = |A~'| |L_c^-T|.
  var    |dvar_i| <= F eps ( (m + 1) (sigma_i + sum_l B_il^2) + 2 m sum_l |B_il| H_il + kappa (g_W / eps) sum_l B_il^2 ), and never
         negative: max(., 0) is exact, so a negative entry is an error whatever its size (ratio() returns inf for it).
  m = 0 with a mean: X + mu, one rounding: F eps (|x| + |mu|).
  residual (the project's existing bound, the row's own length in place of n): |A X_c - e| <= 2 d_r eps (|A| |X_c| + |e|).

MUTANTS (mutant=...): named wrong restatements, each a mistake the kernels could make; tests/test_constraint_edges_host.py checks
that each one exceeds these bounds with F = 16 on the case of tests/constraint_edges.py that names it.

CHUNK, COLTILE, GROUPS restate csrc/kernels.h (kConChunk, kConColTile, kConApplyGroups), COLBATCH restates kConColBatch of
csrc/device_constraint.cpp; the host test checks them against the source."""
import numpy as np
import scipy.sparse as sp

CHUNK, COLTILE, GROUPS, COLBATCH = 4096, 8, 2048, 1024
EPS = 2.0 ** -52
LD = np.longdouble
FACTOR = 16
REDUCTION_MUTANTS = ("drop_lone", "drop_last_chunk", "neighbour_chunks", "clamped_column")
MUTANTS = ("drop_lone", "drop_last_chunk", "neighbour_chunks", "clamped_column", "round_m_to_4", "masked_reads_last", "skip_second_piece",
           "first_member_linv", "no_clamp")


def csr(A):
    A = sp.csr_matrix(A, dtype=np.float64, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    return A


def chunks(A):
    """(entries per row, chunks per row, chunk offsets) as Device::con_rows_upload counts them"""
    lens = np.diff(A.indptr).astype(np.int64)
    nch = -(-lens // CHUNK)
    return lens, nch, np.r_[0, np.cumsum(nch)]


def depth(A):
    """roundings on the longest path of the device's sum over each row of A"""
    lens, nch, _ = chunks(A)
    return 24 + nch


def template(m, with_mean=False):
    """the kernel launch_con_apply picks (None: nothing is launched)"""
    if m <= 0:
        return "vec<0>" if with_mean else None
    if m <= 3:
        return f"vec<{m}>"
    return f"mfma<{[q for q in (1, 2, 4, 8, 16) if m <= 4 * q][0]}>"


def padded_m(m):
    """the k-extent of the product: 4 MQ in the MFMA template, m itself in the vector template"""
    t = template(m)
    return 4 * int(t[5:-1]) if t and t.startswith("mfma") else m


def pieces(nvec):
    """the column pieces of Device::con_correct"""
    return [(j0, min(COLBATCH, nvec - j0)) for j0 in range(0, nvec, COLBATCH)]


def pair_census(A, r, ldx, off, k):
    """how k_con_ax_part fetches row r of A over the k columns of X at X0 + off doubles (X0 16-byte aligned), leading dimension ldx:
    counts of entry pairs fetched by one 16-byte load, by two 8-byte loads, and of lone last entries (per column, summed)"""
    p0, p1 = int(A.indptr[r]), int(A.indptr[r + 1])
    out = {"vec16": 0, "two8": 0, "lone": 0}
    for c0 in range(p0, p1, CHUNK):
        c1 = min(p1, c0 + CHUNK)
        for p in range(c0, c1, 2):
            if p + 1 >= c1:
                out["lone"] += k
                continue
            adj = A.indices[p + 1] == A.indices[p] + 1
            for j in range(k):
                out["vec16" if adj and (off + j * ldx + int(A.indices[p])) % 2 == 0 else "two8"] += 1
    return out


# ---- the m x m part in `dtype` (numpy's linalg does not take long double) --------------------------------------------------------------
def chol_lower(W):
    """L (lower) with L L' = the symmetric matrix whose LOWER triangle is W's"""
    m = W.shape[0]
    L = np.zeros_like(W)
    for j in range(m):
        d = W[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (W[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_inverse(L):
    X = np.zeros_like(L)
    for i in range(L.shape[0]):
        X[i, i] = 1 / L[i, i]
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X


def cond_lower(W):
    """cond_2 of the symmetric matrix whose lower triangle is W's, float64"""
    W = np.tril(np.asarray(W, np.float64))
    if W.shape[0] == 0:
        return 1.0
    ev = np.linalg.eigvalsh(W + np.tril(W, -1).T)
    return float(ev[-1] / ev[0])


# ---- A X the way the two reduction kernels form it --------------------------------------------------------------------------------------
def ax(A, X, dtype, absolute=False, mutant=None):
    """(A X)[r, j] (|A| |X| with absolute) through chunk sums; m x k"""
    m, k = A.shape[0], X.shape[1]
    lens, nch, choff = chunks(A)
    part = np.zeros((int(choff[-1]), k), dtype)
    for r in range(m):
        for c in range(int(nch[r])):
            p0 = int(A.indptr[r]) + c * CHUNK
            p1 = min(int(A.indptr[r + 1]), p0 + CHUNK)
            if mutant == "drop_lone" and (p1 - p0) % 2:
                p1 -= 1                                             # `two` taken for "there is an entry": the lone last one is skipped
            t = np.asarray(A.data[p0:p1], dtype)[:, None] * X[A.indices[p0:p1], :]
            part[choff[r] + c] = (np.abs(t) if absolute else t).sum(axis=0)
    if mutant == "clamped_column" and k % COLTILE:
        # the store's `j0 + tid < k` dropped: column k - 1, re-read for the columns past the edge, lands in part[(q) k + k ...], the
        # first columns of the next chunk sum
        over = min(COLTILE - k % COLTILE, k)
        stored = part.copy()
        for q in range(1, part.shape[0]):
            part[q, :over] = stored[q - 1, k - 1]
    out = np.zeros((m, k), dtype)
    for r in range(m):
        lo, hi = int(choff[r]), int(choff[r + 1])
        if mutant == "drop_last_chunk" and hi - lo > 1:
            hi -= 1                                                 # c < chunks - 1
        if mutant == "neighbour_chunks":
            hi = min(lo + int(nch.max()), part.shape[0])            # the early return's row count taken from the longest row
        out[r] = part[lo:hi].sum(axis=0)
    return out


def prepare(A, e, At, dtype=LD, mutant=None, linv=None):
    """everything that does not depend on X: W, L_c, L_c^-1, log det W, B and the absolute sums of their bounds.
    linv: another member's L_c^-1 (the mutant first_member_linv)"""
    A = csr(A)
    m, n = A.shape
    At = np.asarray(At, dtype).reshape(n, m)
    c = {"A": A, "e": np.asarray(e, dtype), "m": m, "n": n, "At": At, "dtype": dtype, "d": depth(A), "mutant": mutant}
    if m == 0:
        return c
    c["W"] = ax(A, At, dtype, mutant=mutant)            # what the handle reports
    c["absW"] = ax(A, np.abs(At), dtype, absolute=True)
    # a mutant of the reduction is planted in one product at a time: the factor is the clean W's (a wrong W may have no factor at all)
    c["L"] = chol_lower(c["W"] if mutant not in REDUCTION_MUTANTS else ax(A, At, dtype))
    c["Linv"] = lower_inverse(c["L"]) if linv is None else np.asarray(linv, dtype)
    c["logdet"] = (2 * np.log(np.diag(c["L"]))).sum()
    c["logdet_abs"] = np.abs(2 * np.log(np.diag(c["L"]))).sum()
    c["B"] = At @ c["Linv"].T
    c["H"] = np.abs(At) @ np.abs(c["Linv"]).T
    c["kappa"] = cond_lower(c["W"])
    W64 = np.tril(np.asarray(c["W"], np.float64))
    c["cW"] = float(np.linalg.norm(np.asarray(c["absW"], np.float64)) / np.linalg.norm(W64 + np.tril(W64, -1).T, 2))
    return c


def correct(c, X, mu=None):
    """X_c = X (+ mu) - B L_c^-1 (A X (+ A mu) - e) column by column, with R, T and the absolute sums of the bound"""
    dtype, m, n, A, mutant = c["dtype"], c["m"], c["n"], c["A"], c["mutant"]
    X = np.asarray(X, dtype).reshape(n, -1)
    mu_ = None if mu is None else np.asarray(mu, dtype).reshape(n, 1)
    base = X if mu_ is None else X + mu_
    absbase = np.abs(X) + (0 if mu_ is None else np.abs(mu_))
    if m == 0:
        return {"Xc": base, "S": absbase, "m": 0}
    R = ax(A, X, dtype, mutant=mutant)
    rabs = ax(A, np.abs(X), dtype, absolute=True)
    if mu_ is not None:
        R = R + (ax(A, mu_, dtype, mutant=mutant) - c["e"][:, None])
        rabs = rabs + ax(A, np.abs(mu_), dtype, absolute=True) + np.abs(c["e"])[:, None]
    else:
        R = R - c["e"][:, None]
        rabs = rabs + np.abs(c["e"])[:, None]
    T = c["Linv"] @ R
    B = c["B"]
    if mutant == "round_m_to_4" and m >= 4:
        BT = B[:, :4 * (m // 4)] @ T[:4 * (m // 4)]                # the last, partly masked k-step is not run
    else:
        BT = B @ T
        if mutant == "masked_reads_last":
            # the masked k-steps l >= m read index m - 1 of both operands instead of zeros
            BT = BT + (padded_m(m) - m) * np.outer(B[:, m - 1], T[m - 1])
    Xc = base - BT
    if mutant == "skip_second_piece":
        for j0, k in pieces(X.shape[1])[1:2]:
            Xc[:, j0:j0 + k] = X[:, j0:j0 + k]
    return {"Xc": Xc, "R": R, "T": T, "rabs": rabs, "m": m, "S": absbase + np.abs(B) @ np.abs(T),
            "tpath": np.abs(B) @ (np.abs(c["Linv"]) @ ((c["d"] + 2)[:, None] * rabs + m * np.abs(R))),
            "bpath": c["H"] @ np.abs(T),
            "cs": np.outer(np.sqrt((B * B).sum(axis=1)), np.sqrt((T * T).sum(axis=0)))}


def variance(c, sigma):
    dtype = c["dtype"]
    sigma = np.asarray(sigma, dtype)
    if c["m"] == 0:
        return {"var": sigma, "abs": sigma, "s2": 0 * sigma, "bh": 0 * sigma}
    B = c["B"]
    s2 = (B * B).sum(axis=1)
    v = sigma - s2
    return {"var": v if c["mutant"] == "no_clamp" else np.maximum(v, 0), "abs": sigma + s2, "s2": s2, "bh": (np.abs(B) * c["H"]).sum(axis=1)}


# ---- the bounds of the module docstring ---------------------------------------------------------------------------------------------------
def _gw(c):
    m = c["m"]
    return float(c["d"].max()) * c["cW"] + 3 * m * (m + 1)


def bound_W(c, factor=FACTOR):
    return factor * EPS * c["d"][:, None] * c["absW"]


def bound_logdet(c, factor=FACTOR):
    m = c["m"]
    return factor * EPS * (m * c["kappa"] * (float(c["d"].max()) * c["cW"] + m * (m + 1)) + (m + 2) * c["logdet_abs"])


def bound_X(c, r, factor=FACTOR):
    m = c["m"]
    if m == 0:
        return factor * EPS * r["S"]
    return factor * EPS * ((m + 1) * r["S"] + r["tpath"] + m * r["bpath"] + c["kappa"] * _gw(c) * r["cs"])


def bound_var(c, v, factor=FACTOR):
    m = c["m"]
    if m == 0:
        return 0 * v["abs"]
    return factor * EPS * ((m + 1) * v["abs"] + 2 * m * v["bh"] + c["kappa"] * _gw(c) * v["s2"])


def ratio(got, ref, bound, nonnegative=False):
    """the largest error / bound over the entries (0 / 0 counts as 0); inf where `got` is not finite or, with nonnegative, below zero"""
    got = np.asarray(got)
    err = np.abs(np.asarray(got, LD) - np.asarray(ref, LD))
    bound = np.broadcast_to(np.asarray(bound, LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0, err / bound)
    if not np.isfinite(got).all() or (nonnegative and (got < 0).any()):
        return float("inf")
    return float(np.max(q)) if q.size else 0.0


def residual_ratio(A, e, Xc):
    """max over rows and columns of |A X_c - e| / (2 d_r eps (|A| |X_c| + |e|)), A X_c in long double"""
    A = csr(A)
    Xc = np.asarray(Xc, LD).reshape(A.shape[1], -1)
    e = np.asarray(e, LD)[:, None]
    res = np.abs(ax(A, Xc, LD) - e)
    bound = 2 * depth(A)[:, None] * EPS * (ax(A, np.abs(Xc), LD, absolute=True) + np.abs(e))
    return ratio(res, 0 * res, bound)
