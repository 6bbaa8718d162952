"""The cases of tests/test_gpu_constraint_edges.py: every launch edge of the constraint kernels (csrc/constraint.hip) and of their
drivers (csrc/device_constraint.cpp), each by the smallest input that reaches it. tests/test_constraint_edges_host.py checks WITHOUT
a device that every case reaches the edge it names; tests/constraint_ref.py has the restatement and the bounds.

Precisions: tridiagonal, diagonally dominant, negative off-diagonals (fisher_ref.banded(n, 1)): any n is cheap, cond(Q) is about 10,
and Q^-1 > 0 entry by entry, so that a positive A has |A| |A~'| = W.
Rows of A ("blocks"): row r is positive, uniform(0.5, 1.5), on the r-th of m contiguous blocks that cover 0 .. n - 1: O(1) entries,
disjoint supports, no cancellation in A X for the positive X and mu of the corrections, every row of X moved by the correction
(a row tile that is not walked shows), block lengths within a factor 2 of each other. e_r = (A 1)_r uniform(0.8, 1.2): the
correction is of the size of X. Condition of every case: kappa = cond_2(A Q^-1 A') <= KAPPA_MAX = 1e3 (checked by the host test).

GROUPS (group -> what the cases pin; every case runs every check of the GPU test):
  choice    m in {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64} at n = 83, nvec = 17: the nine kernels of launch_con_apply (m = 0 with
            a mean: choice_m0), the partly masked k-step and the clamped read B[., min(l, m - 1)] at m = 5, 9, 17, 33
  rows      n in {1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257} with m = min(n, 3) (one thread per row, 256 per workgroup) and
            m = min(n, 5) (16 rows per wave, 64 per workgroup, rows past n clamped)
  cols      nvec in {1, 7, 8, 9, 15, 16, 17, 48, 49, 63, 64, 65, 1023, 1024, 1025, 2049} at m = 2 and m = 5, n = 37: the reduction's
            column tiles of 8, the apply kernels' blocks of 64 and sub-tiles of 16, the driver's pieces of 1024 (the second and third)
  rowlen    n = 8200, one A with rows of 1, 4095, 4096, 4097, 8191, 8192, 8193 entries: 1, 1, 1, 2, 2, 2, 3 chunks in ONE launch (the
            early return of k_con_ax_part, choff). These supports must overlap, and overlapping positive rows are nearly collinear
            (kappa >> 1e3), so the long rows are SIGNED: uniform(0.5, 1.5) times the r-th Rademacher function (half period
            n / 2^r >= 128 entries, far above Q^-1's correlation length), the one-entry row is 8. A X cancels here; the bounds stay
            relative to |A| |X|, of which a dropped entry is 1 / 8193, against 16 d eps = 1e-13.
  pairs     rows that are all-adjacent, stride-2, of odd length (a lone last entry) and starting at an odd p0, at nvec = 3 on the four
            layouts (ldx even / odd) x (offset 0 / 1 doubles): 16-byte and 8-byte loads both occur in every layout, same bits
  staging   the pairs' A given through set_constraints_csr with unsorted columns and with duplicates whose sum is exact
  tiles     n = 2048 * 64 + 17, m = 5 and n = 2048 * 256 + 3, m = 2 (nvec = 2): the walk rt += gridDim.x runs a second time, for one
            partial tile. The only large cases.
  batched   B = 2 members with different values, m in {2, 31, 32, 33, 63, 64}, n = 83: k_batch_con_chol, the member strides
  pinned    16 rows with one entry each: sigma - rowsum(B^2) is 0 up to rounding at the pinned nodes, of either sign before max(., 0)
  scatter   (every plain case) constraint_fields()[0] has the bits of backend_solve of the dense A'

MEASURED error / bound ratios (largest over the cases of a group; bounds of tests/constraint_ref.py).
Control, F = 1 (float64 restatement, numpy's summation order, against long double; tests/test_constraint_edges_host.py prints them):
  group    kappa  W      X      X+mu    logdet  var    residual
  choice   47     0.078  0.059  0.5     0.026   0.19   0.056      (X+mu 0.5 is m = 0: one rounding of x + mu against eps (|x| + |mu|))
  rows     3.8    0.11   0.063  0.028   0.036   0.10   0.059
  cols     1.7    0.038  0.038  0.033   0.017   0.072  0.053
  rowlen   299    0.54   1.2e-4 1.4e-4  2.6e-5  0.011  0.30       (numpy adds a row's 8193 terms one after the other: deeper than d_r = 27)
  pairs    3.6    0.022  0.010  0.0052  0.0032  0.023  0.011
  pinned   12     0.019  0.0014 8.3e-4  2.3e-5  0.011  0.036
  tiles    1.0    0.13   0.047  0.028   0.0060  0.17   0.060
  batched  26     0.056  0.037  0.033   0.026   0.11   0.061
Device, F = 16 (MI355X; tests/test_gpu_constraint_edges.py prints them):
  group    kappa  W       correct  sample   sample+mu  mean     logdet   var      residual
  choice   47     0.0040  0.0019   0.0021   0.031      0.0015   0.0013   0.012    0.090     (sample+mu 0.031 is m = 0)
  rows     3.8    0.0027  0.0019   0.0015   0.0028     0.0019   0.0022   0.0064   0.035
  cols     1.7    0.0018  0.0022   0.0017   0.0032     0.0016   8.2e-4   0.0034   0.036
  rowlen   299    0.0028  1.4e-6   1.5e-6   1.6e-6     1.2e-6   2.5e-6   6.8e-4   0.040
  pairs    3.6    0.0014  0.0015   3.0e-4   6.7e-4     6.5e-4   4.0e-4   0.0013   0.017
  pinned   12     0.0012  1.6e-4   2.9e-5   1.1e-4     1.6e-4   1.5e-6   6.8e-4   0.034
  tiles    1.0    0.0019  0.0017   9.2e-4   0.0026     0.0015   4.1e-4   0.010    0.0072
  batched  47     0.0024  0.0012   8.0e-4   0.0017     0.0011   5.4e-4   0.0075   0.070
Every bit-for-bit comparison held (host / _dev forms, the layouts, two runs, staged rows, A~' against backend_solve). The handles
of the two tiles cases took 0.08 s and 0.20 s to build, their tests 0.4 s and 1.2 s.
"""
import numpy as np
import scipy.sparse as sp

import constraint_ref as cr
from fisher_ref import banded

KAPPA_MAX = 1e3
CHOICE_M = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
ROWS_N = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257)
COLS_NVEC = (1, 7, 8, 9, 15, 16, 17, 48, 49, 63, 64, 65, 1023, 1024, 1025, 2049)
ROWLEN = (1, 4095, 4096, 4097, 8191, 8192, 8193)
BATCH_M = (2, 31, 32, 33, 63, 64)
TILES = ((2048 * 64 + 17, 5), (2048 * 256 + 3, 2))
# (ldx - n, offset in doubles) of the window in its buffer
LAYOUTS = {"even_ld": (1, 0), "odd_ld": (2, 0), "even_ld_off1": (1, 1), "odd_ld_off1": (2, 1)}      # n = 41: ldx = 42, 43


class Case:
    def __init__(self, name, group, n, m, nvecs, rows="blocks", members=1, seed=0):
        self.name, self.group, self.n, self.m, self.nvecs, self.rows, self.members, self.seed = name, group, n, m, tuple(nvecs), rows, members, seed

    def __repr__(self):
        return self.name

    def Q(self, member=0):
        """tridiagonal; the members of a batched case share the pattern and differ in every value"""
        return banded(self.n, 1, seed=member)

    def A_e(self):
        rng = np.random.default_rng(1000 + 7 * self.n + self.m + self.seed)
        if self.m == 0:
            return sp.csr_matrix((0, self.n)), np.zeros(0)
        A = _ROWS[self.rows](self.n, self.m, rng)
        e = np.asarray(abs(A).sum(axis=1)).ravel() * rng.uniform(0.8, 1.2, A.shape[0])
        return A, e

    def operands(self, nvec):
        """(Y, Z, mu): positive columns to correct, standard normals to sample from, a positive mean"""
        rng = np.random.default_rng(77 + self.n + 3 * nvec + self.seed)
        return rng.uniform(0.5, 1.5, (self.n, nvec)), rng.standard_normal((self.n, nvec)), rng.uniform(0.5, 1.5, self.n)


def block_rows(n, m, rng):
    cut = np.linspace(0, n, m + 1).round().astype(int)
    rows = np.repeat(np.arange(m), np.diff(cut))
    return cr.csr(sp.csr_matrix((rng.uniform(0.5, 1.5, n), (rows, np.arange(n))), shape=(m, n)))


def rowlen_rows(n, m, rng):
    """row 0: one entry; row r >= 1: ROWLEN[r] entries from column 0 (even r) or up to column n - 1 (odd r), signed by the r-th
    Rademacher function of the column"""
    assert n == 8200 and m == len(ROWLEN)
    ri, ci, va = [0], [n // 2], [8.0]
    for r in range(1, m):
        ln = ROWLEN[r]
        cols = np.arange(ln) + (0 if r % 2 == 0 else n - ln)
        sign = 1.0 - 2.0 * ((cols * 2 ** r // n) % 2)
        ri += [r] * ln
        ci += list(cols)
        va += list(sign * rng.uniform(0.5, 1.5, ln))
    return cr.csr(sp.csr_matrix((va, (ri, ci)), shape=(m, n)))


PAIR_COLS = (np.arange(0, 10), np.arange(10, 29, 2), np.arange(30, 37), np.arange(37, 41))


def pair_rows(n, m, rng):
    """row 0: 10 adjacent columns from column 0 (p0 = 0); row 1: 10 columns of stride 2 (no adjacent pair); row 2: 7 adjacent columns
    (odd length: a lone last entry); row 3: 4 adjacent columns from the odd column 37, its entries from the odd p0 = 27"""
    assert n == 41 and m == 4
    ri = np.concatenate([[r] * len(c) for r, c in enumerate(PAIR_COLS)])
    ci = np.concatenate(PAIR_COLS)
    return cr.csr(sp.csr_matrix((rng.uniform(0.5, 1.5, len(ci)), (ri, ci)), shape=(m, n)))


def pinned_rows(n, m, rng):
    nodes = np.linspace(0, n - 1, m).round().astype(int)
    return cr.csr(sp.csr_matrix((rng.uniform(0.5, 1.5, m), (np.arange(m), nodes)), shape=(m, n)))


_ROWS = {"blocks": block_rows, "rowlen": rowlen_rows, "pairs": pair_rows, "pinned": pinned_rows}


def staged_forms(A):
    """A's CSR arrays given unsorted and with duplicates whose sum is exact: (name, rowptr, colind, values). A dyadic quarter of
    every entry is split off (x - x / 4 and x / 4 are exact, and so is their sum); the columns of each row are reversed."""
    rp, ci, va = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    rev = np.concatenate([np.arange(rp[r], rp[r + 1])[::-1] for r in range(A.shape[0])])
    yield "unsorted", rp, ci[rev], va[rev]
    q = va / 4
    assert np.array_equal((va - q) + q, va)
    c2, v2, p2 = [], [], [0]
    for r in range(A.shape[0]):
        s = slice(rp[r], rp[r + 1])
        c2 += [ci[s], ci[s][::-1]]
        v2 += [(va - q)[s], q[s][::-1]]
        p2.append(p2[-1] + 2 * (rp[r + 1] - rp[r]))
    yield "duplicates", np.array(p2, np.int64), np.concatenate(c2), np.concatenate(v2)


def cases():
    out = [Case(f"choice_m{m}", "choice", 83, m, (17,)) for m in CHOICE_M]
    out.append(Case("choice_m0", "choice", 83, 0, (17,)))
    for n in ROWS_N:
        for m in sorted({min(n, 3)} | ({min(n, 5)} if n >= 5 else set())):
            out.append(Case(f"rows_n{n}_m{m}", "rows", n, m, (5,)))
    out += [Case(f"cols_m{m}_k{k}", "cols", 37, m, (k,)) for m in (2, 5) for k in COLS_NVEC]
    out.append(Case("rowlen", "rowlen", 8200, len(ROWLEN), (1, 9), rows="rowlen"))
    out.append(Case("pairs", "pairs", 41, 4, (3,), rows="pairs"))
    out.append(Case("pinned", "pinned", 83, 16, (3,), rows="pinned"))
    out += [Case(f"tiles_n{n}_m{m}", "tiles", n, m, (2,)) for n, m in TILES]
    out += [Case(f"batched_m{m}", "batched", 83, m, (3,), members=2) for m in BATCH_M]
    return out


CASES = {c.name: c for c in cases()}
# the case each mutant of constraint_ref.MUTANTS must exceed the device bound on, and the columns it is run with
MUTANT_CASE = {"drop_lone": ("pairs", 3), "drop_last_chunk": ("rowlen", 1), "neighbour_chunks": ("rowlen", 1), "clamped_column": ("cols_m5_k9", 9),
               "round_m_to_4": ("choice_m33", 17), "masked_reads_last": ("choice_m33", 17), "skip_second_piece": ("cols_m5_k1025", 1025),
               "first_member_linv": ("batched_m33", 3), "no_clamp": ("pinned", 3)}
