"""Problems, layouts and buffer builders of test_gpu_layout.py: a column-major n x ncol WINDOW (leading dimension ld, base offset
off, both in doubles) inside a larger flat buffer that the test fills on the host and uploads.

An INPUT buffer is NaN everywhere outside its window, so that a kernel that reads padding shows it in its result; an OUTPUT buffer
is SENTINEL everywhere, so that a write outside the window is seen. Every buffer keeps ld spare doubles behind its last column: a
clamped load one column too far stays inside the allocation."""
import numpy as np
import scipy.sparse as sp

from gmrfx import spde

SENTINEL = -1.25e300            # the value test_gpu_batch_edges.py fills its gaps with

# right-hand-side counts: both sides of the narrow / wide permute switch at 8, a full 64-column pass, a pass plus one column, two
# passes (one per lane) and two passes plus one
NRHS = (1, 2, 8, 9, 17, 63, 64, 65, 128, 129)
NVEC = (1, 3, 5)

# name -> (ldb - n, ldx - n, base offset of B, base offset of X); a torch allocation is at least 16-byte aligned (asserted in the
# tests), so an odd offset makes the base 8-byte aligned only, and an odd ld makes the column starts alternate
LAYOUTS = {
    "contig": (0, 0, 0, 0),
    "odd_ld": (1, 3, 0, 0),
    "wide_in": (8, 0, 0, 0),
    "wide_out": (0, 5, 0, 0),
    "odd_base": (1, 3, 1, 1),
    "mixed_base": (2, 2, 1, 0),
}
# the distinct (ldx - n, offset) pairs of the X column above: the layouts of a quadratic form's only array
X_LAYOUTS = {"contig": (0, 0), "odd_ld": (3, 0), "wide_out": (5, 0), "odd_base": (3, 1), "mixed_base": (2, 0)}


def _sym_csc(Q):
    """sorted CSC with EXACTLY symmetric values on the same pattern: Q.toarray() is then the matrix the handle factors, whichever
    triangle it reads (the assembled Matern values differ between the triangles in the last bit)"""
    Q = sp.csc_matrix(Q)
    Q = sp.csc_matrix((Q + Q.T) * 0.5)
    Q.sort_indices()
    return Q


def problems():
    """name -> Q. The sizes are the smallest at which the permute kernels' blocks (64 rows wide form, 256 rows narrow form) are
    partial, hold a single row, or are all full; PROBLEM_REMAINDERS states what each n must leave modulo 64 and 256."""
    return {
        "scalar": _sym_csc(np.array([[2.5]])),
        "rand20": _sym_csc(spde.random_spd_precision(20)),
        "matern513": _sym_csc(spde.matern_precision(spde.grid_mesh_2d(27, 19, jitter=0.25, seed=1), 0, 0.3)),
        "matern768": _sym_csc(spde.matern_precision(spde.grid_mesh_2d(32, 24, jitter=0.25, seed=1), 0, 0.3)),
    }


PROBLEM_REMAINDERS = {"scalar": (1, 1, 1), "rand20": (20, 20, 20), "matern513": (513, 1, 1), "matern768": (768, 0, 0)}   # n, n % 64, n % 256


def diag_positions(Q):
    """positions of the diagonal entries in Q's CSC value array: the Hessian -> Q map of a diagonal Hessian"""
    out = np.empty(Q.shape[0], np.int64)
    for j in range(Q.shape[0]):
        r = Q.indices[Q.indptr[j]:Q.indptr[j + 1]]
        out[j] = Q.indptr[j] + int(np.flatnonzero(r == j)[0])
    return out


def buffer_len(ncol, ld, off):
    return off + ld * ncol + ld


def window_index(n, ncol, ld, off):
    """flat indices of the window, shape (n, ncol)"""
    return off + np.arange(n)[:, None] + ld * np.arange(ncol)[None, :]


def input_buffer(W, ld, off):
    """W (n, ncol) laid out in a NaN-filled flat buffer"""
    n, ncol = W.shape
    buf = np.full(buffer_len(ncol, ld, off), np.nan)
    buf[window_index(n, ncol, ld, off)] = W
    return buf


def output_buffer(ncol, ld, off):
    return np.full(buffer_len(ncol, ld, off), SENTINEL)


def split(buf, n, ncol, ld, off):
    """(the window as an (n, ncol) array, everything else as a flat array)"""
    idx = window_index(n, ncol, ld, off)
    rest = np.ones(buf.shape[0], bool)
    rest[idx] = False
    return buf[idx], buf[rest]


def same_bits(a, b):
    """equal as raw 64-bit words (NaN payloads and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
