"""MI355XBackend -- mirror of the reference's `WorkspaceBackend` protocol
(src/workspace/backend.jl:8-30) for the libgmrfx.so backend. Method names, argument meaning,
laziness/caching and error behaviour follow `CHOLMODBackend` (backend.jl:51-284) so that the
parity tests read like test/workspace/test_gmrf_workspace.jl. All arithmetic is done by the HIP
kernels behind the C ABI; this file only marshals arrays."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import GmrfxOpts, GmrfxStats, check, lib, ptr


@dataclass
class SymbolicInfo:
    super_first: np.ndarray
    super_parent: np.ndarray
    row_ptr: np.ndarray
    rows: np.ndarray
    rel: np.ndarray
    panel_ptr: np.ndarray
    panel_ld: np.ndarray
    level: np.ndarray
    q_src: np.ndarray
    q_dst: np.ndarray
    cb_arena: int


def _as_csc(Q) -> sp.csc_matrix:
    if not sp.isspmatrix_csc(Q):
        Q = sp.csc_matrix(Q)
    if Q.shape[0] != Q.shape[1]:
        raise ValueError("Q must be square")      # ArgumentError in gmrf_workspace.jl:68
    if not Q.has_sorted_indices:
        Q = Q.copy()
        Q.sort_indices()
    return Q


# -- Rao-Blackwellised Monte Carlo marginal variances (gmrfx_rbmc_*): shared by the plain and the batched backend --------------
def _rbmc_plan(h, enclosure_size: int, index_base: int = 0) -> dict:
    """The blocks of BlockRBMCStrategy(enclosure_size) (host analysis; works on symbolic-only handles): block_ptr, rows (S first),
    n_interior, owner (1 where the block writes the node), max_block."""
    counts = np.zeros(3, np.int64)
    check(lib().gmrfx_rbmc_plan(h, int(enclosure_size), int(index_base), ptr(counts), None, None, None, None), h)
    nb, tot = int(counts[0]), int(counts[1])
    out = {"block_ptr": np.empty(nb + 1, np.int64), "rows": np.empty(tot, np.int64), "n_interior": np.empty(nb, np.int64),
           "owner": np.empty(tot, np.int64)}
    check(lib().gmrfx_rbmc_plan(h, int(enclosure_size), int(index_base), ptr(counts), ptr(out["block_ptr"]), ptr(out["rows"]),
                                ptr(out["n_interior"]), ptr(out["owner"])), h)
    out["max_block"] = int(counts[2])
    return out


def _rbmc_var(h, n: int, nnz: int, Z, enclosure_size: int, nzval) -> np.ndarray:
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[0] != n:
        raise ValueError(f"Z must have shape (n, nsamples) with n = {n}, got {Z.shape}")
    Zf = np.asfortranarray(Z)
    nz = None if nzval is None else np.ascontiguousarray(nzval, dtype=np.float64)
    if nz is not None and nz.shape != (nnz,):
        raise ValueError("nzval length does not match the pattern")
    out = np.empty(n)
    check(lib().gmrfx_rbmc_var(h, ptr(nz), ptr(Zf), n, Zf.shape[1], int(enclosure_size), ptr(out)), h)
    return out


class MI355XBackend:
    """`MI355XBackend(Symmetric(Q); ordering=nothing, coords=nothing)`.

    ordering: None (own nested dissection), "natural", an explicit permutation vector (0-based here; the Julia
    shim passes 1-based with index_base=1), a callable pattern -> permutation (where Julia passes a CliqueTrees
    algorithm object) or `PinDenseColumns(inner, frac)` -- resolved by `gmrfx.ordering.ordering_permutation`, the
    host logic of `CHOLMODBackend(Q; ordering)` / `ordering_permutation`, backend.jl:86-153. Unknown forms raise.
    """

    def __init__(self, Q, ordering=None, coords=None, device: int = -1, symbolic_only: bool = False,
                 check_posdef: bool = False, uplo: str = "U", nd_leaf: int = 0, relax_cols: int = 0,
                 relax_zeros: float = 0.0, factorize: bool = True, shard_rank: int = 0, shard_world: int = 1, shard_min_top: int = 0):
        Q = _as_csc(Q)
        self.n = Q.shape[0]
        self._colptr = np.ascontiguousarray(Q.indptr, dtype=np.int64)
        self._rowval = np.ascontiguousarray(Q.indices, dtype=np.int64)
        self._nnz = int(self._colptr[-1])
        opts = GmrfxOpts()
        opts.struct_size = C.sizeof(GmrfxOpts)
        opts.uplo = 0 if uplo.upper().startswith("U") else 1
        opts.device = device
        self.device = device            # HIP device ordinal the handle was asked for (-1: the current device)
        opts.symbolic_only = int(symbolic_only)
        opts.check_posdef = int(check_posdef)
        opts.nd_leaf = nd_leaf
        opts.relax_cols = relax_cols
        opts.relax_zeros = relax_zeros
        opts.shard_rank = shard_rank
        opts.shard_world = shard_world
        opts.shard_min_top = shard_min_top      # > 0 with shard_world == 1: a sharded handle of ONE rank (include/gmrfx.h)
        self.shard_rank, self.shard_world = shard_rank, shard_world
        from .ordering import ordering_permutation as _resolve
        perm = _resolve(Q, ordering, coords)
        if isinstance(perm, str):           # "natural"
            opts.ordering = 1
            perm = None
        self._coords = None
        if coords is not None:
            self._coords = np.ascontiguousarray(coords, dtype=np.float64)
            if self._coords.ndim != 2 or self._coords.shape[0] != self.n:
                raise ValueError("coords must be n x dim")
            opts.coord_dim = self._coords.shape[1]
            opts.coords = self._coords.ctypes.data
        h = C.c_void_p()
        check(lib().gmrfx_create(self.n, ptr(self._colptr), ptr(self._rowval), 0, ptr(perm), C.byref(opts), C.byref(h)))
        self._h = h
        self.symbolic_only = symbolic_only
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = 0
        if factorize and not symbolic_only and shard_world <= 1 and shard_min_top <= 0:
            self.refactorize_values(Q.data)

    # -- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib().gmrfx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone(self) -> "MI355XBackend":
        """deepcopy(cache) semantics (arithmetic/condition/gaussian_approximation.jl:103-109)."""
        other = object.__new__(MI355XBackend)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("_h", "_rd_plans")})   # plans live in the handle
        h = C.c_void_p()
        check(lib().gmrfx_clone(self._h, C.byref(h)))
        other._h = h
        other._selinv_cache = None
        other._selinv_diag_cache = None
        return other

    # -- WorkspaceBackend protocol ----------------------------------------------------------
    def refactorize(self, Q) -> None:
        """refactorize!(b, Q::Symmetric): same pattern guaranteed by the caller (backend.jl:178)."""
        Q = _as_csc(Q)
        if Q.nnz != self._nnz:
            raise ValueError(f"buffer holds {self._nnz} values but Q has {Q.nnz} nonzeros; "
                             "the sparsity pattern must be invariant across refactorizations")
        self.refactorize_values(Q.data)

    def refactorize_values(self, nzval) -> None:
        nz = np.ascontiguousarray(nzval, dtype=np.float64)
        if nz.shape != (self._nnz,):
            raise ValueError("nzval length does not match the pattern")
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize(self._h, ptr(nz), C.byref(info)), self._h)
        self.last_info = info.value
        self._selinv_cache = None
        self._selinv_diag_cache = None

    def backend_solve(self, rhs):
        """`F \\ b` / `F \\ B` (backend.jl:191-209). Returns a fresh array; input untouched."""
        B = np.asarray(rhs, dtype=np.float64)
        if B.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        vec = B.ndim == 1
        Bf = np.asfortranarray(B.reshape(self.n, -1))
        X = np.empty_like(Bf, order="F")
        check(lib().gmrfx_solve(self._h, Bf.ctypes.data, self.n, Bf.shape[1], X.ctypes.data, self.n), self._h)
        return X[:, 0].copy() if vec else X

    def compute_logdet(self) -> float:
        out = C.c_double(0.0)
        check(lib().gmrfx_logdet(self._h, C.byref(out)), self._h)
        return out.value

    def sqmahal(self, x, mean=None, nzval=None):
        """(x - mean)' Q (x - mean) on the device: `dot(r, d.precision * r)` of logpdf (workspace_gmrf.jl:288-292)
        and sqmahal (gmrf.jl:94-97). x: n vector or n x k matrix (one value per column). nzval: Q's values in the
        pattern's order; None = the values of the last refactorisation."""
        X = np.asarray(x, dtype=np.float64)
        if X.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        vec = X.ndim == 1
        Xf = np.asfortranarray(X.reshape(self.n, -1))
        mu = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        if mu is not None and mu.shape != (self.n,):
            raise ValueError("dimension mismatch")
        nz = None if nzval is None else np.ascontiguousarray(nzval, dtype=np.float64)
        if nz is not None and nz.shape != (self._nnz,):
            raise ValueError("nzval length does not match the pattern")
        out = np.empty(Xf.shape[1])
        check(lib().gmrfx_quadform(self._h, ptr(nz), ptr(Xf), self.n, Xf.shape[1], ptr(mu), ptr(out)), self._h)
        return float(out[0]) if vec else out

    def logpdf(self, z, mean=None) -> float:
        """logpdf(d::WorkspaceGMRF, z) without constraints (workspace_gmrf.jl:288-292):
        -0.5 r'Qr + 0.5 logdet(Q) - 0.5 n log(2 pi), on the values of the last refactorisation."""
        return -0.5 * self.sqmahal(z, mean) + 0.5 * self.compute_logdet() - 0.5 * self.n * np.log(2.0 * np.pi)

    def compute_selinv(self) -> None:
        """Lazy like the CHOLMOD backend (backend.jl:215-221): the getters trigger the work."""
        return None

    def get_selinv(self) -> sp.csc_matrix:
        if self._selinv_cache is None:
            nnz = C.c_int64(0)
            check(lib().gmrfx_selinv_nnz(self._h, C.byref(nnz)), self._h)
            colptr = np.empty(self.n + 1, np.int64)
            rowval = np.empty(nnz.value, np.int64)
            nzval = np.empty(nnz.value, np.float64)
            check(lib().gmrfx_selinv_csc(self._h, 0, ptr(colptr), ptr(rowval), ptr(nzval)), self._h)
            self._selinv_cache = sp.csc_matrix((nzval, rowval, colptr), shape=(self.n, self.n))
        return self._selinv_cache

    def get_selinv_diag(self) -> np.ndarray:
        if self._selinv_diag_cache is None:
            out = np.empty(self.n)
            check(lib().gmrfx_selinv_diag(self._h, ptr(out)), self._h)
            self._selinv_diag_cache = out
        return self._selinv_diag_cache

    def backend_backward_solve(self, x):
        """`F.UP \\ x` = P' L^-T x (backend.jl:281-284); accepts views, vectors or n x k."""
        Z = np.asarray(x, dtype=np.float64)
        if Z.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        vec = Z.ndim == 1
        Zf = np.asfortranarray(Z.reshape(self.n, -1))
        X = np.empty_like(Zf, order="F")
        check(lib().gmrfx_backward_solve(self._h, Zf.ctypes.data, self.n, Zf.shape[1], X.ctypes.data, self.n), self._h)
        return X[:, 0].copy() if vec else X

    def selinv_extract_at(self, B) -> sp.csc_matrix:
        """Sigma on B's pattern, 0 outside the factor pattern (backend.jl:275-279)."""
        B = _as_csc(B)
        if B.shape != (self.n, self.n):
            raise ValueError("dimension mismatch")
        colptr = np.ascontiguousarray(B.indptr, dtype=np.int64)
        rowval = np.ascontiguousarray(B.indices, dtype=np.int64)
        out = np.empty(len(rowval))
        check(lib().gmrfx_selinv_extract(self._h, self.n, ptr(colptr), ptr(rowval), 0, ptr(out)), self._h)
        return sp.csc_matrix((out, rowval.copy(), colptr.copy()), shape=B.shape)

    def selinv_dot(self, B) -> float:
        """tr(Q^-1 B) for pattern(B) within the factor pattern (backend.jl:265). The values of
        Sigma are gathered on the device; the final dot stays on the host so that, as in the
        reference, B may carry dual numbers."""
        B = _as_csc(B)
        return float(np.dot(self.selinv_extract_at(B).data, B.data))

    def selinv_dot_device(self, B) -> float:
        """tr(Q^-1 B) for a Float64 B, contracted on the device (gmrfx_selinv_dot)."""
        B = _as_csc(B)
        if B.shape != (self.n, self.n):
            raise ValueError("dimension mismatch")
        colptr = np.ascontiguousarray(B.indptr, dtype=np.int64)
        rowval = np.ascontiguousarray(B.indices, dtype=np.int64)
        vals = np.ascontiguousarray(B.data, dtype=np.float64)
        out = C.c_double(0.0)
        check(lib().gmrfx_selinv_dot(self._h, self.n, ptr(colptr), ptr(rowval), ptr(vals), 0, C.byref(out)), self._h)
        return out.value

    def row_diag_ASigmaAt(self, A) -> np.ndarray:
        """diag(A Sigma A') for a sparse design matrix A (m x n): the predictor marginal variances of
        linear_predictor_marginals.jl:125-165, contracted on the device from the selected-inverse panels
        (Sigma = 0 outside the factor pattern, as there). The pair plan of A's pattern is kept on the device and
        reused while the pattern stays the same (the hyper-parameter loop changes Q, not A)."""
        A = sp.csr_matrix(A)
        if A.shape[1] != self.n:
            raise ValueError("dimension mismatch")
        A.sum_duplicates()
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        colind = np.ascontiguousarray(A.indices, dtype=np.int64)
        vals = np.ascontiguousarray(A.data, dtype=np.float64)
        import zlib
        key = (A.shape[0], len(colind), zlib.crc32(rowptr.tobytes()), zlib.crc32(colind.tobytes()))
        plans = self.__dict__.setdefault("_rd_plans", {})
        if key not in plans:
            if len(plans) >= 4:                                   # a handful of design matrices at most
                old_key = next(iter(plans))
                check(lib().gmrfx_selinv_row_diag_free(self._h, plans.pop(old_key)), self._h)
            pid = C.c_int64(-1)
            check(lib().gmrfx_selinv_row_diag_plan(self._h, A.shape[0], ptr(rowptr), ptr(colind), 0, C.byref(pid)), self._h)
            plans[key] = pid.value
        out = np.empty(A.shape[0])
        check(lib().gmrfx_selinv_row_diag_apply(self._h, plans[key], ptr(vals), ptr(out)), self._h)
        return out

    def row_diag_ASigmaAt_once(self, A) -> np.ndarray:
        """One-shot form (gmrfx_selinv_row_diag): plans, contracts and forgets."""
        A = sp.csr_matrix(A)
        if A.shape[1] != self.n:
            raise ValueError("dimension mismatch")
        A.sum_duplicates()
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        colind = np.ascontiguousarray(A.indices, dtype=np.int64)
        vals = np.ascontiguousarray(A.data, dtype=np.float64)
        out = np.empty(A.shape[0])
        check(lib().gmrfx_selinv_row_diag(self._h, A.shape[0], ptr(rowptr), ptr(colind), ptr(vals), 0, ptr(out)), self._h)
        return out

    # -- extras --------------------------------------------------------------------------------
    def ordering_permutation(self) -> np.ndarray:
        """Elimination order actually used (0-based): pass it to CHOLMOD to factor the same PQP'."""
        p = np.empty(self.n, np.int64)
        check(lib().gmrfx_get_perm(self._h, 0, ptr(p)))
        return p

    def stats(self) -> dict:
        st = GmrfxStats()
        check(lib().gmrfx_get_stats(self._h, C.byref(st), C.sizeof(GmrfxStats)))
        return st.asdict()

    def symbolic(self) -> SymbolicInfo:
        sizes = np.zeros(8, np.int64)
        check(lib().gmrfx_symbolic_sizes(self._h, ptr(sizes)))
        ns, sr, _, _, cb, nq = (int(x) for x in sizes[:6])
        a = dict(super_first=np.empty(ns + 1, np.int64), super_parent=np.empty(ns, np.int64),
                 row_ptr=np.empty(ns + 1, np.int64), rows=np.empty(sr, np.int64), rel=np.empty(sr, np.int64),
                 panel_ptr=np.empty(ns + 1, np.int64), panel_ld=np.empty(ns, np.int64), level=np.empty(ns, np.int64),
                 q_src=np.empty(nq, np.int64), q_dst=np.empty(nq, np.int64))
        check(lib().gmrfx_symbolic_get(self._h, *[ptr(a[k]) for k in (
            "super_first", "super_parent", "row_ptr", "rows", "rel", "panel_ptr", "panel_ld", "level", "q_src", "q_dst")]))
        return SymbolicInfo(cb_arena=cb, **a)

    def sweep_tasks(self):
        """(rows_cap, first, last, lrow): the bottom subtrees whose sweeps run on an LDS-resident local vector."""
        nt, cap = C.c_int64(0), C.c_int64(0)
        check(lib().gmrfx_symbolic_sweep_tasks(self._h, C.byref(nt), C.byref(cap), None, None, None))
        sizes = np.zeros(8, np.int64)
        check(lib().gmrfx_symbolic_sizes(self._h, ptr(sizes)))
        first, last = np.empty(nt.value, np.int64), np.empty(nt.value, np.int64)
        lrow = np.empty(int(sizes[1]), np.int64)
        check(lib().gmrfx_symbolic_sweep_tasks(self._h, C.byref(nt), C.byref(cap), ptr(first), ptr(last), ptr(lrow)))
        return int(cap.value), first, last, lrow

    def sweep_chunks(self) -> dict:
        """The tasks' chunks (include/gmrfx.h: gmrfx_symbolic_sweep_chunks): task_ptr (ntasks + 1 x 2: first forward / backward
        record), slot (ntasks x 8), fwd / bwd (records x 8: pa, ld, o, cc, nt, lr, nbar, id), rows (padded target-row lists)."""
        nc, nr = np.zeros(2, np.int64), C.c_int64(0)
        check(lib().gmrfx_symbolic_sweep_chunks(self._h, ptr(nc), C.byref(nr), None, None, None, None, None))
        nt = C.c_int64(0)
        check(lib().gmrfx_symbolic_sweep_tasks(self._h, C.byref(nt), None, None, None, None))
        out = dict(task_ptr=np.empty((nt.value + 1, 2), np.int64), slot=np.empty((nt.value, 8), np.int64),
                   fwd=np.empty((int(nc[0]), 8), np.int64), bwd=np.empty((int(nc[1]), 8), np.int64), rows=np.empty(nr.value, np.int64))
        check(lib().gmrfx_symbolic_sweep_chunks(self._h, ptr(nc), C.byref(nr), *[ptr(out[k]) for k in ("task_ptr", "slot", "fwd", "bwd", "rows")]))
        return out

    def factor_values(self) -> np.ndarray:
        sizes = np.zeros(8, np.int64)
        check(lib().gmrfx_symbolic_sizes(self._h, ptr(sizes)))
        out = np.empty(int(sizes[2]))
        check(lib().gmrfx_get_factor_values(self._h, ptr(out)), self._h)
        return out

    def factor_csc(self) -> sp.csc_matrix:
        """The numeric factor L (elimination order) as a sparse matrix, from the panels."""
        sy = self.symbolic()
        vals = self.factor_values()
        I, J, V = [], [], []
        for s in range(len(sy.super_parent)):
            f, l1 = sy.super_first[s], sy.super_first[s + 1]
            rows = sy.rows[sy.row_ptr[s]:sy.row_ptr[s + 1]]
            ld = sy.panel_ld[s]
            for j in range(l1 - f):
                col = vals[sy.panel_ptr[s] + j * ld: sy.panel_ptr[s] + j * ld + len(rows)]
                I.append(rows[j:]); J.append(np.full(len(rows) - j, f + j)); V.append(col[j:])
        return sp.csc_matrix((np.concatenate(V), (np.concatenate(I), np.concatenate(J))), shape=(self.n, self.n))

    # -- device-resident entry points (HBM in, HBM out) for benchmarks / chained GPU use -----------
    def refactorize_dev(self, d_nzval_ptr: int) -> int:
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_dev(self._h, d_nzval_ptr, C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return info.value

    def refactorize_solve_dev(self, d_nzval_ptr: int, d_B: int, ldb: int, nrhs: int, d_X: int, ldx: int) -> int:
        """`workspace_solve` on a workspace with new values (gmrf_workspace.jl:170-178, 207-215): numeric factorisation and
        solve as one pipelined call; same bits as refactorize_dev + solve_dev."""
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_solve_dev(self._h, d_nzval_ptr, d_B, ldb, nrhs, d_X, ldx, C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return info.value

    def refactorize_logpdf_dev(self, d_nzval_ptr: int, d_X: int, ldx: int, nvec: int, d_mu: int = 0):
        """One logpdf evaluation of the hyper-parameter loop in one call (gmrfx_refactorize_logpdf_dev): new values -> numeric
        factorisation; returns (quadratic forms (x_k - mu)' Q (x_k - mu), log det Q). logpdf = -q / 2 + logdet / 2 - n log(2 pi) / 2
        (workspace_gmrf.jl:288-292)."""
        quad = np.empty(max(nvec, 0))
        ld = C.c_double(0.0)
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_logpdf_dev(self._h, d_nzval_ptr, d_X or None, ldx, nvec, d_mu or None, ptr(quad), C.byref(ld), C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return quad, ld.value

    def refactorize_solve(self, nzval, rhs):
        """Host-array form of refactorize_solve_dev: new values of Q (pattern order) and right-hand sides -> X (fresh array)."""
        nz = np.ascontiguousarray(nzval, dtype=np.float64)
        if nz.shape != (self._nnz,):
            raise ValueError("nzval length does not match the pattern")
        B = np.asarray(rhs, dtype=np.float64)
        if B.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        vec = B.ndim == 1
        Bf = np.asfortranarray(B.reshape(self.n, -1))
        X = np.empty_like(Bf, order="F")
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_solve(self._h, ptr(nz), ptr(Bf), self.n, Bf.shape[1], ptr(X), self.n, C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return X[:, 0].copy() if vec else X

    def dense_apply_dev(self, d_D: int, n1: int, d_T: int, n2: int, d_R: int) -> None:
        """R = D T on the device (gmrfx_dense_apply_dev): row-major D (n1 x n1), T and R (n1 x n2); the dense-operator leg of the
        Kronecker path (separable.jl:122-172). T needs 8 readable bytes behind it when n2 is odd."""
        check(lib().gmrfx_dense_apply_dev(self._h, n1, n2, d_D, d_T, d_R), self._h)

    def transpose_dev(self, d_src: int, rows: int, cols: int, d_dst: int) -> None:
        """dst (cols x rows) = src' for a row-major rows x cols device array (gmrfx_transpose_dev)."""
        check(lib().gmrfx_transpose_dev(self._h, rows, cols, d_src, d_dst), self._h)

    def refactorize_solve_ptr(self, nzval_ptr: int, B_ptr: int, ldb: int, nrhs: int, X_ptr: int, ldx: int) -> int:
        """gmrfx_refactorize_solve on raw HOST pointers (column-major B / X the caller keeps alive; page-locked memory is handed to
        the DMA engine directly, pageable memory is staged by the library): the call a Julia `workspace_solve(ws, B::Matrix)` makes."""
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_solve(self._h, nzval_ptr, B_ptr, ldb, nrhs, X_ptr, ldx, C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return info.value

    # -- Newton loop on the device (src/workspace/gaussian_approximation.jl:63-129) --------
    def set_prior(self, prior_nzval, hess_map) -> None:
        """prior_nzval: values of the prior precision in the pattern's CSC order; hess_map: 0-based positions
        into nzval of the Hessian's entries (`_diag_indices` / `_sparse_hessian_map` of the reference)."""
        pv = np.ascontiguousarray(prior_nzval, dtype=np.float64)
        if pv.shape != (self._nnz,):
            raise ValueError(f"prior precision has {pv.size} stored entries but the workspace pattern has {self._nnz}")
        hm = np.ascontiguousarray(hess_map, dtype=np.int64)
        self._hess_cnt = int(hm.size)
        check(lib().gmrfx_set_prior(self._h, ptr(pv), ptr(hm), hm.size, 0), self._h)

    def refactorize_update(self, hvals) -> int:
        """Q <- Q_prior - H (entries at hess_map), refactorise; only `hvals` crosses PCIe."""
        hv = np.ascontiguousarray(hvals, dtype=np.float64)
        if hv.size != getattr(self, "_hess_cnt", -1):
            raise ValueError("Hessian values do not match the index map passed to set_prior")
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_update(self._h, ptr(hv), C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return info.value

    def refactorize_update_solve(self, hvals, rhs):
        """One Newton iterate in one pipelined call: Q <- Q_prior - H, refactorise, solve Q X = rhs (gmrfx_refactorize_update_solve)."""
        hv = np.ascontiguousarray(hvals, dtype=np.float64)
        if hv.size != getattr(self, "_hess_cnt", -1):
            raise ValueError("Hessian values do not match the index map passed to set_prior")
        B = np.asarray(rhs, dtype=np.float64)
        if B.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        vec = B.ndim == 1
        Bf = np.asfortranarray(B.reshape(self.n, -1))
        X = np.empty_like(Bf, order="F")
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_update_solve(self._h, ptr(hv), ptr(Bf), self.n, Bf.shape[1], ptr(X), self.n, C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return X[:, 0].copy() if vec else X

    def refactorize_update_solve_dev(self, d_hvals: int, d_B: int, ldb: int, nrhs: int, d_X: int, ldx: int) -> int:
        """Device-pointer form of refactorize_update_solve (gmrfx_refactorize_update_solve_dev): the Hessian values, B and X stay in HBM."""
        info = C.c_int64(0)
        check(lib().gmrfx_refactorize_update_solve_dev(self._h, d_hvals, d_B, ldb, nrhs, d_X, ldx, C.byref(info)), self._h)
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        return info.value

    # -- Fisher scoring on the device (src/workspace/gaussian_approximation.jl:191-313; include/gmrfx.h "Fisher scoring") ------
    OBS_FAMILIES = {"normal": 0, "poisson": 1, "bernoulli": 2, "binomial": 3, "negbin": 4, "gamma": 5}

    def set_observations(self, family, y, indices=None, aux=None, param: float = 0.0, index_base: int = 0) -> None:
        """The observation likelihood as state of the handle (gmrfx_obs_set). family: a name of OBS_FAMILIES or its id; y: one value
        per observation; indices: the observed nodes (None: every node in order); aux: log exposure (Poisson, NegBin) or trials
        (Binomial); param: sigma (Normal), r (NegBin), phi (Gamma). An empty y removes the likelihood."""
        fam = self.OBS_FAMILIES[family] if isinstance(family, str) else int(family)
        yy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        ax = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64).reshape(-1)
        if (idx is not None and idx.size != yy.size) or (ax is not None and ax.size != yy.size):
            raise ValueError("indices / aux do not have one entry per observation")
        check(lib().gmrfx_obs_set(self._h, fam, yy.size, ptr(idx), int(index_base), ptr(yy), ptr(ax), float(param)), self._h)

    def observations_info(self) -> dict:
        fam, nobs, c = C.c_int32(0), C.c_int64(0), C.c_double(0.0)
        check(lib().gmrfx_obs_info(self._h, C.byref(fam), C.byref(nobs), C.byref(c)), self._h)
        return {"family": fam.value, "nobs": nobs.value, "loglik_const": c.value}

    def set_design_observations(self, family, y, A, offset=None, aux=None, param: float = 0.0) -> None:
        """The likelihood observed through eta = A x + offset (gmrfx_obs_set_design; the reference's LinearlyTransformedLikelihood).
        A: any scipy sparse matrix, nobs x n, converted to sorted CSC (explicit zeros are kept, duplicates summed). The other
        arguments as in set_observations, one entry per row of A. set_prior then takes observations_hess_map()."""
        fam = self.OBS_FAMILIES[family] if isinstance(family, str) else int(family)
        yy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        Ac = sp.csc_matrix(A, dtype=np.float64)
        if Ac.shape != (yy.size, self.n):
            raise ValueError(f"A must be nobs x n = {yy.size} x {self.n}, got {Ac.shape}")
        if not Ac.has_canonical_format:
            Ac = Ac.copy()
            Ac.sum_duplicates()
        off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64).reshape(-1)
        ax = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64).reshape(-1)
        if (off is not None and off.size != yy.size) or (ax is not None and ax.size != yy.size):
            raise ValueError("offset / aux do not have one entry per observation")
        cp = np.ascontiguousarray(Ac.indptr, dtype=np.int64)
        rv = np.ascontiguousarray(Ac.indices, dtype=np.int64)
        nz = np.ascontiguousarray(Ac.data, dtype=np.float64)
        check(lib().gmrfx_obs_set_design(self._h, fam, yy.size, ptr(cp), ptr(rv), ptr(nz), 0, ptr(off), ptr(yy), ptr(ax), float(param)), self._h)

    def observations_hess_map(self) -> np.ndarray:
        """0-based positions into nzval of the entries of A' D A, ascending (gmrfx_obs_hess_map): the hess_map of set_prior, and the
        order of the Hessian values fisher_eval and gaussian_approximation return in design form."""
        cnt = C.c_int64(0)
        check(lib().gmrfx_obs_hess_map(self._h, C.byref(cnt), None), self._h)
        m = np.empty(cnt.value, np.int64)
        check(lib().gmrfx_obs_hess_map(self._h, C.byref(cnt), ptr(m)), self._h)
        return m

    def observations_design_info(self) -> dict:
        a, c, t = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().gmrfx_obs_design_info(self._h, C.byref(a), C.byref(c), C.byref(t)), self._h)
        return {"nnz": a.value, "cnt": c.value, "terms": t.value}

    def _hess_len(self) -> int:
        """entries of the Hessian vector of the evaluation: n in node form, the map's cnt in design form"""
        cnt = self.observations_design_info()["cnt"]
        return self.n if cnt < 0 else cnt

    def fisher_eval(self, x, mean=None, want_score: bool = True, want_hess: bool = True):
        """(score, hess, energy, loglik) at the point x (gmrfx_fisher_eval): score = Q_p x - Q_p mean - loggrad(x), hess = the diagonal
        of loghessian(x) (design form: the values of A' D A in the order of observations_hess_map()), energy = x' Q_p x / 2 -
        x' Q_p mean, loglik(x); Q_p = the values of set_prior. score / hess are None when not asked for."""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        mu = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        if xx.shape != (self.n,) or (mu is not None and mu.shape != (self.n,)):
            raise ValueError("dimension mismatch")
        score = np.empty(self.n) if want_score else None
        hess = np.empty(self._hess_len()) if want_hess else None
        out = np.empty(2)
        check(lib().gmrfx_fisher_eval(self._h, ptr(xx), ptr(mu), ptr(score), ptr(hess), ptr(out)), self._h)
        return score, hess, float(out[0]), float(out[1])

    def fisher_eval_dev(self, d_x: int, d_mu: int = 0, d_score: int = 0, d_hess: int = 0):
        """Device pointers: x (n), mean (n, 0 = zero), score (n) and hess (n; design form: cnt) outputs (0 = not computed); returns
        (energy, loglik)."""
        if not d_x:
            raise ValueError("fisher_eval_dev: null pointer")
        out = np.empty(2)
        check(lib().gmrfx_fisher_eval_dev(self._h, d_x, d_mu or None, d_score or None, d_hess or None, ptr(out)), self._h)
        return float(out[0]), float(out[1])

    @staticmethod
    def _ga_flags(adaptive_stepsize, step_recovery, predictive_convergence, refactorize_final):
        if step_recovery not in ("retry_full", "sqrt"):
            raise ValueError("step_recovery must be 'retry_full' or 'sqrt'")
        return int(adaptive_stepsize) | (int(step_recovery == "retry_full") << 1) | (int(predictive_convergence) << 2) | (int(refactorize_final) << 3)

    @staticmethod
    def _ga_info(res, dec, alp):
        used = ~np.isnan(dec)
        return {"iterations": int(res[0]), "converged": bool(res[1]), "alpha": float(res[2]), "newton_decrement": float(res[3]),
                "factorizations": int(res[4]), "solves": int(res[5]), "merit_evaluations": int(res[6]), "frozen_finish": bool(res[7]),
                "dec_trace": dec[used].copy(), "alpha_trace": alp[used].copy()}

    def gaussian_approximation(self, mean=None, x0=None, max_iter: int = 50, mean_change_tol: float = 1e-4, newton_dec_tol: float = 1e-5,
                               adaptive_stepsize: bool = True, max_linesearch_iter: int = 10, step_recovery: str = "retry_full",
                               predictive_convergence: bool = True, refactorize_final: bool = False):
        """The reference's gaussian_approximation(prior::WorkspaceGMRF, obs_lik) on the device (gmrfx_gaussian_approximation): prior =
        the values of set_prior with mean `mean`, likelihood = set_observations. Returns (mode, hess = the diagonal of
        loghessian(mode), info dict of the counters and the decrement / alpha traces). A failed factorisation raises PosDefException;
        last_info holds the failing step."""
        mu = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        xs = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64)
        if (mu is not None and mu.shape != (self.n,)) or (xs is not None and xs.shape != (self.n,)):
            raise ValueError("dimension mismatch")
        x, hess, res = np.empty(self.n), np.empty(self._hess_len()), np.zeros(8)
        dec, alp = np.full(max_iter + 1, np.nan), np.full(max_iter + 1, np.nan)
        info = C.c_int64(0)
        flags = self._ga_flags(adaptive_stepsize, step_recovery, predictive_convergence, refactorize_final)
        rc = lib().gmrfx_gaussian_approximation(self._h, ptr(mu), ptr(xs), max_iter, max_linesearch_iter, float(mean_change_tol),
                                                float(newton_dec_tol), flags, ptr(x), ptr(hess), ptr(res), ptr(dec), ptr(alp), C.byref(info))
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        self.last_x = x
        check(rc, self._h)
        return x, hess, self._ga_info(res, dec, alp)

    def gaussian_approximation_dev(self, d_x: int, d_hess: int = 0, d_mu: int = 0, d_x0: int = 0, max_iter: int = 50,
                                   mean_change_tol: float = 1e-4, newton_dec_tol: float = 1e-5, adaptive_stepsize: bool = True,
                                   max_linesearch_iter: int = 10, step_recovery: str = "retry_full", predictive_convergence: bool = True,
                                   refactorize_final: bool = False) -> dict:
        """Device pointers: the mode x (n) and hess (n; design form: cnt; 0 = not wanted) outputs, mean and x0 (n each, 0 = none).
        Returns the info dict."""
        if not d_x:
            raise ValueError("gaussian_approximation_dev: null pointer")
        res = np.zeros(8)
        dec, alp = np.full(max_iter + 1, np.nan), np.full(max_iter + 1, np.nan)
        info = C.c_int64(0)
        flags = self._ga_flags(adaptive_stepsize, step_recovery, predictive_convergence, refactorize_final)
        rc = lib().gmrfx_gaussian_approximation_dev(self._h, d_mu or None, d_x0 or None, max_iter, max_linesearch_iter, float(mean_change_tol),
                                                    float(newton_dec_tol), flags, d_x, d_hess or None, ptr(res), ptr(dec), ptr(alp), C.byref(info))
        self._selinv_cache = None
        self._selinv_diag_cache = None
        self.last_info = info.value
        check(rc, self._h)
        return self._ga_info(res, dec, alp)

    # -- the pullback of gaussian_approximation (src/workspace/autodiff.jl:140-202; include/gmrfx.h "The pullback of the Gaussian approximation")
    def ga_pullback(self, x, mean=None, mubar=None, Qbar=None, project: bool = False, refactorize: bool = False,
                    want_Qbar_prior: bool = True, want_mubar_prior: bool = True, want_lambda: bool = True):
        """The implicit-function rule at the mode x (gmrfx_ga_pullback). mubar (n) / Qbar (nnz, on the pattern, the convention of
        logpdf_grad): the cotangents of the posterior mean / precision, either None (zero). Returns (Qbar_prior, mubar_prior, lambda,
        param_bar, lambda' xbar); the arrays not asked for are None. project: lambda <- lambda - A~' W^-1 (A lambda) with the
        constraint set; refactorize: factorise Q_prior - H(x) first (otherwise the handle holds it: gaussian_approximation with
        refactorize_final=True)."""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        mu = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        mb = None if mubar is None else np.ascontiguousarray(mubar, dtype=np.float64)
        qb = None if Qbar is None else np.ascontiguousarray(Qbar, dtype=np.float64)
        if xx.shape != (self.n,) or any(v is not None and v.shape != (self.n,) for v in (mu, mb)) or (qb is not None and qb.shape != (self._nnz,)):
            raise ValueError("dimension mismatch")
        qp = np.empty(self._nnz) if want_Qbar_prior else None
        mp = np.empty(self.n) if want_mubar_prior else None
        lam = np.empty(self.n) if want_lambda else None
        out = np.empty(2)
        flags = int(bool(project)) | (int(bool(refactorize)) << 1)
        rc = lib().gmrfx_ga_pullback(self._h, ptr(xx), ptr(mu), ptr(mb), ptr(qb), flags, ptr(qp), ptr(mp), ptr(lam), ptr(out))
        if refactorize:
            self._selinv_cache = None
            self._selinv_diag_cache = None
        check(rc, self._h)
        return qp, mp, lam, float(out[0]), float(out[1])

    def ga_pullback_dev(self, d_x: int, d_mu: int = 0, d_mubar: int = 0, d_Qbar: int = 0, d_Qbar_prior: int = 0, d_mubar_prior: int = 0,
                        d_lambda: int = 0, project: bool = False, refactorize: bool = False):
        """Device pointers (0 = absent); d_Qbar_prior may be d_Qbar. Returns (param_bar, lambda' xbar)."""
        if not d_x:
            raise ValueError("ga_pullback_dev: null pointer")
        out = np.empty(2)
        flags = int(bool(project)) | (int(bool(refactorize)) << 1)
        rc = lib().gmrfx_ga_pullback_dev(self._h, d_x, d_mu or None, d_mubar or None, d_Qbar or None, flags, d_Qbar_prior or None,
                                         d_mubar_prior or None, d_lambda or None, ptr(out))
        if refactorize:
            self._selinv_cache = None
            self._selinv_diag_cache = None
        check(rc, self._h)
        return float(out[0]), float(out[1])

    def observations_design_rows(self):
        """(ptr, pos, w): the design plan's terms by observation (gmrfx_obs_design_rows) -- row i's pairs at ptr[i] .. ptr[i + 1] as
        0-based positions into nzval, ascending, and weights A_ij A_ik, doubled off the diagonal."""
        terms = self.observations_design_info()["terms"]
        nobs = self.observations_info()["nobs"]
        p, pos, w = np.empty(nobs + 1, np.int64), np.empty(max(terms, 0), np.int64), np.empty(max(terms, 0))
        check(lib().gmrfx_obs_design_rows(self._h, ptr(p), ptr(pos), ptr(w)), self._h)
        return p, pos, w

    # -- the linear predictor's marginals and the predictive scores (src/linear_predictor_marginals.jl:58-195; include/gmrfx.h
    # "Linear-predictor marginals and predictive scores")
    def observations_pointwise_const(self) -> np.ndarray:
        """c_i: the terms of every observation's log density that do not depend on x (gmrfx_obs_pointwise_const); no device needed."""
        c = np.empty(self.observations_info()["nobs"])
        check(lib().gmrfx_obs_pointwise_const(self._h, ptr(c)), self._h)
        return c

    def predictor_marginals(self, x, constraint_correction: bool = False, want_mean: bool = True, want_var: bool = True,
                            want_pll: bool = True):
        """(mu_eta, v_eta, pll) per observation in the caller's order (gmrfx_predictor_marginals): mean and variance of the linear
        predictor under N(x, Sigma) with Sigma the inverse of the matrix the handle holds factorised (gaussian_approximation with
        refactorize_final=True leaves Q_post), and the full log density at the mean. constraint_correction: subtract the constraint's
        term from the variance and clamp at 0. The arrays not asked for are None."""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        if xx.shape != (self.n,):
            raise ValueError("dimension mismatch")
        nobs = self.observations_info()["nobs"]
        mu = np.empty(nobs) if want_mean else None
        v = np.empty(nobs) if want_var else None
        pll = np.empty(nobs) if want_pll else None
        check(lib().gmrfx_predictor_marginals(self._h, ptr(xx), int(bool(constraint_correction)), ptr(mu), ptr(v), ptr(pll)), self._h)
        return mu, v, pll

    def predictor_marginals_dev(self, d_x: int, d_mu_eta: int = 0, d_v_eta: int = 0, d_pll: int = 0, constraint_correction: bool = False) -> None:
        """Device pointers: x (n) and the outputs (nobs each, 0 = not computed)."""
        if not d_x:
            raise ValueError("predictor_marginals_dev: null pointer")
        check(lib().gmrfx_predictor_marginals_dev(self._h, d_x, int(bool(constraint_correction)), d_mu_eta or None, d_v_eta or None,
                                                  d_pll or None), self._h)

    @staticmethod
    def gauss_hermite(K: int):
        """(nodes, weights) of the K-point Gauss-Hermite rule for the standard normal, the weights divided by their sum."""
        z, w = np.polynomial.hermite_e.hermegauss(int(K))
        return np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(w / w.sum(), dtype=np.float64)

    @staticmethod
    def _score_totals(out):
        return {"lpd": float(out[0]), "lcpo": float(out[1]), "elp": float(out[2]), "p_waic": float(out[3]),
                "waic": float(-2.0 * (out[0] - out[3]))}

    def predictive_scores(self, mu_eta, v_eta, nodes, weights, want_arrays: bool = True):
        """((lpd, lcpo, elp, vlp), totals) over eta_i ~ N(mu_eta_i, v_eta_i) with the caller's quadrature rule of the standard normal
        (gmrfx_predictive_scores; gauss_hermite(K) gives one): log pointwise predictive density, log CPO, expected log density and
        its variance per observation, and the dict of their totals lpd, lcpo, elp, p_waic, waic = -2 (lpd - p_waic)."""
        mu = np.ascontiguousarray(mu_eta, dtype=np.float64)
        v = np.ascontiguousarray(v_eta, dtype=np.float64)
        z = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        nobs = self.observations_info()["nobs"]
        if mu.shape != (nobs,) or v.shape != (nobs,) or z.shape != w.shape:
            raise ValueError("dimension mismatch")
        arrs = tuple(np.empty(nobs) for _ in range(4)) if want_arrays else (None,) * 4
        out = np.empty(4)
        check(lib().gmrfx_predictive_scores(self._h, ptr(mu), ptr(v), z.size, ptr(z), ptr(w), *(ptr(a) for a in arrs), ptr(out)), self._h)
        return arrs, self._score_totals(out)

    def predictive_scores_dev(self, d_mu_eta: int, d_v_eta: int, nodes, weights, d_lpd: int = 0, d_lcpo: int = 0, d_elp: int = 0,
                              d_vlp: int = 0) -> dict:
        """Device pointers for mu_eta, v_eta and the outputs (nobs each; 0 = not wanted); nodes and weights on the host. Returns the
        totals."""
        if not d_mu_eta or not d_v_eta:
            raise ValueError("predictive_scores_dev: null pointer")
        z = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if z.shape != w.shape:
            raise ValueError("dimension mismatch")
        out = np.empty(4)
        check(lib().gmrfx_predictive_scores_dev(self._h, d_mu_eta, d_v_eta, z.size, ptr(z), ptr(w), d_lpd or None, d_lcpo or None,
                                                d_elp or None, d_vlp or None, ptr(out)), self._h)
        return self._score_totals(out)

    # -- sharded factorisation (include/gmrfx.h "sharded factorisation"; driver: gmrfx/shard.py) -------
    def refactorize_phase_dev(self, d_nzval_ptr: int, phase: int) -> None:
        check(lib().gmrfx_refactorize_phase(self._h, d_nzval_ptr, phase), self._h)

    def shard_info(self) -> dict:
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().gmrfx_shard_info(self._h, C.byref(a), C.byref(b), C.byref(c)), self._h)
        st = self.stats()
        return {"n_edges": a.value, "n_top_fronts": b.value, "shard_level": c.value, "n_top_levels": int(st["nlevels"] - c.value)}

    def shard_edges(self) -> dict:
        """Cross-rank tree edges child -> parent, ordered by the level of the parent: child, src (owner of the
        child), dst (owner of the parent), level, and where the child's contribution block / update vector live
        (offset + count in doubles into device_ptr(0); first row + rows of device_ptr(3))."""
        k = self.shard_info()["n_edges"]
        names = ("child", "src", "dst", "level", "cb_offset", "cb_count", "w_row0", "w_nrows", "zb_offset", "child_level")
        arr = {nm: np.zeros(k, np.int64) for nm in names}
        if k:
            check(lib().gmrfx_shard_edges(self._h, *[ptr(arr[nm]) for nm in names]), self._h)
        return arr

    def selinv_phase(self, what: int, hi: int = 0, lo: int = 0) -> None:
        """Sharded selected inversion (include/gmrfx.h): 0 begin, 1 gather for other ranks at level hi, 2 own levels hi-1..lo, 3 end."""
        self._selinv_cache = None
        self._selinv_diag_cache = None
        check(lib().gmrfx_selinv_phase(self._h, what, hi, lo), self._h)

    def shard_owner(self, with_top: bool = False):
        ns = self.stats()["nsuper"]
        out, top = np.zeros(ns, np.int64), np.zeros(ns, np.int64)
        check(lib().gmrfx_shard_owner(self._h, ptr(out), ptr(top)), self._h)
        return (out, top.astype(bool)) if with_top else out

    def solve_phase_dev(self, d_B: int, ldb: int, nrhs: int, d_X: int, ldx: int, phase: int) -> None:
        check(lib().gmrfx_solve_phase(self._h, d_B, ldb, nrhs, d_X, ldx, phase), self._h)

    def shard_rows(self, kind: int):
        """(owner, first row, rows, level) of the X row blocks the sharded solve moves (2: own columns of the top
        fronts, broadcast by their owners; 3: columns of the assigned subtrees, gathered on rank 0)."""
        k = C.c_int64(0)
        check(lib().gmrfx_shard_rows(self._h, kind, C.byref(k), None, None, None, None), self._h)
        owner, r0, nr, lv = (np.zeros(k.value, np.int64) for _ in range(4))
        if k.value:
            check(lib().gmrfx_shard_rows(self._h, kind, C.byref(k), ptr(owner), ptr(r0), ptr(nr), ptr(lv)), self._h)
        return owner, r0, nr, lv

    def shard_dist_fronts(self) -> dict:
        """The distributed top fronts of a sharded handle (csrc/symbolic.h: Symbolic::dist_fronts): per front its supernode,
        columns, rows, the panel's place in device_ptr(1), tree level and GROUP (the ranks that factor it together: panel block b
        of 256 columns on group[b % g], contribution-block block q on group[(panel blocks + q) % g])."""
        cnt = np.zeros(4, np.int64)
        check(lib().gmrfx_shard_dist_fronts(self._h, ptr(cnt), *([None] * 8)))
        nf, ng = int(cnt[0]), int(cnt[1])
        a = {nm: np.empty(nf, np.int64) for nm in ("front", "cols", "rows", "panel_offset", "panel_ld", "level")}
        gptr, grank = np.zeros(nf + 1, np.int64), np.empty(ng, np.int64)
        check(lib().gmrfx_shard_dist_fronts(self._h, ptr(cnt), *[ptr(a[nm]) for nm in ("front", "cols", "rows", "panel_offset", "panel_ld", "level")],
                                            ptr(gptr), ptr(grank)))
        a["group"] = [[int(r) for r in grank[gptr[k]:gptr[k + 1]]] for k in range(nf)]
        a["world"] = int(cnt[3])
        return a

    def shard_transfers(self) -> dict:
        """Every contribution-block transfer of the sharded factorisation (whole columns of `child`'s block: `count` doubles at
        `offset` of device_ptr(0), src -> dst, before the fronts of `level` are assembled), ordered by level."""
        cnt = np.zeros(4, np.int64)
        check(lib().gmrfx_shard_dist_fronts(self._h, ptr(cnt), *([None] * 8)))
        k = int(cnt[2])
        names = ("child", "src", "dst", "level", "offset", "count", "col0")
        a = {nm: np.empty(k, np.int64) for nm in names}
        check(lib().gmrfx_shard_transfers(self._h, *[ptr(a[nm]) for nm in names]))
        return a

    def dist_front_phase(self, d_nzval_ptr: int, front: int, what: int, block: int = 0) -> None:
        check(lib().gmrfx_dist_front_phase(self._h, d_nzval_ptr, front, what, block), self._h)

    def set_stream(self, hip_stream: int, use_external: bool = True, async_phases: bool = False) -> None:
        """The caller's HIP stream becomes the handle's main stream (sharded drivers: torch's current stream)."""
        check(lib().gmrfx_set_stream(self._h, C.c_void_p(int(hip_stream)), int(use_external), int(async_phases)), self._h)

    def level_times(self, which: int) -> np.ndarray:
        """ms per tree level of the last factorisation (0) / forward (1) / backward (2) sweep ([0] = the sweep tasks); empty
        unless the handle was created under GMRFX_LEVEL_MARK=1."""
        out = np.zeros(int(self.stats()["nlevels"]) + 1)
        cnt = C.c_int64(0)
        check(lib().gmrfx_level_times(self._h, which, ptr(out), out.size, C.byref(cnt)), self._h)
        return out[:cnt.value]

    def dist_front_block(self, front: int, block: int):
        """(offset, count) in doubles of THIS rank's copy of panel block `block` of the distributed front `front` inside
        device_ptr(1): the whole panel on the front's owner, own blocks + a two-block window on a member with block-cyclic storage"""
        off, cnt = C.c_int64(0), C.c_int64(0)
        check(lib().gmrfx_dist_front_block(self._h, int(front), int(block), C.byref(off), C.byref(cnt)), self._h)
        return off.value, cnt.value

    def device_ptr(self, which: int) -> int:
        return int(lib().gmrfx_device_ptr(self._h, which) or 0)

    def logdet_partial(self) -> float:
        out = C.c_double(0.0)
        check(lib().gmrfx_logdet_partial(self._h, C.byref(out)), self._h)
        return out.value

    def solve_dev(self, d_B: int, ldb: int, nrhs: int, d_X: int, ldx: int) -> None:
        check(lib().gmrfx_solve_dev(self._h, d_B, ldb, nrhs, d_X, ldx), self._h)

    def backward_solve_dev(self, d_Z: int, ldz: int, nrhs: int, d_X: int, ldx: int) -> None:
        check(lib().gmrfx_backward_solve_dev(self._h, d_Z, ldz, nrhs, d_X, ldx), self._h)

    def quadform_dev(self, d_nzval: int, d_X: int, ldx: int, nvec: int, d_mu: int = 0) -> np.ndarray:
        """Device-pointer form of sqmahal; d_nzval / d_mu may be 0 (see gmrfx_quadform_dev)."""
        out = np.empty(nvec)
        check(lib().gmrfx_quadform_dev(self._h, d_nzval or None, d_X, ldx, nvec, d_mu or None, ptr(out)), self._h)
        return out

    def selinv_compute_dev(self) -> None:
        check(lib().gmrfx_selinv_compute(self._h), self._h)

    # -- linear equality constraints A x = e, computed on the device (include/gmrfx.h "linear equality constraints") ------------
    def set_constraints(self, A, e) -> None:
        """`ConstraintInfo(ws, mu, A, e)`'s A and e (workspace_gmrf.jl:22-40) become state of the handle: m <= 64 sparse rows.
        Everything derived (A~' = Q^-1 A', W = A A~', L_c, B) is built lazily on the device, once per factorisation."""
        A = sp.csr_matrix(A, dtype=np.float64)
        e = np.ascontiguousarray(e, dtype=np.float64).reshape(-1)
        if A.shape[1] != self.n:
            raise ValueError(f"Constraint matrix size {A.shape} incompatible with workspace size {self.n}")
        if A.shape[0] != e.shape[0]:
            raise ValueError(f"Constraint matrix rows {A.shape[0]} != constraint vector length {e.shape[0]}")
        self.set_constraints_csr(A.shape[0], A.indptr, A.indices, A.data, e)

    def set_constraints_csr(self, m: int, rowptr, colind, values, e) -> None:
        """The raw form: CSR arrays as given (0-based), checked by the library."""
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        ci = np.ascontiguousarray(colind, dtype=np.int64)
        va = np.ascontiguousarray(values, dtype=np.float64)
        ev = np.ascontiguousarray(e, dtype=np.float64)
        if rp.shape != (m + 1,) or ev.shape != (m,) or ci.shape != va.shape or (m > 0 and ci.shape[0] < rp[-1]):
            raise ValueError("constraints: array lengths do not match m")
        check(lib().gmrfx_constraints_set(self._h, m, ptr(rp), ptr(ci), ptr(va), 0, ptr(ev)), self._h)

    def clear_constraints(self) -> None:
        check(lib().gmrfx_constraints_set(self._h, 0, None, None, None, 0, None), self._h)

    def constraint_info(self) -> dict:
        """m, log det(A A') and -- on a numeric handle, building the cached operands if needed -- log det W = logdet(L_c) and the
        GPU time of the most recent preparation."""
        m, ldw, lda, ms = C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        if self.symbolic_only:
            check(lib().gmrfx_constraints_info(self._h, C.byref(m), None, C.byref(lda), None), self._h)
            return {"m": m.value, "logdet_AAt": lda.value}
        check(lib().gmrfx_constraints_info(self._h, C.byref(m), C.byref(ldw), C.byref(lda), C.byref(ms)), self._h)
        return {"m": m.value, "logdet_W": ldw.value, "logdet_AAt": lda.value, "ms": ms.value}

    def _con_m(self) -> int:
        m = C.c_int64(0)
        check(lib().gmrfx_constraints_info(self._h, C.byref(m), None, None, None), self._h)
        return m.value

    def constraint_fields(self):
        """(A_tilde_T, W): the n x m solve Q^-1 A' and W = A A~' (ConstraintInfo.A_tilde_T; L_c = cholesky(Symmetric(W)))."""
        m = self._con_m()
        At = np.empty((self.n, m), order="F")
        W = np.empty((m, m), order="F")
        check(lib().gmrfx_constraints_get(self._h, ptr(At), self.n, ptr(W)), self._h)
        return At, W

    def constrained_mean(self, mu=None):
        """(mean_c, log_constraint_correction) of workspace_gmrf.jl:43-51; mu None = zero mean."""
        mu = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64)
        if mu is not None and mu.shape != (self.n,):
            raise ValueError("dimension mismatch")
        out = np.empty(self.n)
        lc = C.c_double(0.0)
        check(lib().gmrfx_constraints_mean(self._h, ptr(mu), ptr(out), C.byref(lc)), self._h)
        return out, lc.value

    def constrained_var(self) -> np.ndarray:
        """var(d) of workspace_gmrf.jl:260-273: max(diag Sigma - rowsum(B^2), 0); without constraints = get_selinv_diag()."""
        out = np.empty(self.n)
        check(lib().gmrfx_constraints_var(self._h, ptr(out)), self._h)
        return out

    def constraint_correct(self, X):
        """x - A~' (L_c \\ (A x - e)) on every column (workspace_gmrf.jl:280-284). Returns a fresh array; input untouched."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim not in (1, 2) or X.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        vec = X.ndim == 1
        Xf = np.array(X.reshape(self.n, -1), order="F", copy=True)
        check(lib().gmrfx_constraints_correct(self._h, ptr(Xf), self.n, Xf.shape[1]), self._h)
        return Xf[:, 0].copy() if vec else Xf

    def constraint_correct_dev(self, d_X: int, ldx: int, nvec: int) -> None:
        if nvec < 0 or (nvec > 0 and (not d_X or ldx < self.n)):
            raise ValueError("constraint_correct_dev: null pointer, nvec < 0 or ldx < n")
        check(lib().gmrfx_constraints_correct_dev(self._h, d_X, ldx, nvec), self._h)

    def sample(self, Z, mean=None):
        """`_rand!` on given standard-normal draws (workspace_gmrf.jl:275-286): P' L^-T Z + mean, then the constraint correction."""
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim not in (1, 2) or Z.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        mu = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        if mu is not None and mu.shape != (self.n,):
            raise ValueError("dimension mismatch")
        vec = Z.ndim == 1
        Zf = np.asfortranarray(Z.reshape(self.n, -1))
        X = np.empty_like(Zf, order="F")
        check(lib().gmrfx_sample(self._h, ptr(Zf), self.n, Zf.shape[1], ptr(mu), ptr(X), self.n), self._h)
        return X[:, 0].copy() if vec else X

    def sample_dev(self, d_Z: int, ldz: int, nrhs: int, d_X: int, ldx: int, d_mu: int = 0) -> None:
        if nrhs < 0 or (nrhs > 0 and (not d_Z or not d_X or ldz < self.n or ldx < self.n)):
            raise ValueError("sample_dev: null pointer, nrhs < 0 or leading dimension < n")
        check(lib().gmrfx_sample_dev(self._h, d_Z, ldz, nrhs, d_mu or None, d_X, ldx), self._h)

    # -- Rao-Blackwellised Monte Carlo marginal variances (src/solvers/rbmc.jl) -----------------------------------------------
    def rbmc_var(self, Z, enclosure_size: int = -1, nzval=None) -> np.ndarray:
        """`var(d, RBMCStrategy(k))` (enclosure_size = -1) / `var(d, BlockRBMCStrategy(k; enclosure_size))` on the standard normals
        Z (n, k) the caller drew. nzval: Q's values in the pattern's order; None = the values of the last refactorisation."""
        return _rbmc_var(self._h, self.n, self._nnz, Z, enclosure_size, nzval)

    def rbmc_var_dev(self, d_Z: int, ldz: int, nsamples: int, d_out: int, enclosure_size: int = -1, d_nzval: int = 0) -> None:
        if not d_Z or not d_out:
            raise ValueError("rbmc_var_dev: null pointer")
        check(lib().gmrfx_rbmc_var_dev(self._h, d_nzval or None, d_Z, ldz, nsamples, int(enclosure_size), d_out), self._h)

    def rbmc_plan(self, enclosure_size: int, index_base: int = 0) -> dict:
        return _rbmc_plan(self._h, enclosure_size, index_base)

    # -- log-density gradients on Q's own pattern (src/autodiff/logpdf.jl, src/workspace/autodiff.jl) ---------------------------
    def logpdf_grad(self, z, mean=None, ybar: float = 1.0, nzval=None):
        """The pullback of logpdf (+ log_correction with a constraint set) at cotangent ybar: (Qbar, mubar) with Qbar a csc matrix on
        Q's own pattern and mubar (n,); zbar = -mubar. nzval: Q's values in the pattern's order; None = the values of the last
        refactorisation."""
        zz = np.ascontiguousarray(z, dtype=np.float64)
        mu = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        if zz.shape != (self.n,) or (mu is not None and mu.shape != (self.n,)):
            raise ValueError("dimension mismatch")
        nz = None if nzval is None else np.ascontiguousarray(nzval, dtype=np.float64)
        if nz is not None and nz.shape != (self._nnz,):
            raise ValueError("nzval length does not match the pattern")
        qbar, mubar = np.empty(self._nnz), np.empty(self.n)
        check(lib().gmrfx_logpdf_grad(self._h, ptr(nz), ptr(zz), ptr(mu), float(ybar), ptr(qbar), ptr(mubar)), self._h)
        return sp.csc_matrix((qbar, self._rowval.copy(), self._colptr.copy()), shape=(self.n, self.n)), mubar

    def logpdf_grad_dev(self, d_z: int, d_Qbar: int = 0, d_mubar: int = 0, d_mu: int = 0, ybar: float = 1.0, d_nzval: int = 0) -> None:
        """Device pointers: z (n), Qbar (nnz) and mubar (n) outputs (0 = not computed, not both), mu (n, 0 = zero mean), Q's values."""
        if not d_z or (not d_Qbar and not d_mubar):
            raise ValueError("logpdf_grad_dev: null pointer")
        check(lib().gmrfx_logpdf_grad_dev(self._h, d_nzval or None, d_z, d_mu or None, float(ybar), d_Qbar or None, d_mubar or None), self._h)

    def pattern_dot(self, G, J) -> np.ndarray:
        """out[k] = sum_e w_e G[e] J[e, k] over the stored entries of Q (w_e: the Symmetric(Q) weights of sqmahal): dlogpdf/dtheta_k
        from G = Qbar's values (nnz,) or a csc matrix on Q's pattern, and the Jacobian J (nnz, p) of Q's values."""
        g = np.ascontiguousarray(G.data if sp.issparse(G) else G, dtype=np.float64)
        Jf = np.asarray(J, dtype=np.float64)
        if g.shape != (self._nnz,) or Jf.shape[0] != self._nnz or Jf.ndim > 2:
            raise ValueError("G must have nnz values and J nnz rows")
        Jf = np.asfortranarray(Jf.reshape(self._nnz, -1))
        if Jf.shape[1] < 1:
            raise ValueError("J must have at least one column")
        out = np.empty(Jf.shape[1])
        check(lib().gmrfx_pattern_dot(self._h, ptr(g), ptr(Jf), max(self._nnz, 1), Jf.shape[1], ptr(out)), self._h)
        return out

    def pattern_dot_dev(self, d_G: int, d_J: int, ldj: int, p: int) -> np.ndarray:
        if not d_G or not d_J or p < 1 or ldj < self._nnz:
            raise ValueError("pattern_dot_dev: null pointer, p < 1 or ldj < nnz")
        out = np.empty(p)
        check(lib().gmrfx_pattern_dot_dev(self._h, d_G, d_J, ldj, p, ptr(out)), self._h)
        return out


class MI355XBatchBackend:
    """B precision matrices with ONE pattern, factored in one pass (gmrfx_create_batched, include/gmrfx.h): the hyper-parameter
    loop of docs/src/literate-tutorials/workspace_factorization_reuse.jl evaluates logpdf for many values of one pattern, and
    WorkspacePool (src/workspace/workspace_pool.jl:5-22) runs such evaluations side by side. The handle is an ordinary handle of
    diag(Q_1 .. Q_B); the member's order is computed once (ordering / coords as in MI355XBackend) and replicated.

    Shapes: member values NZ (nnz, B) (column k = Q_k's values in Q's CSC order); right-hand sides (n, B) or (n, r, B); results in
    the same layout. Every shape is checked (ValueError) before the library is called."""

    def __init__(self, Q, nbatch: int, ordering=None, coords=None, device: int = -1, symbolic_only: bool = False,
                 check_posdef: bool = False, uplo: str = "U"):
        Q = _as_csc(Q)
        if isinstance(nbatch, bool) or not isinstance(nbatch, (int, np.integer)):
            raise ValueError("nbatch must be an integer")
        self.n = Q.shape[0]
        self.nbatch = int(nbatch)
        self._colptr = np.ascontiguousarray(Q.indptr, dtype=np.int64)
        self._rowval = np.ascontiguousarray(Q.indices, dtype=np.int64)
        self._nnz = int(self._colptr[-1])
        opts = GmrfxOpts()
        opts.struct_size = C.sizeof(GmrfxOpts)
        opts.uplo = 0 if uplo.upper().startswith("U") else 1
        opts.device = device
        opts.symbolic_only = int(symbolic_only)
        opts.check_posdef = int(check_posdef)
        self.device, self.symbolic_only = device, symbolic_only
        from .ordering import ordering_permutation as _resolve
        perm = _resolve(Q, ordering, coords)
        if isinstance(perm, str):           # "natural"
            opts.ordering = 1
            perm = None
        cr = None
        if coords is not None:
            cr = np.ascontiguousarray(coords, dtype=np.float64)
            if cr.ndim != 2 or cr.shape[0] != self.n:
                raise ValueError("coords must be n x dim")
            opts.coord_dim = cr.shape[1]
            opts.coords = cr.ctypes.data
        h = C.c_void_p()
        check(lib().gmrfx_create_batched(self.n, ptr(self._colptr), ptr(self._rowval), 0, ptr(perm), self.nbatch, C.byref(opts),
                                         C.byref(h)))
        self._h = h
        self._info = np.zeros(self.nbatch, np.int64)

    # -- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib().gmrfx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone(self) -> "MI355XBatchBackend":
        other = object.__new__(MI355XBatchBackend)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        other._info = self._info.copy()
        h = C.c_void_p()
        check(lib().gmrfx_clone(self._h, C.byref(h)))
        other._h = h
        return other

    # -- shape checks (before any ctypes call) ---------------------------------------------
    def _values(self, NZ) -> np.ndarray:
        NZ = np.asarray(NZ, dtype=np.float64)
        if NZ.shape != (self._nnz, self.nbatch):
            raise ValueError(f"NZ must have shape (nnz, nbatch) = ({self._nnz}, {self.nbatch}), got {NZ.shape}")
        return np.asfortranarray(NZ)

    def _members(self, R, what: str):
        """(n, B) or (n, r, B) -> Fortran array, columns per member, member stride"""
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 2 and R.shape == (self.n, self.nbatch):
            return np.asfortranarray(R), 1, self.n
        if R.ndim == 3 and R.shape[0] == self.n and R.shape[2] == self.nbatch:
            return np.asfortranarray(R), R.shape[1], self.n * R.shape[1]
        raise ValueError(f"{what} must have shape (n, nbatch) or (n, r, nbatch) with n = {self.n}, nbatch = {self.nbatch}, got {R.shape}")

    def _mean(self, mean):
        if mean is None:
            return None
        mu = np.asarray(mean, dtype=np.float64)
        if mu.shape == (self.n,):
            mu = np.repeat(mu[:, None], self.nbatch, axis=1)
        if mu.shape != (self.n, self.nbatch):
            raise ValueError(f"mean must have shape (n,) or (n, nbatch), got {mu.shape}")
        return np.asfortranarray(mu)

    # -- numeric ---------------------------------------------------------------------------
    def refactorize_values(self, NZ) -> np.ndarray:
        """All members from their values; returns info (B,): 0, or 1 + the member's first failing pivot (elimination order)."""
        nz = self._values(NZ)
        info = np.zeros(self.nbatch, np.int64)
        code = lib().gmrfx_batch_refactorize(self._h, ptr(nz), ptr(info))
        self._info = info
        check(code, self._h)
        return info.copy()

    def info(self) -> np.ndarray:
        return self._info.copy()

    def logdet(self) -> np.ndarray:
        out = np.empty(self.nbatch)
        check(lib().gmrfx_batch_logdet(self._h, ptr(out)), self._h)
        return out

    def _solve(self, R, name: str):
        Rf, r, s = self._members(R, "R" if name == "gmrfx_batch_solve" else "Z")
        X = np.empty_like(Rf, order="F")
        check(getattr(lib(), name)(self._h, Rf.ctypes.data, self.n, s, r, X.ctypes.data, self.n, s), self._h)
        return X

    def solve(self, R) -> np.ndarray:
        """X_k = Q_k^-1 R_k for R of shape (n, B) or (n, r, B)."""
        return self._solve(R, "gmrfx_batch_solve")

    def backward_solve(self, Z) -> np.ndarray:
        """X_k = P' L_k^-T Z_k (samples of member k) for Z of shape (n, B) or (n, r, B)."""
        return self._solve(Z, "gmrfx_batch_backward_solve")

    def sqmahal(self, X, mean=None, nzval=None) -> np.ndarray:
        """(x_vk - mu_k)' Q_k (x_vk - mu_k): X (n, B) -> (1, B), X (n, nvec, B) -> (nvec, B). mean: (n,) for every member or
        (n, B); nzval: (nnz, B), None = the values of the last refactorize_values."""
        Xf, nvec, s = self._members(X, "X")
        mu = self._mean(mean)
        nz = None if nzval is None else self._values(nzval)
        out = np.empty((nvec, self.nbatch), order="F")
        check(lib().gmrfx_batch_quadform(self._h, ptr(nz), ptr(Xf), self.n, s, nvec, ptr(mu), out.ctypes.data), self._h)
        return out

    def refactorize_logpdf(self, NZ, X, mean=None):
        """The logpdf terms of every member with new values: (logdet (B,), quad (nvec, B), info (B,));
        logpdf_k = -quad / 2 + logdet_k / 2 - n log(2 pi) / 2 (workspace_gmrf.jl:288-292)."""
        nz = self._values(NZ)
        Xf, _, _ = self._members(X, "X")
        mu = self._mean(mean)
        info = self.refactorize_values(nz)
        return self.logdet(), self.sqmahal(Xf, mu), info

    def selinv_diag(self) -> np.ndarray:
        """diag(Q_k^-1) of every member: (n, B)."""
        out = np.empty((self.n, self.nbatch), order="F")
        check(lib().gmrfx_selinv_diag(self._h, out.ctypes.data), self._h)
        return out

    # -- extras ----------------------------------------------------------------------------
    def batch_size(self):
        nb, nm = C.c_int64(0), C.c_int64(0)
        check(lib().gmrfx_batch_size(self._h, C.byref(nb), C.byref(nm)))
        return nb.value, nm.value

    def ordering_permutation(self) -> np.ndarray:
        """The MEMBER's elimination order (0-based); the handle's is this one replicated with offsets k n."""
        p = np.empty(self.n * self.nbatch, np.int64)
        check(lib().gmrfx_get_perm(self._h, 0, ptr(p)))
        return p[:self.n].copy()

    def forest_permutation(self) -> np.ndarray:
        p = np.empty(self.n * self.nbatch, np.int64)
        check(lib().gmrfx_get_perm(self._h, 0, ptr(p)))
        return p

    def stats(self) -> dict:
        st = GmrfxStats()
        check(lib().gmrfx_get_stats(self._h, C.byref(st), C.sizeof(GmrfxStats)))
        return st.asdict()

    def factor_values(self) -> np.ndarray:
        sizes = np.zeros(8, np.int64)
        check(lib().gmrfx_symbolic_sizes(self._h, ptr(sizes)))
        out = np.empty(int(sizes[2]))
        check(lib().gmrfx_get_factor_values(self._h, ptr(out)), self._h)
        return out

    # -- device-resident entry points (HBM in, HBM out) -------------------------------------
    def refactorize_dev(self, d_nzval: int) -> np.ndarray:
        info = np.zeros(self.nbatch, np.int64)
        code = lib().gmrfx_batch_refactorize_dev(self._h, d_nzval, ptr(info))
        self._info = info
        check(code, self._h)
        return info.copy()

    def solve_dev(self, d_B: int, ldb: int, sb: int, nrhs: int, d_X: int, ldx: int, sx: int) -> None:
        check(lib().gmrfx_batch_solve_dev(self._h, d_B, ldb, sb, nrhs, d_X, ldx, sx), self._h)

    def backward_solve_dev(self, d_Z: int, ldz: int, sz: int, nrhs: int, d_X: int, ldx: int, sx: int) -> None:
        check(lib().gmrfx_batch_backward_solve_dev(self._h, d_Z, ldz, sz, nrhs, d_X, ldx, sx), self._h)

    def quadform_dev(self, d_nzval: int, d_X: int, ldx: int, sx: int, nvec: int, d_mu: int = 0) -> np.ndarray:
        out = np.empty((max(nvec, 0), self.nbatch), order="F")
        check(lib().gmrfx_batch_quadform_dev(self._h, d_nzval or None, d_X, ldx, sx, nvec, d_mu or None, out.ctypes.data), self._h)
        return out

    def refactorize_logpdf_dev(self, d_nzval: int, d_X: int, ldx: int, sx: int, nvec: int, d_mu: int = 0):
        """gmrfx_batch_refactorize_logpdf_dev: (logdet (B,), quad (nvec, B), info (B,)) in one call, one synchronisation."""
        quad = np.empty((max(nvec, 0), self.nbatch), order="F")
        ld = np.empty(self.nbatch)
        info = np.zeros(self.nbatch, np.int64)
        code = lib().gmrfx_batch_refactorize_logpdf_dev(self._h, d_nzval, d_X or None, ldx, sx, nvec, d_mu or None, quad.ctypes.data,
                                                        ptr(ld), ptr(info))
        self._info = info
        check(code, self._h)
        return ld, quad, info.copy()

    # -- one constraint A x = e for every member, computed per member on the device (include/gmrfx.h, gmrfx_batch_constraints_*) --
    def set_constraints(self, A, e) -> None:
        """ONE A (m <= 64 sparse rows over the member's n columns) and e for all members. What is derived (A~'_k = Q_k^-1 A',
        W_k = A A~'_k, L_ck, B_k) is built lazily per member on the device, once per factorisation."""
        A = sp.csr_matrix(A, dtype=np.float64)
        e = np.ascontiguousarray(e, dtype=np.float64).reshape(-1)
        if A.shape[1] != self.n:
            raise ValueError(f"Constraint matrix size {A.shape} incompatible with member size {self.n}")
        if A.shape[0] != e.shape[0]:
            raise ValueError(f"Constraint matrix rows {A.shape[0]} != constraint vector length {e.shape[0]}")
        self.set_constraints_csr(A.shape[0], A.indptr, A.indices, A.data, e)

    def set_constraints_csr(self, m: int, rowptr, colind, values, e) -> None:
        """The raw form: CSR arrays as given (0-based), checked by the library."""
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        ci = np.ascontiguousarray(colind, dtype=np.int64)
        va = np.ascontiguousarray(values, dtype=np.float64)
        ev = np.ascontiguousarray(e, dtype=np.float64)
        if rp.shape != (m + 1,) or ev.shape != (m,) or ci.shape != va.shape or (m > 0 and ci.shape[0] < rp[-1]):
            raise ValueError("constraints: array lengths do not match m")
        check(lib().gmrfx_batch_constraints_set(self._h, m, ptr(rp), ptr(ci), ptr(va), 0, ptr(ev)), self._h)

    def clear_constraints(self) -> None:
        check(lib().gmrfx_batch_constraints_set(self._h, 0, None, None, None, 0, None), self._h)

    def constraint_info(self, check_posdef: bool = True) -> dict:
        """m, log det(A A') and -- on a numeric handle, preparing the members if needed -- logdet_W (B,), cinfo (B,) (0, 1 + the
        failing pivot of W_k, -1 = member k's factorisation failed) and the GPU time of the most recent preparation.
        check_posdef = False returns the dictionary also when some W_k is not positive definite."""
        m, lda, ms = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        if self.symbolic_only:
            check(lib().gmrfx_batch_constraints_info(self._h, C.byref(m), None, C.byref(lda), None, None), self._h)
            return {"m": m.value, "logdet_AAt": lda.value}
        ldw = np.zeros(self.nbatch)
        ci = np.zeros(self.nbatch, np.int64)
        code = lib().gmrfx_batch_constraints_info(self._h, C.byref(m), ptr(ldw), C.byref(lda), ptr(ci), C.byref(ms))
        if check_posdef or code != _lib.ERR_NOT_POSDEF:
            check(code, self._h)
        return {"m": m.value, "logdet_W": ldw, "logdet_AAt": lda.value, "cinfo": ci, "ms": ms.value}

    def _con_m(self) -> int:
        m = C.c_int64(0)
        check(lib().gmrfx_batch_constraints_info(self._h, C.byref(m), None, None, None, None), self._h)
        return m.value

    def constraint_fields(self, member: int):
        """(A_tilde_T, W) of one member: the n x m solve Q_k^-1 A' and W_k = A A~'_k."""
        m = self._con_m()
        At = np.empty((self.n, m), order="F")
        W = np.empty((m, m), order="F")
        check(lib().gmrfx_batch_constraints_get(self._h, int(member), ptr(At), self.n, ptr(W)), self._h)
        return At, W

    def constrained_mean(self, mu=None):
        """(mean_c (n, B), log_constraint_correction (B,)) of workspace_gmrf.jl:43-51 per member; mu: (n,), (n, B) or None = 0."""
        mu = self._mean(mu)
        out = np.empty((self.n, self.nbatch), order="F")
        lc = np.empty(self.nbatch)
        check(lib().gmrfx_batch_constraints_mean(self._h, ptr(mu), ptr(out), ptr(lc)), self._h)
        return out, lc

    def constrained_var(self) -> np.ndarray:
        """max(diag Sigma_k - rowsum(B_k^2), 0): (n, B); without a constraint = selinv_diag()."""
        out = np.empty((self.n, self.nbatch), order="F")
        check(lib().gmrfx_batch_constraints_var(self._h, ptr(out)), self._h)
        return out

    def constraint_correct(self, X) -> np.ndarray:
        """x - A~'_k (L_ck \\ (A x - e)) on every column of every member: X (n, B) or (n, r, B). Returns a fresh array."""
        Xf, r, s = self._members(X, "X")
        Xf = np.array(Xf, order="F", copy=True)
        check(lib().gmrfx_batch_constraints_correct(self._h, ptr(Xf), self.n, s, r), self._h)
        return Xf

    def constraint_correct_dev(self, d_X: int, ldx: int, sx: int, nvec: int) -> None:
        check(lib().gmrfx_batch_constraints_correct_dev(self._h, d_X or None, ldx, sx, nvec), self._h)

    def sample(self, Z, mean=None) -> np.ndarray:
        """`_rand!` per member on given standard-normal draws: P' L_k^-T Z_k + mean_k, then the constraint correction."""
        Zf, r, s = self._members(Z, "Z")
        mu = self._mean(mean)
        X = np.empty_like(Zf, order="F")
        check(lib().gmrfx_batch_sample(self._h, ptr(Zf), self.n, s, r, ptr(mu), ptr(X), self.n, s), self._h)
        return X

    def sample_dev(self, d_Z: int, ldz: int, sz: int, nrhs: int, d_X: int, ldx: int, sx: int, d_mu: int = 0) -> None:
        check(lib().gmrfx_batch_sample_dev(self._h, d_Z or None, ldz, sz, nrhs, d_mu or None, d_X or None, ldx, sx), self._h)

    def constrained_logpdf_dev(self, d_nzval: int, d_X: int, ldx: int, sx: int, nvec: int, d_mu: int = 0, check_posdef: bool = True):
        """gmrfx_batch_constrained_logpdf_dev: (logdet (B,), quad (nvec, B), log_correction (B,), info (B,), cinfo (B,)) in one call.
        logpdf_k = -quad / 2 + logdet_k / 2 - n log(2 pi) / 2 + log_correction_k (workspace_gmrf.jl:288-305).
        check_posdef = False returns the tuple also when a member or some W_k is not positive definite."""
        quad = np.empty((max(nvec, 0), self.nbatch), order="F")
        ld = np.empty(self.nbatch)
        lc = np.empty(self.nbatch)
        info = np.zeros(self.nbatch, np.int64)
        ci = np.zeros(self.nbatch, np.int64)
        code = lib().gmrfx_batch_constrained_logpdf_dev(self._h, d_nzval, d_X or None, ldx, sx, nvec, d_mu or None, quad.ctypes.data,
                                                        ptr(ld), ptr(lc), ptr(info), ptr(ci))
        self._info = info
        if check_posdef or code != _lib.ERR_NOT_POSDEF:
            check(code, self._h)
        return ld, quad, lc, info.copy(), ci

    def constrained_logpdf(self, NZ, X, mean=None):
        """The host-array form of constrained_logpdf_dev (operands staged through torch device tensors)."""
        import torch
        nz = self._values(NZ)
        Xf, nvec, s = self._members(X, "X")
        mu = self._mean(mean)
        dev = torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device())
        d_nz = torch.from_numpy(np.ascontiguousarray(nz.T)).to(dev)
        d_x = torch.from_numpy(np.ascontiguousarray(Xf.reshape(self.n, -1, order="F").T)).to(dev)
        d_mu = None if mu is None else torch.from_numpy(np.ascontiguousarray(mu.T)).to(dev)
        out = self.constrained_logpdf_dev(d_nz.data_ptr(), d_x.data_ptr(), self.n, s, nvec, 0 if d_mu is None else d_mu.data_ptr())
        torch.cuda.synchronize(dev)
        return out

    # -- Rao-Blackwellised Monte Carlo marginal variances: the calls act on the forest diag(Q_1 .. Q_B) --------------------------
    def rbmc_var(self, Z, enclosure_size: int = -1, nzval=None) -> np.ndarray:
        """Z: (n B, k) standard normals in the forest's row order (member k's rows at k n); nzval (nnz, B) or None (held values).
        Returns the (n, B) variances."""
        nz = None if nzval is None else self._values(nzval).reshape(-1, order="F")
        v = _rbmc_var(self._h, self.n * self.nbatch, self._nnz * self.nbatch, Z, enclosure_size, nz)
        return v.reshape(self.n, self.nbatch, order="F")

    def rbmc_var_dev(self, d_Z: int, ldz: int, nsamples: int, d_out: int, enclosure_size: int = -1, d_nzval: int = 0) -> None:
        if not d_Z or not d_out:
            raise ValueError("rbmc_var_dev: null pointer")
        check(lib().gmrfx_rbmc_var_dev(self._h, d_nzval or None, d_Z, ldz, nsamples, int(enclosure_size), d_out), self._h)

    def rbmc_plan(self, enclosure_size: int, index_base: int = 0) -> dict:
        """Blocks over the forest's B n nodes (blocks never cross members)."""
        return _rbmc_plan(self._h, enclosure_size, index_base)

    # -- log-density gradients on Q's own pattern, per member ---------------------------------------------------------------------
    def logpdf_grad(self, z, mean=None, ybar=1.0, nzval=None):
        """Per member: (Qbar (nnz, B) in the pattern's order, mubar (n, B), info (B,)). z (n, B); mean (n,) or (n, B); ybar a scalar
        or (B,); nzval (nnz, B), None = the held values. info[k]: 0, -1 (factorisation failed) or 1 + the failing pivot of W_k; such
        a member's columns are NaN."""
        Z = np.asarray(z, dtype=np.float64)
        if Z.shape != (self.n, self.nbatch):
            raise ValueError(f"z must have shape (n, nbatch) = ({self.n}, {self.nbatch}), got {Z.shape}")
        Zf = np.asfortranarray(Z)
        mu = self._mean(mean)
        nz = None if nzval is None else self._values(nzval)
        yb = np.ascontiguousarray(np.broadcast_to(np.asarray(ybar, dtype=np.float64), (self.nbatch,)))
        qbar = np.empty((self._nnz, self.nbatch), order="F")
        mubar = np.empty((self.n, self.nbatch), order="F")
        info = np.zeros(self.nbatch, np.int64)
        check(lib().gmrfx_batch_logpdf_grad(self._h, ptr(nz), ptr(Zf), self.n, ptr(mu), ptr(yb), ptr(qbar), ptr(mubar), ptr(info)), self._h)
        return qbar, mubar, info

    def logpdf_grad_dev(self, d_z: int, sz: int, ybar, d_Qbar: int = 0, d_mubar: int = 0, d_mu: int = 0, d_nzval: int = 0) -> np.ndarray:
        """Device pointers (member k's z at + k sz, Qbar at + k nnz, mu / mubar at + k n); ybar a scalar or (B,); returns info (B,)."""
        if not d_z or (not d_Qbar and not d_mubar) or (self.nbatch > 1 and sz < self.n):
            raise ValueError("logpdf_grad_dev: null pointer or member stride < n")
        yb = np.ascontiguousarray(np.broadcast_to(np.asarray(ybar, dtype=np.float64), (self.nbatch,)))
        info = np.zeros(self.nbatch, np.int64)
        check(lib().gmrfx_batch_logpdf_grad_dev(self._h, d_nzval or None, d_z, sz, d_mu or None, ptr(yb), d_Qbar or None, d_mubar or None,
                                                ptr(info)), self._h)
        return info

    def pattern_dot(self, G, J) -> np.ndarray:
        """out[k, b] = sum_e w_e G[e, b] J[e, k, b]: G (nnz, B), J (nnz, p, B) or (nnz, B) (p = 1); returns (p, B)."""
        g = self._values(G)
        Jf = np.asarray(J, dtype=np.float64)
        if Jf.ndim == 2:
            Jf = Jf[:, None, :]
        if Jf.ndim != 3 or Jf.shape[0] != self._nnz or Jf.shape[2] != self.nbatch or Jf.shape[1] < 1:
            raise ValueError(f"J must have shape (nnz, p, nbatch) with nnz = {self._nnz}, nbatch = {self.nbatch}, got {Jf.shape}")
        Jf = np.asfortranarray(Jf)
        p = Jf.shape[1]
        out = np.empty((p, self.nbatch), order="F")
        check(lib().gmrfx_batch_pattern_dot(self._h, ptr(g), ptr(Jf), max(self._nnz, 1), self._nnz * p, p, out.ctypes.data), self._h)
        return out

    def pattern_dot_dev(self, d_G: int, d_J: int, ldj: int, sj: int, p: int) -> np.ndarray:
        if not d_G or not d_J or p < 1 or ldj < self._nnz or (self.nbatch > 1 and sj < ldj * p):
            raise ValueError("pattern_dot_dev: null pointer, p < 1, ldj < nnz or member stride < ldj * p")
        out = np.empty((p, self.nbatch), order="F")
        check(lib().gmrfx_batch_pattern_dot_dev(self._h, d_G, d_J, ldj, sj, p, out.ctypes.data), self._h)
        return out


def gauss_hermite(K: int):
    """(nodes, weights) of the K-point Gauss-Hermite rule for the standard normal (numpy.polynomial.hermite_e.hermegauss), the weights
    divided by their sum: the rule predictive_scores takes."""
    return MI355XBackend.gauss_hermite(K)
