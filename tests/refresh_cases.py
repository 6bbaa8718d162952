"""Is every read-out fresh after every way of refactorising? The problems, the value sets, the tables of routes and read-outs and
the protocol of tests/test_gpu_refresh.py (on the device) and tests/test_refresh_host.py (structure, separation, coverage and the
mock control, without one).

The handle keeps many lazily built pieces that belong to ONE factorisation (csrc/device.h: the factor_serial_ tags rdiag_for_,
dtile_for_, logdet_for_, bdiag_for_, con_.serial, bcon_.serial, grad_.bt_serial; the flags selinv_valid, inverse_pending,
inverse_full_, nz_held_, info_cached_; tables dropped by setters). A missed invalidation returns plausible numbers of the PREVIOUS
factor. The oracle is sharp: the project promises the same bits on every route, so a fresh handle factorised once, by the plain call,
at the same values must agree bit for bit.

protocol(make, A, route, table, order):
  1. factorise a new handle at A by the plain host call, run every read-out (every cache now holds A's state): stale_i;
  2. route -> the handle is at B (RouteResult.values; held = the handle holds those values itself);
  3. run every read-out again, in table order or reversed: got_i. Where the route left Q's values with the caller, the read-outs
     that need them (NEEDS_VALUES) must refuse without nzval and are then given it;
  4. a fresh handle of the same make(), factorised once at B by refactorize_values, same read-outs, same order: want_i;
  5. same_bits(got_i, want_i) for every i -- no tolerance;
  6. got_i differs from stale_i (test_refresh_host.py shows that A and B are at least 1e-3 apart in every read-out, so a stale result
     cannot pass 5 by rounding luck).

Problems (the smallest at which the state exists; test_refresh_host.py proves both claims on symbolic-only handles and prints the counts):
  P_SMALL  grid(34, 34), default knobs: the smallest square grid with a sweep task (rdiag, dtile), level fronts of the small classes
           outside the tasks AND a level front wider than 64 columns (the level kernels and one dense-inverse stage, ev_inv_ /
           inverse_pending; below 34 x 34 no front is wider than 64 columns or has more than 64 rows).
  P_CAP    grid3(12, 12, 9) under GMRFX_INV_CAP=64: the smallest a x a x c slab (c <= a) with a front wider than 128 columns, so that
           inverse_full_ is false after a factorisation and the selected inversion has two doubling stages to add on demand.
Both carry + 0.3 I as the project's other grids do: well conditioned, the one-time inverse-cap decision leaves the cap alone."""
import numpy as np
import scipy.sparse as sp

from layout_buffers import diag_positions, same_bits


# ---- the problems ---------------------------------------------------------------------------------------------------------------------
def _csc(D):
    Q = sp.csc_matrix(D)
    Q.sort_indices()
    return Q


def _lap(n):
    e = np.ones(n)
    return sp.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1])


def grid(nx, ny):
    """the grid of tests/test_gpu_logpdf_grad.py"""
    return _csc(sp.kron(sp.eye(ny), _lap(nx)) + sp.kron(_lap(ny), sp.eye(nx)) + 0.3 * sp.eye(nx * ny))


def grid3(nx, ny, nz):
    I = sp.eye
    return _csc(sp.kron(I(nz), sp.kron(I(ny), _lap(nx))) + sp.kron(I(nz), sp.kron(_lap(ny), I(nx)))
                + sp.kron(_lap(nz), sp.kron(I(ny), I(nx))) + 0.3 * I(nx * ny * nz))


P_SMALL_SHAPE = (34, 34)
P_CAP_SHAPE = (12, 12, 9)
CAP_ENV = {"GMRFX_INV_CAP": "64"}
NRHS_ROUTE = (1, 17, 65)            # the wave form, the chunk form, two lanes
M_CON = 3


def values_b(Q):
    """B = 1.5 A + a positive, non-constant diagonal: no power-of-two rescaling of A"""
    v = 1.5 * Q.data
    v[diag_positions(Q)] += 0.25 + 0.125 * (np.arange(Q.shape[0]) % 7)
    return v


def structure(Q, setting):
    """counts on a symbolic-only handle: fronts, sweep tasks, chunks, small-class and big level fronts outside the tasks, widest front,
    most rows of a front, whether the permutation is the identity"""
    import gmrfx
    import sweep_shapes as sw
    be = gmrfx.MI355XBackend(Q, symbolic_only=True)
    try:
        fr = sw.fronts(be)
        levels, tasks = sw.sweep_levels(fr, sw.knobs(setting))
        _, first, _, _ = be.sweep_tasks()
        chunks = be.sweep_chunks()
        assert len(first) == len(tasks)             # the restated task rule and the library agree
        perm = be.ordering_permutation()
        return {"n": Q.shape[0], "fronts": len(fr), "tasks": len(first), "chunks": len(chunks["fwd"]),
                "small": [sum(len(L.small[q]) for L in levels.values()) for q in range(4)], "big": sum(len(L.big) for L in levels.values()),
                "max_cols": max(f[1] for f in fr), "max_rows": max(f[1] + f[2] for f in fr), "over128": sum(f[1] > 128 for f in fr),
                "identity": bool(np.array_equal(perm, np.arange(len(perm))))}
    finally:
        be.close()


def small_ok(s):
    return s["tasks"] >= 1 and sum(s["small"]) >= 1 and s["big"] >= 1 and s["max_cols"] > 64


def cap_ok(s):
    return s["over128"] >= 1


class Problem:
    """One pattern with everything the routes and read-outs take, fixed once: value sets A and B, right-hand sides, draws, the
    constraint sets, a design matrix for diag(A Sigma A'), a matrix on Q's pattern for tr(Sigma B), the two likelihoods."""

    def __init__(self, name, Q, env):
        self.name, self.Q, self.env = name, Q, dict(env)
        n = self.n = Q.shape[0]
        self.nnz = Q.nnz
        self.A = Q.data.copy()
        self.B = values_b(Q)
        self.dpos = diag_positions(Q)
        rng = np.random.default_rng(n)
        self.R = rng.standard_normal((n, 65))
        self.Zs = rng.standard_normal((n, 3))
        self.Zr = rng.standard_normal((n, 32))
        self.x = 0.3 * rng.standard_normal(n)
        self.mu = 0.2 * rng.standard_normal(n)
        self.X2 = rng.standard_normal((n, 2))
        i = np.arange(n)
        # constraint A1: three weighted sums over the residue classes mod 3; A2: one sum over everything
        self.con1 = (sp.csr_matrix(((1.0 + 0.1 * (i % 3)), (i % 3, i)), shape=(M_CON, n)), np.array([0.1, -0.2, 0.3]))
        self.con2 = (sp.csr_matrix(np.full((1, n), 0.5)), np.array([0.05]))
        # 40 rows of three entries for diag(D Sigma D')
        cols = rng.integers(0, n, (40, 3))
        self.D = sp.csr_matrix((rng.uniform(0.5, 1.5, 120), (np.repeat(np.arange(40), 3), cols.ravel())), shape=(40, n))
        self.Bm = sp.csc_matrix((rng.standard_normal(Q.nnz), Q.indices.copy(), Q.indptr.copy()), shape=Q.shape)
        # Poisson counts: on every third node (node form); through rows that see a node and its successor (design form: the pairs
        # (j, j + 1) are entries of Q wherever both lie in one grid line; taken where Q has the entry)
        self.obs_idx = np.arange(1, n, 3)
        self.obs_y = rng.poisson(2.0, len(self.obs_idx)).astype(np.float64)
        Qc = Q.tocsr()
        pairs = [j for j in range(0, n - 1, 2) if Qc[j, j + 1] != 0][: n // 4]
        r = np.arange(len(pairs))
        self.obs_design = sp.csc_matrix((np.r_[np.ones(len(pairs)), np.full(len(pairs), 0.5)], (np.r_[r, r], np.r_[pairs, np.add(pairs, 1)])),
                                        shape=(len(pairs), n))
        self.obs_design_y = rng.poisson(2.0, len(pairs)).astype(np.float64)
        assert len(pairs) != len(self.obs_idx)
        # Newton routes: prior - H = B exactly (2 b - b = b in floating point)
        self.prior = self.B.copy()
        self.prior[self.dpos] = 2.0 * self.B[self.dpos]
        self.H = self.prior[self.dpos] - self.B[self.dpos]

    def bad_values(self):
        """not positive definite: a negative diagonal"""
        v = self.B.copy()
        v[self.dpos] = -v[self.dpos]
        return v

    def make(self, form="node", con="con1", check_posdef=False):
        """a new handle, not factorised, with the constraint and the likelihood set; the environment is the caller's (monkeypatch)"""
        import gmrfx
        be = gmrfx.MI355XBackend(self.Q, device=0, factorize=False, check_posdef=check_posdef)
        try:
            if con:
                be.set_constraints(*getattr(self, con))
            self.set_obs(be, form)
        except Exception:
            be.close()
            raise
        return be

    def set_obs(self, be, form):
        if form == "node":
            be.set_observations("poisson", self.obs_y, self.obs_idx)
        else:
            be.set_design_observations("poisson", self.obs_design_y, self.obs_design)


_PROBLEMS = {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = Problem("P_small", grid(*P_SMALL_SHAPE), {}) if name == "P_small" else Problem("P_cap", grid3(*P_CAP_SHAPE), CAP_ENV)
    return _PROBLEMS[name]


# ---- read-outs of a plain handle: name -> (function(handle, problem, nzval) -> arrays, backend methods it stands for) --------------------
def _arr(*xs):
    return tuple(np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in xs)


def _solve(k):
    return lambda be, p, nz: _arr(be.backend_solve(p.R[:, 0] if k == 1 else p.R[:, :k]))


def _bsolve(k):
    return lambda be, p, nz: _arr(be.backend_backward_solve(p.R[:, 0] if k == 1 else p.R[:, :k]))


def _constraint_info(be, p, nz):
    d = be.constraint_info()
    return _arr(d["m"], d["logdet_W"], d["logdet_AAt"])


def _constrained_mean(be, p, nz):
    m, lc = be.constrained_mean(p.mu)
    return _arr(m, lc)


def _logpdf_grad(be, p, nz):
    q, m = be.logpdf_grad(p.x, mean=p.mu, ybar=-1.3, nzval=nz)
    return _arr(q.data, m)


READOUTS = {
    "solve1": (_solve(1), ("backend_solve",)), "solve16": (_solve(16), ()), "solve17": (_solve(17), ()), "solve64": (_solve(64), ()),
    "solve65": (_solve(65), ()),
    "bsolve1": (_bsolve(1), ("backend_backward_solve",)), "bsolve17": (_bsolve(17), ()),
    "logdet": (lambda be, p, nz: _arr(be.compute_logdet()), ("compute_logdet",)),
    "factor_values": (lambda be, p, nz: _arr(be.factor_values()), ("factor_values",)),
    "selinv_diag": (lambda be, p, nz: _arr(be.get_selinv_diag()), ("get_selinv_diag", "compute_selinv")),
    "selinv_extract": (lambda be, p, nz: _arr(be.selinv_extract_at(p.Q).data), ("selinv_extract_at",)),
    "selinv_dot": (lambda be, p, nz: _arr(be.selinv_dot(p.Bm), be.selinv_dot_device(p.Bm)), ("selinv_dot", "selinv_dot_device")),
    "row_diag": (lambda be, p, nz: _arr(be.row_diag_ASigmaAt(p.D)), ("row_diag_ASigmaAt",)),          # the plan is kept from step 1
    "constraint_fields": (lambda be, p, nz: _arr(*be.constraint_fields()), ("constraint_fields",)),
    "constraint_info": (_constraint_info, ("constraint_info",)),
    "constrained_mean": (_constrained_mean, ("constrained_mean",)),
    "constrained_var": (lambda be, p, nz: _arr(be.constrained_var()), ("constrained_var",)),
    "constraint_correct": (lambda be, p, nz: _arr(be.constraint_correct(p.Zs)), ("constraint_correct",)),
    "sample": (lambda be, p, nz: _arr(be.sample(p.Zs, mean=p.mu)), ("sample",)),
    "logpdf_grad": (_logpdf_grad, ("logpdf_grad",)),
    "rbmc_plain": (lambda be, p, nz: _arr(be.rbmc_var(p.Zr, -1, nzval=nz)), ("rbmc_var",)),
    "rbmc_block": (lambda be, p, nz: _arr(be.rbmc_var(p.Zr, 1, nzval=nz)), ()),
    "sqmahal": (lambda be, p, nz: _arr(be.sqmahal(p.X2, mean=p.mu, nzval=nz)), ("sqmahal",)),
    "predictor_marginals": (lambda be, p, nz: _arr(*be.predictor_marginals(p.x, constraint_correction=be._con_m() > 0)), ("predictor_marginals",)),
}
NEEDS_CONSTRAINT = ("constraint_fields", "constraint_info", "constrained_mean", "constraint_correct")     # refused with m = 0
NEEDS_VALUES = ("logpdf_grad", "rbmc_plain", "rbmc_block", "sqmahal")                                    # read Q's values
NEEDS_NO_CONSTRAINT = ("rbmc_plain", "rbmc_block")           # refused with a constraint set (the constrained estimator is not implemented)
REFUSAL = "does not hold Q's values"


def table(con=True):
    return {k: v[0] for k, v in READOUTS.items() if k not in (NEEDS_NO_CONSTRAINT if con else NEEDS_CONSTRAINT)}


def run_readouts(be, p, tab, order="table", nz=None):
    names = list(tab) if order == "table" else list(tab)[::-1]
    out = {}
    for name in names:
        out[name] = tab[name](be, p, nz if name in NEEDS_VALUES else None)
    return out


def refused(be, p, tab):
    """the read-outs of NEEDS_VALUES that did NOT give the documented refusal without nzval"""
    wrong = []
    for name in tab:
        if name in NEEDS_VALUES:
            try:
                tab[name](be, p, None)
                wrong.append(name + ": returned numbers")
            except ValueError as ex:
                if REFUSAL not in str(ex):
                    wrong.append(f"{name}: {ex}")
    return wrong


def bits_equal(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


# ---- routes of a plain handle: name -> (function(handle, problem) -> RouteResult, backend methods it stands for) -------------------------
class RouteResult:
    """values: what the handle is now factorised at; held: the handle holds them itself; extras: [(name, arrays the route returned,
    function(fresh handle) -> the arrays they must equal)]"""

    def __init__(self, values, held, extras=()):
        self.values, self.held, self.extras = values, held, list(extras)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _rhs(p, k):
    return np.asfortranarray(p.R[:, :k])


def _dev_cols(M):
    """column-major n x k on the device (a row-major k x n tensor)"""
    return _dev(np.ascontiguousarray(M.T))


def _host_cols(t):
    import torch
    torch.cuda.synchronize()
    return np.asfortranarray(t.cpu().numpy().T)


def r_values(be, p):
    be.refactorize_values(p.B)
    return RouteResult(p.B, True)


def r_matrix(be, p):
    be.refactorize(sp.csc_matrix((p.B, p.Q.indices, p.Q.indptr), shape=p.Q.shape))
    return RouteResult(p.B, True)


def r_dev(be, p):
    d = _dev(p.B)
    assert be.refactorize_dev(d.data_ptr()) == 0
    return RouteResult(p.B, False)


def r_solve(k):
    def f(be, p):
        X = be.refactorize_solve(p.B, _rhs(p, k))
        return RouteResult(p.B, True, [("X", _arr(X), lambda fr: _arr(fr.backend_solve(_rhs(p, k))))])
    return f


def r_solve_dev(k):
    def f(be, p):
        import torch
        d, dB = _dev(p.B), _dev_cols(_rhs(p, k))
        dX = torch.zeros_like(dB)
        assert be.refactorize_solve_dev(d.data_ptr(), dB.data_ptr(), p.n, k, dX.data_ptr(), p.n) == 0
        return RouteResult(p.B, False, [("X", _arr(_host_cols(dX)), lambda fr: _arr(fr.backend_solve(_rhs(p, k))))])
    return f


def r_solve_ptr(be, p):
    k = 17
    nz, Bf = np.ascontiguousarray(p.B), _rhs(p, k)
    X = np.zeros_like(Bf, order="F")
    assert be.refactorize_solve_ptr(nz.ctypes.data, Bf.ctypes.data, p.n, k, X.ctypes.data, p.n) == 0
    return RouteResult(p.B, True, [("X", _arr(X), lambda fr: _arr(fr.backend_solve(Bf)))])


def r_logpdf_dev(be, p):
    d, dX, dmu = _dev(p.B), _dev_cols(p.X2), _dev(p.mu)
    quad, ld = be.refactorize_logpdf_dev(d.data_ptr(), dX.data_ptr(), p.n, 2, dmu.data_ptr())
    return RouteResult(p.B, False, [("quad", _arr(quad), lambda fr: _arr(fr.sqmahal(p.X2, mean=p.mu))),
                                    ("logdet", _arr(ld), lambda fr: _arr(fr.compute_logdet()))])


def r_update(be, p):
    be.set_prior(p.prior, p.dpos)
    assert be.refactorize_update(p.H) == 0
    return RouteResult(p.B, True)


def r_update_solve(k):
    def f(be, p):
        be.set_prior(p.prior, p.dpos)
        X = be.refactorize_update_solve(p.H, _rhs(p, k))
        return RouteResult(p.B, True, [("X", _arr(X), lambda fr: _arr(fr.backend_solve(_rhs(p, k))))])
    return f


def r_update_solve_dev(be, p):
    import torch
    k = 17
    be.set_prior(p.prior, p.dpos)
    dh, dB = _dev(p.H), _dev_cols(_rhs(p, k))
    dX = torch.zeros_like(dB)
    assert be.refactorize_update_solve_dev(dh.data_ptr(), dB.data_ptr(), p.n, k, dX.data_ptr(), p.n) == 0
    return RouteResult(p.B, True, [("X", _arr(_host_cols(dX)), lambda fr: _arr(fr.backend_solve(_rhs(p, k))))])


def newton_values(prior, hmap, hess):
    """Q_prior - H formed on the host as the device forms it: nz = prior; nz[map] -= hess"""
    nz = np.array(prior, dtype=np.float64, copy=True)
    nz[hmap] -= hess
    return nz


def r_gaussian_approximation(be, p):
    """node or design form, whichever make() set: the handle is left at Q_prior - H(x_final)"""
    design = be.observations_design_info()["cnt"] >= 0
    hmap = be.observations_hess_map() if design else p.dpos
    be.set_prior(p.A, hmap)
    x, hess, info = be.gaussian_approximation(refactorize_final=True)
    assert info["converged"] and be.last_info == 0
    return RouteResult(newton_values(p.A, hmap, hess), True)


def r_ga_pullback(be, p):
    be.set_prior(p.A, p.dpos)
    _, hess, _, _ = be.fisher_eval(p.x)
    be.ga_pullback(p.x, mubar=p.mu, refactorize=True)
    return RouteResult(newton_values(p.A, p.dpos, hess), True)


ROUTES = {
    "refactorize_values": (r_values, ("refactorize_values",)),
    "refactorize": (r_matrix, ("refactorize",)),
    "refactorize_dev": (r_dev, ("refactorize_dev",)),
    **{f"refactorize_solve[{k}]": (r_solve(k), ("refactorize_solve",)) for k in NRHS_ROUTE},
    **{f"refactorize_solve_dev[{k}]": (r_solve_dev(k), ("refactorize_solve_dev",)) for k in NRHS_ROUTE},
    "refactorize_solve_ptr[17]": (r_solve_ptr, ("refactorize_solve_ptr",)),
    "refactorize_logpdf_dev": (r_logpdf_dev, ("refactorize_logpdf_dev",)),
    "refactorize_update": (r_update, ("refactorize_update", "set_prior")),
    **{f"refactorize_update_solve[{k}]": (r_update_solve(k), ("refactorize_update_solve",)) for k in NRHS_ROUTE},
    "refactorize_update_solve_dev[17]": (r_update_solve_dev, ("refactorize_update_solve_dev",)),
    "gaussian_approximation": (r_gaussian_approximation, ("gaussian_approximation", "observations_hess_map", "observations_design_info")),
    "ga_pullback": (r_ga_pullback, ("ga_pullback", "fisher_eval")),
}
# the tests of test_gpu_refresh.py that are routes or setter sequences of their own: what they call
OTHER_TESTS = {
    "clone": ("clone",), "failed_factorisation": ("refactorize_values", "logpdf_grad"),
    "constraint_change": ("set_constraints", "clear_constraints"),
    "observation_change": ("set_observations", "set_design_observations", "set_prior", "fisher_eval", "ga_pullback", "predictor_marginals"),
}

# Methods of MI355XBackend that are neither a route nor a read-out of the tables above, each with the reason.
EXCLUDED = {
    # lifetime and introspection: no factor-dependent result
    "close": "lifetime", "stats": "introspection (inv_cap is asserted equal on both handles)", "symbolic": "symbolic structure only",
    "sweep_tasks": "symbolic structure only", "sweep_chunks": "symbolic structure only", "ordering_permutation": "symbolic structure only",
    "rbmc_plan": "host analysis of the pattern", "observations_info": "the likelihood's host copy", "observations_design_rows": "the design plan",
    "observations_pointwise_const": "host arithmetic on the likelihood", "gauss_hermite": "quadrature rule", "level_times": "timing",
    "device_ptr": "raw pointer", "shard_info": "sharded handles", "shard_edges": "sharded handles", "shard_owner": "sharded handles",
    "shard_rows": "sharded handles", "shard_dist_fronts": "sharded handles", "shard_transfers": "sharded handles",
    "dist_front_block": "sharded handles", "logdet_partial": "sharded handles: a rank's part of log det",
    # the sharded / phase entry points: another protocol (two phases with an exchange in between), tests/test_shard_gloo.py
    "refactorize_phase_dev": "sharded phase entry point", "selinv_phase": "sharded phase entry point", "solve_phase_dev": "sharded phase entry point",
    "dist_front_phase": "sharded phase entry point", "set_stream": "the sharded drivers' stream; refactorize_solve then takes the plain sequence",
    # pure setters whose sequences have tests of their own (OTHER_TESTS) or that hold no factor-dependent state
    "set_constraints_csr": "the raw form of set_constraints (same gmrfx_constraints_set)",
    # factor-independent arithmetic
    "pattern_dot": "contraction of caller arrays", "pattern_dot_dev": "contraction of caller arrays", "dense_apply_dev": "dense operator, no factor",
    "transpose_dev": "no factor", "predictive_scores": "quadrature over caller arrays", "predictive_scores_dev": "quadrature over caller arrays",
    "fisher_eval_dev": "reads the prior, not the factor; the host form is in the observation-change test",
    # compositions of read-outs that are in the table
    "logpdf": "-sqmahal / 2 + compute_logdet / 2 + const on the host", "get_selinv": "the panels gathered entry by entry; selinv_extract_at reads the same panels",
    "factor_csc": "factor_values rearranged on the host", "row_diag_ASigmaAt_once": "row_diag_ASigmaAt with a plan it forgets",
    "selinv_compute_dev": "the selected inversion every selinv read-out triggers",
    # device-pointer twins: the same Device method behind another stager; tests/test_gpu_layout.py pins twin = host form bit for bit
    "solve_dev": "twin of backend_solve", "backward_solve_dev": "twin of backend_backward_solve", "quadform_dev": "twin of sqmahal",
    "constraint_correct_dev": "twin of constraint_correct", "sample_dev": "twin of sample", "rbmc_var_dev": "twin of rbmc_var",
    "logpdf_grad_dev": "twin of logpdf_grad", "predictor_marginals_dev": "twin of predictor_marginals",
    "gaussian_approximation_dev": "twin of gaussian_approximation (same loop, same final refactorisation)",
    "ga_pullback_dev": "twin of ga_pullback",
}


# ---- batched handles ---------------------------------------------------------------------------------------------------------------
BATCH_SHAPE, NBATCH, M_BCON = (9, 8), 3, 2


class BatchProblem:
    def __init__(self):
        Q = self.Q = grid(*BATCH_SHAPE)
        n, B = Q.shape[0], NBATCH
        self.n, self.nnz = n, Q.nnz
        self.dpos = diag_positions(Q)
        self.A = np.stack([(1.0 + 0.35 * k) * Q.data for k in range(B)], axis=1)
        self.B = np.stack([values_b(Q) * (1.0 + 0.2 * k) for k in range(B)], axis=1)
        rng = np.random.default_rng(7)
        self.R = rng.standard_normal((n, 5, B))
        self.Z = rng.standard_normal((n, B))
        self.MU = 0.2 * rng.standard_normal((n, B))
        self.Zr = rng.standard_normal((n * B, 32))
        i = np.arange(n)
        self.con = (sp.csr_matrix(((1.0 + 0.1 * (i % 2)), (i % 2, i)), shape=(M_BCON, n)), np.array([0.1, -0.2]))

    def bad(self, V, member=1):
        """V with member `member` not positive definite (a negative diagonal)"""
        W = V.copy()
        W[self.dpos, member] = -W[self.dpos, member]
        return W

    def make(self, con=True):
        import gmrfx
        bb = gmrfx.MI355XBatchBackend(self.Q, NBATCH, device=0)
        if con:
            bb.set_constraints(*self.con)
        return bb


def _b_constraint_info(bb, p, nz):
    d = bb.constraint_info(check_posdef=False)
    return _arr(d["m"], d["logdet_W"], d["logdet_AAt"], d["cinfo"])


def _b_logpdf_grad(bb, p, nz):
    return _arr(*bb.logpdf_grad(p.Z, mean=p.MU, ybar=[1.0, -0.6, 2.5], nzval=nz))


BATCH_READOUTS = {
    "info": (lambda bb, p, nz: _arr(bb.info()), ("info",)),
    "logdet": (lambda bb, p, nz: _arr(bb.logdet()), ("logdet",)),
    "solve": (lambda bb, p, nz: _arr(bb.solve(p.R)), ("solve",)),
    "backward_solve": (lambda bb, p, nz: _arr(bb.backward_solve(p.R)), ("backward_solve",)),
    "selinv_diag": (lambda bb, p, nz: _arr(bb.selinv_diag()), ("selinv_diag",)),
    "constraint_info": (_b_constraint_info, ("constraint_info",)),
    "constrained_mean": (lambda bb, p, nz: _arr(*bb.constrained_mean(p.MU)), ("constrained_mean",)),
    "constrained_var": (lambda bb, p, nz: _arr(bb.constrained_var()), ("constrained_var",)),
    "sample": (lambda bb, p, nz: _arr(bb.sample(p.R, mean=p.MU)), ("sample",)),
    "rbmc_var": (lambda bb, p, nz: _arr(bb.rbmc_var(p.Zr, -1, nzval=nz)), ("rbmc_var",)),
    "logpdf_grad": (_b_logpdf_grad, ("logpdf_grad",)),
}
BATCH_NEEDS_VALUES = ("rbmc_var", "logpdf_grad")
BATCH_NEEDS_NO_CONSTRAINT = ("rbmc_var",)         # refused with a constraint set, as on a plain handle
BATCH_NEEDS_CONSTRAINT = ("constraint_info", "constrained_mean")        # with m = 0 they do not depend on the factor


def batch_table(con=True):
    return {k: v[0] for k, v in BATCH_READOUTS.items() if k not in (BATCH_NEEDS_NO_CONSTRAINT if con else BATCH_NEEDS_CONSTRAINT)}


def run_batch_readouts(bb, p, tab, order="table", nz=None):
    names = list(tab) if order == "table" else list(tab)[::-1]
    return {name: tab[name](bb, p, nz if name in BATCH_NEEDS_VALUES else None) for name in names}


def _members_dev(V):
    """(x, B) member columns -> one device array, member k at + k x"""
    return _dev(np.ascontiguousarray(V.T))


def br_values(bb, p, V):
    bb.refactorize_values(V)
    return RouteResult(V, True)


def br_dev(bb, p, V):
    d = _members_dev(V)
    bb.refactorize_dev(d.data_ptr())
    return RouteResult(V, False)


def _b_logpdf_extras(p, ld, quad, info):
    return [("logdet", _arr(ld), lambda fr: _arr(fr.logdet())), ("quad", _arr(quad), lambda fr: _arr(fr.sqmahal(p.Z, mean=p.MU))),
            ("info", _arr(info), lambda fr: _arr(fr.info()))]


def br_logpdf(bb, p, V):
    ld, quad, info = bb.refactorize_logpdf(V, p.Z, mean=p.MU)
    return RouteResult(V, True, _b_logpdf_extras(p, ld, quad, info))


def br_logpdf_dev(bb, p, V):
    d, dz, dmu = _members_dev(V), _members_dev(p.Z), _members_dev(p.MU)
    ld, quad, info = bb.refactorize_logpdf_dev(d.data_ptr(), dz.data_ptr(), p.n, p.n, 1, dmu.data_ptr())
    return RouteResult(V, False, _b_logpdf_extras(p, ld, quad, info))


def _b_con_extras(p, out):
    ld, quad, lc, info, ci = out
    return _b_logpdf_extras(p, ld, quad, info) + [("cinfo", _arr(ci), lambda fr: _arr(fr.constraint_info(check_posdef=False)["cinfo"]))]


def br_constrained_logpdf(bb, p, V):
    return RouteResult(V, False, _b_con_extras(p, bb.constrained_logpdf(V, p.Z, mean=p.MU)))


def br_constrained_logpdf_dev(bb, p, V):
    d, dz, dmu = _members_dev(V), _members_dev(p.Z), _members_dev(p.MU)
    out = bb.constrained_logpdf_dev(d.data_ptr(), dz.data_ptr(), p.n, p.n, 1, dmu.data_ptr(), check_posdef=False)
    return RouteResult(V, False, _b_con_extras(p, out))


BATCH_ROUTES = {
    "refactorize_values": (br_values, ("refactorize_values",)),
    "refactorize_dev": (br_dev, ("refactorize_dev",)),
    "refactorize_logpdf": (br_logpdf, ("refactorize_logpdf", "sqmahal")),
    "refactorize_logpdf_dev": (br_logpdf_dev, ("refactorize_logpdf_dev",)),
    "constrained_logpdf": (br_constrained_logpdf, ("constrained_logpdf",)),
    "constrained_logpdf_dev": (br_constrained_logpdf_dev, ("constrained_logpdf_dev",)),
}
BATCH_EXCLUDED = {
    "close": "lifetime", "clone": "the plain handle's clone test covers gmrfx_clone; a batch clone copies the same panels",
    "stats": "introspection", "batch_size": "introspection", "ordering_permutation": "symbolic structure only",
    "forest_permutation": "symbolic structure only", "rbmc_plan": "host analysis of the pattern", "factor_values": "the panels; compared through solve and logdet per member",
    "set_constraints": "set once by make(); the plain handle's constraint-change test covers the setter's drop",
    "set_constraints_csr": "the raw form of set_constraints", "clear_constraints": "see set_constraints",
    "constraint_fields": "one member's operands; constrained_mean / constrained_var read all of them",
    "constraint_correct": "the correction sample applies", "pattern_dot": "contraction of caller arrays", "pattern_dot_dev": "contraction of caller arrays",
    "solve_dev": "twin of solve", "backward_solve_dev": "twin of backward_solve", "quadform_dev": "twin of sqmahal",
    "constraint_correct_dev": "twin of constraint_correct", "sample_dev": "twin of sample", "rbmc_var_dev": "twin of rbmc_var",
    "logpdf_grad_dev": "twin of logpdf_grad",
}


def public_methods(cls):
    return sorted(k for k, v in vars(cls).items() if not k.startswith("_") and (callable(v) or isinstance(v, staticmethod)))


def covered(routes, readouts, others=()):
    out = set()
    for t in (routes, readouts):
        for _, methods in t.values():
            out.update(methods)
    for methods in others:
        out.update(methods)
    return out


# ---- the protocol ------------------------------------------------------------------------------------------------------------------
def protocol(make, A, route, run, order="table", refusals=None, same=bits_equal, invariant=None, may_stay=()):
    """make() -> a new handle with refactorize_values and close; route(handle) -> RouteResult; run(handle, order, nz) -> {name: arrays}.
    refusals(handle) -> the list of wrong refusals, asked when the route left the values with the caller. may_stay: read-outs that A
    and B may share (status words that are 0 at both). Returns (stale, got, want);
    raises AssertionError naming the read-outs that are stale (step 5) or unchanged (step 6)."""
    be, fresh = make(), None
    try:
        be.refactorize_values(A)
        stale = run(be, "table", None)
        res = route(be)
        if not res.held and refusals is not None:
            wrong = refusals(be)
            assert not wrong, f"no refusal without nzval: {wrong}"
        got = run(be, order, None if res.held else res.values)
        fresh = make()
        fresh.refactorize_values(res.values)
        if invariant is not None:
            invariant(be, fresh)
        want = run(fresh, order, None)
        bad = [name for name in got if not same(got[name], want[name])]
        bad += [f"route:{name}" for name, g, wf in res.extras if not same(g, wf(fresh))]
        assert not bad, f"not the fresh handle's bits after the route ({order} order): {bad}"
        same_as_stale = [name for name in got if name not in may_stay and same(got[name], stale[name])]
        assert not same_as_stale, f"unchanged by the route: {same_as_stale}"
        return stale, got, want
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


# ---- dense float64 counterparts at one value set (test_refresh_host.py: the separation of A and B) ----------------------------------------
def dense_readouts(p, vals):
    Qd = sp.csc_matrix((vals, p.Q.indices, p.Q.indptr), shape=p.Q.shape).toarray()
    Qd = np.triu(Qd) + np.triu(Qd, 1).T
    S = np.linalg.inv(Qd)
    Ac, e = p.con1
    Ad = Ac.toarray()
    At = S @ Ad.T
    W = Ad @ At
    r = p.x - p.mu
    cols = np.repeat(np.arange(p.n), np.diff(p.Q.indptr))
    Sc = S - At @ np.linalg.solve(W, At.T)
    return {"solve": S @ p.R[:, :3], "logdet": np.array([np.linalg.slogdet(Qd)[1]]), "selinv_diag": np.diag(S).copy(),
            "selinv_pattern": S[p.Q.indices, cols], "constrained_mean": p.mu - At @ np.linalg.solve(W, Ad @ p.mu - e),
            "constrained_var": np.diag(Sc).copy(), "gradient": 0.5 * (S[p.Q.indices, cols] - r[p.Q.indices] * r[cols]),
            "backward_scale": np.sqrt(np.diag(S))}
