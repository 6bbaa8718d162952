"""References for Fisher scoring on the device (csrc/fisher.hip, gmrfx_obs_set / gmrfx_fisher_eval), no device.

* pointwise(): g = dl/deta, d = d2l/deta2 and the x-dependent part of l for the six families, in np.longdouble, in the stable forms of
  csrc/fisher.hip; pointwise_naive(): the same from the textbook formulas of the reference (canonical_implementations.jl:146-327),
  which are well-conditioned for moderate eta only; loglik_const(): the x-independent terms.
* eval_ref(): score, hess, energy, loglik of gmrfx_fisher_eval on Symmetric(Q) in np.longdouble, with the sums of absolute terms the
  error bounds of tests/test_gpu_fisher.py are made of.
* the shape cases and observation sets of the tests.

R, W and FINAL restate csrc/kernels.h (kFisherRows, kFisherLanes, kFisherFinal); tests/test_fisher_host.py checks them against the source."""
import numpy as np
import scipy.sparse as sp
from scipy.special import gammaln

R, W, FINAL = 16, 16, 256          # rows per workgroup, lanes per row, threads (= partial pairs per pass) of the final kernel
EPS = 2.0 ** -52
LD = np.longdouble
FAMILIES = {"normal": 0, "poisson": 1, "bernoulli": 2, "binomial": 3, "negbin": 4, "gamma": 5}


def _logistic(t):
    t = np.asarray(t)
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, 1 / (1 + e), e / (1 + e))


def _log1pexp(t):
    t = np.asarray(t)
    return np.maximum(t, 0) + np.log1p(np.exp(-np.abs(t)))


def pointwise(family, eta, y, aux, param, dtype=LD):
    """(g, d, ll, mean) per observation in `dtype` (long double by default), stable for every eta; mean = E[y] (the mu of the error bound)"""
    eta, y = np.asarray(eta, dtype), np.asarray(y, dtype)
    aux = np.zeros_like(eta) if aux is None else np.asarray(aux, dtype)
    p = dtype(param)
    if family == 0:
        inv = 1 / (p * p)
        r = y - eta
        return r * inv, np.full_like(eta, -inv), -(inv * r * r) / 2, eta
    if family == 1:
        e = eta + aux
        m = np.exp(e)
        return y - m, -m, y * e - m, m
    if family in (2, 3):
        nt = aux if family == 3 else np.ones_like(eta)
        m, q = _logistic(eta), _logistic(-eta)
        return y - nt * m, -(nt * m * q), y * eta - nt * _log1pexp(eta), nt * m
    if family == 4:
        e = eta + aux
        lr = np.log(p)
        s, q = _logistic(e - lr), _logistic(lr - e)
        return y * q - p * s, -((p + y) * s * q), y * e - (p + y) * (np.maximum(lr, e) + np.log1p(np.exp(-np.abs(e - lr)))), np.exp(e)
    if family == 5:
        w = y * np.exp(-eta)
        return p * (w - 1), -(p * w), -(p * eta) - p * w, np.exp(eta)
    raise ValueError(family)


def pointwise_naive(family, eta, y, aux, param):
    """(g, d) as the reference writes them (canonical_implementations.jl:146-327), in long double"""
    eta, y = np.asarray(eta, LD), np.asarray(y, LD)
    aux = np.zeros_like(eta) if aux is None else np.asarray(aux, LD)
    p = LD(param)
    if family == 0:
        return (y - eta) / p ** 2, np.full_like(eta, -1 / p ** 2)
    if family == 1:
        m = np.exp(eta + aux)
        return y - m, -m
    if family in (2, 3):
        nt = aux if family == 3 else 1
        m = 1 / (1 + np.exp(-eta))
        return y - nt * m, -nt * m * (1 - m)
    if family == 4:
        m = np.exp(eta + aux)
        return p * (y - m) / (p + m), -p * m * (p + y) / (p + m) ** 2
    m = np.exp(eta)
    return p * (y / m - 1), -p * y / m


def loglik_const_terms(family, y, aux, param):
    """the x-independent terms of loglik, one array entry per term (summed by the caller; their absolute sum feeds the bounds)"""
    y = np.asarray(y, np.float64)
    k = y.size
    p = float(param)
    if family == 0:
        return np.full(k, -0.5 * np.log(2 * np.pi) - np.log(p)).astype(LD)
    if family == 1:
        return (-gammaln(y + 1)).astype(LD)
    if family == 2:
        return np.zeros(k, LD)
    if family == 3:
        nt = np.asarray(aux, np.float64)
        return np.r_[gammaln(nt + 1), -gammaln(y + 1), -gammaln(nt - y + 1)].astype(LD)
    if family == 4:
        return np.r_[gammaln(y + p), np.full(k, -gammaln(p)), -gammaln(y + 1), np.full(k, p * np.log(p))].astype(LD)
    return np.r_[np.full(k, p * np.log(p) - gammaln(p)), (p - 1) * np.log(y)].astype(LD)


def loglik_const(family, y, aux, param):
    t = loglik_const_terms(family, y, aux, param)
    return t.sum(dtype=LD), np.abs(t).sum(dtype=LD)


class Obs:
    """an observation set: family id, 0-based indices (None: all nodes in order), y, aux (or None), param"""

    def __init__(self, family, idx, y, aux, param):
        self.family, self.idx, self.y, self.aux, self.param = family, idx, np.asarray(y, np.float64), aux, param


def make_obs(family, n, rng, which="all", with_aux=True):
    """which: 'all' (indices None), 'subset' (a strict subset, unsorted)"""
    if which == "all":
        idx, k = None, n
    else:
        k = max(1, (2 * n) // 3) if n > 1 else 1
        idx = rng.permutation(n)[:k]
    aux, param = None, 0.0
    if family == 0:
        y, param = rng.standard_normal(k), 0.7
    elif family == 1:
        y = rng.poisson(3.0, k).astype(float)
        aux = rng.uniform(-0.5, 0.5, k) if with_aux else None
    elif family == 2:
        y = rng.integers(0, 2, k).astype(float)
    elif family == 3:
        aux = rng.integers(1, 12, k).astype(float)
        y = np.floor(rng.uniform(0, 1, k) * (aux + 1)).clip(0, aux)
    elif family == 4:
        y, param = rng.poisson(4.0, k).astype(float), 2.5
        aux = rng.uniform(-0.5, 0.5, k) if with_aux else None
    else:
        y, param = rng.gamma(2.0, 1.0, k) + 0.05, 2.0
    return Obs(family, idx, y, aux, param)


def symmetric_coo(Q, uplo):
    """Symmetric(Q, uplo) as (rows, cols, vals, entries per row): the triangle in use mirrored, the other one ignored"""
    C = sp.coo_matrix(Q)
    keep = (C.row >= C.col) if uplo == "L" else (C.row <= C.col)
    r, c, v = C.row[keep], C.col[keep], C.data[keep]
    off = r != c
    rows, cols, vals = np.r_[r, c[off]], np.r_[c, r[off]], np.r_[v, v[off]]
    return rows, cols, vals.astype(LD), np.bincount(rows, minlength=Q.shape[0])


def eval_ref(Q, uplo, x, mu, obs):
    """long-double gmrfx_fisher_eval. Returns a dict: score, hess (n), energy, loglik, and for the bounds: k (entries per row),
    absrow_i = sum_j |Q_ij| |x_j|, absh_i = sum_j |Q_ij| |mu_j|, h, ymask (|y| by node), mean (|E y| by node), eta, en_abs, ll_abs"""
    n = Q.shape[0]
    rows, cols, vals, k = symmetric_coo(Q, uplo)
    xl = np.asarray(x, LD)
    ml = np.zeros(n, LD) if mu is None else np.asarray(mu, LD)
    Qx, h, ax, ah = (np.zeros(n, LD) for _ in range(4))
    np.add.at(Qx, rows, vals * xl[cols])
    np.add.at(h, rows, vals * ml[cols])
    np.add.at(ax, rows, np.abs(vals * xl[cols]))
    np.add.at(ah, rows, np.abs(vals * ml[cols]))
    idx = np.arange(n) if obs.idx is None else np.asarray(obs.idx)
    g, d, ll, ybn, mean = (np.zeros(n, LD) for _ in range(5))
    go, do, lo, mo = pointwise(obs.family, xl[idx], obs.y, obs.aux, obs.param)
    g[idx], d[idx], ll[idx], mean[idx], ybn[idx] = go, do, lo, np.abs(mo), np.abs(obs.y)
    auxn = np.zeros(n, LD)
    if obs.aux is not None:
        auxn[idx] = np.abs(obs.aux)
    c, cabs = loglik_const(obs.family, obs.y, obs.aux, obs.param)
    en_i = 0.5 * xl * Qx - xl * h
    observed = np.zeros(n, bool)
    observed[idx] = True
    return {"score": (Qx - h) - g, "hess": d, "energy": en_i.sum(dtype=LD), "loglik": ll.sum(dtype=LD) + c, "k": k, "absrow": ax, "absh": ah,
            "h": h, "y": ybn, "mean": mean, "eta": np.abs(xl), "observed": observed, "const": c,
            "en_abs": (np.abs(xl) * (ax + ah)).sum(dtype=LD),
            "ll_abs": (np.abs(ll) + ybn * (np.abs(xl) + auxn) + mean * (1 + np.abs(xl))).sum(dtype=LD) + cabs}


def reduction_depth(n):
    """additions on the longest path of the two-level sum of n row terms: the workgroup's tree (log2 R), the final kernel's strided
    loop (ceil(blocks / FINAL)) and its tree (log2 FINAL)"""
    blocks = -(-n // R)
    return int(np.log2(R)) + -(-blocks // FINAL) + int(np.log2(FINAL))


# ---- shapes: every size at which fisher.hip takes another path -------------------------------------------------------------------------
def _csc(M):
    Q = sp.csc_matrix(M)
    Q.sort_indices()
    return Q


def banded(n, half, seed=0):
    """symmetric, diagonally dominant, `half` off-diagonals on each side: interior rows have 2 half + 1 stored entries"""
    rng = np.random.default_rng(seed + 31 * n + half)
    diags, offs = [], []
    for o in range(1, min(half, n - 1) + 1):
        v = -rng.uniform(0.1, 1.0, n - o)
        diags += [v, v]
        offs += [o, -o]
    T = sp.diags(diags, offs, shape=(n, n)) if diags else sp.csc_matrix((n, n))
    d = np.asarray(abs(sp.csc_matrix(T)).sum(1)).ravel() + rng.uniform(0.5, 1.5, n)
    return _csc(sp.csc_matrix(T) + sp.diags(d))


def hub(n):
    """an arrowhead: row 0 has n >= 4 W + 3 entries, every other row two"""
    D = sp.lil_matrix((n, n))
    D.setdiag(3.0 + n / 8)
    D[0, 1:] = -0.1
    D[1:, 0] = -0.1
    return _csc(D)


def shape_cases():
    """name -> (Q, uplo). Tridiagonal at n = 1, R - 1, R, R + 1 and FINAL R + 1 (one more partial pair than the final pass is wide);
    bands whose interior rows hold W - 1, W, W + 1 entries; the hub; the same band stored as one triangle only, the other one junk."""
    cases = {f"tri{n}": (banded(n, 1), "U") for n in (1, R - 1, R, R + 1, FINAL * R + 1)}
    for ent in (W - 1, W, W + 1):
        # a row of a band with `half` off-diagonals holds 2 half + 1 entries; an even count takes one long-range pair more
        Q = banded(40, (ent - 1) // 2, seed=ent).tolil()
        if ent % 2 == 0:
            for i in range(20):
                Q[i, i + 20] = Q[i + 20, i] = -0.05
            Q.setdiag(Q.diagonal() + 0.1)
        cases[f"row{ent}"] = (_csc(Q), "U")
    cases["hub"] = (hub(4 * W + 3), "U")
    B = banded(37, 3, seed=5)
    cols = np.repeat(np.arange(37), np.diff(B.indptr))
    for uplo in ("L", "U"):
        J = B.copy()
        J.data[(J.indices < cols) if uplo == "L" else (J.indices > cols)] = 1e3       # junk in the triangle not in use
        cases[f"stored{uplo}"] = (J, uplo)
    return cases


def _solve(Qk, B):
    """Qk^-1 B in B's dtype: LAPACK in float64; for long double, float64 solves refined three times on the long-double residual"""
    if B.dtype == np.float64:
        return np.linalg.solve(Qk, B)
    Q64 = np.asarray(Qk, np.float64)
    x = np.asarray(np.linalg.solve(Q64, np.asarray(B, np.float64)), B.dtype)
    for _ in range(3):
        x = x + np.asarray(np.linalg.solve(Q64, np.asarray(B - Qk @ x, np.float64)), B.dtype)
    return x


# ---- the loop: _workspace_newton_loop restated line by line (src/workspace/gaussian_approximation.jl:230-313 with _ga_line_search,
# _predict_converged, _frozen_finish of src/arithmetic/condition/gaussian_approximation.jl:231-409), dense solves, in `dtype` -----------
def newton_loop(S, mu, obs, x0=None, A=None, dtype=np.float64, max_iter=50, max_ls=10, mean_tol=1e-4, dec_tol=1e-5, adaptive=True,
                retry_full=True, predictive=True):
    """S: dense symmetric prior precision. Returns a dict: x (the mode), hess, iterations, converged, alpha, dec, factorizations, solves,
    merit_evaluations, frozen, dec_trace, alpha_trace, events (the branches taken, in order), margins ((kind, distance from the threshold,
    scale) of every merit comparison, as tests/fisher_design_ref.py: newton_loop records them) and tiny ((alpha |step|_inf, dec_tol / 1000)
    of every tiny-step comparison) and rounds ([full-step retry 0 / 1, probes of the search, chord solves] per iterate). The merit's noise floor uses the float64 eps in every dtype: the long-double run follows the
    decisions a float64 loop is meant to take, with exact-er numbers."""
    n = S.shape[0]
    S = np.asarray(S, dtype)
    mu = np.zeros(n, dtype) if mu is None else np.asarray(mu, dtype)
    h = S @ mu
    idx = np.arange(n) if obs.idx is None else np.asarray(obs.idx)
    c = dtype(loglik_const(obs.family, obs.y, obs.aux, obs.param)[0])
    A = None if A is None else np.asarray(A, dtype)
    cnt = {"fact": 0, "solve": 0, "merit": 0}
    events, margins, tiny, floor, rounds = [], [], [], [0.0], []

    def point(x):
        g, d = np.zeros(n, dtype), np.zeros(n, dtype)
        go, do, lo, _ = pointwise(obs.family, x[idx], obs.y, obs.aux, obs.param, dtype)
        g[idx], d[idx] = go, do
        return g, d, lo.sum() + c

    def energy(x):
        return x @ (S @ x) / 2 - x @ h

    def merit(x, accept):
        cnt["merit"] += 1
        m = energy(x) - point(x)[2]
        margins.append(("merit", float(abs(m - accept)), floor[0]))
        return m

    def solve_step(Qk, rhs):
        cnt["solve"] += 1
        step = _solve(Qk, rhs)
        if A is not None:
            At = _solve(Qk, np.ascontiguousarray(A.T))
            step = step - At @ _solve(A @ At, A @ step)
        return step

    def neg_score(x):
        return (S @ x - h) - point(x)[0]

    def result(x, iters, converged, frozen):
        return {"x": x, "hess": point(x)[1], "iterations": iters, "converged": converged, "alpha": float(alpha), "dec": float(dec),
                "factorizations": cnt["fact"], "solves": cnt["solve"], "merit_evaluations": cnt["merit"], "frozen": frozen,
                "dec_trace": np.array(dec_trace, dtype), "alpha_trace": np.array(alpha_trace, np.float64), "events": events,
                "margins": margins, "tiny": tiny, "rounds": rounds}

    x_k = mu.copy() if x0 is None else np.asarray(x0, dtype).copy()
    alpha, dec_prev, dec = dtype(1), dtype(0), dtype("nan")
    dec_trace, alpha_trace = [], []
    for it in range(1, max_iter + 1):
        rounds.append([0, 0, 0])
        g, d, ll_k = point(x_k)
        en_k = energy(x_k)
        Qk = S - np.diag(d)
        cnt["fact"] += 1
        score = (S @ x_k - h) - g
        step = solve_step(Qk, score)
        alpha_prev = alpha
        if adaptive:
            floor[0] = float(64 * EPS * max(abs(en_k) + abs(ll_k), 1))
            obj_accept = (en_k - ll_k) + 64 * EPS * max(abs(en_k) + abs(ll_k), 1)
            done = False
            if retry_full and alpha < 1:
                rounds[-1][0] = 1
                x_full = x_k - step
                if merit(x_full, obj_accept) <= obj_accept:
                    x_new, alpha, done = x_full, dtype(1), True
                    events.append("retry_full_accept")
                else:
                    events.append("retry_full_reject")
            if not done:
                accept = False
                x_new = x_k - alpha * step
                for _ in range(max_ls):
                    rounds[-1][1] += 1
                    cand = x_k - alpha * step
                    if merit(cand, obj_accept) <= obj_accept:
                        x_new, alpha, accept = cand, np.sqrt(alpha), True
                        break
                    alpha = alpha * dtype(0.1)
                    events.append("backtrack")
                    tiny.append((float(alpha * np.abs(step).max()), dec_tol / 1000))
                    if alpha * np.abs(step).max() < dec_tol / 1000:
                        x_new, accept = cand, True
                        events.append("tiny_step_exit")
                        break
                if not accept:
                    x_new = x_k - alpha * step
                    events.append("linesearch_exhausted")
        else:
            x_new = x_k - step
        dec = score @ step
        mc = np.sqrt(((x_new - x_k) ** 2).sum())
        mcr = mc / max(np.sqrt((x_k ** 2).sum()), 1e-10)
        dec_trace.append(dec)
        alpha_trace.append(float(alpha))
        if dec < dec_tol or mc < mean_tol or mcr < mean_tol:
            return result(x_new, it, True, False)
        if predictive and it > 1 and alpha == 1 and alpha_prev == 1 and dec * (dec / dec_prev) ** 2 < dec_tol:
            events.append("lookahead_fire")
            x, ok = x_new.copy(), True
            for j in (1, 2, 3):
                rounds[-1][2] += 1
                gs = neg_score(x)
                st = solve_step(Qk, gs)
                if j == 1:
                    if not gs @ st < dec_tol:
                        ok = False
                        events.append("lookahead_reject")
                        break
                    dec = gs @ st
                    dec_trace.append(dec)
                    alpha_trace.append(float(alpha))
                x = x - st
            if ok:
                events.append("frozen_return")
                return result(x, it + 1, True, True)
        dec_prev, x_k = dec, x_new
    events.append("max_iter")
    return result(x_k, max_iter, False, False)


def decrement_at(S, mu, obs, x, A=None):
    """the long-double Newton decrement at x: score' (Q_p - H)^-1 score, constraint-projected"""
    r = newton_loop(S, mu, obs, x0=x, A=A, dtype=LD, max_iter=1, adaptive=False, predictive=False, mean_tol=0.0, dec_tol=0.0)
    return float(r["dec_trace"][0])
