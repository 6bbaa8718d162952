"""References for Fisher scoring through a sparse design matrix, eta = A x + b (csrc/fisher_design.hip, gmrfx_obs_set_design), no device.

* hess_map(): the positions of pattern(A'A) in Q's stored triangle and the term lists, restated in Python.
* eval_ref(): eta, g, d, A' g, A' D A on the map's positions, score, energy, loglik in np.longdouble (eps_ld = 2^-63), with the sums of
  absolute terms the bounds are made of; bounds(): the per-entry error bounds (derived in tests/test_gpu_fisher_design.py).
* eval_f64(): the same in float64 numpy (the control of the bounds), with the named mutants of tests/test_fisher_design_host.py.
* newton_loop(): the loop of tests/fisher_ref.py with a design matrix, in float64 or long double, recording every merit comparison's
  margin; the case builders of the evaluation and loop tests.

LANES, ROWS and CHUNK restate csrc/kernels.h (kDesignLanes, kDesignRows, kDesignChunk); tests/test_fisher_design_host.py checks them."""
import numpy as np
import scipy.sparse as sp

import fisher_ref as ref

LANES, ROWS, CHUNK = 16, 16, 512
EPS, LD = ref.EPS, ref.LD


# ---- the map and the term lists ------------------------------------------------------------------------------------------------------------
def position(Q, uplo, j, k):
    """position in Q.data (sorted CSC) of entry {j, k} in the triangle in use, or -1"""
    lo, hi = min(j, k), max(j, k)
    r, c = (lo, hi) if uplo == "U" else (hi, lo)
    a, b = Q.indptr[c], Q.indptr[c + 1]
    q = a + np.searchsorted(Q.indices[a:b], r)
    return int(q) if q < b and Q.indices[q] == r else -1


def hess_map(Q, uplo, A):
    """(map, tptr, tobs, ta, tb, tj, tk): positions ascending; per position the terms (i, A_ij, A_ik) in ascending i; the pair (j, k)"""
    R = sp.csr_matrix(A)
    R.sort_indices()
    terms = {}
    for i in range(R.shape[0]):
        cols, vals = R.indices[R.indptr[i]:R.indptr[i + 1]], R.data[R.indptr[i]:R.indptr[i + 1]]
        for a in range(len(cols)):
            for b in range(a, len(cols)):
                p = position(Q, uplo, int(cols[a]), int(cols[b]))
                if p < 0:
                    raise KeyError((int(cols[a]), int(cols[b])))
                terms.setdefault(p, []).append((i, vals[a], vals[b], int(cols[a]), int(cols[b])))
    m = np.array(sorted(terms), np.int64)
    tptr = np.zeros(len(m) + 1, np.int64)
    flat = []
    for s, p in enumerate(m):
        flat += terms[p]
        tptr[s + 1] = len(flat)
    cols = list(zip(*flat)) if flat else [[], [], [], [], []]
    return (m, tptr, np.array(cols[0], np.int64), np.array(cols[1], float), np.array(cols[2], float), np.array(cols[3], np.int64),
            np.array(cols[4], np.int64))


def seg_depth(length):
    """additions on a segment's longest path besides the lane's own chain: the butterfly (log2 LANES); a chunked segment: the
    chunk's tree (log2 256), the lane's chain over the chunk sums and the butterfly"""
    length = np.asarray(length)
    nch = -(-length // CHUNK)
    return np.where(length <= CHUNK, 4, 4 + 8 + -(-nch // LANES))


def _segsum(ptr, vals, dtype=LD):
    out = np.zeros(len(ptr) - 1, dtype)
    np.add.at(out, np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), vals)
    return out


# ---- the evaluation -------------------------------------------------------------------------------------------------------------------------
def eval_ref(c, obs, x, mu, tm=None):
    """long-double design evaluation of case c (Q, uplo, A, b) with observations obs. Returns score (n), hess (cnt), energy, loglik and
    the ingredients of bounds()"""
    Q, uplo, A, b = c["Q"], c["uplo"], sp.csr_matrix(c["A"]), c["b"]
    n, nobs = Q.shape[0], A.shape[0]
    tm = hess_map(Q, uplo, A) if tm is None else tm
    m, tptr, tobs, ta, tb = tm[:5]
    xl = np.asarray(x, LD)
    ml = np.zeros(n, LD) if mu is None else np.asarray(mu, LD)
    rows, cols, vals, k = ref.symmetric_coo(Q, uplo)
    Qx, h, ax, ah = (np.zeros(n, LD) for _ in range(4))
    np.add.at(Qx, rows, vals * xl[cols])
    np.add.at(h, rows, vals * ml[cols])
    np.add.at(ax, rows, np.abs(vals * xl[cols]))
    np.add.at(ah, rows, np.abs(vals * ml[cols]))
    ri = np.repeat(np.arange(nobs), np.diff(A.indptr))
    av = A.data.astype(LD)
    eta, eta_abs = np.zeros(nobs, LD), np.zeros(nobs, LD)
    np.add.at(eta, ri, av * xl[A.indices])
    np.add.at(eta_abs, ri, np.abs(av * xl[A.indices]))
    if b is not None:
        eta, eta_abs = eta + np.asarray(b, LD), eta_abs + np.abs(np.asarray(b, LD))
    g, d, ll, mean = ref.pointwise(obs.family, eta, obs.y, obs.aux, obs.param)
    ag, ag_abs = np.zeros(n, LD), np.zeros(n, LD)
    np.add.at(ag, A.indices, av * g[ri])
    np.add.at(ag_abs, A.indices, np.abs(av * g[ri]))
    w = ta.astype(LD) * tb.astype(LD)
    hess, hess_abs = _segsum(tptr, w * d[tobs]), _segsum(tptr, np.abs(w * d[tobs]))
    const, cabs = ref.loglik_const(obs.family, obs.y, obs.aux, obs.param)
    auxa = np.zeros(nobs, LD) if obs.aux is None else np.abs(np.asarray(obs.aux, LD))
    return {"score": (Qx - h) - ag, "hess": hess, "energy": (0.5 * xl * Qx - xl * h).sum(dtype=LD), "loglik": ll.sum(dtype=LD) + const,
            "eta": eta, "g": g, "d": d, "mean": np.abs(mean), "k": k, "absrow": ax, "absh": ah, "h": h, "eta_abs": eta_abs,
            "r": np.diff(A.indptr), "ccount": np.bincount(A.indices, minlength=n), "ag_abs": ag_abs, "hess_abs": hess_abs,
            "tlen": np.diff(tptr), "tptr": tptr, "tobs": tobs, "w": w, "A": A, "ri": ri, "y": np.abs(np.asarray(obs.y, LD)),
            "en_abs": (np.abs(xl) * (ax + ah)).sum(dtype=LD),
            "ll_abs": (np.abs(ll) + np.abs(np.asarray(obs.y, LD)) * (np.abs(eta) + auxa) + np.abs(mean) * (1 + np.abs(eta))).sum(dtype=LD) + cabs,
            "n": n, "nobs": nobs}


def bounds(r, factor):
    """(score n, hess cnt, energy, loglik, eta nobs, point nobs): the bounds of tests/test_gpu_fisher_design.py, times `factor`"""
    e_eta = (r["r"] + 1) * EPS * r["eta_abs"]
    lip = np.maximum(r["mean"], np.abs(r["d"]))
    e_pt = 4 * EPS * (r["y"] + lip * (1 + np.abs(r["eta"]))) + lip * e_eta
    A, ri = r["A"], r["ri"]
    carry_s = np.zeros(r["n"], LD)
    np.add.at(carry_s, A.indices, np.abs(A.data) * e_pt[ri])
    b_score = (r["k"] + 4) * EPS * (r["absrow"] + np.abs(r["h"])) + (r["ccount"] + seg_depth(r["ccount"]) + 2) * EPS * r["ag_abs"] + carry_s
    carry_h = _segsum(r["tptr"], np.abs(r["w"]) * e_pt[r["tobs"]])
    b_hess = (r["tlen"] + seg_depth(r["tlen"]) + 1) * EPS * r["hess_abs"] + carry_h
    b_en = (int(r["k"].max()) + 4 + ref.reduction_depth(r["n"])) * EPS * r["en_abs"]
    b_ll = (4 + ref.reduction_depth(r["nobs"])) * EPS * r["ll_abs"] + (np.abs(r["g"]) * e_eta).sum(dtype=LD)
    return factor * b_score, factor * b_hess, factor * b_en, factor * b_ll, factor * e_eta, factor * e_pt


MUTANTS = ("no_offset", "drop_last_chunk", "drop_last_term", "square_weight", "wrong_obs")


def eval_f64(c, obs, x, mu, tm, mutant=None):
    """float64 numpy control: (score, hess, energy, loglik); mutant: one of MUTANTS, a deliberately wrong evaluation"""
    Q, uplo, A, b = c["Q"], c["uplo"], sp.csr_matrix(c["A"]), c["b"]
    n, nobs = Q.shape[0], A.shape[0]
    m, tptr, tobs, ta, tb, tj, tk = tm
    rows, cols, vals, _ = ref.symmetric_coo(Q, uplo)
    S = sp.csr_matrix((vals.astype(float), (rows, cols)), shape=(n, n))
    x = np.asarray(x, float)
    Qx = S @ x
    h = np.zeros(n) if mu is None else S @ np.asarray(mu, float)
    eta = A @ x
    if b is not None and mutant != "no_offset":
        eta = eta + b
    g, d, ll, _ = ref.pointwise(obs.family, eta, obs.y, obs.aux, obs.param, np.float64)
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    ag = np.zeros(n)
    for j in range(n):
        a, e = Ac.indptr[j], Ac.indptr[j + 1]
        if mutant == "drop_last_chunk" and e - a > CHUNK:
            e = a + ((e - a - 1) // CHUNK) * CHUNK
        ag[j] = np.dot(Ac.data[a:e], g[Ac.indices[a:e]])
    w = ta * tb
    if mutant == "square_weight":
        w = np.where(tj != tk, ta * ta, w)
    dd = d[(tobs + 1) % nobs] if mutant == "wrong_obs" else d[tobs]
    terms = w * dd
    if mutant == "drop_last_term":
        terms = terms.copy()
        terms[tptr[1:] - 1] = 0.0
    hess = _segsum(tptr, terms, np.float64)
    const = float(ref.loglik_const(obs.family, obs.y, obs.aux, obs.param)[0])
    return (Qx - h) - ag, hess, float(x @ Qx / 2 - x @ h), float(ll.sum() + const)


def exceeds(c, obs, x, mu, tm, r, got, factor=16):
    """the largest error / bound ratio of an evaluation `got` = (score, hess, energy, loglik) against the long-double r"""
    bs, bh, be, bl = bounds(r, factor)[:4]
    tiny = LD(1e-300)
    ratios = [np.max(np.abs(got[0] - r["score"]) / (bs + tiny)), np.max(np.abs(got[1] - r["hess"]) / (bh + tiny)) if len(bh) else 0.0,
              abs(got[2] - r["energy"]) / (be + tiny), abs(got[3] - r["loglik"]) / (bl + tiny)]
    return float(max(ratios))


# ---- cases of the evaluation tests ---------------------------------------------------------------------------------------------------------
def with_pattern(Q0, A, storage):
    """pattern(Q0) united with pattern(A'A) (explicit zeros), stored as `storage`: 'U' / 'L' (the other triangle holds junk) or 'full'"""
    P = sp.csr_matrix(A, copy=True)
    P.data[:] = 1.0
    P = sp.coo_matrix(P.T @ P)
    C = sp.coo_matrix(Q0)
    Q = sp.csc_matrix((np.r_[C.data, np.zeros(P.nnz)], (np.r_[C.row, P.row], np.r_[C.col, P.col])), shape=Q0.shape)
    Q.sort_indices()
    if storage != "full":
        cols = np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))
        Q.data[(Q.indices < cols) if storage == "L" else (Q.indices > cols)] = 1e3
    return Q, ("L" if storage == "L" else "U")


def _rows_matrix(n, counts, rng, positive=True):
    """one row per entry of counts with that many entries at random columns, weights summing to 1 (barycentric style)"""
    r, c, v = [], [], []
    for i, k in enumerate(counts):
        cols = np.sort(rng.choice(n, k, replace=False))
        w = rng.uniform(0.2, 1.0, k)
        w = w / w.sum() if positive else w * rng.choice([-1.0, 1.0], k)
        r += [i] * k
        c += list(cols)
        v += list(w)
    return sp.csr_matrix((v, (r, c)), shape=(len(counts), n))


def eval_cases():
    """name -> dict(Q, uplo, A, b): the smallest shapes that reach every branch of fisher_design.hip (coverage: test_fisher_design_host.py)"""
    out = {}
    rng = np.random.default_rng(7)
    # mesh: rows of three neighbouring nodes, an empty row, single-entry rows, node 5 observed by two single-entry rows; offset; upper
    n = 37
    r, c, v = [], [], []
    for i in range(40):
        j = i % (n - 2)
        w = rng.dirichlet(np.ones(3))
        r += [i] * 3
        c += [j, j + 1, j + 2]
        v += list(w)
    r += [41, 42, 43]           # row 40 is empty
    c += [5, 5, 36]
    v += [1.0, 0.5, 2.0]
    A = sp.csr_matrix((v, (r, c)), shape=(44, n))
    Q, u = with_pattern(ref.banded(n, 3, seed=5), A, "U")
    out["mesh"] = dict(Q=Q, uplo=u, A=A, b=rng.uniform(-0.3, 0.3, 44))
    # rows of 0, 1, 3, LANES, LANES + 1 and 2 LANES + 1 entries; no offset; lower
    n = 40
    A = _rows_matrix(n, [0, 1, 3, LANES, LANES + 1, 2 * LANES + 1, 3, 1], rng)
    Q, u = with_pattern(ref.banded(n, 2, seed=1), A, "L")
    out["rows"] = dict(Q=Q, uplo=u, A=A, b=None)
    # columns of 0, 1, LANES - 1, LANES, LANES + 1, CHUNK - 1, CHUNK, CHUNK + 1 entries (and term lists of the same lengths: their
    # diagonal positions); offset; full storage
    n, nobs = 20, CHUNK + 1
    counts = [0, 1, LANES - 1, LANES, LANES + 1, CHUNK - 1, CHUNK, CHUNK + 1]
    r, c, v = [], [], []
    for j, k in enumerate(counts):
        rows_j = np.sort(rng.choice(nobs, k, replace=False))
        r += list(rows_j)
        c += [j + 3] * k
        v += list(rng.uniform(0.05, 0.3, k) * rng.choice([-1.0, 1.0], k))
    A = sp.csr_matrix((v, (r, c)), shape=(nobs, n))
    Q, u = with_pattern(ref.banded(n, 2, seed=2), A, "full")
    out["cols"] = dict(Q=Q, uplo=u, A=A, b=rng.uniform(-0.3, 0.3, nobs))
    # an intercept column over nobs = 3 CHUNK + 1 > n rows (its diagonal position has nobs terms: three full chunks and one of a single
    # entry) beside one node per row; no offset; upper
    n, nobs = 30, 3 * CHUNK + 1
    i = np.arange(nobs)
    A = sp.csr_matrix((np.r_[np.full(nobs, 0.25), rng.uniform(0.5, 1.0, nobs)], (np.r_[i, i], np.r_[np.zeros(nobs, int), 1 + i % (n - 1)])),
                      shape=(nobs, n))
    Q, u = with_pattern(ref.banded(n, 1, seed=3), A, "U")
    out["intercept"] = dict(Q=Q, uplo=u, A=A, b=None)
    # one observation
    n = ROWS + 1
    A = sp.csr_matrix(([0.4, 0.6], ([0, 0], [2, 3])), shape=(1, n))
    Q, u = with_pattern(ref.banded(n, 1, seed=4), A, "L")
    out["one"] = dict(Q=Q, uplo=u, A=A, b=np.array([0.1]))
    return out


def make_obs(family, nobs, seed):
    o = ref.make_obs(family, nobs, np.random.default_rng(seed), "all")
    o.idx = None
    return o


def coverage(c):
    """what a case reaches: sets of row counts, column counts, term-list lengths, chunk lengths; flags"""
    A = sp.csr_matrix(c["A"])
    tm = hess_map(c["Q"], c["uplo"], A)
    cc = np.bincount(A.indices, minlength=A.shape[1])
    tl = np.diff(tm[1])
    chunks = set()
    for L in list(cc) + list(tl):
        if L > CHUNK:
            chunks |= {CHUNK, int(L - (-(-L // CHUNK) - 1) * CHUNK)}
    single = np.diff(A.indptr) == 1          # a node observed by two rows: two single-entry rows sharing their column
    twice = bool((np.bincount(A.indices[A.indptr[:-1][single]], minlength=A.shape[1]) >= 2).any())
    return {"rows": set(np.diff(A.indptr).tolist()), "cols": set(cc.tolist()), "terms": set(tl.tolist()), "chunk_lengths": chunks,
            "offset": c["b"] is not None, "uplo": c["uplo"], "nobs": A.shape[0], "n": A.shape[1], "node_twice": twice}


# ---- the loop: fisher_ref.newton_loop with eta = A x + b and H = A' D A ------------------------------------------------------------------
def newton_loop(S, mu, obs, Ad, b=None, x0=None, A=None, dtype=np.float64, max_iter=50, max_ls=10, mean_tol=1e-4, dec_tol=1e-5, adaptive=True,
                retry_full=True, predictive=True):
    """S: dense symmetric prior precision, Ad: dense design matrix (nobs x n), A: dense constraint matrix or None. Returns the dict of
    fisher_ref.newton_loop plus `margins`: (kind, distance from the threshold, scale) of every comparison -- a merit against obj_accept
    with the merit's noise floor 64 eps max(|energy| + |loglik|, 1) as scale, the convergence and look-ahead tests with their tolerance
    --, tiny: (alpha |step|_inf, dec_tol / 1000) of every tiny-step comparison, rounds as in fisher_ref.newton_loop, and hess_dense = A' D A at the mode."""
    n = S.shape[0]
    S, Ad = np.asarray(S, dtype), np.asarray(Ad, dtype)
    mu = np.zeros(n, dtype) if mu is None else np.asarray(mu, dtype)
    bb = np.zeros(Ad.shape[0], dtype) if b is None else np.asarray(b, dtype)
    h = S @ mu
    c = dtype(ref.loglik_const(obs.family, obs.y, obs.aux, obs.param)[0])
    A = None if A is None else np.asarray(A, dtype)
    cnt = {"fact": 0, "solve": 0, "merit": 0}
    events, margins, tiny, floor, rounds = [], [], [], [0.0], []

    def point(x):
        g, d, lo, _ = ref.pointwise(obs.family, Ad @ x + bb, obs.y, obs.aux, obs.param, dtype)
        return Ad.T @ g, Ad.T @ (d[:, None] * Ad), lo.sum() + c

    def energy(x):
        return x @ (S @ x) / 2 - x @ h

    def merit(x, accept):
        cnt["merit"] += 1
        m = energy(x) - point(x)[2]
        margins.append(("merit", float(abs(m - accept)), floor[0]))
        return m

    def solve_step(Qk, rhs):
        cnt["solve"] += 1
        step = ref._solve(Qk, rhs)
        if A is not None:
            At = ref._solve(Qk, np.ascontiguousarray(A.T))
            step = step - At @ ref._solve(A @ At, A @ step)
        return step

    def result(x, iters, converged, frozen):
        return {"x": x, "hess_dense": point(x)[1], "iterations": iters, "converged": converged, "alpha": float(alpha), "dec": float(dec),
                "factorizations": cnt["fact"], "solves": cnt["solve"], "merit_evaluations": cnt["merit"], "frozen": frozen,
                "dec_trace": np.array(dec_trace, dtype), "alpha_trace": np.array(alpha_trace, np.float64), "events": events,
                "margins": margins, "tiny": tiny, "rounds": rounds, "Qk": Qk}

    x_k = mu.copy() if x0 is None else np.asarray(x0, dtype).copy()
    alpha, dec_prev, dec = dtype(1), dtype(0), dtype("nan")
    dec_trace, alpha_trace = [], []
    Qk = S
    for it in range(1, max_iter + 1):
        rounds.append([0, 0, 0])
        g, H, ll_k = point(x_k)
        en_k = energy(x_k)
        Qk = S - H
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
        margins.append(("dec", float(abs(dec - dec_tol)), dec_tol))
        margins.append(("mean", float(min(abs(mc - mean_tol), abs(mcr - mean_tol))), mean_tol))
        if dec < dec_tol or mc < mean_tol or mcr < mean_tol:
            return result(x_new, it, True, False)
        if predictive and it > 1 and alpha == 1 and alpha_prev == 1:
            pred = dec * (dec / dec_prev) ** 2
            margins.append(("predict", float(abs(pred - dec_tol)), dec_tol))
            if pred < dec_tol:
                events.append("lookahead_fire")
                x, ok = x_new.copy(), True
                for j in (1, 2, 3):
                    rounds[-1][2] += 1
                    gs = (S @ x - h) - point(x)[0]
                    st = solve_step(Qk, gs)
                    if j == 1:
                        margins.append(("dec", float(abs(gs @ st - dec_tol)), dec_tol))
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


MERIT_MARGIN, TOL_MARGIN = 1000.0, 1e-3


def far_from_thresholds(margins):
    """the selection rule of the loop cases: every merit lies at least MERIT_MARGIN noise floors (64 eps max(|energy| + |loglik|, 1), the
    slack the loop itself grants to rounding) away from its acceptance threshold, and every convergence / look-ahead quantity at
    least TOL_MARGIN of its tolerance away from it: an evaluation that is accurate to a few floors takes the same branches"""
    return all(dist >= MERIT_MARGIN * scale if kind == "merit" else dist >= TOL_MARGIN * scale for kind, dist, scale in margins)


def loop_cases():
    """name -> dict(Q, uplo, A (design), b, obs, x0, C (constraint or None), events): point observations on a small mesh (three
    barycentric weights per row), the same with an intercept column, with and without a sum-to-zero constraint on the field"""
    import fisher_loop_cases as lc
    M = lc.load("matern2d_16x16_a2")
    n = M.shape[0]
    rng = np.random.default_rng(11)
    nobs = 300
    r, c, v = [], [], []
    for i in range(nobs):           # a point inside the triangle (j, j + 1, j + 16) of the 16 x 16 grid
        j = int(rng.integers(0, 15)) + 16 * int(rng.integers(0, 15))
        r += [i] * 3
        c += [j, j + 1, j + 16]
        v += list(rng.dirichlet(np.ones(3)))
    A = sp.csr_matrix((v, (r, c)), shape=(nobs, n))
    y = rng.poisson(200.0, nobs).astype(float)
    obs = ref.Obs(1, None, y, None, 0.0)
    out = {}
    Q, u = with_pattern(M, A, "full")
    out["mesh_far0"] = dict(Q=Q, uplo=u, A=A, b=None, obs=obs, x0=None, C=None, events={"backtrack"})
    out["mesh_far8"] = dict(Q=Q, uplo=u, A=A, b=None, obs=obs, x0=np.full(n, 8.0), C=None, events={"frozen_return"})
    out["mesh_sum0"] = dict(Q=Q, uplo=u, A=A, b=np.full(nobs, 5.0), obs=obs, x0=None, C=np.ones((1, n)), events=set())
    # the field plus an intercept: node n is the intercept with a proper N(0, 1 / 0.01) prior, every row observes it with weight 1
    Mi = sp.block_diag([M, sp.csc_matrix([[0.01]])], format="csc")
    Ai = sp.hstack([A, sp.csr_matrix(np.ones((nobs, 1)))], format="csr")
    Qi, ui = with_pattern(Mi, Ai, "full")
    out["intercept_far0"] = dict(Q=Qi, uplo=ui, A=Ai, b=None, obs=obs, x0=None, C=None, events={"backtrack"})
    return out


def restate_loop(c, dtype):
    D = c["Q"].toarray()
    S = np.triu(D) + np.triu(D, 1).T
    return newton_loop(S, None, c["obs"], c["A"].toarray(), b=c["b"], x0=c["x0"], A=c["C"], dtype=dtype)
