"""References for the linear predictor's marginals and the predictive scores (csrc/predictive.hip; gmrfx_predictor_marginals,
gmrfx_predictive_scores, gmrfx_obs_pointwise_const), no device.

* marginals(): mu_eta, v_eta (with the constraint's correction and clamp) and pll restated in np.longdouble (eps_ld = 2^-63) on small
  dense matrices, or, as the control, in float64. It is fed the handle's own inputs -- Sigma on pattern(Q) (gmrfx_selinv_extract) and the
  constraint's At and W (gmrfx_constraints_get; B = At L_c^-T through tests/constraint_ref.py) -- so the bounds cover the new arithmetic
  only. scores(): lpd, lcpo, elp, vlp and their totals the same way.
* bounds: per entry, first order, k eps sum |terms| with k counted from the length of each sum (below), independent of the order inside a
  lane group; times FACTOR = 16, the project's safety factor (tests/constraint_ref.py). The float64 control has to stay inside them
  WITHOUT the factor.
* MUTANTS: named wrong rules, each of which has to leave the bounds (with the factor) on at least one case.

Counting (eps = 2^-52; r_i entries in row i of A, T_i = r_i (r_i + 1) / 2 its pairs; a lane group's sum of k terms: at most ceil(k / 16)
fused multiply-adds on a lane's chain and 4 additions in the butterfly, bounded by k + 4 roundings):
  mu_eta_i  node form: a copy, exact. Design form: (r_i + 1) eps (sum |A_ik| |x_k| + |b_i|), as tests/fisher_design_ref.py.
  v_eta_i   node form: a copy, exact. Design form: (T_i + 6) eps sum |w| |Sigma|: the sum and one rounding in w = A_ij A_ik.
  correction  with ab_l = (a_i B)_l, S2_i = sum_l (|a_i| |B|)_l^2 and H = |At| |L_c^-1|' (constraint_ref.prepare):
            eps ((m + 1) (|v_i| + S2_i) + 2 m sum_l (|a_i| |B|)_l (|a_i| H)_l + kappa gw S2_i + 2 (r_i + 5) S2_i)
            -- bound_var of tests/constraint_ref.py (the handle's B against At L_c^-T in long double: its own roundings, and those of
            W and L_c through kappa gw) carried through a row of A, plus the (r_i + 4) roundings of each ab_l, twice (the square).
            The clamp moves the value towards the reference's or leaves it: no term.
  l(eta)    4 eps S(eta) + |g(eta)| e_eta, S = the sizes of the terms of l without their cancellation: Normal |l|; Poisson y |e| +
            m (1 + |e|); logit families y |eta| + n (|eta| + 1); NegBin y |e| + (r + y) (max(|log r|, |e|) + 1); Gamma phi |eta| +
            phi w (1 + |eta|) (e = eta + aux; the exponential's argument moves it by |e| ulp).
  pll_i     the above at mu_eta_i + eps (|l_i| + |c_i|) (the addition; c_i itself is the handle's own number).
  l_k       eta_k = fma(s, z_k, mu): eps (|eta_k| + |s z_k|) (the fma, the square root); then as pll.
  elp_i     sum_k w_k e_lk + (ceil(K / 16) + 5) eps sum_k w_k |l_k|.
  vlp_i     d_k = l_k - elp: e_d = e_lk + e_elp + eps |d_k|; sum_k w_k (2 |d_k| e_d + (ceil(K / 16) + 7) eps d_k^2).
  lpd_i     with p_k = w_k exp(l_k - M) / sum: sum_k p_k (e_lk + eps (|l_k - M| + 2)) + (ceil(K / 16) + 6) eps + eps (|log sum| + |M| +
            |lpd|): a moved l_k moves the log of the sum by p_k times as much, the exponential's argument by |l_k - M| ulp, the
            exponential and the logarithm are good to an ulp or two. lcpo_i the same with -l_k.
  totals    against the sum of the returned arrays: (4 + 8 + ceil(blocks / 256) + 1) eps sum_i |value_i| (the tree of 16, the final tree of
            256 and its strided loop)."""
import numpy as np

import constraint_ref as cref
import fisher_ref as ref

EPS, LD, FACTOR, LANES = ref.EPS, ref.LD, 16, 16
MUTANTS = ("no_factor_2", "no_clamp", "always_clamp", "no_offset", "At_for_B", "no_const", "lpd_no_max", "lcpo_sign", "vlp_about_0",
           "nodes_unscaled")


# ---- the constants ------------------------------------------------------------------------------------------------------------------------
def pointwise_const(obs):
    """(c_i, sum of |terms| of c_i) in long double; lgamma from mpmath at 40 digits"""
    import mpmath
    mpmath.mp.dps = 40
    lg = lambda v: np.array([LD(mpmath.nstr(mpmath.loggamma(mpmath.mpf(float(t))), 30)) for t in np.atleast_1d(v)], LD)      # noqa: E731
    y = np.asarray(obs.y, np.float64)
    k, p, f = y.size, LD(obs.param), obs.family
    z = np.zeros(k, LD)
    if f == 0:
        t = [z - LD(0.5) * np.log(2 * np.arccos(LD(-1))), z - np.log(p)]
    elif f == 1:
        t = [-lg(y + 1)]
    elif f == 2:
        t = [z]
    elif f == 3:
        nt = np.asarray(obs.aux, np.float64)
        t = [lg(nt + 1), -lg(y + 1), -lg(nt - y + 1)]
    elif f == 4:
        lgp = LD(mpmath.nstr(mpmath.loggamma(mpmath.mpf(float(obs.param))), 30))
        t = [np.array([LD(mpmath.nstr(mpmath.loggamma(mpmath.mpf(float(v)) + mpmath.mpf(float(obs.param))), 30)) for v in y], LD), z - lgp, -lg(y + 1),
             z + p * np.log(p)]
    else:
        lgp = LD(mpmath.nstr(mpmath.loggamma(mpmath.mpf(float(obs.param))), 30))
        t = [z + p * np.log(p), z - lgp, (p - 1) * np.log(np.asarray(y, LD))]
    return sum(t), sum(np.abs(v) for v in t)


def ll_sizes(family, eta, y, aux, param):
    """S(eta): the sizes of the terms of l(eta) without their cancellation (module docstring)"""
    eta, y = np.asarray(eta, LD), np.abs(np.asarray(y, LD))
    aux = np.zeros_like(eta) if aux is None else np.asarray(aux, LD)
    p = LD(param)
    _, _, ll, mean = ref.pointwise(family, eta, y, aux if family in (1, 3, 4) else None, param)
    if family == 0:
        return np.abs(ll)
    if family == 1:
        e = np.abs(eta + aux)
        return y * e + np.abs(mean) * (1 + e)
    if family in (2, 3):
        nt = aux if family == 3 else np.ones_like(eta)
        return y * np.abs(eta) + nt * (np.abs(eta) + 1)
    if family == 4:
        e = np.abs(eta + aux)
        return y * e + (p + y) * (np.maximum(abs(np.log(p)), e) + 1)
    w = y * np.exp(-eta)
    return p * np.abs(eta) + p * w * (1 + np.abs(eta))


def _point(obs, eta, dtype):
    g, _, ll, _ = ref.pointwise(obs.family, eta, obs.y, obs.aux, obs.param, dtype)
    return g, ll


# ---- the marginals --------------------------------------------------------------------------------------------------------------------------
def marginals(Ad, b, x, Sigma, obs, c, con=None, correct=False, dtype=LD, mutant=None, node=False):
    """Ad: dense nobs x n (node form: rows of the identity, node=True); Sigma: dense symmetric, the handle's entries on pattern(Q);
    c: the handle's constants; con: constraint_ref.prepare(...) of the handle's At (None: no constraint). Returns the three arrays and
    the ingredients of bounds()."""
    Ad, x, S = np.asarray(Ad, dtype), np.asarray(x, dtype), np.asarray(Sigma, dtype)
    nobs = Ad.shape[0]
    bb = np.zeros(nobs, dtype) if (b is None or mutant == "no_offset") else np.asarray(b, dtype)
    mu = Ad @ x + bb
    Sv = (S + np.diag(np.diag(S))) / 2 if mutant == "no_factor_2" else S          # (the off-diagonal pairs counted once)
    v0 = np.einsum("ij,jk,ik->i", Ad, Sv, Ad)
    v, corr = v0, np.zeros(nobs, dtype)
    if con is not None and (correct or mutant == "always_clamp"):
        if correct:
            Bm = np.asarray(con["At"] if mutant == "At_for_B" else con["B"], dtype)
            ab = Ad @ Bm
            corr = (ab * ab).sum(axis=1)
        v = v0 - corr
        if mutant != "no_clamp":
            v = np.where(np.isnan(v), v, np.maximum(v, 0))
    elif mutant == "always_clamp":
        v = np.maximum(v0, 0)
    g, ll = _point(obs, mu, dtype)
    cc = np.zeros(nobs, dtype) if mutant == "no_const" else np.asarray(c, dtype)
    return {"mu_eta": mu, "v_eta": v, "pll": ll + cc, "v0": v0, "corr": corr, "g": g, "ll": ll, "node": node}


def marginal_bounds(Ad, b, x, Sigma, obs, c, r, con=None, correct=False, factor=FACTOR):
    aA, ax, aS = np.abs(np.asarray(Ad, LD)), np.abs(np.asarray(x, LD)), np.abs(np.asarray(Sigma, LD))
    nobs = aA.shape[0]
    nzr = (aA != 0).sum(axis=1) if not r["node"] else np.zeros(nobs, int)
    T = nzr * (nzr + 1) // 2
    ab = np.zeros(nobs, LD) if b is None else np.abs(np.asarray(b, LD))
    e_mu = np.zeros(nobs, LD) if r["node"] else (nzr + 1) * EPS * (aA @ ax + ab)
    e_v = np.zeros(nobs, LD) if r["node"] else (T + 6) * EPS * np.einsum("ij,jk,ik->i", aA, aS, aA)
    if con is not None and correct:
        m = con["m"]
        aB = aA @ np.abs(con["B"])
        S2 = (aB * aB).sum(axis=1)
        bh = (aB * (aA @ con["H"])).sum(axis=1)
        e_v = e_v + EPS * ((m + 1) * (np.abs(r["v0"]) + S2) + 2 * m * bh + con["kappa"] * cref._gw(con) * S2 + 2 * (nzr + 5) * S2)
    S = ll_sizes(obs.family, r["mu_eta"], obs.y, obs.aux, obs.param)
    e_pll = 4 * EPS * S + np.abs(r["g"]) * e_mu + EPS * (np.abs(r["ll"]) + np.abs(np.asarray(c, LD)))
    return {"mu_eta": factor * e_mu, "v_eta": factor * e_v, "pll": factor * e_pll}


# ---- the scores -----------------------------------------------------------------------------------------------------------------------------
def _lse(l, w, dtype, no_max=False):
    """M + log sum_k w_k exp(l_k - M) row by row; -inf where M is"""
    M = l.max(axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Ms = np.where(np.isfinite(M), M, 0)
        if no_max:
            return np.log((w * np.exp(l)).sum(axis=1)), M, np.ones_like(l)
        s = (w * np.exp(l - Ms[:, None])).sum(axis=1)
        out = np.where(M == -np.inf, -np.inf, Ms + np.log(s))
        p = w * np.exp(l - Ms[:, None]) / np.where(s > 0, s, 1)[:, None]
    return out, M, p


def scores(mu, v, z, w, obs, c, dtype=LD, mutant=None):
    """lpd, lcpo, elp, vlp (nobs each), their totals, and the ingredients of score_bounds(); NaN rows where v is NaN or negative"""
    mu, v = np.asarray(mu, dtype), np.asarray(v, dtype)
    z, w = np.asarray(z, dtype), np.asarray(w, dtype)
    bad = ~(v >= 0)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.where(bad, 0, v))
    sz = np.broadcast_to(z, (mu.size, z.size)) * (1 if mutant == "nodes_unscaled" else s[:, None])
    eta = mu[:, None] + sz
    cc = np.zeros(mu.size, dtype) if mutant == "no_const" else np.asarray(c, dtype)
    yk = np.repeat(np.asarray(obs.y, np.float64)[:, None], z.size, axis=1)
    ak = None if obs.aux is None else np.repeat(np.asarray(obs.aux, np.float64)[:, None], z.size, axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        g, _, ll, _ = ref.pointwise(obs.family, eta, yk, ak, obs.param, dtype)
        lk = ll + cc[:, None]
        elp = (w * lk).sum(axis=1)
        d = lk - (0 if mutant == "vlp_about_0" else elp[:, None])
        vlp = (w * d * d).sum(axis=1)
    lpd, M, p = _lse(lk, w, dtype, no_max=mutant == "lpd_no_max")
    neg, Mn, pn = _lse(-lk, w, dtype)
    lcpo = neg if mutant == "lcpo_sign" else -neg
    out = {"lpd": lpd, "lcpo": lcpo, "elp": elp, "vlp": vlp}
    for k in out:
        out[k] = np.where(bad, np.nan, out[k])
    out["totals"] = np.array([out[k].sum(dtype=dtype) for k in ("lpd", "lcpo", "elp", "vlp")], dtype)
    out.update(lk=lk, eta=eta, sz=sz, g=g, p=p, pn=pn, M=M, Mn=Mn, d=d, bad=bad, cc=cc)
    return out


def score_bounds(z, w, obs, r, factor=FACTOR):
    """per-observation bounds of the four outputs against scores() = r (finite rows; the others are compared as they are)"""
    w = np.asarray(w, LD)
    K = w.size
    nk = -(-K // LANES)
    nobs = r["eta"].shape[0]
    yk = np.repeat(np.asarray(obs.y, np.float64)[:, None], K, axis=1)
    ak = None if obs.aux is None else np.repeat(np.asarray(obs.aux, np.float64)[:, None], K, axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        S = ll_sizes(obs.family, r["eta"], yk, ak, obs.param)
        e_eta = EPS * (np.abs(r["eta"]) + np.abs(r["sz"]))
        e_l = 4 * EPS * S + np.abs(r["g"]) * e_eta + EPS * (np.abs(r["lk"]) + np.abs(r["cc"])[:, None])
        e_elp = (w * e_l).sum(axis=1) + (nk + 5) * EPS * (w * np.abs(r["lk"])).sum(axis=1)
        d = r["d"]
        e_d = e_l + e_elp[:, None] + EPS * np.abs(d)
        e_vlp = (w * (2 * np.abs(d) * e_d + (nk + 7) * EPS * d * d)).sum(axis=1)

        def lse_bound(l, M, p, val):
            return (p * (e_l + EPS * (np.abs(l - M[:, None]) + 2))).sum(axis=1) + (nk + 6) * EPS + EPS * (np.abs(val - M) + np.abs(M) + np.abs(val))
        e_lpd = lse_bound(r["lk"], r["M"], r["p"], r["lpd"])
        e_lcpo = lse_bound(-r["lk"], r["Mn"], r["pn"], -r["lcpo"])
    assert e_l.shape == (nobs, K)
    return {"lpd": factor * e_lpd, "lcpo": factor * e_lcpo, "elp": factor * e_elp, "vlp": factor * e_vlp}


def total_bound(values, factor=FACTOR):
    """the handle's total against the long-double sum of the array it returned"""
    nobs = len(values)
    blocks = -(-nobs // 16)
    return factor * (4 + 8 + -(-blocks // 256) + 1) * EPS * np.abs(np.asarray(values, LD)).sum()


def ratio(got, want, bound, nonnegative=False):
    """largest error / bound over the entries; entries where the reference is not finite have to match it exactly (NaN for NaN, -inf
    for -inf) and count as 0, or inf when they do not. nonnegative: a value below zero, or -0.0, is inf too (the clamp)"""
    got, want, bound = np.asarray(got, LD), np.asarray(want, LD), np.asarray(bound, LD)
    if nonnegative and np.signbit(got[~np.isnan(got)]).any():
        return float("inf")
    fin = np.isfinite(want)
    same = np.where(np.isnan(want), np.isnan(got), got == want)
    if not same[~fin].all() or not np.isfinite(got[fin]).all():
        return float("inf")
    err = np.abs(got[fin] - want[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0, err / bound[fin])
    return float(q.max()) if q.size else 0.0


# ---- closed forms of the Normal family ----------------------------------------------------------------------------------------------------
def normal_closed(mu, v, y, sigma):
    """(elp, vlp, lpd) of y ~ N(eta, sigma^2), eta ~ N(mu, v), exact: elp and vlp also of any rule exact to degree 4 (K >= 3)"""
    mu, v, y, s2 = np.asarray(mu, LD), np.asarray(v, LD), np.asarray(y, LD), LD(sigma) ** 2
    half_log_2pi = np.log(2 * np.arccos(LD(-1))) / 2
    r = y - mu
    elp = -np.log(LD(sigma)) - half_log_2pi - (r * r + v) / (2 * s2)
    vlp = (4 * r * r * v + 2 * v * v) / (4 * s2 * s2)          # Var[(r - s z)^2] / (2 sigma^2)^2
    lpd = -np.log(s2 + v) / 2 - half_log_2pi - r * r / (2 * (s2 + v))
    return elp, vlp, lpd


# ---- the cases of tests/test_predictive_host.py and tests/test_gpu_predictive.py --------------------------------------------------------
NODE_NOBS = (1, 255, 256, 257)
DESIGN_NOBS = (1, 15, 16, 17, 33)
ROW_COUNTS = (0, 1, 3, 16, 17, 33)          # term lists of 0, 1, 6, 136, 153, 561 terms
CON_M = (1, 3, 4, 64)
SCORE_K = (1, 2, 16, 17, 64)


def grid(nx=17):
    """the prior: a Matern precision on a jittered nx x nx grid (n = 289: a dense inverse is cheap), full storage"""
    import scipy.sparse as sp
    from gmrfx import spde
    mesh = spde.grid_mesh_2d(nx, nx, jitter=0.2, seed=2)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.4))
    Q.sort_indices()
    return Q


def node_case(Q, nobs, family, seed=0):
    """shuffled indices, nobs < n"""
    n = Q.shape[0]
    rng = np.random.default_rng(100 * family + nobs + seed)
    obs = ref.make_obs(family, nobs, rng, "all")
    obs.idx = rng.permutation(n)[:nobs]
    Ad = np.zeros((nobs, n))
    Ad[np.arange(nobs), obs.idx] = 1.0
    return dict(Q=Q, uplo="U", A=None, Ad=Ad, b=None, obs=obs, x=0.4 * rng.standard_normal(n), node=True)


def design_case(Q0, nobs, family, offset, seed=0, extra_rows=None):
    """rows of every count of ROW_COUNTS (as far as nobs reaches; one observation: 17 entries), random columns (nodes repeat across
    rows), one explicit zero, with or without an offset; extra_rows: dense rows appended (the constraint's)"""
    import scipy.sparse as sp
    import fisher_design_ref as dref
    n = Q0.shape[0]
    rng = np.random.default_rng(1000 * family + 10 * nobs + int(offset) + seed)
    k0 = nobs - (0 if extra_rows is None else len(extra_rows))
    counts = [17] if k0 == 1 else (list(ROW_COUNTS) * 6)[:k0]
    A = sp.csr_matrix(dref._rows_matrix(n, counts, rng, positive=False))
    if A.nnz > 1:
        A.data[1] = 0.0         # (stays stored)
    if extra_rows is not None:
        A = sp.vstack([A, sp.csr_matrix(extra_rows)]).tocsr()
    Q, uplo = dref.with_pattern(Q0, A, "full")
    obs = dref.make_obs(family, nobs, 10 * family + 1 + seed)
    b = rng.uniform(-0.3, 0.3, nobs) if offset else None
    return dict(Q=Q, uplo=uplo, A=A, Ad=A.toarray(), b=b, obs=obs, x=0.4 * rng.standard_normal(n), node=False)


def constraint_rows(n, m):
    """m rows of ones over disjoint blocks of n // m nodes, dense"""
    k = n // m
    C = np.zeros((m, n))
    for r in range(m):
        C[r, r * k:(r + 1) * k] = 1.0
    return C


def dense_posterior(c):
    """(Sigma on the pattern as a dense symmetric float64 matrix, the full inverse in long double) of the case's Symmetric(Q): the
    stand-in for the handle's own read-outs where there is no device"""
    rows, cols, vals, _ = ref.symmetric_coo(c["Q"], c["uplo"])
    S = np.zeros(c["Q"].shape, LD)
    S[rows, cols] = vals
    inv = ref._solve(S, np.eye(S.shape[0], dtype=LD))
    inv = (inv + inv.T) / 2
    P = np.zeros(S.shape)
    P[rows, cols] = np.asarray(inv[rows, cols], np.float64)
    return P, inv


def score_inputs(family, nobs, seed=0):
    """(obs, mu, v) of the score tests: variances of every kind among ordinary ones"""
    rng = np.random.default_rng(7 * family + nobs + seed)
    obs = ref.make_obs(family, nobs, rng, "all")
    mu = 0.5 * rng.standard_normal(nobs)
    v = rng.uniform(0.01, 0.8, nobs)
    if nobs >= 8:
        v[1], v[3], v[5] = 0.0, np.nan, -0.25
    return obs, mu, v
