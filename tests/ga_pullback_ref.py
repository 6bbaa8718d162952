"""References for the pullback of gaussian_approximation (csrc/ga_pullback.hip, gmrfx_ga_pullback), no device.

* restate(): the rule of src/workspace/autodiff.jl:154-199 line by line on small dense matrices, in np.longdouble (eps_ld = 2^-63) or,
  as the control, in float64; the closed forms of d3 = dd/deta, gp = dg/dparam, dp = dd/dparam in point3().
      hess_pullback(-Qbar):  H = A' D A, so Hbar = -Qbar gives x_tangent = -A' (c . d3) and the parameter tangent -sum c dp, c_i = a_i' Qbar a_i
      b_ift = mubar + x_tangent;  lam = Q_post \\ b_ift  (projected with the constraint when asked)
      grad_pullback(-lam) through Q_p (x - mu) - loggrad(x):  Qbar_p = -sym(lam r'), mubar_p = Q_p lam, parameter tangent (A lam)' gp
      prior_tangent += Qbar
  Everything behind the solve can be formed from a given lam (the handle's own): that separates the solve's error from the kernels'.
* bounds(): per-entry bounds k eps sum |terms|, k counted from the operations of the kernels (below), times FACTOR = 16, the project's
  safety factor (tests/constraint_ref.py). The float64 control has to stay inside them WITHOUT the factor.
* MUTANTS: named wrong rules, each of which has to leave the bounds with the factor.

Counting (eps = 2^-52; r_i entries in row i of A, T_i = r_i (r_i + 1) / 2 its pairs, c_j entries in column j of A, k_i entries in row i of
Symmetric(Q); a lane group's sum of m terms: at most ceil(m / 16) fused multiply-adds on a lane's chain and 4 additions in the butterfly,
bounded by m + 4 roundings; a chunked column: fisher_design_ref.seg_depth):
  c_i      node form: a copy, exact. Design form: (T_i + 6) eps sum |w| |G|: the sum, one rounding in w = A_ij A_ik (the doubling is exact).
  eta_i    (r_i + 1) eps (sum |A_ik| |x_k| + |b_i|), as tests/test_gpu_fisher_design.py.
  d3_i     8 eps M_i (1 + |arg_i|) + M_i e_eta_i. M_i is the size of d3 without its cancelling factor: 0 (Normal), m (Poisson), n m q
           (logit families; |q - m| <= 1), (r + y) s q (NegBin), phi w (Gamma); a few operations on numbers each good to an ulp, the
           exponential's argument arg_i (eta + aux - log r) moving it by |arg_i| ulp; |d d3 / d eta| <= M_i for all of them.
  t_i      = c_i d3_i: |c_i| e_d3_i + |d3_i| e_c_i + eps |t_i|.
  xbar_j   (c_j + depth_j + 2) eps sum_i |A_ij| |t_i| + sum_i |A_ij| e_t_i + eps (|mubar_j| + |(A' t)_j|).
  Qbar_prior[e]  4 eps (|G_e| + |lam_i| |r_j| + |lam_j| |r_i|): r (one rounding each), two products, their sum, the difference (x 0.5 exact).
  mubar_prior_i  (k_i + 5) eps sum_j |Q_ij| |lam_j|.
  out[0]   (depth + 4) eps (sum |(A lam)_i| |gp_i| + sum |c_i| |dp_i|) + sum |gp_i| e_Alam_i + sum |(A lam)_i| e_gp_i + sum |c_i| e_dp_i
           + sum |dp_i| e_c_i, with e_Alam_i = (r_i + 5) eps sum_k |A_ik| |lam_k|, e_gp / e_dp = 8 eps P_i (1 + |arg_i|) + P_i e_eta_i for the
           sizes P_i of gp and dp without cancellation (Normal 2 (|y| + |eta|) / sigma^3 and 2 / sigma^3; NegBin s ((r + y) q / r + 1) and
           s q (1 + (r + y) / r); Gamma w + 1 and w), depth = the workgroup tree (8) + the final pass (fisher_ref.reduction_depth).
  out[1]   (n / 4096 + 12 + 8 + 2) eps sum |lam_i| |xbar_i| + sum |lam_i| e_xbar_i: chunks of 4096 entries, 256 threads, an LDS tree.
lam itself is held to the normwise bound the one-right-hand-side solve tests use (tests/test_gpu_parity.py: |Q X - B| / |B| < 1e-10)."""
import numpy as np
import scipy.sparse as sp

import fisher_design_ref as dref
import fisher_ref as ref

EPS, LD, FACTOR = ref.EPS, ref.LD, 16
SOLVE_RESIDUAL = 1e-10          # tests/test_gpu_parity.py: norm(Q X - B) / norm(B)
MUTANTS = ("d3_sign", "no_factor_2", "unsymmetrised", "x_for_r", "no_dp", "always_project")
HAS_PARAM = (0, 4, 5)


def point3(family, eta, y, aux, param, dtype=LD):
    """(d3, gp, dp, M, Pg, Pd, arg): the closed forms and the sizes the bounds use"""
    eta, y = np.asarray(eta, dtype), np.asarray(y, dtype)
    aux = np.zeros_like(eta) if aux is None else np.asarray(aux, dtype)
    p, z = dtype(param), np.zeros_like(eta)
    if family == 0:
        i3 = 1 / (p * p * p)
        return z, -(2 * (y - eta) * i3), z + 2 * i3, z, 2 * (np.abs(y) + np.abs(eta)) * i3, z + 2 * i3, np.abs(eta)
    if family == 1:
        m = np.exp(eta + aux)
        return -m, z, z, m, z, z, np.abs(eta) + np.abs(aux)
    if family in (2, 3):
        nt = aux if family == 3 else np.ones_like(eta)
        m, q = ref._logistic(eta), ref._logistic(-eta)
        return -(nt * m * q * (q - m)), z, z, nt * m * q, z, z, np.abs(eta)
    if family == 4:
        lr = np.log(p)
        t = (eta + aux) - lr
        s, q = ref._logistic(t), ref._logistic(-t)
        c = (p + y) * s * q * (q - s)
        return (-c, s * ((p + y) * q / p - 1), c / p - s * q, (p + y) * s * q, s * ((p + y) * q / p + 1), s * q * (1 + (p + y) / p),
                np.abs(eta) + np.abs(aux) + abs(lr))
    w = y * np.exp(-eta)
    return p * w, w - 1, -w, p * w, w + 1, w, np.abs(eta)


def _sym(Q, uplo):
    """dense Symmetric(Q, uplo) in long double from a sparse Q whose other triangle may hold junk"""
    rows, cols, vals, _ = ref.symmetric_coo(Q, uplo)
    S = np.zeros(Q.shape, LD)
    S[rows, cols] = vals
    return S


def restate(S, mu, Ad, b, obs, x, mubar, G, dtype=LD, lam=None, C=None, project=False, mutant=None):
    """S: dense symmetric prior precision; Ad: dense design matrix (node form: rows of the identity); G: dense symmetric cotangent of
    the posterior precision or None; mubar or None; C: dense constraint matrix or None. lam: a given solution (the handle's)."""
    S, Ad, x = np.asarray(S, dtype), np.asarray(Ad, dtype), np.asarray(x, dtype)
    n, nobs = S.shape[0], Ad.shape[0]
    mu = np.zeros(n, dtype) if mu is None else np.asarray(mu, dtype)
    eta = Ad @ x + (0 if b is None else np.asarray(b, dtype))
    g, d, _, _ = ref.pointwise(obs.family, eta, obs.y, obs.aux, obs.param, dtype)
    d3, gp, dp = point3(obs.family, eta, obs.y, obs.aux, obs.param, dtype)[:3]
    if mutant == "d3_sign":
        d3 = -d3
    if mutant == "no_dp":
        dp = np.zeros_like(dp)
    Qpost = S - Ad.T @ (d[:, None] * Ad)
    # hess_pullback(-Qbar)
    if G is None:
        c = np.zeros(nobs, dtype)
    else:
        Gd = np.asarray(G, dtype)
        if mutant == "no_factor_2":       # the off-diagonal pairs counted once
            Gd = (Gd + np.diag(np.diag(Gd))) / 2
        c = np.einsum("ij,jk,ik->i", Ad, Gd, Ad)
    x_tangent = -(Ad.T @ (c * d3))
    b_ift = (np.zeros(n, dtype) if mubar is None else np.asarray(mubar, dtype)) + x_tangent
    if lam is None:
        lam = ref._solve(Qpost, b_ift)
        if C is not None and (project or mutant == "always_project"):
            Cd = np.asarray(C, dtype)
            At = ref._solve(Qpost, np.ascontiguousarray(Cd.T))
            lam = lam - At @ ref._solve(Cd @ At, Cd @ lam)
    else:
        lam = np.asarray(lam, dtype)
    # grad_pullback(-lam)
    r = x if mutant == "x_for_r" else x - mu
    outer = np.outer(lam, r)
    Qbar_p = -outer if mutant == "unsymmetrised" else -(outer + outer.T) / 2
    if G is not None:
        Qbar_p = np.asarray(G, dtype) + Qbar_p
    Alam = Ad @ lam
    return {"c": c, "eta": eta, "d3": d3, "t": c * d3, "xbar": b_ift, "lam": lam, "Qpost": Qpost, "Qbar_prior": Qbar_p, "mubar_prior": S @ lam,
            "param": (Alam * gp).sum() - (c * dp).sum(), "check": lam @ b_ift, "Alam": Alam, "gp": gp, "dp": dp, "r": x - mu}


def bounds(S, Ad, b, obs, x, mubar, G, r, lam, factor=FACTOR, krow=None):
    """per-entry bounds for the outputs formed from `lam`, against restate(..., lam=lam) = r: dict of xbar (n), Qbar_prior (n x n),
    mubar_prior (n), param, check"""
    S, Ad = np.abs(np.asarray(S, LD)), np.asarray(Ad, LD)
    n, nobs = S.shape[0], Ad.shape[0]
    aA, ax, al = np.abs(Ad), np.abs(np.asarray(x, LD)), np.abs(np.asarray(lam, LD))
    nzr = (Ad != 0).sum(1)
    nzc = (Ad != 0).sum(0)
    selection = bool((nzr <= 1).all() and set(np.unique(Ad)) <= {0, 1})
    T = nzr * (nzr + 1) // 2
    aG = np.zeros((n, n), LD) if G is None else np.abs(np.asarray(G, LD))
    e_c = np.zeros(nobs, LD) if selection else (T + 6) * EPS * np.einsum("ij,jk,ik->i", aA, aG, aA)
    e_eta = (nzr + 1) * EPS * (aA @ ax + (0 if b is None else np.abs(np.asarray(b, LD))))
    _, _, _, M, Pg, Pd, arg = point3(obs.family, r["eta"], obs.y, obs.aux, obs.param)
    e_d3 = 8 * EPS * M * (1 + arg) + M * e_eta
    e_gp = 8 * EPS * Pg * (1 + arg) + Pg * e_eta
    e_dp = 8 * EPS * Pd * (1 + arg) + Pd * e_eta
    ac, at = np.abs(r["c"]), np.abs(r["t"])
    e_t = ac * e_d3 + np.abs(r["d3"]) * e_c + EPS * at
    amb = np.zeros(n, LD) if mubar is None else np.abs(np.asarray(mubar, LD))
    e_xbar = (nzc + dref.seg_depth(nzc) + 2) * EPS * (aA.T @ at) + aA.T @ e_t + EPS * (amb + aA.T @ at)
    ar = np.abs(r["r"])
    e_Q = 4 * EPS * (aG + np.outer(al, ar) + np.outer(ar, al))
    e_mu = (((S != 0).sum(1) if krow is None else np.asarray(krow)) + 5) * EPS * (S @ al)          # krow: stored entries per row of Symmetric(Q)
    depth = 8 + ref.reduction_depth(max(n, nobs))
    aAl = np.abs(r["Alam"])
    e_Alam = (nzr + 5) * EPS * (aA @ al)
    e_param = ((depth + 4) * EPS * ((aAl * np.abs(r["gp"])).sum() + (ac * np.abs(r["dp"])).sum()) + (np.abs(r["gp"]) * e_Alam).sum()
               + (aAl * e_gp).sum() + (ac * e_dp).sum() + (np.abs(r["dp"]) * e_c).sum())
    axb = np.abs(r["xbar"])
    e_check = (n // 4096 + 22) * EPS * (al * axb).sum() + (al * e_xbar).sum()
    return {"xbar": factor * e_xbar, "Qbar_prior": factor * e_Q, "mubar_prior": factor * e_mu, "param": factor * e_param,
            "check": factor * e_check}


def ratios(got, r, bd):
    """the largest error / bound ratio per output of `got` (a dict with some of xbar, Qbar_prior, mubar_prior, param, check)"""
    tiny = LD(1e-300)
    return {k: float(np.max(np.abs(np.asarray(got[k], LD) - r[k]) / (bd[k] + tiny))) for k in got if k in bd}


# ---- the pattern: dense symmetric matrices <-> the nnz values of the handle -------------------------------------------------------------
def pattern_rc(Q):
    return Q.indices, np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))


def to_pattern(Q, M):
    rows, cols = pattern_rc(Q)
    return np.asarray(M)[rows, cols]


def random_cotangent(Q, rng):
    """(values on the pattern, the dense symmetric matrix): an entry carries its value whichever triangle it lies in"""
    rows, cols = pattern_rc(Q)
    n = Q.shape[0]
    R = rng.standard_normal((n, n))
    R = (R + R.T) / 2
    G = np.zeros((n, n))
    G[rows, cols] = R[rows, cols]
    G[cols, rows] = R[rows, cols]
    return G[rows, cols].copy(), G


def term_rows_brute(Q, uplo, A):
    """the transposed term table by brute force: per row of A the (position, weight) of every pair j <= k, positions ascending"""
    R = sp.csr_matrix(A)
    R.sort_indices()
    ptr, pos, w = [0], [], []
    for i in range(R.shape[0]):
        cols, vals = R.indices[R.indptr[i]:R.indptr[i + 1]], R.data[R.indptr[i]:R.indptr[i + 1]]
        lst = []
        for a in range(len(cols)):
            for bb in range(a, len(cols)):
                lst.append((dref.position(Q, uplo, int(cols[a]), int(cols[bb])), (1.0 if a == bb else 2.0) * (vals[a] * vals[bb])))
        lst.sort()
        pos += [p for p, _ in lst]
        w += [v for _, v in lst]
        ptr.append(len(pos))
    return np.array(ptr, np.int64), np.array(pos, np.int64), np.array(w, float)


# ---- the Laplace objective and its finite differences (tests/test_ga_pullback_host.py) ------------------------------------------------------
def _chol_logdet(M):
    M = np.array(M, LD)
    n = M.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        L[j, j] = np.sqrt(M[j, j] - (L[j, :j] ** 2).sum())
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return 2 * np.log(np.diag(L)).sum()


def mode(S, mu, Ad, b, obs, x0, C=None, iters=40):
    """the mode in long double: plain Newton steps (projected with C) far past convergence"""
    x = np.asarray(x0, LD).copy()
    bb = 0 if b is None else np.asarray(b, LD)
    for _ in range(iters):
        g, d, _, _ = ref.pointwise(obs.family, Ad @ x + bb, obs.y, obs.aux, obs.param)
        Qk = S - Ad.T @ (d[:, None] * Ad)
        step = ref._solve(Qk, S @ (x - mu) - Ad.T @ g)
        if C is not None:
            At = ref._solve(Qk, np.ascontiguousarray(C.T))
            step = step - At @ ref._solve(C @ At, C @ step)
        x = x - step
    return x


def loglik(obs, eta, param):
    """the whole log-likelihood in long double as a function of the parameter (lgamma / digamma in float64: 1e-16 relative)"""
    from scipy.special import gammaln
    y, p = np.asarray(obs.y, LD), LD(param)
    aux = np.zeros_like(eta) if obs.aux is None else np.asarray(obs.aux, LD)
    f = obs.family
    if f == 0:
        return (-np.log(p) - (y - eta) ** 2 / (2 * p * p)).sum()
    if f == 4:
        e = eta + aux
        return (LD(1) * gammaln(np.float64(y) + float(p)) - LD(gammaln(float(p))) + p * np.log(p) + y * e - (p + y) * np.log(p + np.exp(e))).sum()
    if f == 5:
        return (p * np.log(p) - LD(gammaln(float(p))) + (p - 1) * np.log(y) - p * eta - p * y * np.exp(-eta)).sum()
    return ref.pointwise(f, eta, obs.y, obs.aux, param)[2].sum()


def dloglik_dparam(obs, eta, param):
    from scipy.special import digamma
    y, p = np.asarray(obs.y, LD), LD(param)
    aux = np.zeros_like(eta) if obs.aux is None else np.asarray(obs.aux, LD)
    f = obs.family
    if f == 0:
        return (-1 / p + (y - eta) ** 2 / (p * p * p)).sum()
    if f == 4:
        m = np.exp(eta + aux)
        return (LD(1) * digamma(np.float64(y) + float(p)) - LD(digamma(float(p))) + np.log(p) + 1 - np.log(p + m) - (p + y) / (p + m)).sum()
    if f == 5:
        return (np.log(p) + 1 - LD(digamma(float(p))) + np.log(y) - eta - y * np.exp(-eta)).sum()
    return LD(0)


def objective(S0, theta, mu, Ad, b, obs, param, wlin, x0):
    """Laplace marginal likelihood (constants dropped) + wlin' x*: logpdf(prior, x*) + loglik(x*) - logpdf(posterior, x*) with the prior
    precision theta S0, the mode re-solved"""
    o = ref.Obs(obs.family, obs.idx, obs.y, obs.aux, float(param))
    S = LD(theta) * np.asarray(S0, LD)
    x = mode(S, mu, Ad, b, o, x0)
    eta = Ad @ x + (0 if b is None else np.asarray(b, LD))
    d = ref.pointwise(o.family, eta, o.y, o.aux, LD(param))[1]
    Qpost = S - Ad.T @ (d[:, None] * Ad)
    r = x - mu
    val = _chol_logdet(S) / 2 - (r @ (S @ r)) / 2 + loglik(o, eta, LD(param)) - _chol_logdet(Qpost) / 2 + wlin @ x
    return val, x


def rule_derivatives(S0, theta, mu, Ad, b, obs, wlin, x0, mutant=None, C=None):
    """(dL/dtheta, dL/dparam) of objective() by the rule: the direct terms plus the pullback of (mubar, Qbar) = (dL/dx*, -Q_post^-1 / 2)"""
    S = LD(theta) * np.asarray(S0, LD)
    x = mode(S, mu, Ad, b, obs, x0)
    eta = Ad @ x + (0 if b is None else np.asarray(b, LD))
    g, d, _, _ = ref.pointwise(obs.family, eta, obs.y, obs.aux, obs.param)
    Qpost = S - Ad.T @ (d[:, None] * Ad)
    n = S.shape[0]
    G = -ref._solve(Qpost, np.eye(n, dtype=LD)) / 2
    G = (G + G.T) / 2
    mubar = wlin + (Ad.T @ g - S @ (x - mu))            # (the second term vanishes at the mode)
    R = restate(S, mu, Ad, b, obs, x, mubar, G, mutant=mutant, C=C)
    r = x - mu
    direct_Q = ref._solve(S, np.eye(n, dtype=LD)) / 2 - np.outer(r, r) / 2
    # contracted as gmrfx_pattern_dot does: weight 1 on the diagonal, 2 in the triangle in use, 0 in the other one
    wgt = np.triu(np.full((n, n), LD(2)), 1) + np.eye(n, dtype=LD)
    dtheta = (wgt * (direct_Q + R["Qbar_prior"]) * np.asarray(S0, LD)).sum()
    dparam = dloglik_dparam(obs, eta, obs.param) + R["param"]
    return dtheta, dparam


def small_case(family, seed=0, n=9, design=True):
    """a dense little problem for the host tests: a banded prior, three-entry rows with an offset (or a strict subset of the nodes)"""
    rng = np.random.default_rng(100 * family + seed)
    S0 = np.asarray(ref.banded(n, 2, seed=seed).toarray(), LD)
    if design:
        nobs = n + 3
        A = dref._rows_matrix(n, [3] * (nobs - 2) + [1, 0], rng).toarray()
        b = rng.uniform(-0.2, 0.2, nobs)
    else:
        idx = np.sort(rng.permutation(n)[: (2 * n) // 3])
        nobs = len(idx)
        A = np.zeros((nobs, n))
        A[np.arange(nobs), idx] = 1.0
        b = None
    obs = ref.make_obs(family, nobs, rng, "all")
    mu = 0.3 * rng.standard_normal(n)
    wlin = rng.standard_normal(n)
    return S0, np.asarray(mu, LD), np.asarray(A, LD), b, obs, np.asarray(wlin, LD)
