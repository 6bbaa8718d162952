"""Problems and restatements of the batched predictive tests (gmrfx_batch_predictor_marginals, gmrfx_batch_predictive_scores,
gmrfx_batch_predictive_mixture; tests/test_batch_predictive_host.py, tests/test_gpu_batch_predictive.py), built from what exists: the
17 x 17 grid and the cases, restatements and bounds of tests/predictive_ref.py, the member rule Q_k = s_k Q + c_k I of
tests/batch_design_cases.py and the per-member parameters of tests/batch_laplace_cases.family_params. The members' matrices stand for
the posterior precisions Q_post,k: the handles are factorised at them directly -- the read-outs' arithmetic is the same for any factor.

B = 3 (SC; a B = 1 batch takes member 1). nobs = 257 in node form and 33 in design form give every member two workgroups of
k_pred_node / three of k_pred_design and 17 / 3 partial quadruples of k_pred_scores, so a wrong per-member offset of part, c, zoff or
the outputs lands in another member's data. The failing member: Q - c I in the middle with lambda_min = -2
(batch_laplace_cases.fail_shift returns lambda_min + 3 for a likelihood that adds I: it is fed Q - I).

THE MIXTURE's restatement and bound. With omega_k the library's weights (formed in long double, rounded once: an ulp of double each,
as is log omega_k), B' the number of included members, eps = 2^-52 and every chain of B' fused multiply-adds bounded by B' roundings:
  mix_mu_i   (B' + 1) eps sum_k omega_k |mu_ik|                      the chain, and omega_k's own ulp
  mix_v_i    d_k = mu_ik - mix_mu_i: e_d = e_mu + eps |d_k|; t_k = fma(d_k, d_k, v_ik): e_t = 2 |d_k| e_d + eps |t_k|;
             sum_k omega_k e_t + (B' + 1) eps sum_k omega_k |t_k|
  mix_lpd_i  a_k = log omega_k + lpd_ik: e_a = eps (|a_k| + |log omega_k|); with p_k = exp(a_k - M) / sum:
             sum_k p_k (e_a + eps (|a_k - M| + 2)) + (B' + 1) eps + eps (|log sum| + |M| + |mix_lpd_i|)
             -- predictive_ref.score_bounds' rule for lpd with unit weights: a moved a_k moves the log of the sum by p_k times as much
  total      against the sum of the returned array: predictive_ref.total_bound (its count of 4 + 8 + ... roundings per value is for
             a tree of 16; the mixture's workgroup tree has 8 levels, 4 more, far inside the factor of 16 it carries).
All times predictive_ref.FACTOR; the float64 control has to stay inside them without the factor."""
import numpy as np
import scipy.sparse as sp

import batch_design_cases as dc
import batch_laplace_cases as bc
import fisher_ref as ref
import predictive_ref as pref

LD, EPS, FACTOR = pref.LD, pref.EPS, pref.FACTOR
SC = [(1.0, 0.0), (2.5, 0.3), (0.4, 1.0)]
NODE_TWO_BLOCKS, DESIGN_THREE_BLOCKS = 257, 33
MIX_B, MIX_NOBS = (1, 2, 3, 17), (1, 255, 256, 257)
MUTANTS = ("c_member_0", "Z_member_0", "param_0")
MIX_MUTANTS = ("no_between_term", "unnormalised")
_GRID = None


def grid():
    global _GRID
    if _GRID is None:
        _GRID = pref.grid()
    return _GRID


def problem(design, nobs, family, offset=False, B=3, extra_rows=None, seed=0):
    """the case of predictive_ref with B members, their parameters and their points X (n, B)"""
    c = pref.design_case(grid(), nobs, family, offset, seed=seed, extra_rows=extra_rows) if design else pref.node_case(grid(), nobs, family, seed=seed)
    sc = SC if B == 3 else [SC[1]] if B == 1 else [(1.0 + 0.5 * k, 0.1 * k) for k in range(B)]
    n = c["Q"].shape[0]
    rng = np.random.default_rng(31 * family + nobs + 7 * B + seed)
    X = np.asfortranarray(c["x"][:, None] + 0.3 * rng.standard_normal((n, B)))
    params = bc.family_params(family, 3)[[1]] if B == 1 else bc.family_params(family, B)
    return dict(c, Qs=dc.members(c["Q"], sc), params=params, X=X, B=B, n=n, nobs=nobs, design=design)


def member_obs(p, k, param=None):
    o = p["obs"]
    return ref.Obs(o.family, o.idx, o.y, o.aux, float(p["params"][k] if param is None else param))


def select(p, ks):
    ks = list(ks)
    return dict(p, Qs=[p["Qs"][k] for k in ks], params=p["params"][ks], X=np.asfortranarray(p["X"][:, ks]), B=len(ks))


def with_failing_member(p):
    """member 1 replaced by Q - c I with lambda_min = -2 (fail_shift: lambda_min + 3 of what it is fed, here Q - I)"""
    S = dc.sym_dense(p["Q"], p["uplo"])
    c = bc.fail_shift(sp.csc_matrix(S - np.eye(p["n"])))
    Qs = list(p["Qs"])
    Qs[1] = dc.shifted(p["Q"], 1.0, -c)
    return dict(p, Qs=Qs)


def member_case(p, k):
    """the predictive_ref case of member k: its precision, its point, its parameter"""
    return dict(p, Q=p["Qs"][k], x=p["X"][:, k], obs=member_obs(p, k))


def consts(p, dtype=np.float64):
    """c (nobs, B) from predictive_ref.pointwise_const at every member's parameter"""
    return np.stack([np.asarray(pref.pointwise_const(member_obs(p, k))[0], dtype) for k in range(p["B"])], axis=1)


def batch_marginals(p, Sigmas, C, dtype=LD, mutant=None, con=None, correct=False):
    """member by member through predictive_ref.marginals; the mutants read another member's data"""
    out = []
    for k in range(p["B"]):
        kc = 0 if mutant == "c_member_0" else k
        kz = 0 if mutant == "Z_member_0" else k
        kp = 0 if mutant == "param_0" else k
        o = member_obs(p, k, p["params"][kp])
        out.append(pref.marginals(p["Ad"], p["b"], p["X"][:, k], Sigmas[kz], o, C[:, kc], con=None if con is None else con[k], correct=correct,
                                  dtype=dtype, node=p["node"]))
    return out


def batch_bounds(p, Sigmas, C, r, con=None, correct=False, factor=FACTOR):
    return [pref.marginal_bounds(p["Ad"], p["b"], p["X"][:, k], Sigmas[k], member_obs(p, k), C[:, k], r[k], con=None if con is None else con[k],
                                 correct=correct, factor=factor) for k in range(p["B"])]


# ---- the mixture ------------------------------------------------------------------------------------------------------------------------
def weights(logw):
    """(omega, log omega) as the library forms them: long double, each rounded to double once; excluded members 0 and -inf"""
    lw = np.asarray(logw, LD)
    inc = lw != -np.inf
    mx = lw[inc].max()
    e = np.where(inc, np.exp(np.where(inc, lw - mx, 0)), 0)
    s = e.sum()
    om = np.asarray(e / s, np.float64)
    lo = np.where(inc, np.asarray(np.where(inc, lw - mx, 0) - np.log(s), np.float64), -np.inf)
    return om, lo


def mixture(logw, mu, v, lpd, dtype=LD, mutant=None):
    """mix_mu, mix_v, mix_lpd (nobs each), the total, and the ingredients of mixture_bounds(); mu, v, lpd: (nobs, B)"""
    om, lo = weights(logw)
    if mutant == "unnormalised":
        om, lo = np.exp(np.asarray(logw, np.float64)), np.asarray(logw, np.float64)
    inc = np.flatnonzero(lo != -np.inf)
    om, lo = np.asarray(om[inc], dtype), np.asarray(lo[inc], dtype)
    mu, v = np.asarray(mu, dtype)[:, inc], np.asarray(v, dtype)[:, inc]
    mm = (om * mu).sum(axis=1)
    d = mu - mm[:, None]
    t = v if mutant == "no_between_term" else d * d + v
    mv = (om * t).sum(axis=1)
    out = {"mix_mu": mm, "mix_v": mv, "om": om, "lo": lo, "mu": mu, "d": d, "t": t, "nb": len(inc)}
    if lpd is not None:
        a = lo + np.asarray(lpd, dtype)[:, inc]
        nan = np.isnan(a).any(axis=1)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            M = np.where(nan, np.nan, np.nanmax(np.where(np.isnan(a), -np.inf, a), axis=1))
            Ms = np.where(np.isfinite(M), M, 0)
            s = np.exp(a - Ms[:, None]).sum(axis=1)
            ml = np.where(nan, np.nan, np.where(M == -np.inf, -np.inf, Ms + np.log(s)))
            pk = np.exp(a - Ms[:, None]) / np.where(s > 0, s, 1)[:, None]
        out.update(mix_lpd=ml, a=a, M=M, p=pk, s=s, total=ml.sum(dtype=dtype))
    return out


def mixture_bounds(r, factor=FACTOR):
    nb, om = r["nb"], np.asarray(r["om"], LD)
    e_mu = (nb + 1) * EPS * (om * np.abs(r["mu"])).sum(axis=1)
    d, t = np.abs(np.asarray(r["d"], LD)), np.abs(np.asarray(r["t"], LD))
    e_d = e_mu[:, None] + EPS * d
    e_t = 2 * d * e_d + EPS * t
    e_v = (om * e_t).sum(axis=1) + (nb + 1) * EPS * (om * t).sum(axis=1)
    out = {"mix_mu": factor * e_mu, "mix_v": factor * e_v}
    if "a" in r:
        with np.errstate(invalid="ignore"):
            a, M = np.asarray(r["a"], LD), np.asarray(r["M"], LD)
            e_a = EPS * (np.abs(a) + np.abs(np.asarray(r["lo"], LD)))
            val = np.asarray(r["mix_lpd"], LD)
            e_l = (r["p"] * (e_a + EPS * (np.abs(a - M[:, None]) + 2))).sum(axis=1) + (nb + 1) * EPS + EPS * (np.abs(val - M) + np.abs(M) + np.abs(val))
        out["mix_lpd"] = factor * e_l
    return out


def mixture_inputs(B, nobs, seed=0):
    """(logw, mu, v, lpd): unnormalised log weights of very different sizes, means that differ between the members"""
    rng = np.random.default_rng(100 * B + nobs + seed)
    logw = rng.uniform(-30.0, 5.0, B)
    mu = np.asfortranarray(rng.standard_normal((nobs, B)) + np.linspace(-1, 1, B))
    v = np.asfortranarray(rng.uniform(0.01, 0.8, (nobs, B)))
    lpd = np.asfortranarray(-rng.uniform(0.1, 40.0, (nobs, B)))
    return logw, mu, v, lpd
