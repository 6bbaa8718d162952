"""The loop cases of gmrfx_gaussian_approximation, chosen on the CPU with the restatement of tests/fisher_ref.py (newton_loop): Poisson with
large counts and far-off starting points on the golden matrices, and the reference's own small constrained input
(test/workspace/test_workspace_constrained.jl:87-110: Q = I, n = 8, sum to zero). Each case names the branches its float64 trace must
reach (tests/test_fisher_loop_host.py asserts them); the float64 and long-double restatements take the same alpha trace on every case
(no case sits on a rounding knife-edge). A look-ahead that fires and is REJECTED was found: sprand60_far0. besag9x7_* is an intrinsic
model of tests/intrinsic_models.py (Besag on a 9 x 7 torus + 1e-6 I: nearly singular, real fill) with its sum-to-zero constraint, under
both step-recovery policies; matern_sqrt0 runs the :sqrt policy without a constraint. (:sqrt from x0 = -6 on the Matern prior was tried
first and dropped: it stops on the mean-change test with a Newton decrement of 2.8e-5 at its mode, above newton_dec_tol, so the
"decrement at the returned mode" check cannot hold for it in any arithmetic.)
Measured on the CPU, float64 against long-double restatement, max over the decrement trace / over the mode:
  matern_far0 4.7e-10 / 5.1e-16   matern_far8 3.5e-11 / 4.9e-16   matern_farm6 1.4e-7 / 5.1e-16   sprand60_far0 2.7e-12 / 8.0e-16
  sprand60_maxiter 1.2e-10 / 4.9e-15   eye8_sum0 5.0e-16 / 1.7e-16   besag9x7_sum0 9.9e-10 / 1.8e-13   besag9x7_sqrt 9.9e-10 / 1.2e-13
  matern_sqrt0 4.7e-10 / 5.1e-16"""
import os

import numpy as np
import scipy.sparse as sp

import fisher_ref as ref
import intrinsic_models as im

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    n, cp = int(z["n"]), z["colptr"]
    base = int(cp[0])
    Q = sp.csc_matrix((z["nzval"], z["rowval"] - base, cp - base), shape=(n, n))
    Q.sort_indices()
    return Q


def _poisson(n, lam, seed):
    return ref.Obs(1, None, np.random.default_rng(seed).poisson(lam, n).astype(float), None, 0.0)


def cases():
    """name -> dict(Q, obs, x0, A, kw, events): kw = the loop's keyword arguments, events = branches the trace must contain"""
    M, P = load("matern2d_16x16_a2"), load("sprand_spd_60")
    out = {
        "matern_far0": dict(Q=M, obs=_poisson(256, 200.0, 1), x0=None, events={"backtrack", "retry_full_reject", "retry_full_accept"}),
        "matern_far8": dict(Q=M, obs=_poisson(256, 200.0, 1), x0=np.full(256, 8.0), events={"lookahead_fire", "frozen_return"}),
        "matern_farm6": dict(Q=M, obs=_poisson(256, 200.0, 1), x0=np.full(256, -6.0), events={"backtrack", "retry_full_accept"}),
        "sprand60_far0": dict(Q=P, obs=_poisson(60, 200.0, 1), x0=None, events={"lookahead_fire", "lookahead_reject", "frozen_return"}),
        "sprand60_maxiter": dict(Q=P, obs=_poisson(60, 200.0, 1), x0=np.full(60, 8.0), kw=dict(max_iter=3), events={"max_iter"}),
        "eye8_sum0": dict(Q=sp.identity(8, format="csc"), obs=ref.Obs(1, None, [2, 1, 3, 0, 4, 1, 2, 3], None, 0.0), x0=None,
                          A=np.ones((1, 8)), events={"frozen_return"}),
    }
    B = im.besag_torus((9, 7), 1e-6).Q
    out["besag9x7_sum0"] = dict(Q=B, obs=_poisson(63, 200.0, 1), x0=None, A=np.ones((1, 63)),
                                events={"backtrack", "retry_full_reject", "retry_full_accept", "lookahead_fire", "frozen_return"})
    out["besag9x7_sqrt"] = dict(Q=B, obs=_poisson(63, 200.0, 1), x0=None, A=np.ones((1, 63)), kw=dict(retry_full=False), events={"backtrack"})
    out["matern_sqrt0"] = dict(Q=M, obs=_poisson(256, 200.0, 1), x0=None, kw=dict(retry_full=False), events={"backtrack"})
    for c in out.values():
        c.setdefault("A", None)
        c.setdefault("kw", {})
    return out


def dense(Q):
    D = Q.toarray()
    return np.triu(D) + np.triu(D, 1).T


def restate(c, dtype):
    return ref.newton_loop(dense(c["Q"]), None, c["obs"], x0=c["x0"], A=c["A"], dtype=dtype, **c["kw"])
