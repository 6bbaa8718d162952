"""max_iter = 0, which both loops accept (csrc/device_fisher.cpp, csrc/device_batch_fisher.cpp): no iterate is taken. The mode is the
starting point bit for bit (x0, or the mean, or zero), iterations = 0, converged is False, the decrement is NaN and both traces hold
nothing but their NaN slot, hess has the bits of fisher_eval at the starting point, nothing is factorised -- and with refactorize_final
exactly one factorisation is, that of Q_p - H(x0): log det has the bits of a fresh handle's. A plain handle and a batch of three."""
import numpy as np
import pytest

import batch_laplace_cases as bc
import fisher_loop_cases as lc
import gmrfx
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu


def _problem():
    M = lc.load("sprand_spd_60")
    return M, lc._poisson(60, 200.0, 1).y


@pytest.mark.parametrize("start", ["x0", "mean", "zero"])
def test_plain_handle(start):
    M, y = _problem()
    n = M.shape[0]
    v = np.random.default_rng(3).uniform(3.0, 6.0, n)
    kw = {"x0": dict(x0=v, mean=0.5 * v), "mean": dict(mean=v), "zero": {}}[start]
    at = np.zeros(n) if start == "zero" else v
    be, fresh = gmrfx.MI355XBackend(M, device=0, factorize=False), gmrfx.MI355XBackend(M, device=0, factorize=False)
    try:
        for b in (be, fresh):
            b.set_prior(M.data, diag_positions(M))
        be.set_observations(1, y)
        x, hess, info = be.gaussian_approximation(max_iter=0, **kw)
        assert same_bits(x, at)
        assert info["iterations"] == 0 and info["converged"] is False and info["frozen_finish"] is False and np.isnan(info["newton_decrement"])
        assert info["alpha"] == 1.0 and len(info["dec_trace"]) == 0 and len(info["alpha_trace"]) == 0
        assert (info["factorizations"], info["solves"], info["merit_evaluations"]) == (0, 0, 0)
        assert same_bits(hess, be.fisher_eval(at, mean=kw.get("mean"))[1])
        x2, h2, i2 = be.gaussian_approximation(max_iter=0, refactorize_final=True, **kw)
        assert same_bits(x2, at) and same_bits(h2, hess) and i2["iterations"] == 0 and not i2["converged"]
        assert (i2["factorizations"], i2["solves"], i2["merit_evaluations"]) == (1, 0, 0)
        assert fresh.refactorize_update(hess) == 0
        assert be.compute_logdet() == fresh.compute_logdet()
    finally:
        be.close()
        fresh.close()


@pytest.mark.parametrize("start", ["x0", "mean", "zero"])
def test_batch_of_three(start):
    M, y = _problem()
    n, B = M.shape[0], 3
    Qs = bc.members(M, [(1.0, 0.0), (3.0, 0.5), (0.5, 2.0)])
    NZ = bc.values(Qs)
    V = np.asfortranarray(np.random.default_rng(4).uniform(3.0, 6.0, (n, B)))
    kw = {"x0": dict(x0=V, mean=0.5 * V), "mean": dict(mean=V), "zero": {}}[start]
    at = np.zeros((n, B)) if start == "zero" else V
    bb, fresh = gmrfx.MI355XBatchLaplace(M, B, device=0), gmrfx.MI355XBatchBackend(M, B, device=0)
    try:
        bb.set_prior(NZ)
        bb.set_observations(1, y)
        X, H, info = bb.gaussian_approximation(max_iter=0, **kw)
        assert same_bits(X, at) and info["posdef"] and (info["info"] == 0).all()
        assert (info["iterations"] == 0).all() and not info["converged"].any() and not info["frozen_finish"].any() and np.isnan(info["decrement"]).all()
        assert (info["alpha"] == 1.0).all() and all(len(t) == 0 for t in info["dec_trace"] + info["alpha_trace"])
        assert not info["factorizations"].any() and not info["solves"].any() and not info["merit_evaluations"].any()
        assert info["totals"] == {"factorizations": 0, "solves": 0, "evaluations": 1}          # (the evaluation at the modes)
        assert same_bits(H, bb.fisher_eval(at, mean=kw.get("mean"))[1])
        X2, H2, i2 = bb.gaussian_approximation(max_iter=0, refactorize_final=True, **kw)
        assert same_bits(X2, at) and same_bits(H2, H) and (i2["iterations"] == 0).all() and not i2["converged"].any()
        assert (i2["factorizations"] == 1).all() and not i2["solves"].any() and i2["totals"]["factorizations"] == 1
        NZpost = NZ.copy(order="F")
        NZpost[diag_positions(M), :] -= H
        assert (fresh.refactorize_values(NZpost) == 0).all()
        assert same_bits(bb.logdet(), fresh.logdet())
    finally:
        bb.close()
        fresh.close()
