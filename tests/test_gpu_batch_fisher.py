"""gmrfx_batch_fisher_eval on the device: member k's score, hess, energy and loglik are, bit for bit, MI355XBackend.fisher_eval_dev on a
plain handle holding Q_p,k and param[k] (whose own test bounds it against tests/fisher_ref.py: the bound carries over through the
equality). Shapes of tests/batch_laplace_cases.py (n = 1, 15, 16, 17, 40 arrowhead, 60, 256, 4097) x B = 1, 2, 3, 50, all six families
with a distinct parameter per member, an observed subset, a shared and a per-member mean, an offset base pointer and a stride above n,
eta = +-700 for the logit families. Host and _dev forms and two runs agree bit for bit; masked-out members keep a NaN frame and leave
the active members' bits alone. The candidate and reduction kernels: max_iter = 1 loops give x_1 = x_0 - alpha_k step_k with the bits
of the plain loop's first iterate on Q_k, with and without adaptive_stepsize."""
import numpy as np
import pytest
import torch

import batch_laplace_cases as bc
import fisher_ref as ref
import gmrfx
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = bc.eval_shapes()
# every shape with B = 3; the batch sizes on the shapes that cross a workgroup (tri17) and a chunk of the reductions (tri4097)
COMBOS = [(s, 3) for s in SHAPES] + [("tri17", 1), ("tri17", 2), ("tri17", 50), ("tri4097", 2), ("matern256", 50)]


def _plain_eval(Q, obs, param, x, mu):
    """(score, hess, energy, loglik) of fisher_eval_dev on a plain handle of Q"""
    n = Q.shape[0]
    be = gmrfx.MI355XBackend(Q, device=0, factorize=False)
    try:
        be.set_prior(Q.data, diag_positions(Q))
        be.set_observations(obs.family, obs.y, obs.idx, obs.aux, param)
        dx = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        dm = None if mu is None else torch.from_numpy(np.ascontiguousarray(mu)).to(DEV)
        ds, dh = (torch.full((n,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
        torch.cuda.synchronize()
        e, l = be.fisher_eval_dev(dx.data_ptr(), 0 if dm is None else dm.data_ptr(), ds.data_ptr(), dh.data_ptr())
        torch.cuda.synchronize()
        return ds.cpu().numpy(), dh.cpu().numpy(), e, l
    finally:
        be.close()


def _batch(Qs, obs, params):
    bb = gmrfx.MI355XBatchLaplace(Qs[0], len(Qs), device=0)
    bb.set_prior(bc.values(Qs))
    bb.set_observations(obs.family, obs.y, obs.idx, obs.aux, params)
    return bb


@pytest.mark.parametrize("shape,B", COMBOS, ids=[f"{s}-B{b}" for s, b in COMBOS])
def test_every_member_has_the_bits_of_its_plain_handle(shape, B):
    M = SHAPES[shape]
    n = M.shape[0]
    Qs = bc.eval_members(M, B)
    rng = np.random.default_rng(n + B)
    for family in range(6):
        which = "subset" if family % 2 else "all"
        obs = ref.make_obs(family, n, rng, which)
        params = bc.family_params(family, B)
        X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, B)))
        if family in (2, 3):           # the logit families at eta = +-700
            X[0, :] = 700.0
            X[-1, :] = -700.0
        shared = family < 3
        mean = rng.standard_normal(n) if shared else np.asfortranarray(rng.standard_normal((n, B)))
        bb = _batch(Qs, obs, params)
        try:
            S, H, en, ll = bb.fisher_eval(X, mean)
            S2, H2, en2, ll2 = bb.fisher_eval(X, mean)
            assert same_bits(S, S2) and same_bits(H, H2) and same_bits(en, en2) and same_bits(ll, ll2)
            # device form: an offset base pointer and a stride above n, inside NaN-filled buffers
            sx = n + 3
            bx = torch.full((B * sx + 1,), float("nan"), dtype=torch.float64, device=DEV)
            bs, bh = (torch.full((B * sx + 1,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
            for k in range(B):
                bx[1 + k * sx:1 + k * sx + n] = torch.from_numpy(X[:, k].copy()).to(DEV)
            dm = torch.from_numpy(np.ascontiguousarray(mean.T if not shared else mean).reshape(-1).copy()).to(DEV)
            torch.cuda.synchronize()
            en3, ll3 = bb.fisher_eval_dev(bx.data_ptr() + 8, sx, dm.data_ptr(), 0 if shared else n, None, bs.data_ptr() + 8, bh.data_ptr() + 8, sx)
            torch.cuda.synchronize()
            hs, hh = bs.cpu().numpy(), bh.cpu().numpy()
            assert np.isnan(hs[0]) and np.isnan(hh[0])
            for k in range(B):
                assert same_bits(hs[1 + k * sx:1 + k * sx + n], S[:, k]) and same_bits(hh[1 + k * sx:1 + k * sx + n], H[:, k])
                assert np.isnan(hs[1 + k * sx + n:1 + (k + 1) * sx]).all() and np.isnan(hh[1 + k * sx + n:1 + (k + 1) * sx]).all()
            assert same_bits(en3, en) and same_bits(ll3, ll)
            for k in (range(B) if B <= 3 else (0, B // 2, B - 1)):
                ps, ph, pe, pl = _plain_eval(Qs[k], obs, params[k], X[:, k], mean if shared else mean[:, k])
                assert same_bits(ps, S[:, k]) and same_bits(ph, H[:, k]), (family, k)
                assert pe == en[k] and pl == ll[k], (family, k, pe, en[k], pl, ll[k])
            assert np.isfinite(S).all() and np.isfinite(H).all()
        finally:
            bb.close()


@pytest.mark.parametrize("shape,B", [("tri17", 3), ("arrow40", 50), ("tri4097", 2)])
def test_masked_members_keep_their_frame(shape, B):
    M = SHAPES[shape]
    n = M.shape[0]
    rng = np.random.default_rng(3)
    obs = ref.make_obs(4, n, rng, "all")
    bb = _batch(bc.eval_members(M, B), obs, bc.family_params(4, B))
    try:
        X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, B)))
        S, H, en, ll = bb.fisher_eval(X)
        active = np.arange(B) % 2 == 0 if B > 2 else np.array([False, True])
        S2, H2, en2, ll2 = bb.fisher_eval(X, active=active)
        assert same_bits(S2[:, active], S[:, active]) and same_bits(H2[:, active], H[:, active])
        assert same_bits(en2[active], en[active]) and same_bits(ll2[active], ll[active])
        assert np.isnan(S2[:, ~active]).all() and np.isnan(H2[:, ~active]).all() and np.isnan(en2[~active]).all() and np.isnan(ll2[~active]).all()
    finally:
        bb.close()


@pytest.mark.parametrize("shape,B,adaptive", [("tri17", 3, False), ("tri17", 3, True), ("tri4097", 2, True), ("arrow40", 50, False),
                                              ("matern256", 3, True)])
def test_first_iterate_has_the_bits_of_the_plain_loop(shape, B, adaptive):
    """max_iter = 1: x_1 = x_0 - alpha_k step_k through k_fisher_candidate and the reductions with more than one member; Poisson with large counts
    from x0 = 0 backtracks under adaptive_stepsize"""
    M = SHAPES[shape]
    n = M.shape[0]
    Qs = bc.eval_members(M, B, seed=1)
    obs = ref.Obs(1, None, np.random.default_rng(5).poisson(200.0, n).astype(float), None, 0.0)
    kw = dict(max_iter=1, adaptive_stepsize=adaptive, predictive_convergence=False, mean_change_tol=0.0, newton_dec_tol=0.0)
    bb = _batch(Qs, obs, np.zeros(B))
    try:
        X, H, info = bb.gaussian_approximation(x0=np.zeros((n, B)), **kw)
        assert (info["info"] == 0).all()
        for k in (range(B) if B <= 3 else (0, B - 1)):
            be = gmrfx.MI355XBackend(Qs[k], device=0, factorize=False)
            try:
                be.set_prior(Qs[k].data, diag_positions(Qs[k]))
                be.set_observations(1, obs.y)
                x, h, pi = be.gaussian_approximation(x0=np.zeros(n), **kw)
            finally:
                be.close()
            assert same_bits(x, X[:, k]) and same_bits(h, H[:, k]), k
            assert pi["alpha"] == info["alpha"][k] and same_bits(pi["dec_trace"], info["dec_trace"][k])
            assert (pi["factorizations"], pi["solves"], pi["merit_evaluations"]) == (
                info["factorizations"][k], info["solves"][k], info["merit_evaluations"][k])
        if adaptive:
            assert (info["alpha"] < 1.0).any()
    finally:
        bb.close()
