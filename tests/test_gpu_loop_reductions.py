"""The four reductions of the Newton loop (csrc/fisher.hip: k_fisher_stats, k_fisher_stats_final) against long double at their size
edges, read off one iterate whose operands are known bit for bit (tests/loop_reduction_ref.py explains each check and derives each
bound; tests/test_loop_reductions_host.py shows that the checks catch a reduction that drops entries):

* sum a b: the decrement of the trace against the long-double score' step within 16 depth(n) eps sum |score_i step_i|;
* sum (c - d)^2, sum d^2: `converged` with mean_change_tol a factor 1 -+ 1e-12 from the long-double deciding value, from x0 = 0 and
  from an x0 of norm >= 1;
* max |b|: the tiny-step exit with newton_dec_tol a factor 1 +- 1e-9 from 1000 * 0.1 * |step|_inf, with |step|_inf placed at the
  first and last entry, both sides of a thread's second entry and both sides of a chunk.

n = 255 .. 8193 on a plain handle and in a batch of two members of different scale; n = 256 * 4096 + 1 (k_fisher_stats_final's strided
loop) on a plain handle."""
import numpy as np
import pytest

import batch_laplace_cases as bc
import gmrfx
import loop_reduction_ref as lr
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
ONE = dict(max_iter=1, adaptive_stepsize=False, predictive_convergence=False, mean_change_tol=0.0, newton_dec_tol=0.0)
SEARCH = dict(max_iter=1, predictive_convergence=False, mean_change_tol=0.0)
SCALES = [(1.0, 0.0), (3.0, 0.5)]


def _plain(Q, y):
    be = gmrfx.MI355XBackend(Q, device=0, factorize=False)
    try:
        be.set_prior(Q.data, diag_positions(Q))
        be.set_observations(1, y)
    except Exception:
        be.close()
        raise
    return be


@pytest.mark.parametrize("n", lr.SIZES + (lr.BIG,))
def test_plain_handle(n):
    Q, y = lr.problem(n)
    z = np.zeros(n)
    be = _plain(Q, y)
    try:
        # sum a b
        x1, _, info = be.gaussian_approximation(x0=z, **ONE)
        step = z - x1                                   # x_1 = 0 - 1 step: exact
        score = be.fisher_eval(z)[0]
        assert same_bits(score, be.fisher_eval(z)[0])
        dec = info["dec_trace"][0]
        err = float(abs(lr.LD(dec) - lr.reduce_ld(score, step, None, None)[0]))
        print(f"n = {n}: decrement {dec:.6e}, error {err:.2e}, bound {lr.dec_bound(score, step):.2e}")
        assert lr.dec_ok(dec, score, step)
        # sum (c - d)^2 alone (x0 = 0), then with sum d^2
        for x0 in (z, lr.start(n)):
            x1 = be.gaussian_approximation(x0=x0, **ONE)[0]
            assert min(lr.smallest_terms(score, step, x1, x0)[1:]) >= lr.TERM_FLOOR
            v = lr.deciding(x1, x0)
            for side in (-1, +1):
                xs, _, i = be.gaussian_approximation(x0=x0, **dict(ONE, mean_change_tol=lr.bracket(v, side)))
                assert same_bits(xs, x1) and i["converged"] == (side > 0), (float(v), side)
        # max |b|
        for p in (lr.peak_positions(n) if n != lr.BIG else [n - 1]):
            be.set_observations(1, lr.peaked(n, p))
            a = np.abs(be.gaussian_approximation(x0=z, **ONE)[0])
            assert int(a.argmax()) == p
            sinf = float(a[p])
            _, _, up = be.gaussian_approximation(x0=z, newton_dec_tol=lr.max_tol(sinf, +1), **SEARCH)
            _, _, dn = be.gaussian_approximation(x0=z, newton_dec_tol=lr.max_tol(sinf, -1), **SEARCH)
            assert up["merit_evaluations"] == 1 and up["alpha"] == 0.1, (p, up)
            assert dn["merit_evaluations"] >= 2, (p, dn)
    finally:
        be.close()


@pytest.mark.parametrize("n", lr.SIZES)
def test_batch_of_two_scales(n):
    Q, y = lr.problem(n)
    Qs = bc.members(Q, SCALES)
    B = len(Qs)
    Z = np.zeros((n, B))
    bb = gmrfx.MI355XBatchLaplace(Q, B, device=0)
    try:
        bb.set_prior(bc.values(Qs))
        bb.set_observations(1, y)
        X1, _, info = bb.gaussian_approximation(x0=Z, **ONE)
        S = bb.fisher_eval(Z)[0]
        assert same_bits(S, bb.fisher_eval(Z)[0])
        for k in range(B):
            step = Z[:, k] - X1[:, k]
            dec = info["dec_trace"][k][0]
            err = float(abs(lr.LD(dec) - lr.reduce_ld(S[:, k], step, None, None)[0]))
            print(f"n = {n} member {k}: decrement {dec:.6e}, error {err:.2e}, bound {lr.dec_bound(S[:, k], step):.2e}")
            assert lr.dec_ok(dec, S[:, k], step), k
        for X0 in (Z, np.repeat(lr.start(n)[:, None], B, axis=1) * np.array([1.0, 1.5])):
            X1 = bb.gaussian_approximation(x0=X0, **ONE)[0]
            for k in range(B):          # one tolerance for all members: member k's bracket decides member k's flag
                v = lr.deciding(X1[:, k], X0[:, k])
                for side in (-1, +1):
                    Xs, _, i = bb.gaussian_approximation(x0=X0, **dict(ONE, mean_change_tol=lr.bracket(v, side)))
                    assert same_bits(Xs, X1) and i["converged"][k] == (side > 0), (k, float(v), side)
        for p in lr.peak_positions(n):
            bb.set_observations(1, lr.peaked(n, p))
            A = np.abs(bb.gaussian_approximation(x0=Z, **ONE)[0])
            assert (A.argmax(0) == p).all()
            assert A[p, 0] != A[p, 1]
            for k in range(B):
                sinf = float(A[p, k])
                _, _, up = bb.gaussian_approximation(x0=Z, newton_dec_tol=lr.max_tol(sinf, +1), **SEARCH)
                _, _, dn = bb.gaussian_approximation(x0=Z, newton_dec_tol=lr.max_tol(sinf, -1), **SEARCH)
                assert up["merit_evaluations"][k] == 1 and up["alpha"][k] == 0.1, (p, k)
                assert dn["merit_evaluations"][k] >= 2, (p, k)
    finally:
        bb.close()
