"""gmrfx_gaussian_approximation on the device against the restatement of the reference's loop (tests/fisher_ref.py: newton_loop).

Per case of tests/fisher_loop_cases.py: the same iteration count, the same alpha trace EXACTLY and the same counters as the float64
restatement; decrement trace and mode against the long-double restatement within 64 x the float64-vs-long-double difference of the
restatement itself on that case (measured on the CPU, printed beside the device's; floor: 64 eps of the quantity's scale, for the
cases where the two restatements agree to the last bit). The measured values of every case are recorded in the header of
tests/fisher_loop_cases.py.
Independently of any tolerance the long-double Newton decrement at the returned mode is below newton_dec_tol for converged cases.
One iterate: the loop's first step is, bit for bit, gmrfx_refactorize_update_solve_dev fed with gmrfx_fisher_eval_dev's outputs (plus
the constraint projection by the untouched gmrfx_constraints_correct_dev on an e = 0 handle, after which A step = 0 within
m eps |A| |step|); on a handle holding e = 0.5 the loop gives the same bits: the projection ignores e. Flag bit 3: logdet and the selected
inverse's diagonal equal those of a handle refactorised with Q_prior - diag(hess_out), bit for bit. An indefinite prior: NOT_POSDEF
with info set, x = x0, and the handle usable. A handle without a likelihood: gmrfx_refactorize_update_solve_dev and
gmrfx_constraints_correct_dev give the same bits before and after the handle has run a loop."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fisher_loop_cases as lc
import fisher_ref as ref
import gmrfx
from gmrfx._lib import PosDefException
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
CASES = lc.cases()
DEV = "cuda:0"


def _backend(c, e=0.0):
    Q = c["Q"]
    be = gmrfx.MI355XBackend(Q, device=0, factorize=False)
    be.set_prior(Q.data, diag_positions(Q))
    o = c["obs"]
    be.set_observations(o.family, o.y, o.idx, o.aux, o.param)
    if c["A"] is not None:
        be.set_constraints(sp.csr_matrix(c["A"]), np.full(c["A"].shape[0], e))
    return be


def _kw(c):
    k = dict(c["kw"])
    out = {}
    if "max_iter" in k:
        out["max_iter"] = k["max_iter"]
    if k.get("retry_full") is False:
        out["step_recovery"] = "sqrt"
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_whole_loop(name):
    c = CASES[name]
    a, b = lc.restate(c, np.float64), lc.restate(c, ref.LD)
    be = _backend(c)
    try:
        x, hess, info = be.gaussian_approximation(x0=c["x0"], **_kw(c))
        assert info["iterations"] == a["iterations"] and info["converged"] == a["converged"] and info["frozen_finish"] == a["frozen"]
        assert np.array_equal(info["alpha_trace"], a["alpha_trace"]), (info["alpha_trace"], a["alpha_trace"])
        assert (info["factorizations"], info["solves"], info["merit_evaluations"]) == (a["factorizations"], a["solves"], a["merit_evaluations"])
        decb = np.asarray(b["dec_trace"], ref.LD)
        own_dec = float(np.abs(np.asarray(a["dec_trace"], ref.LD) - decb).max())
        own_x = float(np.abs(np.asarray(a["x"], ref.LD) - b["x"]).max())
        tol_dec = 64 * max(own_dec, ref.EPS * float(np.abs(decb).max()))
        tol_x = 64 * max(own_x, ref.EPS * float(np.abs(b["x"]).max()))
        err_dec = float(np.abs(info["dec_trace"] - decb).max())
        err_x = float(np.abs(x - b["x"]).max())
        print(f"{name}: restatement f64-vs-ld dec {own_dec:.2e} x {own_x:.2e}; device-vs-ld dec {err_dec:.2e} x {err_x:.2e}")
        assert err_dec <= tol_dec and err_x <= tol_x
        assert np.abs(hess - np.asarray(ref.pointwise(1, x, c["obs"].y, None, 0.0)[1], float)).max() <= 64 * ref.EPS * np.abs(hess).max()
        if c["A"] is not None:       # the iterates never leave the constraint's null space (x0 = 0)
            assert np.abs(c["A"] @ x).max() <= 64 * info["solves"] * ref.EPS * np.abs(c["A"]).sum() * max(np.abs(x).max(), 1.0)
        if info["converged"]:
            assert ref.decrement_at(lc.dense(c["Q"]), None, c["obs"], x, c["A"]) < 1e-5
        # two runs and the device form give the same bits
        x2, h2, i2 = be.gaussian_approximation(x0=c["x0"], **_kw(c))
        assert same_bits(x, x2) and same_bits(hess, h2) and same_bits(info["dec_trace"], i2["dec_trace"])
        dx, dh = torch.empty(len(x), dtype=torch.float64, device=DEV), torch.empty(len(x), dtype=torch.float64, device=DEV)
        d0 = None if c["x0"] is None else torch.from_numpy(c["x0"]).to(DEV)
        torch.cuda.synchronize()
        i3 = be.gaussian_approximation_dev(dx.data_ptr(), dh.data_ptr(), d_x0=0 if d0 is None else d0.data_ptr(), **_kw(c))
        torch.cuda.synchronize()
        assert same_bits(dx.cpu().numpy(), x) and same_bits(dh.cpu().numpy(), hess) and same_bits(i3["dec_trace"], info["dec_trace"])
    finally:
        be.close()


@pytest.mark.parametrize("name", ["matern_far8", "eye8_sum0", "besag9x7_sum0"])
def test_first_step_is_the_existing_entry_points_bit_for_bit(name):
    """x_1 = x_0 - step with step = gmrfx_refactorize_update_solve_dev on gmrfx_fisher_eval_dev's outputs, then (with a constraint, on a
    handle whose e is zero) gmrfx_constraints_correct_dev: the same kernels, s - 0.0 keeps the bits"""
    c = CASES[name]
    n = c["Q"].shape[0]
    be = _backend(c)
    try:
        x0 = np.zeros(n) if c["x0"] is None else c["x0"]
        x1, _, info = be.gaussian_approximation(x0=x0, max_iter=1, adaptive_stepsize=False, predictive_convergence=False,
                                                mean_change_tol=0.0, newton_dec_tol=0.0)
        dxk = torch.from_numpy(x0).to(DEV)
        ds, dh, dst = (torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(3))
        torch.cuda.synchronize()
        be.fisher_eval_dev(dxk.data_ptr(), 0, ds.data_ptr(), dh.data_ptr())
        be.refactorize_update_solve_dev(dh.data_ptr(), ds.data_ptr(), n, 1, dst.data_ptr(), n)
        if c["A"] is not None:
            be.constraint_correct_dev(dst.data_ptr(), n, 1)
        torch.cuda.synchronize()
        step = dst.cpu().numpy()
        assert same_bits(x1, x0 - step)
        if c["A"] is not None:
            A = c["A"]
            assert np.abs(A @ step).max() <= A.shape[0] * ref.EPS * np.abs(A).sum() * np.abs(step).max()
    finally:
        be.close()


@pytest.mark.parametrize("name", ["eye8_sum0", "besag9x7_sum0", "besag9x7_sqrt"])
def test_the_projection_ignores_the_constraint_right_hand_side(name):
    """the step is projected with e = 0 whatever e the handle holds (_workspace_constrain_with_matrix): a handle with e = 0.5 runs the
    loop to the same bits as one with e = 0, and A step = 0 within m eps |A| |step| (an inhomogeneous correction would leave A step = e)"""
    c = CASES[name]
    n = c["Q"].shape[0]
    b0, b1 = _backend(c), _backend(c, e=0.5)
    try:
        x0 = np.zeros(n)
        s0 = b0.gaussian_approximation(x0=x0, max_iter=1, adaptive_stepsize=False, predictive_convergence=False, mean_change_tol=0.0,
                                       newton_dec_tol=0.0)[0]
        s1 = b1.gaussian_approximation(x0=x0, max_iter=1, adaptive_stepsize=False, predictive_convergence=False, mean_change_tol=0.0,
                                       newton_dec_tol=0.0)[0]
        A = c["A"]
        step = x0 - s1
        assert np.abs(step).max() > 0.1
        assert np.abs(A @ step).max() <= A.shape[0] * ref.EPS * np.abs(A).sum() * np.abs(step).max()
        assert same_bits(s0, s1)
        xa, ha, ia = b0.gaussian_approximation(**_kw(c))
        xb, hb, ib = b1.gaussian_approximation(**_kw(c))
        assert same_bits(xa, xb) and same_bits(ha, hb) and same_bits(ia["dec_trace"], ib["dec_trace"])
        assert np.array_equal(ia["alpha_trace"], ib["alpha_trace"])
    finally:
        b0.close()
        b1.close()


def test_flag_bit_3_leaves_the_factor_of_the_mode():
    c = CASES["matern_far8"]
    Q = c["Q"]
    be, other = _backend(c), gmrfx.MI355XBackend(c["Q"], device=0, factorize=False)
    try:
        x, hess, info = be.gaussian_approximation(x0=c["x0"], refactorize_final=True)
        other.set_prior(Q.data, diag_positions(Q))
        other.refactorize_update(hess)
        assert be.compute_logdet() == other.compute_logdet()
        assert same_bits(be.get_selinv_diag(), other.get_selinv_diag())
        assert info["factorizations"] == lc.restate(c, np.float64)["factorizations"] + 1
    finally:
        be.close()
        other.close()


def test_indefinite_prior_is_reported_and_the_handle_stays_usable():
    c = CASES["matern_far8"]
    Q = c["Q"]
    be = _backend(c)
    try:
        bad = Q.data.copy()
        bad[diag_positions(Q)] = -1e6          # (Q_prior - H = Q_prior + mu stays indefinite: mu = 1 at x0 = 0)
        be.set_prior(bad, diag_positions(Q))
        x0 = np.zeros(Q.shape[0])
        with pytest.raises(PosDefException):
            be.gaussian_approximation(x0=x0)
        assert be.last_info > 0 and np.array_equal(be.last_x, x0)
        be.set_prior(Q.data, diag_positions(Q))
        x, _, info = be.gaussian_approximation(x0=c["x0"])
        a = lc.restate(c, np.float64)
        assert info["converged"] and np.array_equal(info["alpha_trace"], a["alpha_trace"])
    finally:
        be.close()


def test_handles_without_a_likelihood_are_unchanged():
    c = CASES["matern_far8"]
    Q = c["Q"]
    n = Q.shape[0]
    A = sp.csr_matrix(np.ones((1, n)))
    rng = np.random.default_rng(4)
    hv, rhs = -rng.uniform(0.1, 1.0, n), rng.standard_normal(n)

    def run(be):
        dh, db = torch.from_numpy(hv).to(DEV), torch.from_numpy(rhs).to(DEV)
        dX = torch.empty(n, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        be.refactorize_update_solve_dev(dh.data_ptr(), db.data_ptr(), n, 1, dX.data_ptr(), n)
        X = dX.cpu().numpy()
        be.constraint_correct_dev(dX.data_ptr(), n, 1)
        torch.cuda.synchronize()
        return X, dX.cpu().numpy()

    plain = gmrfx.MI355XBackend(Q, device=0, factorize=False)
    used = gmrfx.MI355XBackend(Q, device=0, factorize=False)
    try:
        for be in (plain, used):
            be.set_prior(Q.data, diag_positions(Q))
            be.set_constraints(A, np.array([0.5]))
        X0, C0 = run(plain)
        o = c["obs"]
        used.set_observations(o.family, o.y)
        used.gaussian_approximation(x0=c["x0"])
        used.set_observations(1, np.zeros(0))
        X1, C1 = run(used)
        assert same_bits(X0, X1) and same_bits(C0, C1)
    finally:
        plain.close()
        used.close()
