"""gmrfx_gaussian_approximation in design form on the device against the restatement of the reference's loop with a design matrix
(tests/fisher_design_ref.py: newton_loop; cases: loop_cases, selected on the CPU by far_from_thresholds, which
tests/test_fisher_design_host.py re-checks: no merit within 1000 noise floors of its acceptance threshold, no convergence quantity
within 1e-3 of its tolerance).

Per case: the same iteration count, alpha trace EXACTLY and counters as the float64 restatement. The mode against the long-double one:
the device stops where the float64 loop stops, at a point whose distance from the exact mode is governed by the last Newton
decrement, |x - x*|_2 <= sqrt(dec / lambda_min(Q_k)); two runs of the same loop in different arithmetic differ by the rounding of one
Newton step, which is bounded by cond(Q_k) eps |x| -- the bound used is 64 cond(Q_k) eps max|x| (cond(Q_k) of the case, computed here
from the long-double run's last Q_k), printed beside the measured difference. hess (cnt values in map order) against A' D A at the
device's own mode. Independently of any tolerance the long-double Newton decrement at the returned mode is below newton_dec_tol. The decrement trace against the long-double one within 64 x the
restatement's own float64-vs-long-double difference, as the node form's loop test.
A planted indefinite Q_p: NOT_POSDEF with info set, x = x0 and the handle usable."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fisher_design_ref as dref
import fisher_ref as ref
import gmrfx
from gmrfx._lib import PosDefException
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
CASES = dref.loop_cases()
DEV = "cuda:0"


def _backend(c):
    Q = c["Q"]
    be = gmrfx.MI355XBackend(Q, device=0, uplo=c["uplo"], factorize=False)
    o = c["obs"]
    be.set_design_observations(o.family, o.y, c["A"], c["b"], o.aux, o.param)
    be.set_prior(Q.data, be.observations_hess_map())
    if c["C"] is not None:
        be.set_constraints(sp.csr_matrix(c["C"]), np.zeros(c["C"].shape[0]))
    return be


@pytest.mark.parametrize("name", list(CASES))
def test_whole_loop(name):
    c = CASES[name]
    a, b = dref.restate_loop(c, np.float64), dref.restate_loop(c, ref.LD)
    be = _backend(c)
    try:
        n = c["Q"].shape[0]
        x, hess, info = be.gaussian_approximation(x0=c["x0"])
        assert info["iterations"] == a["iterations"] and info["converged"] == a["converged"] and info["frozen_finish"] == a["frozen"]
        assert np.array_equal(info["alpha_trace"], a["alpha_trace"]), (info["alpha_trace"], a["alpha_trace"])
        assert (info["factorizations"], info["solves"], info["merit_evaluations"]) == (a["factorizations"], a["solves"], a["merit_evaluations"])
        cond = float(np.linalg.cond(np.asarray(b["Qk"], np.float64)))
        tol_x = 64 * cond * ref.EPS * float(np.abs(b["x"]).max())
        err_x = float(np.abs(x - b["x"]).max())
        own_x = float(np.abs(np.asarray(a["x"], ref.LD) - b["x"]).max())
        print(f"{name}: cond(Q_k) {cond:.2e} last decrement {float(b['dec_trace'][-1]):.2e}; float64 restatement vs long double {own_x:.2e}, "
              f"device vs long double {err_x:.2e}, bound {tol_x:.2e}")
        assert err_x <= tol_x
        # the decrement trace against the long-double one, as tests/test_gpu_fisher_loop.py: 64 x the restatement's own float64-vs-
        # long-double difference on the case (floor: 64 eps of the trace's scale)
        decb = np.asarray(b["dec_trace"], ref.LD)
        own_dec = float(np.abs(np.asarray(a["dec_trace"], ref.LD) - decb).max())
        tol_dec = 64 * max(own_dec, ref.EPS * float(np.abs(decb).max()))
        err_dec = float(np.abs(info["dec_trace"] - decb).max())
        print(f"{name}: decrement trace, restatement float64 vs long double {own_dec:.2e}, device vs long double {err_dec:.2e}, bound {tol_dec:.2e}")
        assert err_dec <= tol_dec
        # hess = the values of A' D A at the returned mode, in map order
        m = be.observations_hess_map()
        assert hess.shape == m.shape
        r = dref.eval_ref(c, c["obs"], x, None)
        assert (np.abs(hess - r["hess"]) <= dref.bounds(r, 16)[1]).all()
        if c["C"] is not None:
            assert np.abs(c["C"] @ x).max() <= 64 * info["solves"] * ref.EPS * np.abs(c["C"]).sum() * max(np.abs(x).max(), 1.0)
        D = c["Q"].toarray()
        S = np.triu(D) + np.triu(D, 1).T
        one = dref.newton_loop(S, None, c["obs"], c["A"].toarray(), b=c["b"], x0=x, A=c["C"], dtype=ref.LD, max_iter=1, adaptive=False,
                               predictive=False, mean_tol=0.0, dec_tol=0.0)
        assert float(one["dec_trace"][0]) < 1e-5
        # two runs and the device form give the same bits
        x2, h2, i2 = be.gaussian_approximation(x0=c["x0"])
        assert same_bits(x, x2) and same_bits(hess, h2) and same_bits(info["dec_trace"], i2["dec_trace"])
        dx = torch.empty(n, dtype=torch.float64, device=DEV)
        dh = torch.empty(len(m), dtype=torch.float64, device=DEV)
        d0 = None if c["x0"] is None else torch.from_numpy(c["x0"]).to(DEV)
        torch.cuda.synchronize()
        i3 = be.gaussian_approximation_dev(dx.data_ptr(), dh.data_ptr(), d_x0=0 if d0 is None else d0.data_ptr())
        torch.cuda.synchronize()
        assert same_bits(dx.cpu().numpy(), x) and same_bits(dh.cpu().numpy(), hess) and same_bits(i3["dec_trace"], info["dec_trace"])
    finally:
        be.close()


def test_indefinite_prior_is_reported_and_the_handle_stays_usable():
    c = CASES["mesh_far8"]
    Q = c["Q"]
    be = _backend(c)
    try:
        m = be.observations_hess_map()
        bad = Q.data.copy()
        bad[diag_positions(Q)] = -1e6
        be.set_prior(bad, m)
        x0 = np.zeros(Q.shape[0])
        with pytest.raises(PosDefException):
            be.gaussian_approximation(x0=x0)
        assert be.last_info > 0 and np.array_equal(be.last_x, x0)
        be.set_prior(Q.data, m)
        x, _, info = be.gaussian_approximation(x0=c["x0"])
        a = dref.restate_loop(c, np.float64)
        assert info["converged"] and np.array_equal(info["alpha_trace"], a["alpha_trace"])
    finally:
        be.close()
