"""The restatement of the reference's Fisher-scoring loop (tests/fisher_ref.py: newton_loop), host only: it reproduces the reference's
own small inputs, and the chosen loop cases (tests/fisher_loop_cases.py) provably reach every branch -- asserted on the trace."""
import numpy as np
import pytest

import fisher_loop_cases as lc
import fisher_ref as ref

CASES = lc.cases()


def test_normal_identity_is_the_closed_form_after_one_iterate():
    rng = np.random.default_rng(0)
    Q = lc.dense(lc.load("sprand_spd_60"))
    n, sigma = 60, 0.7
    mu, y = rng.standard_normal(n), rng.standard_normal(n)
    obs = ref.Obs(0, None, y, None, sigma)
    r = ref.newton_loop(Q, mu, obs, max_iter=1, adaptive=False, predictive=False, mean_tol=0.0, dec_tol=0.0)
    want = np.linalg.solve(Q + np.eye(n) / sigma ** 2, Q @ mu + y / sigma ** 2)
    assert np.abs(r["x"] - want).max() <= 1e-13 * np.abs(want).max()
    full = ref.newton_loop(Q, mu, obs)
    assert full["converged"] and np.abs(full["x"] - want).max() <= 1e-12 * np.abs(want).max()


def test_reference_constrained_poisson_input():
    c = CASES["eye8_sum0"]
    r = lc.restate(c, np.float64)
    assert r["converged"] and abs(r["x"].sum()) <= 8 * ref.EPS * np.abs(r["x"]).sum()
    # stationarity on the constraint's null space: the projected gradient vanishes
    g = (r["x"] - (c["obs"].y - np.exp(r["x"])))
    assert np.abs(g - g.mean()).max() <= 1e-8


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_branches_and_are_no_knife_edges(name):
    c = CASES[name]
    a, b = lc.restate(c, np.float64), lc.restate(c, ref.LD)
    print(name, a["iterations"], a["alpha_trace"], a["events"])
    assert c["events"] <= set(a["events"]), a["events"]
    assert np.array_equal(a["alpha_trace"], b["alpha_trace"]) and a["iterations"] == b["iterations"] and a["events"] == b["events"]
    if "retry_full_accept" in c["events"]:      # a full-step acceptance AFTER a backtrack
        assert a["events"].index("backtrack") < a["events"].index("retry_full_accept")
    if a["converged"]:
        assert ref.decrement_at(lc.dense(c["Q"]), None, c["obs"], b["x"], c["A"]) < 1e-5


def test_every_branch_is_covered_by_some_case():
    need = {"backtrack", "retry_full_accept", "retry_full_reject", "lookahead_fire", "frozen_return", "lookahead_reject", "max_iter"}
    got = set()
    for c in CASES.values():
        got |= set(lc.restate(c, np.float64)["events"])
    assert need <= got
