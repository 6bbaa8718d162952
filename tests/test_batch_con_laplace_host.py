"""Constrained batched Laplace, host only: the C ABI of gmrfx_batch_constrained_gaussian_approximation[_dev] and
gmrfx_batch_obs_set_param on symbolic-only handles (declared, exported, the refusals in the documented order, then NO_DEVICE;
gmrfx_batch_set_prior accepts a handle that holds a batch constraint; the three refusals of the unconstrained calls still hold), and the
cases of tests/batch_con_laplace_cases.py: every member's float64 restatement converges, the cases contain the branches they are there
for, and cond(W_k) stays within the cap at x0 and at the mode."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_con_laplace_cases as cc
import batch_laplace_cases as bc
import fisher_ref as ref
from gmrfx._lib import EXPORTS, lib, ptr
from test_batch_laplace_host import INVALID_ARG, N, NO_DEVICE, ONES, P3, _eval, _ga, _Handle, _info, _msg, _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gmrfx_batch_constrained_gaussian_approximation", "gmrfx_batch_constrained_gaussian_approximation_dev", "gmrfx_batch_obs_set_param"]
CGA = NEW[:2]
CASES = cc.cases()
A_PTR, A_COL, A_VAL, E = np.array([0, N], np.int64), np.arange(N, dtype=np.int64), np.ones(N), np.zeros(1)


def _bcon(h, m=1):
    return lib().gmrfx_batch_constraints_set(h, m, ptr(A_PTR), ptr(A_COL), ptr(A_VAL), 0, ptr(E))


def _cga(h, B, fn=CGA[0], n=N, x=True, result=True, sx=None, sh=None, sx0=None, smu=None, flags=15, cinfo=True, residual=True):
    X, H, R, X0, mu = np.zeros(n * B), np.zeros(n * B), np.zeros(10 * B), np.zeros(n * B), np.zeros(n * B)
    ci, rs = np.zeros(B, np.int64), np.zeros(B)
    return getattr(lib(), fn)(h, ptr(mu) if smu is not None else None, smu or 0, ptr(X0) if sx0 is not None else None, sx0 or 0, 5, 5, 1e-4,
                              1e-5, flags, ptr(X) if x else None, n if sx is None else sx, ptr(H), n if sh is None else sh,
                              ptr(R) if result else None, None, None, None, None, ptr(ci) if cinfo else None, ptr(rs) if residual else None)


def test_header_declares_and_library_exports_every_new_call():
    hdr = open(os.path.join(ROOT, "include", "gmrfx.h")).read()
    L = lib()
    for nm in NEW:
        assert re.search(r"int32_t " + nm + r"\(", hdr), nm
        assert nm in EXPORTS
        getattr(L, nm)


@pytest.mark.parametrize("fn", CGA)
def test_the_constrained_call_refuses_in_the_documented_order_then_answers_no_device(fn):
    with _Handle(3) as h:
        # no batch constraint held: the message names the unconstrained call
        assert _cga(h, 3, fn) == INVALID_ARG and "no batch constraint" in _msg(h) and "gmrfx_batch_gaussian_approximation" in _msg(h)
        assert _bcon(h) == 0, _msg(h)
        assert _cga(h, 3, fn, x=False) == INVALID_ARG and "x / result is null" in _msg(h)
        assert _cga(h, 3, fn, result=False) == INVALID_ARG and "x / result is null" in _msg(h)
        for flags in (16, -1):
            assert _cga(h, 3, fn, flags=flags) == INVALID_ARG and "flag bits" in _msg(h)
        assert _cga(h, 3, fn) == INVALID_ARG and "no observation likelihood" in _msg(h)
        # the likelihood goes in with the constraint cleared (gmrfx_batch_obs_set stays refused while one is held)
        assert _bcon(h, 0) == 0 and _set(h, 1, ONES, P3) == 0 and _bcon(h) == 0
        for kw in (dict(sx=N - 1), dict(sh=N - 1), dict(sx0=N - 1), dict(smu=N - 1)):
            assert _cga(h, 3, fn, **kw) == INVALID_ARG and "stride smaller than n" in _msg(h)
        before = _info(h, 3)
        assert _cga(h, 3, fn) == NO_DEVICE and "no device state" in _msg(h)
        assert _cga(h, 3, fn, cinfo=False, residual=False, smu=0) == NO_DEVICE
        assert _info(h, 3) == before
    with _Handle() as h:          # a plain constraint is not a batch constraint
        assert lib().gmrfx_constraints_set(h, 1, ptr(A_PTR), ptr(A_COL), ptr(A_VAL), 0, ptr(E)) == 0, _msg(h)
        assert _cga(h, 1, fn) == INVALID_ARG and "plain constraint" in _msg(h)
    with _Handle() as h:          # the design form on a plain handle, with a batch constraint (a plain handle is a batch of one)
        cp, rv = np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int64)
        assert lib().gmrfx_obs_set_design(h, 1, N, ptr(cp), ptr(rv), ptr(np.ones(N)), 0, None, ptr(ONES), None, 0.0) == 0, _msg(h)
        assert _bcon(h) == 0, _msg(h)
        assert _cga(h, 1, fn) == INVALID_ARG and "design form" in _msg(h)
    with _Handle(0, shard_world=2, shard_rank=0) as h:      # (a sharded handle cannot hold a batch constraint: the first refusal answers)
        assert _cga(h, 1, fn) == INVALID_ARG and "no batch constraint" in _msg(h)


def test_set_prior_accepts_a_batch_constraint_and_refuses_a_plain_one():
    nz = np.ones(16 * 3)
    with _Handle(3) as h:
        assert _bcon(h) == 0, _msg(h)
        assert lib().gmrfx_batch_set_prior(h, None) == INVALID_ARG and "null" in _msg(h)
        assert lib().gmrfx_batch_set_prior(h, ptr(nz)) == NO_DEVICE, _msg(h)
    with _Handle() as h:
        assert lib().gmrfx_constraints_set(h, 1, ptr(A_PTR), ptr(A_COL), ptr(A_VAL), 0, ptr(E)) == 0, _msg(h)
        assert lib().gmrfx_batch_set_prior(h, ptr(nz)) == INVALID_ARG and "constraint" in _msg(h)


def test_the_three_pinned_refusals_still_hold():
    with _Handle(3) as h:
        assert _set(h, 1, ONES, P3) == 0 and _bcon(h) == 0
        before = _info(h, 3)
        assert _set(h, 1, 2 * ONES, P3) == INVALID_ARG and "constraint" in _msg(h)
        assert _eval(h, 3) == INVALID_ARG and "constraint" in _msg(h)
        for fn in ("gmrfx_batch_gaussian_approximation", "gmrfx_batch_gaussian_approximation_dev"):
            assert _ga(h, 3, fn=fn) == INVALID_ARG and "constraint" in _msg(h)
        assert lib().gmrfx_batch_obs_set_design(h, 1, N, ptr(np.arange(N + 1, dtype=np.int64)), ptr(np.arange(N, dtype=np.int64)), ptr(np.ones(N)), 0,
                                                None, ptr(ONES), None, ptr(P3)) == INVALID_ARG and "constraint" in _msg(h)
        assert _info(h, 3) == before
    with _Handle(3) as h:          # flags = 16 stays "unknown flag bits" in the unconstrained calls
        assert _set(h, 1, ONES, P3) == 0
        for fn in ("gmrfx_batch_gaussian_approximation", "gmrfx_batch_gaussian_approximation_dev"):
            assert _ga(h, 3, fn=fn, flags=16) == INVALID_ARG and "flag bits" in _msg(h)


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("design", [False, True])
def test_set_param_validates_and_updates_loglik_const(family, design):
    rng = np.random.default_rng(family)
    obs = ref.make_obs(family, N, rng, "all")
    B = 3
    p0, p1 = bc.family_params(family, B), bc.family_params(family, B)[::-1].copy() * 1.5
    cp, rv = np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int64)

    def full(h, p):
        if design:
            return lib().gmrfx_batch_obs_set_design(h, family, N, ptr(cp), ptr(rv), ptr(np.ones(N)), 0, None, ptr(obs.y), ptr(obs.aux), ptr(p))
        return _set(h, family, obs.y, p, aux=obs.aux)
    with _Handle(B) as h, _Handle(B) as g:
        assert lib().gmrfx_batch_obs_set_param(h, ptr(p1)) == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert full(h, p0) == 0, _msg(h)
        assert full(g, p1) == 0, _msg(g)
        assert lib().gmrfx_batch_obs_set_param(h, None) == INVALID_ARG and "param is null" in _msg(h)
        before = _info(h, B)
        if family in (0, 4, 5):
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                p = p1.copy()
                p[1] = bad
                assert lib().gmrfx_batch_obs_set_param(h, ptr(p)) == INVALID_ARG and "member 1: sigma / r / phi must be positive" in _msg(h)
                assert _info(h, B) == before
        assert _bcon(h) == 0, _msg(h)          # with a constraint held
        assert lib().gmrfx_batch_obs_set_param(h, ptr(p1)) == 0, _msg(h)
        assert _info(h, B) == _info(g, B)        # the long-double constants of a full gmrfx_batch_obs_set with these parameters
        want = [float(ref.loglik_const(family, obs.y, obs.aux, p)[0]) for p in p1]
        assert np.allclose(_info(h, B)[2], want, rtol=1e-14, atol=1e-14)
        cl = C.c_void_p()
        assert lib().gmrfx_clone(h, C.byref(cl)) == 0
        try:
            assert _info(cl, B) == _info(g, B)
        finally:
            lib().gmrfx_destroy(cl)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, c in CASES.items():
        if name == "equal_rows":
            continue
        ks = [k for k in range(len(c["Qs"])) if not (name == "one_fails" and k == 1)]
        out[name] = {k: cc.restate(c, k, np.float64) for k in ks}
    return out


def test_every_member_converges_onto_the_constraint(restated):
    for name, rs in restated.items():
        c = CASES[name]
        for k, a in rs.items():
            assert a["converged"], (name, k)
            x = np.asarray(a["x"], float)
            assert np.abs(c["A"] @ x).max() <= cc.residual_bound(c, x, a["iterations"]), (name, k)


def test_the_cases_hold_the_branches_they_are_there_for(restated):
    r = restated["besag"]
    iters = [a["iterations"] for a in r.values()]
    assert len(set(iters)) >= 2, iters                                   # different stopping iterates: the masks differ
    ev = [set(a["events"]) for a in r.values()]
    assert any("backtrack" in e for e in ev) and any("lookahead_fire" in e for e in ev) and any("frozen_return" in e for e in ev)
    fired = ["frozen_return" in e for e in ev]
    assert any(fired) and not all(fired)                                 # the frozen finish's mask is a strict subset
    assert len({a["iterations"] for a in restated["besag50"].values()}) >= 2
    assert CASES["rw1_B1"]["A"].shape[0] < 4 <= CASES["m13_m4"]["A"].shape[0]          # vector path | MFMA path
    assert [CASES[n]["A"].shape[0] for n in ("m13_m4", "m13_m5", "m16_m5", "m16_m64")] == [4, 5, 5, 64]
    assert CASES["m13_m4"]["M"].shape[0] % 64 != 0


def test_no_member_sits_on_a_rounding_knife_edge(restated):
    for name in ("besag", "rw1_B3", "m13_m5", "m16_m64", "design"):
        c = CASES[name]
        for k, a in restated[name].items():
            b = cc.restate(c, k, ref.LD)
            assert np.array_equal(a["alpha_trace"], b["alpha_trace"]) and a["iterations"] == b["iterations"] and a["events"] == b["events"], (name, k)


def test_cond_W_stays_within_the_cap(restated):
    for name in ("m13_m4", "m13_m5", "m16_m5", "m16_m64"):
        c = CASES[name]
        for k, a in restated[name].items():
            assert cc.cond_W(c, k) <= cc.KAPPA_MAX and cc.cond_W(c, k, np.asarray(a["x"], float)) <= cc.KAPPA_MAX, (name, k)


def test_equal_rows_are_singular_and_the_failing_member_is_indefinite():
    c = CASES["equal_rows"]
    assert np.array_equal(c["A"].toarray()[0], c["A"].toarray()[1])
    c = CASES["one_fails"]
    n = c["M"].shape[0]
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(cc.dense(c, 1) + cc.RATE * np.eye(n))           # Q_p - H(0), H(0) = -RATE I for these counts
    assert np.linalg.eigvalsh(cc.dense(c, 1) + cc.RATE * np.eye(n)).min() <= -1.0
    for k in (0, 2):
        np.linalg.cholesky(cc.dense(c, k) + cc.RATE * np.eye(n))
