"""Batched Laplace, host only: the cases of tests/batch_laplace_cases.py contain the branches the lockstep loop must keep apart
(restatement of tests/fisher_ref.py in float64 and long double), and the C ABI of the new calls on symbolic-only handles: declared,
exported, every refusal that needs no device is INVALID_ARG with nothing changed, loglik_const[k] is the plain handle's for param[k],
and the plain calls still refuse batched handles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_laplace_cases as bc
import fisher_loop_cases as lc
import fisher_ref as ref
from gmrfx._lib import EXPORTS, GmrfxOpts, lib, ptr

INVALID_ARG, NO_DEVICE = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gmrfx_batch_set_prior", "gmrfx_batch_obs_set", "gmrfx_batch_obs_info", "gmrfx_batch_fisher_eval", "gmrfx_batch_fisher_eval_dev",
       "gmrfx_batch_gaussian_approximation", "gmrfx_batch_gaussian_approximation_dev"]
CASES = bc.loop_cases()


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name in ("mixed", "negbin3"):
        c = CASES[name]
        out[name] = [(bc.restate(c, k, np.float64), bc.restate(c, k, ref.LD)) for k in range(len(c["Qs"]))]
    return out


def test_mixed_holds_every_branch_of_the_lockstep_loop(restated):
    r = [a for a, _ in restated["mixed"]]
    iters = [a["iterations"] for a in r]
    assert len(set(iters)) >= 3, iters
    first = [a["events"][:a["events"].index("retry_full_reject")].count("backtrack") if "retry_full_reject" in a["events"] else
             a["events"].count("backtrack") for a in r]
    assert len(set(np.round([a["alpha_trace"][0] for a in r], 6))) >= 3 and len(set(first)) >= 3, first      # backtracks in iterate 1
    fired = ["lookahead_fire" in a["events"] for a in r]
    assert any(fired) and not all(fired)
    assert any(a["frozen"] for a in r) and any("lookahead_reject" in a["events"] for a in r)
    assert sum(a["events"][-1] == "max_iter" and not a["converged"] for a in r) == 1
    assert iters[1] == CASES["mixed"]["kw"]["max_iter"]


@pytest.mark.parametrize("name", ["mixed", "negbin3"])
def test_no_member_sits_on_a_rounding_knife_edge(restated, name):
    for a, b in restated[name]:
        assert np.array_equal(a["alpha_trace"], b["alpha_trace"]) and a["iterations"] == b["iterations"] and a["events"] == b["events"]


def test_one_fails_is_indefinite_at_the_first_iterate():
    c = CASES["one_fails"]
    D = lc.dense(c["Qs"][1]) + np.eye(256)          # Q_p - H(x0), H(0) = -exp(0) I for Poisson
    assert np.linalg.eigvalsh(D).min() <= -1.0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(D)
    for k in (0, 2):
        np.linalg.cholesky(lc.dense(c["Qs"][k]) + np.eye(256))
        assert bc.restate(c, k, np.float64)["converged"]


def test_the_two_value_sets_of_the_freshness_check_differ():
    c = CASES["mixed"]
    for k in range(5):
        a, b = lc.dense(c["Qs"][k]), 2.0 * lc.dense(c["Qs"][k])
        la, lb = np.linalg.slogdet(a + np.eye(256))[1], np.linalg.slogdet(b + np.eye(256))[1]
        assert abs(la - lb) > 1e-3 * abs(la)
        assert np.abs(np.diag(np.linalg.inv(a + np.eye(256))) - np.diag(np.linalg.inv(b + np.eye(256)))).min() > 1e-9


def test_header_declares_and_library_exports_every_new_call():
    hdr = open(os.path.join(ROOT, "include", "gmrfx.h")).read()
    L = lib()
    for nm in NEW:
        assert re.search(r"int32_t " + nm + r"\(", hdr), nm
        assert nm in EXPORTS
        getattr(L, nm)


# ---- the C ABI on symbolic-only handles ------------------------------------------------------------------------------------------
N = 6


def _pattern(n=N, diag=True):
    cp, ri = [0], []
    for j in range(n):
        ri += [i for i in (j - 1, j, j + 1) if 0 <= i < n and (diag or i != j)]
        cp.append(len(ri))
    return np.array(cp, dtype=np.int64), np.array(ri, dtype=np.int64)


class _Handle:
    def __init__(self, nbatch=0, n=N, diag=True, **opts):
        self.nbatch, self.n, self.diag, self.opts = nbatch, n, diag, opts

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        for k, v in self.opts.items():
            setattr(o, k, v)
        cp, ri = _pattern(self.n, self.diag)
        if self.nbatch:
            rc = lib().gmrfx_create_batched(self.n, ptr(cp), ptr(ri), 0, None, self.nbatch, C.byref(o), C.byref(self.h))
        else:
            rc = lib().gmrfx_create(self.n, ptr(cp), ptr(ri), 0, None, C.byref(o), C.byref(self.h))
        assert rc == 0 and self.h.value, lib().gmrfx_last_create_error()
        return self.h

    def __exit__(self, *exc):
        lib().gmrfx_destroy(self.h)


def _msg(h):
    return lib().gmrfx_last_error(h).decode()


def _info(h, B):
    fam, nobs, c = C.c_int32(7), C.c_int64(7), np.full(B, 7.0)
    assert lib().gmrfx_batch_obs_info(h, C.byref(fam), C.byref(nobs), ptr(c)) == 0
    return fam.value, nobs.value, c.tolist()


def _set(h, family, y, param, idx=None, aux=None, base=0, nobs=None):
    y = None if y is None else np.ascontiguousarray(y, np.float64)
    idx = None if idx is None else np.ascontiguousarray(idx, np.int64)
    aux = None if aux is None else np.ascontiguousarray(aux, np.float64)
    param = None if param is None else np.ascontiguousarray(param, np.float64)
    return lib().gmrfx_batch_obs_set(h, family, len(y) if nobs is None else nobs, ptr(idx), base, ptr(y), ptr(aux), ptr(param))


def _eval(h, B, n=N, x=True, out=True, sx=None, ss=None, smu=None):
    X, S, O, mu = np.zeros(n * B), np.zeros(n * B), np.zeros(2 * B), np.zeros(n * B)
    return lib().gmrfx_batch_fisher_eval(h, ptr(X) if x else None, n if sx is None else sx, ptr(mu) if smu is not None else None, smu or 0,
                                         None, ptr(S), None, n if ss is None else ss, ptr(O) if out else None)


def _ga(h, B, n=N, x=True, result=True, sx=None, sh=None, sx0=None, smu=None, flags=15, fn="gmrfx_batch_gaussian_approximation"):
    X, H, R, X0, mu = np.zeros(n * B), np.zeros(n * B), np.zeros(10 * B), np.zeros(n * B), np.zeros(n * B)
    return getattr(lib(), fn)(h, ptr(mu) if smu is not None else None, smu or 0, ptr(X0) if sx0 is not None else None, sx0 or 0, 5, 5, 1e-4, 1e-5,
                              flags, ptr(X) if x else None, n if sx is None else sx, ptr(H), n if sh is None else sh, ptr(R) if result else None,
                              None, None, None, None)


ONES, P3 = np.ones(N), np.array([1.0, 2.0, 3.0])
SET_REFUSALS = [
    ("unknown family", dict(family=6, y=ONES, param=P3)),
    ("nobs outside", dict(family=1, y=np.ones(N + 1), idx=np.arange(N + 1), param=P3)),
    ("outside the range", dict(family=1, y=np.ones(2), idx=[0, N], param=P3)),
    ("observed twice", dict(family=1, y=np.ones(3), idx=[2, 4, 2], param=P3)),
    ("indices is null", dict(family=1, y=np.ones(3), param=P3)),
    ("y is null", dict(family=1, y=None, nobs=N, param=P3)),
    ("param is null", dict(family=1, y=ONES, param=None)),
    ("index_base", dict(family=1, y=ONES, base=2, param=P3)),
    ("needs aux", dict(family=3, y=ONES, param=P3)),
    ("member 1: sigma / r / phi must be positive", dict(family=0, y=ONES, param=[1.0, 0.0, 1.0])),
    ("member 2: sigma / r / phi must be positive", dict(family=4, y=ONES, param=[1.0, 2.0, -1.0])),
    ("member 0: sigma / r / phi must be positive", dict(family=5, y=ONES, param=[float("nan"), 1.0, 1.0])),
    ("y is not finite", dict(family=0, y=np.r_[np.ones(N - 1), np.inf], param=P3)),
    ("aux is not finite", dict(family=1, y=ONES, aux=np.r_[np.ones(N - 1), np.inf], param=P3)),
    ("negative count", dict(family=1, y=np.r_[np.ones(N - 1), -1.0], param=P3)),
    ("Bernoulli observation above 1", dict(family=2, y=2 * ONES, param=P3)),
    ("exceeds the number of trials", dict(family=3, y=3 * ONES, aux=2 * ONES, param=P3)),
    ("Gamma observation must be positive", dict(family=5, y=0 * ONES, param=P3)),
]


@pytest.mark.parametrize("what,kw", SET_REFUSALS, ids=[f"{i}-{w[0].split()[0]}" for i, w in enumerate(SET_REFUSALS)])
def test_obs_set_refusals_change_nothing(what, kw):
    with _Handle(3) as h:
        assert _info(h, 3) == (-1, 0, [0.0] * 3)
        assert _set(h, **kw) == INVALID_ARG and what in _msg(h), _msg(h)
        assert _info(h, 3) == (-1, 0, [0.0] * 3)
        assert _set(h, 4, np.array([2.0, 0.0, 5.0]), P3, idx=[4, 0, 2]) == 0
        before = _info(h, 3)
        assert _set(h, **kw) == INVALID_ARG and what in _msg(h), _msg(h)
        assert _info(h, 3) == before


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("B", [1, 3])
def test_loglik_const_is_the_plain_handles_per_member(family, B):
    rng = np.random.default_rng(family)
    obs = ref.make_obs(family, N, rng, "subset")
    params = bc.family_params(family, B)
    with _Handle(B if B > 1 else 0) as h, _Handle() as p:        # (a plain handle is a batch of one)
        assert _set(h, family, obs.y, params, idx=obs.idx, aux=obs.aux) == 0, _msg(h)
        fam, nobs, c = _info(h, B)
        assert (fam, nobs) == (family, len(obs.y))
        for k in range(B):
            assert lib().gmrfx_obs_set(p, family, len(obs.y), ptr(np.ascontiguousarray(obs.idx, np.int64)), 0, ptr(obs.y),
                                       ptr(obs.aux), float(params[k])) == 0
            pc = C.c_double(0.0)
            assert lib().gmrfx_obs_info(p, None, None, C.byref(pc)) == 0
            assert c[k] == pc.value
        cl = C.c_void_p()
        assert lib().gmrfx_clone(h, C.byref(cl)) == 0
        try:
            assert _set(h, family, np.zeros(0), params) == 0
            assert _info(h, B) == (-1, 0, [0.0] * B) and _info(cl, B) == (fam, nobs, c)
        finally:
            lib().gmrfx_destroy(cl)


def test_the_calls_check_then_answer_no_device():
    with _Handle(3) as h:
        assert _eval(h, 3) == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert _ga(h, 3) == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert _set(h, 1, ONES, P3) == 0
        assert _eval(h, 3, x=False) == INVALID_ARG and "x is null" in _msg(h)
        assert _eval(h, 3, out=False) == INVALID_ARG and "out is null" in _msg(h)
        assert _eval(h, 3, sx=N - 1) == INVALID_ARG and "stride smaller than n" in _msg(h)
        assert _eval(h, 3, ss=N - 1) == INVALID_ARG and "stride smaller than n" in _msg(h)
        assert _eval(h, 3, smu=N - 1) == INVALID_ARG and "stride smaller than n" in _msg(h)
        assert _eval(h, 3, smu=0) == NO_DEVICE                   # (smu = 0 shares one mean)
        assert _eval(h, 3) == NO_DEVICE and "no device state" in _msg(h)
        for fn in ("gmrfx_batch_gaussian_approximation", "gmrfx_batch_gaussian_approximation_dev"):
            assert _ga(h, 3, x=False, fn=fn) == INVALID_ARG and "x / result is null" in _msg(h)
            assert _ga(h, 3, result=False, fn=fn) == INVALID_ARG and "x / result is null" in _msg(h)
            assert _ga(h, 3, flags=16, fn=fn) == INVALID_ARG and "flag bits" in _msg(h)
            for kw in (dict(sx=N - 1), dict(sh=N - 1), dict(sx0=N - 1), dict(smu=N - 1)):
                assert _ga(h, 3, fn=fn, **kw) == INVALID_ARG and "stride smaller than n" in _msg(h)
            assert _ga(h, 3, fn=fn) == NO_DEVICE
        nz = np.ones(16 * 3)
        assert lib().gmrfx_batch_set_prior(h, None) == INVALID_ARG and "null" in _msg(h)
        assert lib().gmrfx_batch_set_prior(h, ptr(nz)) == NO_DEVICE
        assert _info(h, 3)[:2] == (1, N)
    with _Handle(2, diag=False) as h:
        assert lib().gmrfx_batch_set_prior(h, ptr(np.ones(64))) == INVALID_ARG and "diagonal" in _msg(h)


def test_unsupported_handles_are_refused_with_nothing_changed():
    A_ptr, A_col, A_val, e = np.array([0, N], np.int64), np.arange(N, dtype=np.int64), np.ones(N), np.zeros(1)
    with _Handle(0, shard_world=2, shard_rank=0) as h:
        assert _set(h, 1, ONES, np.zeros(1)) == INVALID_ARG and "sharded" in _msg(h)
        assert _eval(h, 1) == INVALID_ARG and "sharded" in _msg(h)
        assert _ga(h, 1) == INVALID_ARG and "sharded" in _msg(h)
        assert lib().gmrfx_batch_set_prior(h, ptr(np.ones(16))) == INVALID_ARG and "sharded" in _msg(h)
    with _Handle(3) as h:
        assert _set(h, 1, ONES, P3) == 0
        assert lib().gmrfx_batch_constraints_set(h, 1, ptr(A_ptr), ptr(A_col), ptr(A_val), 0, ptr(e)) == 0, _msg(h)
        before = _info(h, 3)
        assert _set(h, 1, 2 * ONES, P3) == INVALID_ARG and "constraint" in _msg(h)
        assert _eval(h, 3) == INVALID_ARG and "constraint" in _msg(h)
        assert _ga(h, 3) == INVALID_ARG and "constraint" in _msg(h)
        assert _info(h, 3) == before
    with _Handle() as h:          # the design form on a plain handle
        cp, rv = np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int64)
        assert lib().gmrfx_obs_set_design(h, 1, N, ptr(cp), ptr(rv), ptr(np.ones(N)), 0, None, ptr(ONES), None, 0.0) == 0, _msg(h)
        assert _set(h, 1, ONES, np.zeros(1)) == INVALID_ARG and "design form" in _msg(h)
        assert _eval(h, 1) == INVALID_ARG and "design form" in _msg(h)
        assert _ga(h, 1) == INVALID_ARG and "design form" in _msg(h)
    with _Handle(65536, n=1) as h:
        assert _set(h, 1, np.ones(1), np.zeros(65536)) == INVALID_ARG and "65535" in _msg(h)
        assert _eval(h, 65536, n=1) == INVALID_ARG and "65535" in _msg(h)
        assert _ga(h, 65536, n=1) == INVALID_ARG and "65535" in _msg(h)


def test_the_plain_calls_still_refuse_batched_handles():
    x, out = np.zeros(N), np.zeros(2)
    with _Handle(3) as h:
        assert lib().gmrfx_obs_set(h, 1, N, None, 0, ptr(ONES), None, 0.0) == INVALID_ARG and "batched" in _msg(h)
        assert lib().gmrfx_fisher_eval(h, ptr(x), None, None, None, ptr(out)) == INVALID_ARG and "batched" in _msg(h)
        assert lib().gmrfx_gaussian_approximation(h, None, None, 5, 5, 1e-4, 1e-5, 15, ptr(x), None, ptr(np.zeros(8)), None, None,
                                                  None) == INVALID_ARG and "batched" in _msg(h)
