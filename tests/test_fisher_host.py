"""Fisher scoring on the device, host only (gmrfx_obs_set, gmrfx_obs_info, gmrfx_fisher_eval on symbolic-only handles).

1. tests/fisher_ref.py restates the geometry of csrc/fisher.hip (R, W, FINAL) and its shape cases hit every edge of it.
2. The stable pointwise forms against the reference's textbook formulas where those are well-conditioned (|eta| <= 3: both are then
   accurate to a few ulp of long double, bound 64 eps_ld relative to the terms), against scipy.stats' log densities (stable part +
   constants = logpdf, to double precision: 1e-12 relative to the absolute sum of the terms), and finite at eta = +-40, +-700 where the
   mathematics is.
3. The C ABI on symbolic-only handles: every refusal of gmrfx_obs_set is INVALID_ARG with a message and leaves gmrfx_obs_info's answer
   as it was; valid sets are kept (family, nobs, loglik_const against the long-double sum, 8 eps times the absolute sum of the terms:
   the library sums long-double lgamma values, the reference double ones); nobs = 0 removes; gmrfx_clone carries; gmrfx_fisher_eval
   checks its arguments and the likelihood, then answers NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.stats as st

import fisher_ref as ref
from gmrfx._lib import GmrfxOpts, lib, ptr

INVALID_ARG, NO_DEVICE = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6


def test_geometry_is_restated_from_the_source():
    src = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", "kernels.h")).read()
    m = re.search(r"kFisherLanes = (\d+), kFisherRows = (\d+), kFisherFinal = (\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (ref.W, ref.R, ref.FINAL)
    hip = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", "fisher.hip")).read()
    assert "atomic" not in hip.split('#include "kernel_common.h"')[1]          # (the header comment says "No atomics"; the code has none)


def test_shape_cases_hit_every_edge():
    cases = ref.shape_cases()
    ns = {Q.shape[0] for Q, _ in cases.values()}
    assert {1, ref.R - 1, ref.R, ref.R + 1, ref.FINAL * ref.R + 1} <= ns
    counts = set()
    for Q, uplo in cases.values():
        counts |= set(ref.symmetric_coo(Q, uplo)[3].tolist())
    assert {ref.W - 1, ref.W, ref.W + 1} <= counts and max(counts) >= 4 * ref.W + 3
    assert {u for _, u in cases.values()} == {"L", "U"}


@pytest.mark.parametrize("family", range(6))
def test_stable_forms_against_the_textbook_formulas(family):
    rng = np.random.default_rng(family)
    obs = ref.make_obs(family, 200, rng)
    eta = rng.uniform(-3, 3, 200)
    g, d, ll, mean = ref.pointwise(family, eta, obs.y, obs.aux, obs.param)
    gn, dn = ref.pointwise_naive(family, eta, obs.y, obs.aux, obs.param)
    eps_ld = float(np.finfo(np.longdouble).eps)
    scale = np.abs(obs.y) + np.abs(mean) + 1
    assert (np.abs(g - gn) <= 64 * eps_ld * scale * max(obs.param, 1)).all()
    assert (np.abs(d - dn) <= 64 * eps_ld * scale * max(obs.param, 1)).all()
    # the log density itself: Distributions' logpdf is scipy's
    aux = np.zeros(200) if obs.aux is None else obs.aux
    p = obs.param
    want = [lambda: st.norm.logpdf(obs.y, eta, p), lambda: st.poisson.logpmf(obs.y, np.exp(eta + aux)),
            lambda: st.bernoulli.logpmf(obs.y, 1 / (1 + np.exp(-eta))), lambda: st.binom.logpmf(obs.y, aux, 1 / (1 + np.exp(-eta))),
            lambda: st.nbinom.logpmf(obs.y, p, p / (p + np.exp(eta + aux))),
            lambda: st.gamma.logpdf(obs.y, p, scale=np.exp(eta) / p)][family]().sum()
    c, cabs = ref.loglik_const(family, obs.y, obs.aux, p)
    total = float(ll.sum() + c)
    assert abs(total - want) <= 1e-12 * float(np.abs(ll).sum() + cabs + abs(want))


@pytest.mark.parametrize("family", [2, 3])
def test_logit_families_are_finite_at_extreme_eta(family):
    eta = np.array([-700.0, -40.0, 40.0, 700.0])
    y = np.array([1.0, 0.0, 1.0, 0.0])
    g, d, ll, _ = ref.pointwise(family, eta, y, np.full(4, 3.0), 0.0)
    assert np.isfinite(g).all() and np.isfinite(d).all() and np.isfinite(ll).all()
    g, d, ll, _ = ref.pointwise(1, np.array([-700.0, -40.0]), np.array([2.0, 0.0]), None, 0.0)
    assert np.isfinite(g).all() and np.isfinite(d).all() and np.isfinite(ll).all()


# ---- the C ABI on symbolic-only handles ----------------------------------------------------------------------------------------
def _pattern():
    cp, ri = [0], []
    for j in range(N):
        ri += [i for i in (j - 1, j, j + 1) if 0 <= i < N]
        cp.append(len(ri))
    return np.array(cp, dtype=np.int64), np.array(ri, dtype=np.int64)


COLPTR, ROWVAL = _pattern()


class _Handle:
    def __init__(self, nbatch=0, **opts):
        self.nbatch, self.opts = nbatch, opts

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        for k, v in self.opts.items():
            setattr(o, k, v)
        if self.nbatch:
            rc = lib().gmrfx_create_batched(N, ptr(COLPTR), ptr(ROWVAL), 0, None, self.nbatch, C.byref(o), C.byref(self.h))
        else:
            rc = lib().gmrfx_create(N, ptr(COLPTR), ptr(ROWVAL), 0, None, C.byref(o), C.byref(self.h))
        assert rc == 0 and self.h.value, lib().gmrfx_last_create_error()
        return self.h

    def __exit__(self, *exc):
        lib().gmrfx_destroy(self.h)


def _msg(h):
    return lib().gmrfx_last_error(h).decode()


def _info(h):
    fam, nobs, c = C.c_int32(7), C.c_int64(7), C.c_double(7.0)
    assert lib().gmrfx_obs_info(h, C.byref(fam), C.byref(nobs), C.byref(c)) == 0
    return fam.value, nobs.value, c.value


def _set(h, family, y, idx=None, aux=None, param=0.0, base=0, nobs=None):
    y = None if y is None else np.ascontiguousarray(y, np.float64)
    idx = None if idx is None else np.ascontiguousarray(idx, np.int64)
    aux = None if aux is None else np.ascontiguousarray(aux, np.float64)
    return lib().gmrfx_obs_set(h, family, len(y) if nobs is None else nobs, ptr(idx), base, ptr(y), ptr(aux), float(param))


ONES = np.ones(N)
REFUSALS = [
    ("unknown family", dict(family=6, y=ONES)),
    ("unknown family", dict(family=-1, y=ONES)),
    ("nobs outside", dict(family=1, y=np.ones(N + 1), idx=np.arange(N + 1))),
    ("nobs outside", dict(family=1, y=ONES, nobs=-1)),
    ("outside the range", dict(family=1, y=np.ones(2), idx=[0, N])),
    ("outside the range", dict(family=1, y=np.ones(2), idx=[0, 1], base=1)),
    ("observed twice", dict(family=1, y=np.ones(3), idx=[2, 4, 2])),
    ("indices is null", dict(family=1, y=np.ones(3))),
    ("y is null", dict(family=1, y=None, nobs=N)),
    ("index_base", dict(family=1, y=ONES, base=2)),
    ("needs aux", dict(family=3, y=ONES)),
    ("must be positive", dict(family=0, y=ONES, param=0.0)),
    ("must be positive", dict(family=4, y=ONES, param=-1.0)),
    ("must be positive", dict(family=5, y=ONES, param=float("nan"))),
    ("y is not finite", dict(family=0, y=np.r_[np.ones(N - 1), np.inf], param=1.0)),
    ("y is not finite", dict(family=1, y=np.r_[np.nan, np.ones(N - 1)])),
    ("aux is not finite", dict(family=1, y=ONES, aux=np.r_[np.ones(N - 1), np.inf])),
    ("negative count", dict(family=1, y=np.r_[np.ones(N - 1), -1.0])),
    ("negative count", dict(family=4, y=-ONES, param=1.0)),
    ("Bernoulli observation above 1", dict(family=2, y=2 * ONES)),
    ("exceeds the number of trials", dict(family=3, y=3 * ONES, aux=2 * ONES)),
    ("Gamma observation must be positive", dict(family=5, y=0 * ONES, param=1.0)),
]


@pytest.mark.parametrize("what,kw", REFUSALS, ids=[f"{i}-{w[0].split()[0]}" for i, w in enumerate(REFUSALS)])
def test_refusals_change_nothing(what, kw):
    with _Handle() as h:
        assert _info(h) == (-1, 0, 0.0)
        assert _set(h, **kw) == INVALID_ARG and what in _msg(h), _msg(h)
        assert _info(h) == (-1, 0, 0.0)
        y = np.array([2.0, 0.0, 5.0])
        assert _set(h, 1, y, idx=[4, 0, 2]) == 0
        before = _info(h)
        assert before[:2] == (1, 3)
        assert _set(h, **kw) == INVALID_ARG and what in _msg(h), _msg(h)
        assert _info(h) == before


def test_batched_and_sharded_handles_are_refused():
    x, out = np.zeros(N), np.zeros(2)
    for hd, word in ((_Handle(3), "batched"), (_Handle(0, shard_world=2, shard_rank=0), "sharded")):
        with hd as h:
            assert _set(h, 1, ONES) == INVALID_ARG and word in _msg(h)
            assert _info(h) == (-1, 0, 0.0)
            assert lib().gmrfx_fisher_eval(h, ptr(x), None, None, None, ptr(out)) == INVALID_ARG and word in _msg(h)
            assert lib().gmrfx_fisher_eval_dev(h, ptr(x), None, None, None, ptr(out)) == INVALID_ARG and word in _msg(h)


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("which", ["all", "subset"])
def test_valid_sets_are_kept_with_their_constant(family, which):
    rng = np.random.default_rng(10 * family + len(which))
    obs = ref.make_obs(family, N, rng, which)
    with _Handle() as h:
        base = 1 if which == "subset" else 0          # (1-based indices)
        idx = None if obs.idx is None else obs.idx + base
        assert _set(h, family, obs.y, idx=idx, aux=obs.aux, param=obs.param, base=base) == 0, _msg(h)
        fam, nobs, c = _info(h)
        want, wabs = ref.loglik_const(family, obs.y, obs.aux, obs.param)
        print(f"family {family} {which}: loglik_const {c!r} reference {float(want)!r} bound {8 * ref.EPS * float(wabs):.2e}")
        assert (fam, nobs) == (family, len(obs.y))
        assert abs(c - float(want)) <= 8 * ref.EPS * float(wabs)
        # a clone carries the likelihood; nobs = 0 removes it from this handle only
        cl = C.c_void_p()
        assert lib().gmrfx_clone(h, C.byref(cl)) == 0
        try:
            assert _set(h, family, np.zeros(0)) == 0
            assert _info(h) == (-1, 0, 0.0)
            assert _info(cl) == (fam, nobs, c)
        finally:
            lib().gmrfx_destroy(cl)


def test_fisher_eval_checks_then_answers_no_device():
    L = lib()
    x, out, sc = np.zeros(N), np.zeros(2), np.zeros(N)
    with _Handle() as h:
        for f in (L.gmrfx_fisher_eval, L.gmrfx_fisher_eval_dev):
            assert f(h, ptr(x), None, ptr(sc), None, ptr(out)) == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert _set(h, 1, ONES) == 0
        for f in (L.gmrfx_fisher_eval, L.gmrfx_fisher_eval_dev):
            assert f(h, None, None, ptr(sc), None, ptr(out)) == INVALID_ARG and "x is null" in _msg(h)
            assert f(h, ptr(x), None, ptr(sc), None, None) == INVALID_ARG and "out is null" in _msg(h)
            assert f(h, ptr(x), None, ptr(sc), ptr(sc), ptr(out)) == NO_DEVICE and "no device state" in _msg(h)
        assert f(None, ptr(x), None, None, None, ptr(out)) == INVALID_ARG
        assert L.gmrfx_obs_info(None, None, None, None) == INVALID_ARG
