"""Composite likelihoods, what needs no device (gmrfx_obs_set_composite, gmrfx_obs_composite_info, gmrfx_obs_composite_set_param on
symbolic_only handles; the restatement, cases and mutants of tests/composite_ref.py).

1. The C ABI: every refusal with its message and gmrfx_obs_info unchanged afterwards; loglik_const per component and in total against
   the restatement; one component gives the map, the counts and the constant of gmrfx_obs_set_design; a clone carries the composite;
   set_param keeps the map and changes the constants; NaN in aux is ignored on the rows of components that have none.
2. The GPU cases: the cuts they claim (the workgroup edges of k_design_eta_comp, restated from the source), pure and mixed nodes and
   positions in every case that claims them; the float64 control stays inside the bounds WITHOUT their factor 16; each named mutant
   exceeds the bounds (with the factor) on at least one case.
3. The loop cases: no comparison of the float64 restatement near its threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import composite_ref as cref
import fisher_design_ref as dref
import fisher_ref as ref
import gmrfx
from gmrfx._lib import GmrfxOpts, lib, ptr

INVALID_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cref.eval_cases()


class _Handle:
    def __init__(self, Q, uplo="U"):
        self.Q, self.uplo = Q, uplo

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        o.uplo = 0 if self.uplo == "U" else 1
        cp, ri = np.ascontiguousarray(self.Q.indptr, np.int64), np.ascontiguousarray(self.Q.indices, np.int64)
        rc = lib().gmrfx_create(self.Q.shape[0], ptr(cp), ptr(ri), 0, None, C.byref(o), C.byref(self.h))
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


def _dinfo(h):
    a, c, t = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    assert lib().gmrfx_obs_design_info(h, C.byref(a), C.byref(c), C.byref(t)) == 0
    return a.value, c.value, t.value


def _map(h):
    cnt = C.c_int64(-5)
    assert lib().gmrfx_obs_hess_map(h, C.byref(cnt), None) == 0
    m = np.full(cnt.value, -1, np.int64)
    assert lib().gmrfx_obs_hess_map(h, C.byref(cnt), ptr(m)) == 0
    return m


def _cinfo(h):
    nc = C.c_int32(-3)
    assert lib().gmrfx_obs_composite_info(h, C.byref(nc), None, None, None, None) == 0
    fam, par, rp, c = np.full(nc.value, -9, np.int32), np.zeros(nc.value), np.zeros(nc.value + 1, np.int64), np.zeros(nc.value)
    assert lib().gmrfx_obs_composite_info(h, C.byref(nc), ptr(fam), ptr(par), ptr(rp), ptr(c)) == 0
    return nc.value, fam, par, rp, c


def set_case(h, c, **over):
    base = cref.stacked(c)
    s = dict(base, **over)
    ncomp = over.get("ncomp", len(base["family"]))
    nobs = over.get("nobs", len(base["y"]))
    return lib().gmrfx_obs_set_composite(h, ncomp, ptr(s["family"]), ptr(s["param"]), ptr(s["rowptr"]), nobs, ptr(s["cp"]), ptr(s["rv"]),
                                         ptr(s["nz"]), over.get("base", 0), ptr(s["b"]), ptr(s["y"]), ptr(s["aux"]))


def test_geometry_is_restated_from_the_source():
    src = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", "kernels.h")).read()
    m = re.search(r"kDesignLanes = (\d+), kDesignRows = (\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (dref.LANES, dref.ROWS)
    dev = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", "device.h")).read()
    assert f"kObsMaxComponents = {cref.MAX_COMPONENTS}" in dev and f"kObsComposite = {gmrfx.composite.COMPOSITE}" in dev
    hdr = open(os.path.join(ROOT, "include", "gmrfx.h")).read()
    assert f"#define GMRFX_OBS_MAX_COMPONENTS {cref.MAX_COMPONENTS}" in hdr and "#define GMRFX_OBS_COMPOSITE (-2)" in hdr
    for f in ("fisher_design.hip", "predictive.hip"):
        hip = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", f)).read()
        assert "atomic" not in hip.split('#include "kernel_common.h"')[1]


# ---- 1. the C ABI -----------------------------------------------------------------------------------------------------------------------------
def _refusals():
    c = CASES["six"]
    s = cref.stacked(c)
    nobs = len(s["y"])

    def rp(i, v):
        r = s["rowptr"].copy()
        r[i] = v
        return r

    def yv(i, v):
        y = s["y"].copy()
        y[i] = v
        return y

    def av(i, v):
        a = s["aux"].copy()
        a[i] = v
        return a
    fam7 = s["family"].copy()
    fam7[2] = 6
    bad_par = s["param"].copy()
    bad_par[4] = -1.0
    nan_par = s["param"].copy()
    nan_par[0] = np.nan
    return [("ncomp outside [1, 16]", dict(ncomp=0)), ("ncomp outside [1, 16]", dict(ncomp=17)),
            ("family / param / rowptr is null", dict(family=None)), ("family / param / rowptr is null", dict(param=None)),
            ("family / param / rowptr is null", dict(rowptr=None)),
            ("rowptr does not start at 0", dict(rowptr=rp(0, 1))),
            ("rowptr is not strictly increasing (component 2 is empty)", dict(rowptr=rp(3, 14))),
            ("rowptr is not strictly increasing (component 3 is empty)", dict(rowptr=rp(4, 20))),
            ("rowptr does not end at nobs", dict(rowptr=rp(6, nobs - 1))),
            ("component 2: unknown family", dict(family=fam7)),
            ("component 4: sigma / r / phi must be positive and finite", dict(param=bad_par)),
            ("component 0: sigma / r / phi must be positive and finite", dict(param=nan_par)),
            ("component 3: the binomial family needs aux", dict(aux=None)),
            ("nobs must be positive", dict(nobs=0)),
            ("index_base", dict(base=2)),
            ("colptr is null", dict(cp=None)),
            ("rowval / nzval is null", dict(nz=None)),
            ("y is null", dict(y=None)),
            ("component 0: y is not finite (observation 3)", dict(y=yv(3, np.inf))),
            ("component 1: negative count (observation 8)", dict(y=yv(8, -1.0))),
            ("component 1: aux is not finite (observation 9)", dict(aux=av(9, np.nan))),
            ("component 2: a Bernoulli observation above 1 (observation 15)", dict(y=yv(15, 2.0))),
            ("component 3: y exceeds the number of trials (observation 22)", dict(y=yv(22, 50.0))),
            ("component 4: aux is not finite (observation 30)", dict(aux=av(30, np.inf))),
            ("component 5: a Gamma observation must be positive (observation 41)", dict(y=yv(41, 0.0))),
            ("value of A is not finite", dict(nz=np.where(np.arange(len(s["nz"])) == 5, np.nan, s["nz"]))),
            ("component 1: offset is not finite (observation 11)", dict(b=np.where(np.arange(nobs) == 11, np.inf, 0.0))),
            ("outside [0, nobs)", dict(rv=np.where(np.arange(len(s["rv"])) == 0, nobs, s["rv"]))),
            ("not monotone", dict(cp=np.where(np.arange(len(s["cp"])) == 2, s["cp"][3] + 1, s["cp"])))]


@pytest.mark.parametrize("k", range(29))
def test_every_refusal_leaves_the_previous_likelihood_in_place(k):
    want, over = _refusals()[k]
    c = CASES["six"]
    with _Handle(c["Q"], c["uplo"]) as h:
        assert set_case(h, CASES["six"]) == 0, _msg(h)
        before = (_info(h), _dinfo(h), [a.tolist() if hasattr(a, "tolist") else a for a in _cinfo(h)], _map(h).tolist())
        assert before[0][0] == gmrfx.composite.COMPOSITE
        assert set_case(h, c, **over) == INVALID_ARG
        assert _msg(h).startswith("obs_set_composite: ") and want in _msg(h), _msg(h)
        assert (_info(h), _dinfo(h), [a.tolist() if hasattr(a, "tolist") else a for a in _cinfo(h)], _map(h).tolist()) == before


def test_a_pattern_outside_the_handles_is_refused_with_the_pair_named():
    c = CASES["six"]
    with _Handle(ref.banded(c["Q"].shape[0], 1, seed=4), "U") as h:
        assert set_case(h, c) == INVALID_ARG and "is missing" in _msg(h) and _msg(h).startswith("obs_set_composite: ")
        assert _info(h) == (-1, 0, 0.0) and _cinfo(h)[0] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_constants_per_component_and_in_total(name):
    c = CASES[name]
    obs = c["obs"]
    with _Handle(c["Q"], c["uplo"]) as h:
        assert set_case(h, c) == 0, _msg(h)
        nc, fam, par, rp, cc = _cinfo(h)
        assert nc == obs.ncomp and fam.tolist() == obs.families and par.tolist() == obs.params and rp.tolist() == obs.rowptr.tolist()
        terms = cref.const_terms(obs)
        for k in range(nc):
            want, mag = terms[k].sum(dtype=ref.LD), np.abs(terms[k]).sum(dtype=ref.LD)
            assert abs(cc[k] - want) <= 4 * ref.EPS * mag + 1e-300, (k, cc[k], want)       # (lgamma of the C library against scipy's)
        total, mag = cref.loglik_const(obs)
        fam_, nobs_, const_ = _info(h)
        assert (fam_, nobs_) == (gmrfx.composite.COMPOSITE, len(obs.y)) and abs(const_ - total) <= 4 * ref.EPS * mag
        # the sum in component order in long double: within one rounding of the sum of the components' doubles
        assert abs(const_ - float(np.sum(cc.astype(ref.LD)))) <= ref.EPS * (np.abs(cc).sum() + abs(const_))
        # the pointwise constants: every row under its own component
        out = np.zeros(len(obs.y))
        assert lib().gmrfx_obs_pointwise_const(h, ptr(out)) == 0, _msg(h)
        want = cref.pointwise_const(obs)
        assert np.all(np.abs(out - want) <= 8 * ref.EPS * (np.abs(want) + 64)), np.max(np.abs(out - want))
        tm = dref.hess_map(c["Q"], c["uplo"], c["A"])
        assert np.array_equal(_map(h), tm[0])


def test_one_component_is_the_design_form():
    c = CASES["one"]
    s = cref.stacked(c)
    with _Handle(c["Q"], c["uplo"]) as h, _Handle(c["Q"], c["uplo"]) as d:
        assert set_case(h, c) == 0, _msg(h)
        assert lib().gmrfx_obs_set_design(d, int(s["family"][0]), len(s["y"]), ptr(s["cp"]), ptr(s["rv"]), ptr(s["nz"]), 0, ptr(s["b"]), ptr(s["y"]),
                                          ptr(s["aux"]), float(s["param"][0])) == 0, _msg(d)
        assert np.array_equal(_map(h), _map(d)) and _dinfo(h) == _dinfo(d)
        assert _info(h)[1:] == _info(d)[1:] and _info(h)[0] == gmrfx.composite.COMPOSITE and _info(d)[0] == 1
        assert _cinfo(h)[4][0] == _info(d)[2] and _cinfo(d)[0] == 0
        # each form replaces the other, and gmrfx_obs_set with nobs = 0 removes the composite
        assert set_case(d, c) == 0 and _cinfo(d)[0] == 1
        assert lib().gmrfx_obs_set_design(d, 1, len(s["y"]), ptr(s["cp"]), ptr(s["rv"]), ptr(s["nz"]), 0, None, ptr(s["y"]), None, 0.0) == 0
        assert _cinfo(d)[0] == 0 and _info(d)[0] == 1
        assert lib().gmrfx_obs_set(h, 0, 0, None, 0, None, None, 0.0) == 0
        assert _info(h) == (-1, 0, 0.0) and _cinfo(h)[0] == 0 and _dinfo(h) == (-1, -1, -1)


def test_clone_carries_the_composite():
    c = CASES["sixteen"]
    with _Handle(c["Q"], c["uplo"]) as h:
        assert set_case(h, c) == 0, _msg(h)
        k = C.c_void_p()
        assert lib().gmrfx_clone(h, C.byref(k)) == 0
        try:
            assert _info(k) == _info(h) and _dinfo(k) == _dinfo(h) and np.array_equal(_map(k), _map(h))
            assert all(np.array_equal(a, b) for a, b in zip(_cinfo(k), _cinfo(h)))
        finally:
            lib().gmrfx_destroy(k)


def test_set_param_keeps_the_map_and_changes_the_constants():
    c = CASES["six"]
    with _Handle(c["Q"], c["uplo"]) as h, _Handle(c["Q"], c["uplo"]) as f:
        assert set_case(h, c) == 0, _msg(h)
        m0, d0, c0 = _map(h), _dinfo(h), _cinfo(h)
        p = np.array([1.3, 9.0, 9.0, 9.0, 4.0, 0.5])
        assert lib().gmrfx_obs_composite_set_param(h, ptr(p)) == 0, _msg(h)
        assert set_case(f, c, param=p) == 0
        assert np.array_equal(_map(h), m0) and _dinfo(h) == d0
        assert all(np.array_equal(a, b) for a, b in zip(_cinfo(h), _cinfo(f))) and _info(h) == _info(f)
        changed = _cinfo(h)[4] != c0[4]
        assert changed.tolist() == [True, False, False, False, True, True]
        a, b = np.zeros(42), np.zeros(42)
        assert lib().gmrfx_obs_pointwise_const(h, ptr(a)) == 0 and lib().gmrfx_obs_pointwise_const(f, ptr(b)) == 0 and np.array_equal(a, b)
        # refusals: nothing changed
        before = (_info(h), [x.tolist() for x in _cinfo(h)[1:]])
        for bad, want in ((np.array([0.0, 0, 0, 0, 1, 1]), "component 0: sigma"), (np.array([1.0, 0, 0, 0, 1, np.inf]), "component 5: sigma")):
            assert lib().gmrfx_obs_composite_set_param(h, ptr(bad)) == INVALID_ARG and want in _msg(h)
            assert (_info(h), [x.tolist() for x in _cinfo(h)[1:]]) == before
        assert lib().gmrfx_obs_composite_set_param(h, None) == INVALID_ARG and "param is null" in _msg(h)
        assert lib().gmrfx_obs_set(f, 0, 0, None, 0, None, None, 0.0) == 0
        assert lib().gmrfx_obs_composite_set_param(f, ptr(p)) == INVALID_ARG and "no composite likelihood is set" in _msg(f)


def test_pullback_and_batched_calls_refuse_a_composite():
    c = CASES["six"]
    n = c["Q"].shape[0]
    with _Handle(c["Q"], c["uplo"]) as h:
        assert set_case(h, c) == 0
        x, out = np.zeros(n), np.zeros(2)
        assert lib().gmrfx_ga_pullback(h, ptr(x), None, ptr(x), None, 0, None, None, ptr(x), ptr(out)) == INVALID_ARG
        assert "ga_pullback: composite likelihoods are not supported" in _msg(h)
        assert lib().gmrfx_batch_obs_set(h, 1, n, None, 0, ptr(np.ones(n)), None, ptr(np.zeros(1))) == INVALID_ARG
        assert "the design form" in _msg(h)


def test_the_python_builder_stacks_the_components():
    c = CASES["same_nodes"]
    obs, A = c["obs"], sp.csr_matrix(c["A"])
    m = int(obs.rowptr[1])
    nodes = A.indices[:m]
    comp = gmrfx.CompositeObservations(A.shape[1])
    comp.add("normal", obs.y[:m], indices=nodes, param=obs.params[0]).add("poisson", obs.y[m:], A=A[m:], aux=obs.aux[m:])
    s = comp.stacked()
    assert s["family"].tolist() == [0, 1] and s["rowptr"].tolist() == [0, m, 2 * m] and np.array_equal(s["y"], obs.y)
    assert (abs(s["A"] - A)).nnz == 0 and s["offset"] is None and np.isnan(s["aux"][:m]).all() and np.array_equal(s["aux"][m:], obs.aux[m:])
    with pytest.raises(ValueError):
        comp.add("normal", [1.0], A=A[:1], indices=[0])
    with pytest.raises(ValueError):
        gmrfx.CompositeObservations(4).stacked()


# ---- 2. the GPU cases ---------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_what_they_claim():
    R = dref.ROWS
    assert sorted({c["obs"].ncomp for c in CASES.values()} & {1, 2, 6, 16}) == [1, 2, 6, 16]
    cuts = CASES["cuts"]["obs"].rowptr.tolist()
    nobs = cuts[-1]
    assert set(cuts) >= {1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, nobs - 1} and nobs > 2 * R + 1
    A = sp.csr_matrix(CASES["cuts"]["A"])
    assert 0 in np.diff(A.indptr) and CASES["cuts"]["b"] is not None                                # an empty row: eta_i = b_i
    assert 1 in np.diff(CASES["cuts"]["obs"].rowptr) and 1 in np.diff(CASES["sixteen"]["obs"].rowptr)      # one-row components
    S = sp.csr_matrix(CASES["same_nodes"]["A"])
    m = S.shape[0] // 2
    assert CASES["same_nodes"]["obs"].families == [0, 1] and (abs(S[:m] - S[m:])).nnz == 0 and set(np.diff(S.indptr)) == {1}
    for name in ("cuts", "six"):           # a Binomial component next to components whose aux rows hold NaN
        o = CASES[name]["obs"]
        comp = o.comp_of_row()
        assert 3 in o.families and np.isnan(o.aux[np.isin(np.asarray(o.families)[comp], (0, 2, 5))]).all()
    for name, c in CASES.items():
        assert 40 <= c["Q"].shape[0] <= 72, name
        nc, pc = cref.purity(c)
        if c["pure"]:
            for k in range(c["obs"].ncomp):
                assert (nc == k).any() and (pc == k).any(), (name, k)
            assert (nc == -1).any() and (pc == -1).any(), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_control_stays_inside_the_bounds_without_their_factor(name):
    c = CASES[name]
    tm = dref.hess_map(c["Q"], c["uplo"], c["A"])
    r = cref.eval_ref(c, c["x"], c["mu"], tm)
    got = cref.eval_f64(c, c["x"], c["mu"], tm)
    assert cref.exceeds(c, c["x"], c["mu"], tm, r, got, 1) <= 1.0


@pytest.mark.parametrize("mutant", cref.MUTANTS)
def test_every_mutant_exceeds_the_bounds_somewhere(mutant):
    worst = 0.0
    for c in CASES.values():
        tm = dref.hess_map(c["Q"], c["uplo"], c["A"])
        r = cref.eval_ref(c, c["x"], c["mu"], tm)
        worst = max(worst, cref.exceeds(c, c["x"], c["mu"], tm, r, cref.eval_f64(c, c["x"], c["mu"], tm, mutant), 16))
    assert worst > 1.0, worst


# ---- 3. the loop cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cref.loop_cases()))
def test_loop_cases_are_far_from_every_threshold(name):
    c = cref.loop_cases()[name]
    r = cref.newton_loop(c, np.float64)
    assert r["converged"] and r["iterations"] >= 2
    assert dref.far_from_thresholds(r["margins"])
    assert c["obs"].families == [0, 1, 2] and (c["C"] is None) == (name == "joint")
