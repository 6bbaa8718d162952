"""Fisher scoring through a design matrix, what needs no device (gmrfx_obs_set_design, gmrfx_obs_hess_map, gmrfx_obs_design_info on
symbolic_only handles; the references and cases of tests/fisher_design_ref.py).

1. The C ABI: every refusal leaves the previous likelihood in place; the map equals the Python restatement on lower, upper and full
   storage, with 0- and 1-based input; a pattern(A'A) outside pattern(Q) is refused with the pair named; loglik_const equals the node
   form's; a clone carries the state; the counts of gmrfx_obs_design_info.
2. The GPU cases: a coverage table of the class and chunk edges each case claims; a float64 numpy control stays inside the bounds of
   tests/test_gpu_fisher_design.py WITHOUT their factor 16; each named mutant exceeds the bounds (with the factor) on at least one case.
3. The loop cases: the branches they claim, and no comparison of the float64 restatement near its threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import fisher_design_ref as dref
import fisher_ref as ref
from gmrfx._lib import GmrfxOpts, lib, ptr

INVALID_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dref.eval_cases()


def test_geometry_is_restated_from_the_source():
    src = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", "kernels.h")).read()
    m = re.search(r"kDesignLanes = (\d+), kDesignRows = (\d+), kDesignChunk = (\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (dref.LANES, dref.ROWS, dref.CHUNK)
    assert (dref.LANES, dref.ROWS) == (ref.W, ref.R)
    hip = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", "fisher_design.hip")).read()
    assert "atomic" not in hip.split('#include "kernel_common.h"')[1]
    assert '#include "fisher_point.h"' in hip
    old = open(os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc", "fisher.hip")).read()
    assert '#include "fisher_point.h"' in old and "fisher_logistic(double" not in old      # one copy of the family functions


class _Handle:
    def __init__(self, Q, uplo="U", base=0):
        self.Q, self.uplo, self.base = Q, uplo, base

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        o.uplo = 0 if self.uplo == "U" else 1
        cp = np.ascontiguousarray(self.Q.indptr, np.int64) + self.base
        ri = np.ascontiguousarray(self.Q.indices, np.int64) + self.base
        rc = lib().gmrfx_create(self.Q.shape[0], ptr(cp), ptr(ri), self.base, None, C.byref(o), C.byref(self.h))
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


def _set(h, family, y, A=None, offset=None, aux=None, param=0.0, base=0, colptr=None, rowval=None, nzval=None, nobs=None):
    y = np.ascontiguousarray(y, np.float64)
    if A is not None:
        Ac = sp.csc_matrix(A)
        Ac.sort_indices()
        colptr = Ac.indptr if colptr is None else colptr
        rowval = Ac.indices if rowval is None else rowval
        nzval = Ac.data if nzval is None else nzval
    cp = np.ascontiguousarray(colptr, np.int64) + base
    rv = np.ascontiguousarray(rowval, np.int64) + base
    nz = np.ascontiguousarray(nzval, np.float64)
    off = None if offset is None else np.ascontiguousarray(offset, np.float64)
    ax = None if aux is None else np.ascontiguousarray(aux, np.float64)
    return lib().gmrfx_obs_set_design(h, family, len(y) if nobs is None else nobs, ptr(cp), ptr(rv), ptr(nz), base, ptr(off), ptr(y), ptr(ax),
                                      float(param))


def _map(h):
    cnt = C.c_int64(-5)
    assert lib().gmrfx_obs_hess_map(h, C.byref(cnt), None) == 0
    m = np.full(cnt.value, -1, np.int64)
    assert lib().gmrfx_obs_hess_map(h, C.byref(cnt), ptr(m)) == 0
    return m


# a 6-node chain and a 4 x 6 design matrix inside its pattern
N = 6
CHAIN = sp.csc_matrix(sp.diags([np.ones(N - 1), 2 * np.ones(N), np.ones(N - 1)], [-1, 0, 1]))
CHAIN.sort_indices()
A0 = sp.csc_matrix((np.array([0.5, 0.5, 1.0, 0.25, 0.75, 0.0]), (np.array([0, 0, 1, 2, 2, 3]), np.array([0, 1, 2, 2, 3, 5]))), shape=(4, N))
Y0 = np.array([1.0, 2.0, 0.0, 3.0])


def _bad_cases():
    cp, rv, nz = A0.indptr.copy(), A0.indices.copy(), A0.data.copy()
    notmono = cp.copy()
    notmono[2] = notmono[3] + 1
    out = [("not monotone", dict(y=Y0, colptr=notmono, rowval=rv, nzval=nz)),
           ("outside [0, nobs)", dict(y=Y0, colptr=cp, rowval=np.where(np.arange(len(rv)) == 1, 4, rv), nzval=nz)),
           ("outside [0, nobs)", dict(y=Y0, colptr=cp, rowval=np.where(np.arange(len(rv)) == 0, -1, rv), nzval=nz)),
           ("unsorted or repeated", dict(y=Y0, colptr=cp, rowval=np.where(np.arange(len(rv)) == 3, 1, rv), nzval=nz)),      # column 2: 1, 1
           ("unsorted or repeated", dict(y=Y0, colptr=cp, rowval=np.where(np.arange(len(rv)) == 2, 3, rv), nzval=nz)),      # column 2: 3, 2
           ("value of A is not finite", dict(y=Y0, colptr=cp, rowval=rv, nzval=np.where(np.arange(len(nz)) == 4, np.inf, nz))),
           ("offset is not finite", dict(y=Y0, A=A0, offset=[0.0, np.nan, 0.0, 0.0])),
           ("unknown family", dict(y=Y0, A=A0, family=6)),
           ("negative count", dict(y=[1.0, -1.0, 0.0, 0.0], A=A0)),
           ("y is not finite", dict(y=[1.0, np.nan, 0.0, 0.0], A=A0)),
           ("needs aux", dict(y=Y0, A=A0, family=3)),
           ("must be positive and finite", dict(y=Y0, A=A0, family=4, param=0.0)),
           ("index_base", dict(y=Y0, A=A0, base=2)),
           ("nobs must be positive", dict(y=Y0, A=A0, nobs=0)),
           ("is missing", dict(y=Y0, A=sp.csc_matrix(np.array([[1.0, 0, 1.0, 0, 0, 0]] * 4))))]
    return out


@pytest.mark.parametrize("what,kw", _bad_cases())
def test_refusals_leave_the_previous_likelihood_in_place(what, kw):
    kw = dict(kw)
    family = kw.pop("family", 1)
    with _Handle(CHAIN) as h:
        assert _set(h, 1, Y0, A=A0, offset=np.arange(4.0)) == 0
        before = (_info(h), _dinfo(h), _map(h).tolist())
        assert _set(h, family, **kw) == INVALID_ARG
        assert what in _msg(h), _msg(h)
        assert (_info(h), _dinfo(h), _map(h).tolist()) == before
    with _Handle(CHAIN) as h:           # ... also a node-form likelihood
        assert lib().gmrfx_obs_set(h, 1, N, None, 0, ptr(np.ones(N)), None, 0.0) == 0
        before = _info(h)
        assert _set(h, family, **kw) == INVALID_ARG
        assert _info(h) == before and _dinfo(h) == (-1, -1, -1)


def test_a_missing_pair_is_named_in_the_callers_index_base():
    A = sp.csc_matrix(np.array([[0.5, 0.5, 0, 0, 0, 0], [0, 1.0, 0, 0, 1.0, 0]]))
    with _Handle(CHAIN) as h:
        assert _set(h, 1, [1.0, 1.0], A=A) == INVALID_ARG and "entry (1, 4) is missing" in _msg(h)
        assert _set(h, 1, [1.0, 1.0], A=A, base=1) == INVALID_ARG and "entry (2, 5) is missing" in _msg(h)


def test_forms_replace_each_other_and_counts():
    with _Handle(CHAIN) as h:
        assert _dinfo(h) == (-1, -1, -1) and _info(h)[0] == -1
        cnt = C.c_int64(0)
        assert lib().gmrfx_obs_hess_map(h, C.byref(cnt), None) == INVALID_ARG and "no design likelihood" in _msg(h)
        assert _set(h, 1, Y0, A=A0) == 0
        # pairs: (0,0) (0,1) (1,1) | (2,2) twice | (2,3) (3,3) | (5,5): 7 positions, 8 terms, 6 stored entries (one explicit zero)
        assert _dinfo(h) == (6, 7, 8) and _info(h)[:2] == (1, 4)
        assert lib().gmrfx_obs_set(h, 1, N, None, 0, ptr(np.ones(N)), None, 0.0) == 0
        assert _dinfo(h) == (-1, -1, -1) and _info(h)[:2] == (1, N)
        assert _set(h, 1, Y0, A=A0) == 0 and _dinfo(h) == (6, 7, 8)
        assert lib().gmrfx_obs_set(h, 1, 0, None, 0, None, None, 0.0) == 0
        assert _dinfo(h) == (-1, -1, -1) and _info(h)[:2] == (-1, 0)


def test_sizes_at_two_to_the_31_are_refused_before_anything_is_read():
    big = 1 << 31
    with _Handle(CHAIN) as h:
        assert _set(h, 1, Y0, A=A0) == 0
        before = (_info(h), _dinfo(h))
        forged = np.r_[np.zeros(N, np.int64), big]            # nnz(A) = 2^31 by its colptr: rowval and nzval are never read
        assert _set(h, 1, Y0, colptr=forged, rowval=[0], nzval=[1.0]) == INVALID_ARG and "2^31 or above" in _msg(h)
        assert _set(h, 1, Y0, A=A0, nobs=big) == INVALID_ARG and "2^31 or above" in _msg(h)       # y is never read at that length
        assert (_info(h), _dinfo(h)) == before


def test_a_term_count_at_two_to_the_31_is_refused():
    n = 1 << 16                 # one row with 2^16 entries: 2^16 (2^16 + 1) / 2 >= 2^31 terms
    Q = ref.banded(n, 1)
    A = sp.csc_matrix(np.ones((1, n)))
    with _Handle(Q) as h:
        assert _set(h, 1, [1.0], A=A) == INVALID_ARG and "2^31 terms or more" in _msg(h)
        assert _dinfo(h) == (-1, -1, -1)


def test_a_design_matrix_without_entries():
    with _Handle(CHAIN) as h:
        assert _set(h, 1, Y0, A=sp.csc_matrix((4, N)), offset=np.arange(4.0)) == 0, _msg(h)
        assert _dinfo(h) == (0, 0, 0) and _map(h).size == 0 and _info(h)[:2] == (1, 4)


@pytest.mark.parametrize("family", range(6))
def test_loglik_const_is_the_node_forms_and_a_clone_carries_the_state(family):
    obs = ref.make_obs(family, N, np.random.default_rng(family), "all")
    A = sp.identity(N, format="csc")
    aux = None if obs.aux is None else np.ascontiguousarray(obs.aux, np.float64)
    with _Handle(CHAIN) as h:
        assert lib().gmrfx_obs_set(h, family, N, None, 0, ptr(np.ascontiguousarray(obs.y)), ptr(aux), float(obs.param)) == 0
        node = _info(h)
        assert _set(h, family, obs.y, A=A, aux=obs.aux, param=obs.param) == 0
        assert _info(h) == node
        c = C.c_void_p()
        assert lib().gmrfx_clone(h, C.byref(c)) == 0
        try:
            assert _info(c) == node and _dinfo(c) == _dinfo(h) == (N, N, N) and np.array_equal(_map(c), _map(h))
        finally:
            lib().gmrfx_destroy(c)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("base", [0, 1])
def test_the_map_equals_the_python_restatement(name, base):
    c = CASES[name]
    want = dref.hess_map(c["Q"], c["uplo"], c["A"])
    y = np.ones(c["A"].shape[0])
    with _Handle(c["Q"], c["uplo"], base) as h:
        assert _set(h, 1, y, A=c["A"], offset=c["b"], base=base) == 0, _msg(h)
        got = _map(h)
        assert np.array_equal(got, want[0]) and (np.diff(got) > 0).all()
        assert _dinfo(h) == (sp.csc_matrix(c["A"]).nnz, len(want[0]), len(want[2]))


def test_the_map_on_every_storage():
    assert {(c["uplo"], bool((sp.tril(c["Q"], -1) != 0).nnz and (sp.triu(c["Q"], 1) != 0).nnz)) for c in CASES.values()} >= {("L", True), ("U", True)}
    c = CASES["mesh"]
    n = c["Q"].shape[0]
    S = sp.csc_matrix(sp.triu(c["Q"]) + sp.triu(c["Q"], 1).T)
    maps = {}
    for storage, Q, uplo in (("upper only", sp.csc_matrix(sp.triu(S)), "U"), ("lower only", sp.csc_matrix(sp.tril(S)), "L"), ("full", S, "U")):
        Q.sort_indices()
        with _Handle(Q, uplo) as h:
            assert _set(h, 1, np.ones(c["A"].shape[0]), A=c["A"]) == 0, _msg(h)
            got = _map(h)
        assert np.array_equal(got, dref.hess_map(Q, uplo, c["A"])[0])
        coo = Q.tocoo()
        maps[storage] = {(min(i, j), max(i, j)) for i, j in zip(coo.row[got], coo.col[got])}
    assert maps["upper only"] == maps["lower only"] == maps["full"]         # the same pairs, wherever they are stored


def test_every_gpu_case_reaches_the_edges_it_claims():
    L, K = dref.LANES, dref.CHUNK
    cov = {k: dref.coverage(c) for k, c in CASES.items()}
    table = {
        "mesh": dict(rows={0, 1, 3}, offset=True, uplo="U", node_twice=True),
        "rows": dict(rows={0, 1, 3, L, L + 1, 2 * L + 1}, offset=False, uplo="L"),
        "cols": dict(cols={0, 1, L - 1, L, L + 1, K - 1, K, K + 1}, terms={1, L - 1, L, L + 1, K - 1, K, K + 1}, chunk_lengths={K, 1}, offset=True),
        "intercept": dict(cols={3 * K + 1}, terms={3 * K + 1}, chunk_lengths={K, 1}, offset=False, uplo="U"),
        "one": dict(nobs=1, offset=True, uplo="L"),
    }
    assert set(table) == set(CASES)
    for name, claim in table.items():
        for key, want in claim.items():
            got = cov[name][key]
            assert (want <= got) if isinstance(want, set) else (got == want), (name, key, want, got)
    assert cov["intercept"]["nobs"] > cov["intercept"]["n"]
    assert all(c["Q"].shape[0] <= 600 for c in CASES.values())


def _point(n, seed):
    rng = np.random.default_rng(seed)
    return 0.8 * rng.standard_normal(n), 0.5 * rng.standard_normal(n)


_TM = {}


def _tm(name):
    if name not in _TM:
        c = CASES[name]
        _TM[name] = dref.hess_map(c["Q"], c["uplo"], c["A"])
    return _TM[name]


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("name", list(CASES))
def test_float64_control_stays_inside_the_bounds_without_the_factor(name, family):
    c = CASES[name]
    obs = dref.make_obs(family, c["A"].shape[0], 10 * family + 1)
    x, mu = _point(c["Q"].shape[0], family)
    r = dref.eval_ref(c, obs, x, mu, _tm(name))
    got = dref.eval_f64(c, obs, x, mu, _tm(name))
    ratio = dref.exceeds(c, obs, x, mu, _tm(name), r, got, factor=1)
    print(f"{name} family {family}: float64 control err / bound (factor 1) {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", dref.MUTANTS)
def test_each_mutant_exceeds_the_bounds_somewhere(mutant):
    worst = 0.0
    for name, c in CASES.items():
        for family in range(6):
            obs = dref.make_obs(family, c["A"].shape[0], 10 * family + 1)
            x, mu = _point(c["Q"].shape[0], family)
            r = dref.eval_ref(c, obs, x, mu, _tm(name))
            worst = max(worst, dref.exceeds(c, obs, x, mu, _tm(name), r, dref.eval_f64(c, obs, x, mu, _tm(name), mutant), factor=16))
    assert worst > 1.0, (mutant, worst)


# ---- the loop cases ------------------------------------------------------------------------------------------------------------------------
LOOP = dref.loop_cases()


@pytest.mark.parametrize("name", list(LOOP))
def test_loop_cases_reach_their_branches_away_from_every_threshold(name):
    c = LOOP[name]
    a, b = dref.restate_loop(c, np.float64), dref.restate_loop(c, ref.LD)
    assert c["events"] <= set(a["events"]), a["events"]
    assert a["converged"] and dref.far_from_thresholds(a["margins"]), [m for m in a["margins"]]
    assert np.array_equal(a["alpha_trace"], b["alpha_trace"]) and a["iterations"] == b["iterations"] and a["events"] == b["events"]


def test_loop_cases_cover_what_they_must():
    ev = {k: set(dref.restate_loop(c, np.float64)["events"]) for k, c in LOOP.items()}
    assert any("backtrack" in e for e in ev.values()) and any("frozen_return" in e for e in ev.values())
    assert any(c["C"] is not None for c in LOOP.values()) and any(c["C"] is None for c in LOOP.values())
    assert any(c["A"].shape[1] == 257 for c in LOOP.values())           # the intercept column
