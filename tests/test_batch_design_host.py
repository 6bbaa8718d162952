"""Batched Laplace through a design matrix, what needs no device.

1. The C ABI of gmrfx_batch_obs_set_design, gmrfx_batch_obs_hess_map and gmrfx_batch_obs_design_info on symbolic_only handles: every
   refusal of gmrfx_obs_set_design (tests/test_fisher_design_host.py) and every per-member refusal of gmrfx_batch_obs_set
   (tests/test_batch_laplace_host.py) is INVALID_ARG with its message and nothing changed; the member's map equals the Python
   restatement (dref.hess_map) for the five evaluation cases and on upper, lower and full storage; the two batch forms replace each
   other; a plain handle holding the plain design form is still refused; the numeric calls check, then answer NO_DEVICE.
2. The loop cases of tests/batch_design_cases.py: every member's float64 restatement stays away from every threshold
   (dref.far_from_thresholds) and takes the branches of the long-double one; across the cases the members stop at different iterates,
   one backtracks beside one that does not, one takes the frozen finish beside one that does not; the failing member is indefinite at
   its first iterate and its neighbours are not."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import batch_design_cases as dc
import batch_laplace_cases as bc
import fisher_design_ref as dref
import fisher_ref as ref
from gmrfx._lib import EXPORTS, GmrfxOpts, lib, ptr

INVALID_ARG, NO_DEVICE = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gmrfx_batch_obs_set_design", "gmrfx_batch_obs_hess_map", "gmrfx_batch_obs_design_info"]
EVAL = dref.eval_cases()
LOOPS = dc.loop_cases()


class _Handle:
    """a symbolic_only handle of nbatch members of Q's pattern (0: a plain handle)"""

    def __init__(self, Q, nbatch=3, uplo="U", **opts):
        self.Q, self.nbatch, self.uplo, self.opts = Q, nbatch, uplo, opts

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        o.uplo = 0 if self.uplo == "U" else 1
        for k, v in self.opts.items():
            setattr(o, k, v)
        cp, ri = np.ascontiguousarray(self.Q.indptr, np.int64), np.ascontiguousarray(self.Q.indices, np.int64)
        if self.nbatch:
            rc = lib().gmrfx_create_batched(self.Q.shape[0], ptr(cp), ptr(ri), 0, None, self.nbatch, C.byref(o), C.byref(self.h))
        else:
            rc = lib().gmrfx_create(self.Q.shape[0], ptr(cp), ptr(ri), 0, None, C.byref(o), C.byref(self.h))
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


def _dinfo(h):
    a, c, t = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    assert lib().gmrfx_batch_obs_design_info(h, C.byref(a), C.byref(c), C.byref(t)) == 0
    return a.value, c.value, t.value


def _map(h):
    cnt = C.c_int64(-5)
    assert lib().gmrfx_batch_obs_hess_map(h, None, 0, C.byref(cnt)) == 0, _msg(h)
    m = np.full(cnt.value, -1, np.int64)
    assert lib().gmrfx_batch_obs_hess_map(h, ptr(m), m.size, C.byref(cnt)) == 0
    return m


def _set(h, family, y, param, A=None, offset=None, aux=None, base=0, colptr=None, rowval=None, nzval=None, nobs=None, null=()):
    y = None if y is None else np.ascontiguousarray(y, np.float64)
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
    pp = None if param is None else np.ascontiguousarray(param, np.float64)
    cp, rv, nz = (None if nm in null else v for nm, v in (("colptr", cp), ("rowval", rv), ("nzval", nz)))          # (null pointers on request)
    return lib().gmrfx_batch_obs_set_design(h, family, len(y) if nobs is None else nobs, ptr(cp), ptr(rv), ptr(nz), base, ptr(off), ptr(y), ptr(ax),
                                            ptr(pp))


def test_header_declares_and_library_exports_every_new_call():
    hdr = open(os.path.join(ROOT, "include", "gmrfx.h")).read()
    for nm in NEW:
        assert re.search(r"int32_t " + nm + r"\(", hdr), nm
        assert nm in EXPORTS
        getattr(lib(), nm)


# a 6-node chain and a 4 x 6 design matrix inside its pattern (the problem of tests/test_fisher_design_host.py)
N = 6
CHAIN = sp.csc_matrix(sp.diags([np.ones(N - 1), 2 * np.ones(N), np.ones(N - 1)], [-1, 0, 1]))
CHAIN.sort_indices()
A0 = sp.csc_matrix((np.array([0.5, 0.5, 1.0, 0.25, 0.75, 0.0]), (np.array([0, 0, 1, 2, 2, 3]), np.array([0, 1, 2, 2, 3, 5]))), shape=(4, N))
Y0, P3 = np.array([1.0, 2.0, 0.0, 3.0]), np.array([1.0, 2.0, 3.0])


def _refusals():
    cp, rv, nz = A0.indptr.copy(), A0.indices.copy(), A0.data.copy()
    notmono = cp.copy()
    notmono[2] = notmono[3] + 1
    at = np.arange(len(rv))
    big = 1 << 31
    # the list of gmrfx_obs_set_design ...
    out = [("not monotone", dict(y=Y0, colptr=notmono, rowval=rv, nzval=nz)),
           ("[0] != index_base", dict(y=Y0, colptr=cp + 1, rowval=rv, nzval=nz)),
           ("outside [0, nobs)", dict(y=Y0, colptr=cp, rowval=np.where(at == 1, 4, rv), nzval=nz)),
           ("outside [0, nobs)", dict(y=Y0, colptr=cp, rowval=np.where(at == 0, -1, rv), nzval=nz)),
           ("unsorted or repeated", dict(y=Y0, colptr=cp, rowval=np.where(at == 3, 1, rv), nzval=nz)),
           ("unsorted or repeated", dict(y=Y0, colptr=cp, rowval=np.where(at == 2, 3, rv), nzval=nz)),
           ("value of A is not finite", dict(y=Y0, colptr=cp, rowval=rv, nzval=np.where(at == 4, np.inf, nz))),
           ("offset is not finite", dict(y=Y0, A=A0, offset=[0.0, np.nan, 0.0, 0.0])),
           ("unknown family", dict(y=Y0, A=A0, family=6)),
           ("colptr is null", dict(y=Y0, A=A0, null=("colptr",))),
           ("rowval / nzval is null", dict(y=Y0, A=A0, null=("rowval",))),
           ("rowval / nzval is null", dict(y=Y0, A=A0, null=("nzval",))),
           ("index_base", dict(y=Y0, A=A0, base=2)),
           ("nobs is negative", dict(y=Y0, A=A0, nobs=-1)),
           ("entry (0, 2) is missing", dict(y=Y0, A=sp.csc_matrix(np.array([[1.0, 0, 1.0, 0, 0, 0]] * 4)))),
           ("entry (1, 3) is missing", dict(y=Y0, A=sp.csc_matrix(np.array([[1.0, 0, 1.0, 0, 0, 0]] * 4)), base=1)),
           ("2^31 or above", dict(y=Y0, colptr=np.r_[np.zeros(N, np.int64), big], rowval=[0], nzval=[1.0])),
           ("2^31 or above", dict(y=Y0, A=A0, nobs=big)),
           # ... and the per-member list of gmrfx_batch_obs_set
           ("y is null", dict(y=None, A=A0, nobs=4)),
           ("param is null", dict(y=Y0, A=A0, param=None)),
           ("needs aux", dict(y=Y0, A=A0, family=3)),
           ("member 1: sigma / r / phi must be positive", dict(y=Y0, A=A0, family=0, param=[1.0, 0.0, 1.0])),
           ("member 2: sigma / r / phi must be positive", dict(y=Y0, A=A0, family=4, param=[1.0, 2.0, -1.0])),
           ("member 0: sigma / r / phi must be positive", dict(y=Y0 + 1, A=A0, family=5, param=[float("nan"), 1.0, 1.0])),
           ("y is not finite", dict(y=[1.0, np.nan, 0.0, 0.0], A=A0)),
           ("aux is not finite", dict(y=Y0, A=A0, aux=[1.0, 1.0, np.inf, 1.0])),
           ("negative count", dict(y=[1.0, -1.0, 0.0, 0.0], A=A0)),
           ("Bernoulli observation above 1", dict(y=Y0, A=A0, family=2)),
           ("exceeds the number of trials", dict(y=Y0, A=A0, family=3, aux=np.ones(4))),
           ("Gamma observation must be positive", dict(y=Y0, A=A0, family=5))]
    return out


@pytest.mark.parametrize("what,kw", _refusals(), ids=[f"{i}-{w[0].split()[0]}" for i, w in enumerate(_refusals())])
def test_refusals_leave_the_previous_likelihood_in_place(what, kw):
    kw = dict(kw)
    family, param = kw.pop("family", 1), kw.pop("param", P3)
    with _Handle(CHAIN) as h:
        assert _info(h, 3) == (-1, 0, [0.0] * 3) and _dinfo(h) == (-1, -1, -1)
        assert _set(h, family, param=param, **kw) == INVALID_ARG and what in _msg(h), _msg(h)
        assert _info(h, 3) == (-1, 0, [0.0] * 3) and _dinfo(h) == (-1, -1, -1)
        assert _set(h, 4, Y0, P3, A=A0, offset=np.arange(4.0)) == 0, _msg(h)
        before = (_info(h, 3), _dinfo(h), _map(h).tolist())
        assert _set(h, family, param=param, **kw) == INVALID_ARG and what in _msg(h), _msg(h)
        assert (_info(h, 3), _dinfo(h), _map(h).tolist()) == before
    with _Handle(CHAIN) as h:           # ... also a node-form batch likelihood
        assert lib().gmrfx_batch_obs_set(h, 1, N, None, 0, ptr(np.ones(N)), None, ptr(P3)) == 0
        before = _info(h, 3)
        assert _set(h, family, param=param, **kw) == INVALID_ARG
        assert _info(h, 3) == before and _dinfo(h) == (-1, -1, -1)


def test_unsupported_handles_are_refused_with_nothing_changed():
    A_ptr, A_col, A_val, e = np.array([0, N], np.int64), np.arange(N, dtype=np.int64), np.ones(N), np.zeros(1)
    with _Handle(CHAIN, 0, shard_world=2, shard_rank=0) as h:
        assert _set(h, 1, Y0, np.zeros(1), A=A0) == INVALID_ARG and "sharded" in _msg(h)
    with _Handle(CHAIN) as h:
        assert _set(h, 1, Y0, P3, A=A0) == 0
        assert lib().gmrfx_batch_constraints_set(h, 1, ptr(A_ptr), ptr(A_col), ptr(A_val), 0, ptr(e)) == 0, _msg(h)
        before = (_info(h, 3), _dinfo(h))
        assert _set(h, 1, 2 * Y0, P3, A=A0) == INVALID_ARG and "constraint" in _msg(h)
        assert (_info(h, 3), _dinfo(h)) == before
    with _Handle(CHAIN, 0) as h:          # the plain design form on a plain handle: the batch calls still refuse it
        cp, rv = np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int64)
        assert lib().gmrfx_obs_set_design(h, 1, N, ptr(cp), ptr(rv), ptr(np.ones(N)), 0, None, ptr(np.ones(N)), None, 0.0) == 0, _msg(h)
        assert _set(h, 1, Y0, np.zeros(1), A=A0) == INVALID_ARG and "design form" in _msg(h)
        assert lib().gmrfx_batch_set_prior(h, ptr(np.ones(CHAIN.nnz))) == INVALID_ARG and "design form" in _msg(h)
    with _Handle(sp.identity(1, format="csc"), 65536) as h:
        assert _set(h, 1, np.ones(1), np.zeros(65536), A=sp.csc_matrix(np.ones((1, 1)))) == INVALID_ARG and "65535" in _msg(h)
    with _Handle(CHAIN) as h:             # and the plain call keeps refusing batched handles
        cp, rv = np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int64)
        assert lib().gmrfx_obs_set_design(h, 1, N, ptr(cp), ptr(rv), ptr(np.ones(N)), 0, None, ptr(np.ones(N)), None, 0.0) == INVALID_ARG
        assert "batched" in _msg(h)


def test_forms_replace_each_other_counts_and_clones():
    with _Handle(CHAIN) as h:
        cnt = C.c_int64(0)
        assert lib().gmrfx_batch_obs_hess_map(h, None, 0, C.byref(cnt)) == INVALID_ARG and "no design likelihood" in _msg(h)
        assert _set(h, 1, Y0, P3, A=A0) == 0
        assert _dinfo(h) == (6, 7, 8) and _info(h, 3)[:2] == (1, 4)         # (the counts of the plain call on this problem)
        m = np.zeros(7, np.int64)
        assert lib().gmrfx_batch_obs_hess_map(h, ptr(m), 6, C.byref(cnt)) == INVALID_ARG and "cap" in _msg(h)
        c = C.c_void_p()
        assert lib().gmrfx_clone(h, C.byref(c)) == 0
        try:
            assert lib().gmrfx_batch_obs_set(h, 1, N, None, 0, ptr(np.ones(N)), None, ptr(P3)) == 0
            assert _dinfo(h) == (-1, -1, -1) and _info(h, 3)[:2] == (1, N)
            assert _dinfo(c) == (6, 7, 8) and _info(c, 3)[:2] == (1, 4)
        finally:
            lib().gmrfx_destroy(c)
        assert _set(h, 1, Y0, P3, A=A0) == 0 and _dinfo(h) == (6, 7, 8)
        assert _set(h, 1, np.zeros(0), P3, A=A0) == 0               # nobs = 0 clears
        assert _dinfo(h) == (-1, -1, -1) and _info(h, 3)[:2] == (-1, 0)
        assert _set(h, 1, Y0, P3, A=sp.csc_matrix((4, N)), offset=np.arange(4.0)) == 0, _msg(h)          # no stored entry: cnt = 0
        assert _dinfo(h) == (0, 0, 0) and _map(h).size == 0


@pytest.mark.parametrize("family", range(6))
def test_loglik_const_is_the_plain_design_handles_per_member(family):
    obs = ref.make_obs(family, 4, np.random.default_rng(family), "all")
    params = bc.family_params(family, 3)
    aux = None if obs.aux is None else np.ascontiguousarray(obs.aux, np.float64)
    cp, rv, nz = (np.ascontiguousarray(a, t) for a, t in ((A0.indptr, np.int64), (A0.indices, np.int64), (A0.data, np.float64)))
    with _Handle(CHAIN) as h, _Handle(CHAIN, 0) as p:
        assert _set(h, family, obs.y, params, A=A0, aux=obs.aux) == 0, _msg(h)
        c = _info(h, 3)[2]
        for k in range(3):
            assert lib().gmrfx_obs_set_design(p, family, 4, ptr(cp), ptr(rv), ptr(nz), 0, None, ptr(np.ascontiguousarray(obs.y)), ptr(aux),
                                              float(params[k])) == 0, _msg(p)
            pc = C.c_double(0.0)
            assert lib().gmrfx_obs_info(p, None, None, C.byref(pc)) == 0
            assert c[k] == pc.value


@pytest.mark.parametrize("name", list(EVAL))
@pytest.mark.parametrize("B", [0, 1, 3])
def test_the_members_map_equals_the_python_restatement(name, B):
    """B = 0: the batch calls on a plain handle (a batch of one); the list is the one gmrfx_obs_hess_map returns on that pattern"""
    c = EVAL[name]
    want = dref.hess_map(c["Q"], c["uplo"], c["A"])
    y = np.ones(c["A"].shape[0])
    with _Handle(c["Q"], B, c["uplo"]) as h, _Handle(c["Q"], 0, c["uplo"]) as p:
        assert _set(h, 1, y, np.zeros(max(B, 1)), A=c["A"], offset=c["b"]) == 0, _msg(h)
        got = _map(h)
        assert np.array_equal(got, want[0]) and (np.diff(got) > 0).all()
        assert _dinfo(h) == (sp.csc_matrix(c["A"]).nnz, len(want[0]), len(want[2]))
        Ac = sp.csc_matrix(c["A"])
        Ac.sort_indices()
        off = None if c["b"] is None else np.ascontiguousarray(c["b"])
        assert lib().gmrfx_obs_set_design(p, 1, len(y), ptr(np.ascontiguousarray(Ac.indptr, np.int64)), ptr(np.ascontiguousarray(Ac.indices, np.int64)),
                                          ptr(np.ascontiguousarray(Ac.data)), 0, ptr(off), ptr(y), None, 0.0) == 0
        cnt = C.c_int64(0)
        plain = np.zeros(len(got), np.int64)
        assert lib().gmrfx_obs_hess_map(p, C.byref(cnt), ptr(plain)) == 0 and cnt.value == len(got) and np.array_equal(plain, got)


def test_the_members_map_on_every_storage():
    c = EVAL["mesh"]
    S = sp.csc_matrix(sp.triu(c["Q"]) + sp.triu(c["Q"], 1).T)
    for Q, uplo in ((sp.csc_matrix(sp.triu(S)), "U"), (sp.csc_matrix(sp.tril(S)), "L"), (S, "U")):
        Q.sort_indices()
        with _Handle(Q, 3, uplo) as h:
            assert _set(h, 1, np.ones(c["A"].shape[0]), np.zeros(3), A=c["A"]) == 0, _msg(h)
            assert np.array_equal(_map(h), dref.hess_map(Q, uplo, c["A"])[0])


def _eval(h, B, n, x=True, sx=None, ss=None, score=True, hess=True):
    ld = 64
    X, S, H, O = np.zeros(ld * B), np.zeros(ld * B), np.zeros(ld * B), np.zeros(2 * B)
    return lib().gmrfx_batch_fisher_eval(h, ptr(X) if x else None, n if sx is None else sx, None, 0, None, ptr(S) if score else None,
                                         ptr(H) if hess else None, ld if ss is None else ss, ptr(O))


def _ga(h, B, n, sh=None, fn="gmrfx_batch_gaussian_approximation"):
    ld = 64
    X, H, R = np.zeros(ld * B), np.zeros(ld * B), np.zeros(10 * B)
    return getattr(lib(), fn)(h, None, 0, None, 0, 5, 5, 1e-4, 1e-5, 15, ptr(X), n, ptr(H), ld if sh is None else sh, ptr(R), None, None, None, None)


def test_the_numeric_calls_check_then_answer_no_device():
    with _Handle(CHAIN) as h:
        assert _set(h, 1, Y0, P3, A=A0) == 0 and _dinfo(h)[1] == 7          # cnt = 7 > n = 6
        assert _eval(h, 3, N, x=False) == INVALID_ARG and "x is null" in _msg(h)
        assert _eval(h, 3, N, sx=N - 1) == INVALID_ARG and "x: member stride smaller than n" in _msg(h)
        assert _eval(h, 3, N, ss=N - 1) == INVALID_ARG and "score: member stride smaller than n" in _msg(h)
        assert _eval(h, 3, N, ss=N) == INVALID_ARG and "hess: member stride smaller than cnt" in _msg(h)
        assert _eval(h, 3, N, ss=N, hess=False) == NO_DEVICE
        assert _eval(h, 3, N, ss=7) == NO_DEVICE and "no device state" in _msg(h)
        for fn in ("gmrfx_batch_gaussian_approximation", "gmrfx_batch_gaussian_approximation_dev"):
            assert _ga(h, 3, N, sh=N, fn=fn) == INVALID_ARG and "hess: member stride smaller than cnt" in _msg(h)
            assert _ga(h, 3, N, sh=7, fn=fn) == NO_DEVICE
        assert lib().gmrfx_batch_set_prior(h, ptr(np.ones(CHAIN.nnz * 3))) == NO_DEVICE


# ---- the loop cases --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    return {name: [dc.restate(c, k, np.float64) for k in range(len(c["Qs"]))] for name, c in LOOPS.items() if name != "one_fails"}


def test_the_cases_start_from_the_loop_cases_of_the_plain_design_form():
    assert set(LOOPS) == {"mesh_far0", "mesh_far8", "intercept_far0", "one_fails"}
    for name, c in LOOPS.items():
        assert len(c["Qs"]) >= 3 and c["base"]["C"] is None
        for Q in c["Qs"]:
            assert np.array_equal(Q.indptr, c["base"]["Q"].indptr) and np.array_equal(Q.indices, c["base"]["Q"].indices)
    for name in dc.LOOP_SC:
        assert np.array_equal(LOOPS[name]["Qs"][0].data, dref.loop_cases()[name]["Q"].data)         # member 0 is the plain case itself


@pytest.mark.parametrize("name", list(dc.LOOP_SC))
def test_every_member_stays_away_from_every_threshold(restated, name):
    for k, a in enumerate(restated[name]):
        assert dref.far_from_thresholds(a["margins"]), (name, k)
        assert a["converged"], (name, k)


def test_no_member_sits_on_a_rounding_knife_edge(restated):
    """the long-double restatement takes the same branches (one case: the others are covered by the margins above and, on the device,
    by tests/test_gpu_batch_design_laplace.py, which restates every member in long double)"""
    c = LOOPS["intercept_far0"]
    for k, a in enumerate(restated["intercept_far0"]):
        b = dc.restate(c, k, ref.LD)
        assert np.array_equal(a["alpha_trace"], b["alpha_trace"]) and a["iterations"] == b["iterations"] and a["events"] == b["events"]


def test_the_cases_hold_the_branches_the_lockstep_loop_must_keep_apart(restated):
    def backtracks(a):
        return a["events"].count("backtrack")
    per_case = {name: r for name, r in restated.items()}
    assert any(len({a["iterations"] for a in r}) >= 2 for r in per_case.values())
    assert len({a["iterations"] for a in per_case["mesh_far0"]}) >= 3
    assert any(any(backtracks(a) > 0 for a in r) and any(backtracks(a) == 0 for a in r) for r in per_case.values())
    assert any(any(a["frozen"] for a in r) and any(not a["frozen"] for a in r) for r in per_case.values())
    for name in ("mesh_far0", "mesh_far8", "intercept_far0"):         # each case by itself mixes frozen finishes with plain stops
        assert {a["frozen"] for a in per_case[name]} == {True, False}, name
    assert len({backtracks(a) for a in per_case["mesh_far0"]}) >= 3


def test_one_fails_is_indefinite_at_the_first_iterate_between_two_healthy_members():
    c = LOOPS["one_fails"]
    Ad = c["base"]["A"].toarray()
    for k in range(3):
        D = dc.sym_dense(c["Qs"][k], c["base"]["uplo"]) + Ad.T @ Ad          # Q_p - H(x0): H(0) = -A' A for Poisson without an offset
        if k == 1:
            assert np.linalg.eigvalsh(D).min() <= -1.0
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(D)
        else:
            np.linalg.cholesky(D)
            a = dc.restate(c, k, np.float64)
            assert a["converged"] and dref.far_from_thresholds(a["margins"])
