"""What tests/test_gpu_batch_predictive.py rests on, no device: the cases of tests/batch_predictive_cases.py sit on the edges they
name, the float64 control of each restatement stays inside the bounds WITHOUT the factor, every named mutant leaves them WITH it, and
the refusals of the batched predictive calls that need no device pass through the C ABI (symbolic-only handles, as
tests/test_api_refusals_host.py)."""
import ctypes as C

import numpy as np
import pytest

import batch_design_cases as dc
import batch_predictive_cases as pc
import predictive_ref as pref
from gmrfx._lib import GmrfxOpts, lib, ptr

LD = pref.LD
INVALID_ARG, NO_DEVICE = 1, 2
_CACHE = {}


def _posterior(p):
    """per member: Sigma on the pattern, float64 (the stand-in for the handle's selected inverse)"""
    key = (p["design"], p["nobs"], p["obs"].family, p["B"])
    if key not in _CACHE:
        _CACHE[key] = [pref.dense_posterior(pc.member_case(p, k))[0] for k in range(p["B"])]
    return _CACHE[key]


def test_the_cases_sit_on_the_edges_they_name():
    assert pc.NODE_TWO_BLOCKS in pref.NODE_NOBS and pc.NODE_TWO_BLOCKS > 256             # kPredNode: two workgroups per member
    assert pc.DESIGN_THREE_BLOCKS in pref.DESIGN_NOBS and -(-pc.DESIGN_THREE_BLOCKS // 16) == 3      # kDesignRows: three, and three partials
    assert -(-pc.NODE_TWO_BLOCKS // 16) == 17                                           # partial quadruples of k_pred_scores per member
    assert {255, 256, 257} <= set(pc.MIX_NOBS) and {1, 17} <= set(pc.MIX_B)             # kPredMix = 256
    for family in (0, 4, 5):
        p = pc.problem(False, 257, family)
        assert len(set(p["params"])) == 3
        C3 = pc.consts(p)
        assert not np.array_equal(C3[:, 0], C3[:, 1]) and not np.array_equal(C3[:, 1], C3[:, 2])
    for family in (1, 2, 3):
        C3 = pc.consts(pc.problem(False, 257, family))
        assert np.array_equal(C3[:, 0], C3[:, 1]) and np.array_equal(C3[:, 0], C3[:, 2])
    p = pc.problem(True, 33, 1, True)
    assert len({Q.data.tobytes() for Q in p["Qs"]}) == 3 and not np.array_equal(p["X"][:, 0], p["X"][:, 1])
    for Q in p["Qs"]:
        assert np.linalg.eigvalsh(dc.sym_dense(Q, p["uplo"])).min() > 0
    f = pc.with_failing_member(p)
    lam = [np.linalg.eigvalsh(dc.sym_dense(Q, p["uplo"])).min() for Q in f["Qs"]]
    assert lam[0] > 0 and lam[2] > 0 and abs(lam[1] + 2.0) < 1e-8
    one = pc.problem(False, 257, 4, B=1)
    assert one["B"] == 1 and one["params"][0] == pc.problem(False, 257, 4)["params"][1]


@pytest.mark.parametrize("design,nobs,family", [(False, 257, 4), (True, 33, 5), (True, 33, 0)])
def test_float64_control_and_the_member_mutants(design, nobs, family):
    p = pc.problem(design, nobs, family, True)
    S, Cc = _posterior(p), pc.consts(p)
    r = pc.batch_marginals(p, S, Cc)
    tight = pc.batch_bounds(p, S, Cc, r, factor=1)
    ctl = pc.batch_marginals(p, S, Cc, dtype=np.float64)
    for k in range(p["B"]):
        assert max(pref.ratio(ctl[k][key], r[k][key], tight[k][key]) for key in ("mu_eta", "v_eta", "pll")) <= 1.0
    wide = pc.batch_bounds(p, S, Cc, r)
    for mutant in pc.MUTANTS:
        m = pc.batch_marginals(p, S, Cc, mutant=mutant)
        worst = max(pref.ratio(np.asarray(m[k][key], np.float64), r[k][key], wide[k][key]) for k in range(1, p["B"]) for key in ("v_eta", "pll"))
        assert worst > 1.0, mutant
    # member 0 is where the mutants read: it must not be what shows them
    assert all(pref.ratio(np.asarray(pc.batch_marginals(p, S, Cc, mutant=mt)[0][key], np.float64), r[0][key], wide[0][key]) <= 1.0
               for mt in pc.MUTANTS for key in ("mu_eta", "v_eta", "pll"))


@pytest.mark.parametrize("nobs", pc.MIX_NOBS)
@pytest.mark.parametrize("B", pc.MIX_B)
def test_mixture_control_and_mutants(B, nobs):
    logw, mu, v, lpd = pc.mixture_inputs(B, nobs)
    r = pc.mixture(logw, mu, v, lpd)
    tight, wide = pc.mixture_bounds(r, factor=1), pc.mixture_bounds(r)
    ctl = pc.mixture(logw, mu, v, lpd, dtype=np.float64)
    keys = ("mix_mu", "mix_v", "mix_lpd")
    assert max(pref.ratio(ctl[k], r[k], tight[k]) for k in keys) <= 1.0
    om, lo = pc.weights(logw)
    assert abs(float(np.asarray(om, LD).sum()) - 1.0) <= (B + 1) * pref.EPS and np.allclose(np.exp(lo), om, rtol=1e-14, atol=0)
    if B > 1:       # (one member: there is no between-member term)
        assert pref.ratio(np.asarray(pc.mixture(logw, mu, v, lpd, mutant="no_between_term")["mix_v"], np.float64), r["mix_v"], wide["mix_v"]) > 1.0
    bad = pc.mixture(logw, mu, v, lpd, mutant="unnormalised")
    assert max(pref.ratio(np.asarray(bad[k], np.float64), r[k], wide[k]) for k in keys) > 1.0
    # the rules for members: an excluded member's NaN does no harm, an included one's propagates, all -inf gives -inf
    if B > 1:
        lw2, mu2 = logw.copy(), mu.copy()
        lw2[0] = -np.inf
        mu2[:, 0] = np.nan
        assert np.isfinite(pc.mixture(lw2, mu2, v, lpd)["mix_mu"]).all()
        assert np.isnan(pc.mixture(logw, mu2, v, lpd)["mix_mu"]).all()
    assert (pc.mixture(logw, mu, v, np.full_like(lpd, -np.inf))["mix_lpd"] == -np.inf).all()


# ---- the refusals that need no device -------------------------------------------------------------------------------------------------------
N = 6


def _pattern():
    cp, ri = [0], []
    for j in range(N):
        ri += [i for i in (j - 1, j, j + 1) if 0 <= i < N]
        cp.append(len(ri))
    return np.array(cp, dtype=np.int64), np.array(ri, dtype=np.int64)


class _Handle:
    """a symbolic-only handle (nbatch = 0: plain) for the duration of a `with` block"""

    def __init__(self, nbatch=0, n=N, **opts):
        self.nbatch, self.n, self.opts = nbatch, n, opts

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        for k, val in self.opts.items():
            setattr(o, k, val)
        cp, ri = _pattern()
        if self.nbatch:
            rc = lib().gmrfx_create_batched(N, ptr(cp), ptr(ri), 0, None, self.nbatch, C.byref(o), C.byref(self.h))
        else:
            rc = lib().gmrfx_create(N, ptr(cp), ptr(ri), 0, None, C.byref(o), C.byref(self.h))
        assert rc == 0 and self.h.value, lib().gmrfx_last_create_error()
        return self.h

    def __exit__(self, *exc):
        lib().gmrfx_destroy(self.h)


def _msg(h):
    return lib().gmrfx_last_error(h).decode()


@pytest.mark.parametrize("nbatch", [0, 3])
def test_refusals_through_the_c_abi(nbatch):
    """nbatch = 0: a plain handle, a batch of one to these calls"""
    L = lib()
    B = max(nbatch, 1)
    nobs = 4
    with _Handle(nbatch) as h:
        X = np.zeros((N, B), order="F")
        outs = [np.full((nobs, B), np.nan, order="F") for _ in range(4)]
        o3, o4 = [ptr(a) for a in outs[:3]], [ptr(a) for a in outs]
        mu, v = np.zeros((nobs, B), order="F"), np.ones((nobs, B), order="F")
        tot, info = np.full((4, B), np.nan, order="F"), np.zeros(B, np.int64)
        z, w = np.zeros(2), np.full(2, 0.5)
        lw = np.zeros(B)
        marg = lambda x=X, sx=N, fl=0, o=o3: L.gmrfx_batch_predictor_marginals(h, ptr(x), sx, fl, *o, ptr(info))      # noqa: E731
        score = lambda K=2, zz=z, ww=w, m_=mu, t_=tot: L.gmrfx_batch_predictive_scores(h, ptr(m_), ptr(v), K, ptr(zz), ptr(ww), *o4, ptr(t_), ptr(info))      # noqa: E731
        mix = lambda l_=lw, lp=None, ml=None, mm=o3[0]: L.gmrfx_batch_predictive_mixture(h, ptr(l_), ptr(mu), ptr(v), lp, mm, o3[1], ml, None)      # noqa: E731
        assert L.gmrfx_batch_obs_pointwise_const(h, o3[0]) == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert marg() == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert score() == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert mix() == INVALID_ARG and "no observation likelihood" in _msg(h)
        y, idx, par = np.array([1.0, 0.0, 3.0, 2.0]), np.array([4, 0, 2, 5], np.int64), np.linspace(0.5, 1.5, B)
        assert L.gmrfx_batch_obs_set(h, 4, nobs, ptr(idx), 0, ptr(y), None, ptr(par)) == 0
        # the constants need no device: the bits of the plain rule at param[k], one column per member
        Cc = np.full((nobs, B), np.nan, order="F")
        assert L.gmrfx_batch_obs_pointwise_const(h, ptr(Cc)) == 0
        import fisher_ref as ref
        for k in range(B):
            want = np.asarray(pref.pointwise_const(ref.Obs(4, idx, y, None, float(par[k])))[0], np.float64)
            assert np.abs(Cc[:, k] - want).max() <= 4 * pref.EPS * np.abs(want).max()
        assert L.gmrfx_batch_obs_pointwise_const(h, None) == INVALID_ARG and "out is null" in _msg(h)
        for call, what in ((lambda: marg(x=None), "x is null"), (lambda: marg(o=[None] * 3), "every output is null"), (lambda: marg(fl=2), "unknown flag bits"),
                         (lambda: marg(fl=-1), "unknown flag bits"), (lambda: marg(fl=1), "needs a batch constraint"), (lambda: marg(sx=N - 1), "member stride smaller than n"),
                         (lambda: score(m_=None), "mu_eta / v_eta is null"), (lambda: score(t_=None), "out is null"), (lambda: score(K=0), "K must be 1 .. 64"),
                         (lambda: score(K=65), "K must be 1 .. 64"), (lambda: score(zz=None), "nodes / weights are null"),
                         (lambda: score(zz=np.array([0.0, np.nan])), "not finite"), (lambda: score(ww=np.array([0.5, np.inf])), "not finite"),
                         (lambda: score(ww=np.array([0.5, 0.0])), "must be positive"), (lambda: score(ww=np.array([0.5, -0.5])), "must be positive"),
                         (lambda: mix(l_=None), "logw is null"), (lambda: mix(ml=o3[2]), "mix_lpd needs lpd"),
                         (lambda: L.gmrfx_batch_predictive_mixture(h, ptr(lw), ptr(mu), ptr(v), None, None, None, None, None), "every output is null"),
                         (lambda: mix(l_=np.full(B, -np.inf)), "every member is excluded"), (lambda: mix(l_=np.r_[np.nan, np.zeros(B - 1)]), "NaN or +inf"),
                         (lambda: mix(l_=np.r_[np.inf, np.zeros(B - 1)]), "NaN or +inf")):
            rc = call()
            assert rc == INVALID_ARG and what in _msg(h), (what, rc, _msg(h))
        # every argument in order: the handle has no device, and says so only now
        for rc in (marg(), score(), mix()):
            assert rc == NO_DEVICE and "no device state" in _msg(h)
        assert all(np.isnan(a).all() for a in outs) and np.isnan(tot).all()
        # the plain calls keep their refusals
        rc = L.gmrfx_predictor_marginals(h, ptr(X), 0, *o3)
        assert rc == INVALID_ARG and (("batched handles are not supported" in _msg(h)) if nbatch else ("no observation likelihood" in _msg(h)))


def test_more_than_65535_members_are_refused():
    L = lib()
    with _Handle(65536) as h:
        X = np.zeros(1)
        info = np.zeros(1, np.int64)
        assert L.gmrfx_batch_predictor_marginals(h, ptr(X), N, 0, ptr(X), None, None, ptr(info)) == INVALID_ARG
        assert "more than 65535 members" in _msg(h)


def _three_calls(h, B=1, nobs=4):
    """the three batched calls with well-formed arguments on NaN-filled outputs: ((name, call), ...), the outputs"""
    L = lib()
    X = np.zeros((N, B), order="F")
    outs = [np.full((nobs, B), np.nan, order="F") for _ in range(4)]
    o3, o4 = [ptr(a) for a in outs[:3]], [ptr(a) for a in outs]
    mu, v = np.zeros((nobs, B), order="F"), np.ones((nobs, B), order="F")
    tot, info = np.full((4, B), np.nan, order="F"), np.zeros(B, np.int64)
    z, w, lw = np.zeros(2), np.full(2, 0.5), np.zeros(B)
    keep = (X, mu, v, tot, info, z, w, lw)
    calls = (("marginals", lambda: L.gmrfx_batch_predictor_marginals(h, ptr(X), N, 0, *o3, ptr(info))),
             ("scores", lambda: L.gmrfx_batch_predictive_scores(h, ptr(mu), ptr(v), 2, ptr(z), ptr(w), *o4, ptr(tot), ptr(info))),
             ("mixture", lambda: L.gmrfx_batch_predictive_mixture(h, ptr(lw), ptr(mu), ptr(v), None, o3[0], o3[1], None, None)))
    return calls, outs + [tot], keep


def _all_refuse(h, what):
    calls, outs, keep = _three_calls(h)
    for name, call in calls:
        rc = call()
        assert rc == INVALID_ARG and what in _msg(h), (name, rc, _msg(h))
    assert all(np.isnan(a).all() for a in outs)


def test_a_sharded_handle_is_refused_with_the_outputs_untouched():
    with _Handle(shard_world=2, shard_rank=0) as h:
        _all_refuse(h, "sharded handles are not supported")


def test_a_plain_constraint_held_is_refused():
    """the batch calls work with the BATCH constraint; a plain handle that holds gmrfx_constraints_set's is refused, as by the pullback"""
    L = lib()
    with _Handle() as h:
        y, idx, par = np.array([1.0, 0.0, 3.0, 2.0]), np.array([4, 0, 2, 5], np.int64), np.array([1.0])
        assert L.gmrfx_batch_obs_set(h, 4, 4, ptr(idx), 0, ptr(y), None, ptr(par)) == 0
        rp, ci, va, e = np.array([0, N], np.int64), np.arange(N, dtype=np.int64), np.ones(N), np.zeros(1)
        assert L.gmrfx_constraints_set(h, 1, ptr(rp), ptr(ci), ptr(va), 0, ptr(e)) == 0, _msg(h)
        _all_refuse(h, "a constraint set is not supported")
        assert L.gmrfx_constraints_set(h, 0, None, None, None, 0, None) == 0
        calls, outs, keep = _three_calls(h)
        assert all(call() == NO_DEVICE for _, call in calls)        # cleared: every argument is in order again


def test_a_plain_design_likelihood_held_is_refused():
    """gmrfx_obs_set_design on the handle: the batch calls refuse it, as gmrfx_batch_obs_set and the batched pullback do"""
    L = lib()
    with _Handle() as h:
        # A = the first four rows of the identity (CSC over the N columns): pattern(A'A) is the diagonal, which the pattern holds
        cp = np.array([0, 1, 2, 3, 4, 4, 4], np.int64)
        ri, va, y = np.arange(4, dtype=np.int64), np.ones(4), np.array([1.0, 0.0, 3.0, 2.0])
        assert L.gmrfx_obs_set_design(h, 1, 4, ptr(cp), ptr(ri), ptr(va), 0, None, ptr(y), None, 0.0) == 0, _msg(h)
        _all_refuse(h, "the design form (eta = A x + b, gmrfx_obs_set_design) is not supported")
