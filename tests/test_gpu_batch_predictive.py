"""The linear predictor's marginals, the predictive scores and the mixture over the sweep for every member of a batched handle on
the device (gmrfx_batch_predictor_marginals[_dev], gmrfx_batch_predictive_scores[_dev], gmrfx_batch_predictive_mixture[_dev];
csrc/predictive.hip with the member in the launch grid) on the problems of tests/batch_predictive_cases.py.

The yardstick is the guarantee the batched pullback already gives: member k of the batch has THE BITS of the plain handle factorised
at the same Q_post,k with param[k] (same_bits) -- after the assertion that the batch's selected inverse has the plain handle's bits on
these shapes. So that the acceptance does not rest on the plain path alone, member 1 of one family per shape is also held to the
long-double restatement of tests/predictive_ref.py fed the plain handle's Sigma, inside the per-entry bounds derived there. Under flag
bit 0 the batch prepares W_k by its own arithmetic: v_eta is held to marginal_bounds(correct=True) with the restatement fed the
member's own constraint_fields(k)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import batch_laplace_cases as bc
import batch_predictive_cases as pc
import constraint_ref as cref
import gmrfx
import predictive_ref as pref
from gmrfx._lib import ERR_INVALID_ARG, ERR_NOT_FACTORIZED, lib, ptr
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
LD = pref.LD
GH = gmrfx.MI355XBackend.gauss_hermite
K = 17
KEYS = ("lpd", "lcpo", "elp", "vlp")
RESTATED_FAMILY = {1: 0, 255: 1, 256: 2, 257: 4, 15: 3, 16: 5, 17: 4, 33: 5}      # nobs -> the family whose member 1 also meets the restatement


def _set_obs(be, p, param):
    o = p["obs"]
    if p["node"]:
        be.set_observations(o.family, o.y, o.idx, o.aux, param)
    else:
        be.set_design_observations(o.family, o.y, p["A"], p["b"], o.aux, param)


def _batch(p):
    bb = gmrfx.MI355XBatchLaplace(p["Q"], p["B"], device=0, uplo=p["uplo"])
    _set_obs(bb, p, p["params"])
    bb.refactorize_values(bc.values(p["Qs"]))
    return bb


def _batch_all(bb, p, nodes=K, **kw):
    """(mu, v, pll, info, scores dict) of the batch"""
    mu, v, pll, info = bb.predictor_marginals(p["X"], **kw)
    sc = bb.predictive_scores(mu, v, nodes)
    return mu, v, pll, info, sc


def _plain_all(be, p, k, nodes=K):
    """member k on the plain handle be: (mu, v, pll, (lpd, lcpo, elp, vlp), totals as an array of four, selinv diag, constants)"""
    _set_obs(be, p, float(p["params"][k]))
    be.refactorize_values(p["Qs"][k].data)
    mu, v, pll = be.predictor_marginals(p["X"][:, k])
    z, w = GH(nodes)
    arrs, tot = be.predictive_scores(mu, v, z, w)
    return mu, v, pll, arrs, np.array([tot["lpd"], tot["lcpo"], tot["elp"], tot["p_waic"]]), be.get_selinv_diag(), be.observations_pointwise_const()


def _member_same(got, k, plain):
    mu, v, pll, info, sc = got
    ok = same_bits(mu[:, k], plain[0]) and same_bits(v[:, k], plain[1]) and same_bits(pll[:, k], plain[2])
    ok = ok and all(same_bits(sc[key][:, k], a) for key, a in zip(KEYS, plain[3]))
    return ok and same_bits(sc["totals"][:, k], plain[4])


def _sigma(be, Q):
    Z = be.selinv_extract_at(Q).tocoo()
    S = np.zeros(Q.shape)
    S[Z.row, Z.col] = Z.data
    return S


def _restated(tag, be, p, k, got):
    """member k against predictive_ref's long-double restatement fed the plain handle's Sigma and constants (be holds member k)"""
    mu, v, pll, info, sc = got
    c = pc.member_case(p, k)
    cc, S = be.observations_pointwise_const(), _sigma(be, c["Q"])
    r = pref.marginals(c["Ad"], c["b"], c["x"], S, c["obs"], cc, node=c["node"])
    bd = pref.marginal_bounds(c["Ad"], c["b"], c["x"], S, c["obs"], cc, r)
    rat = {key: pref.ratio(g[:, k], r[key], bd[key]) for key, g in zip(("mu_eta", "v_eta", "pll"), (mu, v, pll))}
    z, w = GH(K)
    rs = pref.scores(mu[:, k], v[:, k], z, w, c["obs"], cc)
    bs = pref.score_bounds(z, w, c["obs"], rs)
    rat.update({key: pref.ratio(sc[key][:, k], rs[key], bs[key]) for key in KEYS})
    print(f"{tag}: err/bound {rat}")
    assert max(rat.values()) <= 1.0, rat
    for j, key in enumerate(KEYS):
        assert abs(LD(sc["totals"][j, k]) - np.asarray(sc[key][:, k], LD).sum()) <= pref.total_bound(sc[key][:, k])


def _bits_case(p, tag):
    bb = _batch(p)
    be = gmrfx.MI355XBackend(p["Q"], device=0, uplo=p["uplo"], factorize=False)
    try:
        got = _batch_all(bb, p)
        assert (got[3] == 0).all() and (got[4]["info"] == 0).all()
        sd, C = bb.selinv_diag(), bb.observations_pointwise_const()
        for k in range(p["B"]):
            plain = _plain_all(be, p, k)
            assert same_bits(sd[:, k], plain[5]), f"selected inversion: member {k} of the batch does not have the plain handle's bits"
            assert same_bits(C[:, k], plain[6])
            assert _member_same(got, k, plain), (tag, k)
            if k == 1 and p["obs"].family == RESTATED_FAMILY[p["nobs"]]:
                _restated(f"{tag} member 1", be, p, 1, got)
    finally:
        be.close()
        bb.close()


# ---- 1. member k is the plain handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("nobs", pref.NODE_NOBS)
def test_node_form_member_k_has_the_bits_of_its_plain_handle(nobs, family):
    _bits_case(pc.problem(False, nobs, family), f"node nobs {nobs} family {family}")


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("nobs", pref.DESIGN_NOBS)
def test_design_form_member_k_has_the_bits_of_its_plain_handle(nobs, offset, family):
    _bits_case(pc.problem(True, nobs, family, offset), f"design nobs {nobs} offset {offset} family {family}")


# ---- 2. independence, failures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", [False, True])
def test_a_member_does_not_depend_on_the_batch_it_is_in_nor_on_a_failing_neighbour(design):
    p = pc.problem(design, 33 if design else 257, 4, True)
    bb = _batch(p)
    got = _batch_all(bb, p)
    bb.close()

    def member(g, k):
        return (g[0][:, k], g[1][:, k], g[2][:, k], tuple(g[4][key][:, k] for key in KEYS), g[4]["totals"][:, k])
    for ks in ([2, 0], [1]):
        q = pc.select(p, ks)
        b2 = _batch(q)
        g2 = _batch_all(b2, q)
        b2.close()
        for j, k in enumerate(ks):
            assert _member_same(g2, j, member(got, k)), (ks, k)
    # the middle member's factorisation fails: info = -1, NaN in its slices and totals, the others bit for bit what they were
    f = pc.with_failing_member(p)
    bf = gmrfx.MI355XBatchLaplace(f["Q"], f["B"], device=0, uplo=f["uplo"])
    try:
        _set_obs(bf, f, f["params"])
        nz = bc.values(f["Qs"])
        inf = np.zeros(3, np.int64)
        lib().gmrfx_batch_refactorize(bf._h, ptr(nz), ptr(inf))
        assert inf[0] == 0 and inf[1] > 0 and inf[2] == 0
        gf = _batch_all(bf, f)
        assert list(gf[3]) == [0, -1, 0] and list(gf[4]["info"]) == [0, -1, 0]
        assert all(np.isnan(a[:, 1]).all() for a in gf[:3]) and all(np.isnan(gf[4][key][:, 1]).all() for key in KEYS)
        assert np.isnan(gf[4]["totals"][:, 1]).all()
        for k in (0, 2):
            assert _member_same(gf, k, member(got, k)), k
        # the mean and pll need no factor: delivered for the failed member when v_eta is not asked for
        mu, v, pll, info = bf.predictor_marginals(f["X"], want_var=False)
        assert v is None and (info == 0).all() and same_bits(mu, got[0]) and same_bits(pll, got[2])
    finally:
        bf.close()


# ---- 3. per-member parameters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [0, 4, 5])
def test_set_param_drops_the_constants(family):
    p = pc.problem(False, 257, family)
    assert len(set(p["params"])) == 3
    bb = _batch(p)
    try:
        old = _batch_all(bb, p)
        new = dict(p, params=p["params"][::-1].copy() * 1.25)
        bb.set_param(new["params"])
        got = _batch_all(bb, new)
        fresh = _batch(new)
        want, fresh_c = _batch_all(fresh, new), fresh.observations_pointwise_const()
        fresh.close()
        assert same_bits(bb.observations_pointwise_const(), fresh_c)
        assert same_bits(got[2], want[2]) and all(same_bits(got[4][key], want[4][key]) for key in KEYS + ("totals",))
        assert not same_bits(got[2], old[2])
    finally:
        bb.close()


# ---- 4. the constraint (flag bit 0) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", [False, True])
@pytest.mark.parametrize("m", pref.CON_M)
def test_constraint_correction_and_clamp_per_member(m, design):
    """The clamp is held to what rounding allows. In the rows whose exact value is 0 the sign of v - correction is set by the last
    roundings, and the device's differ from the long-double restatement's: measured on the device (m = 3, design form, member 0) the
    restatement's difference is negative in 6 rows and the member has +0.0 in 2 of them and 2.8e-14 .. 4.5e-13 (inside the bound) in the
    other 4. So "exactly +0.0" is asserted where the restatement is negative beyond its bound, never a negative value or -0.0 anywhere,
    every value within the bound, and in design form that the clamp acts at all (in node form the constrained variances of these
    problems are far from 0: nothing there is clamped, and nothing asserts that it is)."""
    n = pc.grid().shape[0]
    Cm = pref.constraint_rows(n, m)
    if design:
        extra = np.vstack([Cm, 2.0 * Cm[: min(m, 8)]])
        p = pc.problem(True, 17 + len(extra), 1, True, extra_rows=extra)
    else:
        p = pc.problem(False, n, 1)             # every node observed, in scrambled order
    bb = _batch(p)
    try:
        raw = bb.predictor_marginals(p["X"])
        bb.set_constraints(sp.csr_matrix(Cm), np.zeros(m))
        again = bb.predictor_marginals(p["X"])                 # without the bit a held constraint is ignored
        assert all(same_bits(a, b) for a, b in zip(raw[:3], again[:3]))
        got = bb.predictor_marginals(p["X"], constraint_correction=True)
        assert (got[3] == 0).all() and same_bits(got[0], raw[0]) and same_bits(got[2], raw[2])
        C = bb.observations_pointwise_const()
        cv = bb.constrained_var()
        be = gmrfx.MI355XBackend(p["Q"], device=0, uplo=p["uplo"], factorize=False)
        nclamped = 0
        try:
            for k in range(p["B"]):
                At, _ = bb.constraint_fields(k)
                con = cref.prepare(sp.csr_matrix(Cm), np.zeros(m), At)
                be.refactorize_values(p["Qs"][k].data)
                S = _sigma(be, p["Qs"][k])
                c = pc.member_case(p, k)
                r = pref.marginals(c["Ad"], c["b"], c["x"], S, c["obs"], C[:, k], con=con, correct=True, node=c["node"])
                bd = pref.marginal_bounds(c["Ad"], c["b"], c["x"], S, c["obs"], C[:, k], r, con=con, correct=True)
                rat = pref.ratio(got[1][:, k], r["v_eta"], bd["v_eta"], nonnegative=True)
                print(f"constraint m {m} design {design} member {k}: v_eta err/bound {rat}")
                assert rat <= 1.0
                # the clamp: where the restatement's difference is negative by more than its bound the member gets exactly +0.0;
                # inside the bound the sign is the rounding's own (see the docstring), and the value is held to the bound above
                diff = np.asarray(r["v0"] - r["corr"], LD)
                neg = diff < -bd["v_eta"]
                zero = got[1][:, k] == 0.0
                nclamped += int((zero & (diff <= bd["v_eta"])).sum())
                print(f"  restatement's difference negative in {int((diff < 0).sum())} rows, beyond its bound in {int(neg.sum())}; +0.0 in {int(zero.sum())}")
                assert zero[neg].all() and not np.signbit(got[1][:, k]).any()
                if not design:      # every node observed: within the same bound of constrained_var()[:, k]
                    assert pref.ratio(got[1][:, k], cv[p["obs"].idx, k], bd["v_eta"], nonnegative=True) <= 1.0
        finally:
            be.close()
        # design form: the rows equal to constraint rows have v - correction = 0 in exact arithmetic, of either sign by rounding; with
        # 3 (m + min(m, 8)) >= 18 such values some are left negative and come back as exactly +0.0
        if design and m >= 3:
            assert nclamped > 0
    finally:
        bb.close()


def test_a_member_whose_W_fails_is_masked_out_alone():
    """two equal constraint rows: every healthy member's W_k has a pivot within rounding of zero; which of them the preparation
    reports is its own affair, so the test reads cinfo and holds the marginals to it"""
    p = pc.problem(True, 17, 1, True)
    bb = _batch(p)
    try:
        raw = bb.predictor_marginals(p["X"])
        row = pref.constraint_rows(p["n"], 1)
        bb.set_constraints(sp.csr_matrix(np.vstack([row, row])), np.zeros(2))
        ci = bb.constraint_info(check_posdef=False)["cinfo"]
        mu, v, pll, info = bb.predictor_marginals(p["X"], constraint_correction=True)
        assert list(info) == list(ci) and (ci > 0).any()
        for k in range(3):
            if ci[k] > 0:
                assert np.isnan(mu[:, k]).all() and np.isnan(v[:, k]).all() and np.isnan(pll[:, k]).all()
            else:
                assert same_bits(mu[:, k], raw[0][:, k]) and np.isfinite(v[:, k]).all()
    finally:
        bb.close()


# ---- 5. states ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", [False, True])
def test_after_the_loop_with_refactorize_final_as_after_an_explicit_refactorisation(design):
    p = pc.problem(design, 33 if design else 257, 1, True)
    bb = gmrfx.MI355XBatchLaplace(p["Q"], p["B"], device=0, uplo=p["uplo"])
    try:
        _set_obs(bb, p, p["params"])
        prior = bc.values(p["Qs"])
        bb.set_prior(prior)
        X, H, info = bb.gaussian_approximation(refactorize_final=True)
        assert info["converged"].all()
        q = dict(p, X=X)
        a = _batch_all(bb, q)
        post = prior.copy()
        pos = bb.observations_hess_map() if design else diag_positions(p["Q"])
        post[pos, :] -= H
        bb.refactorize_values(post)
        b = _batch_all(bb, q)
        assert all(same_bits(u, w) for u, w in zip(a[:3], b[:3])) and all(same_bits(a[4][key], b[4][key]) for key in KEYS + ("totals",))
        # a new likelihood drops the tables
        if design:      # (the pattern of the handle holds this A's pairs: the same rows under another family and other parameters)
            p2 = dict(p, obs=pref.design_case(pc.grid(), 33, 0, True)["obs"], params=bc.family_params(0, 3))
        else:
            p2 = pc.problem(False, 255, 3)
        _set_obs(bb, p2, p2["params"])
        bb.refactorize_values(bc.values(p2["Qs"]))
        g2 = _batch_all(bb, p2)
        f2 = _batch(p2)
        w2 = _batch_all(f2, p2)
        f2.close()
        assert all(same_bits(u, w) for u, w in zip(g2[:3], w2[:3])) and same_bits(g2[4]["totals"], w2[4]["totals"])
    finally:
        bb.close()


class _BatchOfOne(gmrfx.MI355XBatchLaplace):
    """the batch entry points of a plain handle (its own handle pointer, not owned)"""

    def __init__(self, plain):
        self.n, self.nbatch, self._nnz, self._h = plain.n, 1, plain._nnz, plain._h
        self._info = np.zeros(1, np.int64)

    def close(self):
        self._h = None


@pytest.mark.parametrize("design", [False, True])
def test_a_plain_handle_with_a_batch_likelihood_is_a_batch_of_one(design):
    """a handle of gmrfx_create, factorised by the plain gmrfx_refactorize: its first batch call makes it a batch of one"""
    p = pc.problem(design, 33 if design else 257, 4, True, B=1)
    plain = gmrfx.MI355XBackend(p["Q"], device=0, uplo=p["uplo"], factorize=False)
    be = gmrfx.MI355XBackend(p["Q"], device=0, uplo=p["uplo"], factorize=False)
    try:
        plain.refactorize_values(p["Qs"][0].data)
        one = _BatchOfOne(plain)
        _set_obs(one, p, p["params"])
        got = _batch_all(one, p)
        assert (got[3] == 0).all() and _member_same(got, 0, _plain_all(be, p, 0))
        mm, mv, ml, tot = one.predictive_mixture(np.zeros(1), got[0], got[1], got[4]["lpd"])
        assert same_bits(mm, got[0][:, 0]) and same_bits(mv, got[1][:, 0]) and same_bits(ml, got[4]["lpd"][:, 0])
        # a MI355XBatchLaplace of one member (gmrfx_create_batched with nbatch = 1) gives the same bits
        bb = _batch(p)
        g2 = _batch_all(bb, p)
        bb.close()
        assert all(same_bits(u, w) for u, w in zip(got[:3], g2[:3])) and same_bits(got[4]["totals"], g2[4]["totals"])
        one.close()
    finally:
        be.close()
        plain.close()


@pytest.mark.parametrize("design", [False, True])
@pytest.mark.parametrize("nodes", [k for k in pref.SCORE_K if k != K])
def test_every_rule_size_has_the_bits_of_the_plain_handle(nodes, design):
    """K = 1, 2, 16, 64 beside the 17 of every other test: one node, a partly filled first round of the lane group, exactly one round,
    all four rounds of kPredNodesPerLane"""
    p = pc.problem(design, 33 if design else 257, 4, True)
    bb = _batch(p)
    be = gmrfx.MI355XBackend(p["Q"], device=0, uplo=p["uplo"], factorize=False)
    try:
        got = _batch_all(bb, p, nodes=nodes)
        for k in range(p["B"]):
            assert _member_same(got, k, _plain_all(be, p, k, nodes=nodes)), (nodes, k)
    finally:
        be.close()
        bb.close()


def _dev(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize("design", [False, True])
def test_host_device_and_misaligned_forms_agree_bit_for_bit(design):
    p = pc.problem(design, 33 if design else 257, 5, True)
    bb = _batch(p)
    try:
        host = _batch_all(bb, p)
        logw = np.array([0.3, -1.0, 2.0])
        hmix = bb.predictive_mixture(logw, host[0], host[1], host[4]["lpd"])
        n, nobs, B = p["n"], p["nobs"], p["B"]
        dev = torch.device("cuda:0")
        for off in (0, 1, 3):           # doubles: offsets 1 and 3 are 8-byte aligned only
            sx = n + 5
            lens = (sx * B,) + (nobs * B,) * 7 + (nobs,) * 3
            bufs = [torch.full((k + 8,), float("nan"), dtype=torch.float64, device=dev) for k in lens]
            win = [b[off:off + k] for b, k in zip(bufs, lens)]
            Xs = np.full((sx, B), np.nan, order="F")
            Xs[:n] = p["X"]
            win[0].copy_(torch.from_numpy(Xs.T.reshape(-1).copy()))
            torch.cuda.synchronize()
            info = bb.predictor_marginals_dev(_dev(win[0]), sx, _dev(win[1]), _dev(win[2]), _dev(win[3]))
            tot, inf2 = bb.predictive_scores_dev(_dev(win[1]), _dev(win[2]), K, d_lpd=_dev(win[4]), d_lcpo=_dev(win[5]), d_elp=_dev(win[6]), d_vlp=_dev(win[7]))
            mt = bb.predictive_mixture_dev(logw, _dev(win[1]), _dev(win[2]), _dev(win[4]), _dev(win[8]), _dev(win[9]), _dev(win[10]))
            torch.cuda.synchronize()
            assert (info == 0).all() and (inf2 == 0).all() and same_bits(tot, host[4]["totals"]) and same_bits(np.array([mt]), np.array([hmix[3]]))
            want = list(host[:3]) + [host[4][key] for key in KEYS]
            for t, a in zip(win[1:8], want):
                assert same_bits(t.cpu().numpy(), a.T.reshape(-1))
            for t, a in zip(win[8:], hmix[:3]):
                assert same_bits(t.cpu().numpy(), a)
            for b, k in zip(bufs[1:], lens[1:]):        # nothing is written outside the window
                assert bool(torch.isnan(torch.cat([b[:off], b[off + k:]])).all())
    finally:
        bb.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    p = pc.problem(False, 257, 1)
    bb = gmrfx.MI355XBatchLaplace(p["Q"], p["B"], device=0, uplo=p["uplo"])
    L, h = lib(), bb._h
    n, nobs, B = p["n"], p["nobs"], p["B"]
    try:
        outs = [np.full((nobs, B), np.nan, order="F") for _ in range(4)]
        tot, info = np.full((4, B), np.nan, order="F"), np.zeros(B, np.int64)
        z, w = GH(K)
        X = p["X"]
        o3 = [ptr(a) for a in outs[:3]]
        mu, v = np.zeros((nobs, B), order="F"), np.ones((nobs, B), order="F")
        o4 = [ptr(a) for a in outs]

        def refused(rc, what, code=ERR_INVALID_ARG):
            assert rc == code, (what, rc)
            assert all(np.isnan(a).all() for a in outs) and np.isnan(tot).all(), what
        refused(L.gmrfx_batch_predictor_marginals(h, ptr(X), n, 0, *o3, ptr(info)), "no likelihood")
        refused(L.gmrfx_batch_predictive_scores(h, ptr(mu), ptr(v), K, ptr(z), ptr(w), *o4, ptr(tot), ptr(info)), "no likelihood (scores)")
        refused(L.gmrfx_batch_predictive_mixture(h, ptr(np.zeros(B)), ptr(mu), ptr(v), None, o3[0], o3[1], None, None), "no likelihood (mixture)")
        _set_obs(bb, p, p["params"])
        refused(L.gmrfx_batch_predictor_marginals(h, ptr(X), n, 0, *o3, ptr(info)), "not factorised", ERR_NOT_FACTORIZED)
        assert L.gmrfx_batch_predictor_marginals(h, ptr(X), n, 0, o3[0], None, o3[2], ptr(info)) == 0        # mean and pll need no factor
        for a in outs:
            a[:] = np.nan
        bb.refactorize_values(bc.values(p["Qs"]))
        refused(L.gmrfx_batch_predictor_marginals(h, None, n, 0, *o3, ptr(info)), "x null")
        refused(L.gmrfx_batch_predictor_marginals(h, ptr(X), n - 1, 0, *o3, ptr(info)), "sx < n")
        refused(L.gmrfx_batch_predictor_marginals(h, ptr(X), n, 0, None, None, None, ptr(info)), "every output null")
        refused(L.gmrfx_batch_predictor_marginals(h, ptr(X), n, 2, *o3, ptr(info)), "unknown flag bits")
        refused(L.gmrfx_batch_predictor_marginals(h, ptr(X), n, 1, *o3, ptr(info)), "bit 0 without a batch constraint")
        sc = lambda Kk, zz, ww, m_=mu, v_=v, t_=tot: L.gmrfx_batch_predictive_scores(h, ptr(m_), ptr(v_), Kk, ptr(zz), ptr(ww), *o4, ptr(t_), ptr(info))      # noqa: E731
        refused(sc(0, z, w), "K = 0")
        refused(sc(65, np.zeros(65), np.ones(65)), "K = 65")
        refused(sc(K, np.r_[z[:-1], np.inf], w), "a node that is not finite")
        refused(sc(K, z, np.r_[w[:-1], 0.0]), "a weight that is not positive")
        refused(sc(K, z, w, m_=None), "mu_eta null")
        refused(L.gmrfx_batch_predictive_scores(h, ptr(mu), ptr(v), K, ptr(z), ptr(w), *o4, None, ptr(info)), "out null")
        mix = lambda lw, lp=None, ml=None: L.gmrfx_batch_predictive_mixture(h, ptr(lw), ptr(mu), ptr(v), lp, o3[0], o3[1], ml, None)      # noqa: E731
        refused(mix(np.full(B, -np.inf)), "every member excluded")
        refused(mix(np.array([0.0, np.nan, 0.0])), "a NaN weight")
        refused(mix(np.array([0.0, np.inf, 0.0])), "a +inf weight")
        refused(mix(np.zeros(B), None, o3[2]), "mix_lpd without lpd")
        refused(L.gmrfx_batch_predictive_mixture(h, ptr(np.zeros(B)), ptr(mu), ptr(v), None, None, None, None, None), "every output null (mixture)")
        # the plain calls keep refusing the batched handle, with their messages
        assert L.gmrfx_predictor_marginals(h, ptr(X), 0, *o3) == ERR_INVALID_ARG and b"batched" in L.gmrfx_last_error(h)
        assert L.gmrfx_predictive_scores(h, ptr(mu), ptr(v), K, ptr(z), ptr(w), *o4, ptr(tot)) == ERR_INVALID_ARG
        assert all(np.isnan(a).all() for a in outs) and np.isnan(tot).all()
    finally:
        bb.close()


# ---- 7. the mixture -----------------------------------------------------------------------------------------------------------------------------
_MIX = {}


def _mix_handle(B):
    """a batched handle of B members on the grid; the caller sets a likelihood of the nobs it wants (the mixture reads nobs alone)"""
    if B not in _MIX:
        _MIX[B] = gmrfx.MI355XBatchLaplace(pc.grid(), B, device=0)
    return _MIX[B]


@pytest.fixture(scope="module", autouse=True)
def _close_mix_handles():
    yield
    for bb in _MIX.values():
        bb.close()
    _MIX.clear()


@pytest.mark.parametrize("nobs", pc.MIX_NOBS)
@pytest.mark.parametrize("B", pc.MIX_B)
def test_mixture_against_the_long_double_restatement(B, nobs):
    bb = _mix_handle(B)
    bb.set_observations(1, np.ones(nobs), np.arange(nobs))
    logw, mu, v, lpd = pc.mixture_inputs(B, nobs)
    if B == 1:
        logw = np.zeros(1)
    mm, mv, ml, tot = bb.predictive_mixture(logw, mu, v, lpd)
    r = pc.mixture(logw, mu, v, lpd)
    bd = pc.mixture_bounds(r)
    rat = {key: pref.ratio(g, r[key], bd[key]) for key, g in zip(("mix_mu", "mix_v", "mix_lpd"), (mm, mv, ml))}
    print(f"mixture B {B} nobs {nobs}: err/bound {rat}")
    assert max(rat.values()) <= 1.0, rat
    assert abs(LD(tot) - np.asarray(ml, LD).sum()) <= pref.total_bound(ml)
    assert abs(LD(tot) - r["total"]) <= pref.total_bound(ml) + bd["mix_lpd"].sum()
    if B == 1:      # one member of weight 1: the inputs, bit for bit
        assert same_bits(mm, mu[:, 0]) and same_bits(mv, v[:, 0]) and same_bits(ml, lpd[:, 0])
    # bit-reproducible; weights shifted by a constant (exact in double: the log weights are multiples of 2^-40 here) give the same bits
    lq = np.round(logw * 2.0 ** 40) / 2.0 ** 40
    a, b = bb.predictive_mixture(lq, mu, v, lpd), bb.predictive_mixture(lq + 8.0, mu, v, lpd)
    assert all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    assert all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, bb.predictive_mixture(lq, mu, v, lpd)))
    if B < 2:
        return
    # an excluded member is never read: its NaN does no harm, and the result is that of the batch without it
    k = B // 2
    lw2, mu2, v2, lp2 = logw.copy(), mu.copy(), v.copy(), lpd.copy()
    lw2[k] = -np.inf
    mu2[:, k] = v2[:, k] = lp2[:, k] = np.nan
    got = bb.predictive_mixture(lw2, mu2, v2, lp2)
    keep = [j for j in range(B) if j != k]
    small = _mix_handle(B - 1)
    small.set_observations(1, np.ones(nobs), np.arange(nobs))
    want = small.predictive_mixture(logw[keep], mu[:, keep], v[:, keep], lpd[:, keep])
    assert all(np.isfinite(np.asarray(x)).all() for x in got) and all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(got, want))
    # an included member's NaN propagates; lpd = -inf in every included member gives -inf, not NaN
    mu3, lp3 = mu.copy(), lpd.copy()
    mu3[0, 0] = lp3[0, 0] = np.nan
    g3 = bb.predictive_mixture(logw, mu3, v, lp3)
    assert np.isnan(g3[0][0]) and np.isnan(g3[1][0]) and np.isnan(g3[2][0]) and np.isnan(g3[3])
    lp4 = lp2.copy()
    lp4[0, keep] = -np.inf
    g4 = bb.predictive_mixture(lw2, mu2, v2, lp4)
    assert g4[2][0] == -np.inf and g4[3] == -np.inf
