"""The pullback of gaussian_approximation for every member of a batched handle on the device (gmrfx_batch_ga_pullback[_dev],
csrc/ga_pullback.hip with the member in the launch grid) on the problems of tests/batch_ga_pullback_cases.py.

The yardstick is the guarantee the batched loop and batch_logpdf_grad already give: member k of the batch has THE BITS of the plain
handle of Q_p,k, param[k] and its own operands (same_bits). So that the acceptance does not rest on the plain path alone, member 1 of
one family per case is also held to the long-double restatement of tests/ga_pullback_ref.py fed the handle's lam, inside the per-entry
bounds derived there, with the solve's residual below gref.SOLVE_RESIDUAL (the plain test's rule). Projection (flag bit 0): the batch
prepares W_k by its own arithmetic, so lam is held to constraint_ref's bound around the corrected plain lam, not to bits."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import batch_ga_pullback_cases as gc
import batch_laplace_cases as bc
import constraint_ref as cref
import fisher_ref as ref
import ga_pullback_ref as gref
import gmrfx
from gmrfx._lib import ERR_NOT_POSDEF, lib, ptr
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
LD = gref.LD
RESTATED_FAMILY = {"grid": 4, "mesh": 5, "rows": 0, "cols": 4, "intercept": 5}       # the family whose member 1 also meets the restatement
_PLAIN, _BATCH = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    for be in list(_PLAIN.values()) + list(_BATCH.values()):
        be.close()
    _PLAIN.clear()
    _BATCH.clear()


def _set_obs(be, p, param):
    o = p["obs"]
    if p["A"] is None:
        be.set_observations(o.family, o.y, o.idx, o.aux, param)
    else:
        be.set_design_observations(o.family, o.y, p["A"], p["b"], o.aux, param)


def _plain(p, k, Q=None, **kw):
    """member k of p on a plain handle: (Qbar_prior, mubar_prior, lam, param, check) with refactorize=True"""
    if p["name"] not in _PLAIN:
        _PLAIN[p["name"]] = gmrfx.MI355XBackend(p["Q"], device=0, uplo=p["uplo"], factorize=False)
    be = _PLAIN[p["name"]]
    _set_obs(be, p, float(p["params"][k]))
    Qk = p["Qs"][k] if Q is None else Q
    be.set_prior(Qk.data, diag_positions(Qk) if p["A"] is None else be.observations_hess_map())
    args = dict(mean=p["mu"][:, k], mubar=p["mubar"][:, k], Qbar=p["Gv"][:, k], refactorize=True)
    args.update(kw)
    return be.ga_pullback(p["X"][:, k], **args)


def _batch(p, fresh=False):
    """the batched handle of p's case and size with p's likelihood and priors in place"""
    key = (p["name"], p["B"])
    if fresh or key not in _BATCH:
        bb = gmrfx.MI355XBatchLaplace(p["Q"], p["B"], device=0, uplo=p["uplo"])
        if fresh:
            _set_obs(bb, p, p["params"])
            bb.set_prior(bc.values(p["Qs"]))
            return bb
        _BATCH[key] = bb
    bb = _BATCH[key]
    _set_obs(bb, p, p["params"])
    bb.set_prior(bc.values(p["Qs"]))
    return bb


def _run(p, **kw):
    args = dict(mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"], refactorize=True)
    args.update(kw)
    return _batch(p).ga_pullback(p["X"], **args)


def _member(got, k):
    """member k's five of a batch result"""
    return tuple(None if a is None else a[:, k] for a in got[:3]) + (float(got[3][k]), float(got[4][k]))


def _same(a, b):
    """two (Qbar_prior, mubar_prior, lam, param, check) with the same bits"""
    arrays = all((u is None and v is None) or same_bits(u, v) for u, v in zip(a[:3], b[:3]))
    return arrays and same_bits(np.array(a[3:], float), np.array(b[3:], float))


def _restated(tag, p, k, got, mubar=True, G=True, mu=True):
    """member k's five against the restatement fed its own lam: the rule of tests/test_gpu_ga_pullback.py::_check"""
    qp, mp, lam, par, chk = got
    o = gc.member_obs(p, k)
    S = gref._sym(p["Qs"][k], p["uplo"])
    krow = ref.symmetric_coo(p["Qs"][k], p["uplo"])[3]
    mb, Gd = (p["mubar"][:, k] if mubar else None), (p["Gd"][k] if G else None)
    r = gref.restate(S, p["mu"][:, k] if mu else None, p["Ad"], p["b"], o, p["X"][:, k], mb, Gd, lam=lam)
    bd = gref.bounds(S, p["Ad"], p["b"], o, p["X"][:, k], mb, Gd, r, lam, krow=krow)
    xb = r["xbar"]
    nx = float(np.sqrt((xb * xb).sum()))
    resid = r["Qpost"] @ np.asarray(lam, LD) - xb
    rel = float(np.sqrt((resid * resid).sum())) / nx
    got_d = {"param": par, "check": chk}
    if qp is not None:
        got_d["Qbar_prior"] = qp
        r = dict(r, Qbar_prior=gref.to_pattern(p["Q"], r["Qbar_prior"]))
        bd = dict(bd, Qbar_prior=gref.to_pattern(p["Q"], bd["Qbar_prior"]))
    if mp is not None:
        got_d["mubar_prior"] = mp
    rat = gref.ratios(got_d, r, bd)
    print(f"{tag}: solve residual {rel:.2e} err/bound {rat}")
    assert rel < gref.SOLVE_RESIDUAL
    assert (np.abs(resid) <= bd["xbar"] + gref.SOLVE_RESIDUAL * nx).all()
    assert all(np.isfinite(np.asarray(v)).all() for v in got_d.values())
    assert max(rat.values()) <= 1.0, rat


# ---- 1. member k is the plain handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("name", gc.NAMES)
def test_member_k_has_the_bits_of_its_plain_handle(name, family):
    p = gc.problem(name, family)
    got = _run(p)
    assert (got[5] == 0).all()
    for k in range(p["B"]):
        assert _same(_member(got, k), _plain(p, k)), (name, family, k)
    if family not in gref.HAS_PARAM:
        assert (got[3] == 0.0).all()
    if family == RESTATED_FAMILY[name]:
        _restated(f"{name} family {family} member 1", p, 1, _member(got, 1))


# ---- 2. independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.NAMES)
def test_a_member_does_not_depend_on_the_batch_it_is_in(name):
    p = gc.problem(name, 4)
    got = _run(p)
    two = gc.select(p, [2, 0])
    g2 = _run(two)
    assert _same(_member(g2, 0), _member(got, 2)) and _same(_member(g2, 1), _member(got, 0))
    g1 = _run(gc.select(p, [1]))
    assert _same(_member(g1, 0), _member(got, 1))


# ---- 3. one failing member ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "intercept"])
def test_one_failing_member_is_masked_out_alone(name):
    p = gc.problem(name, 1)
    good = _run(p)
    f = gc.with_failing_member(p)
    got = _run(f)
    assert list(got[5]) == [0, -1, 0]
    assert all(np.isnan(a[:, 1]).all() for a in got[:3]) and np.isnan(got[3][1]) and np.isnan(got[4][1])
    for k in (0, 2):
        assert _same(_member(got, k), _member(good, k)), k
    # without info the C call says so, and the healthy members are written all the same
    bb = _batch(f)
    n, nnz, B = p["n"], p["Q"].nnz, p["B"]
    qp, mp, lam = (np.full((r, B), 7.0, order="F") for r in (nnz, n, n))
    out = np.full((2, B), 7.0, order="F")
    rc = lib().gmrfx_batch_ga_pullback(bb._h, ptr(f["X"]), n, ptr(f["mu"]), n, ptr(f["mubar"]), ptr(f["Gv"]), 2, ptr(qp), ptr(mp), ptr(lam), ptr(out), None)
    assert rc == ERR_NOT_POSDEF and "member 1" in lib().gmrfx_last_error(bb._h).decode()
    for k in (0, 2):
        assert _same((qp[:, k], mp[:, k], lam[:, k], out[0, k], out[1, k]), _member(good, k)), k
    assert np.isnan(qp[:, 1]).all() and np.isnan(mp[:, 1]).all() and np.isnan(lam[:, 1]).all() and np.isnan(out[:, 1]).all()
    # a held failure (no bit 1) masks the member just the same
    held = _batch(f).ga_pullback(f["X"], mean=f["mu"], mubar=f["mubar"], Qbar=f["Gv"])
    assert list(held[5]) == [0, -1, 0] and all(_same(_member(held, k), _member(good, k)) for k in (0, 2))


# ---- 4. loop then pullback --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_loop_then_pullback_equals_flag_bit_1_at_the_modes(name):
    p = gc.problem(name, 1)
    bb = _batch(p)
    X, _, info = bb.gaussian_approximation(mean=p["mu"], refactorize_final=True)
    assert info["converged"].all()
    a = bb.ga_pullback(X, mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"])
    b = bb.ga_pullback(X, mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"], refactorize=True)
    assert (a[5] == 0).all() and all(_same(_member(a, k), _member(b, k)) for k in range(p["B"]))


# ---- 5. layouts ---------------------------------------------------------------------------------------------------------------------------------
def _dev(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize("name", ["grid", "intercept"])
def test_host_device_and_misaligned_forms_agree_bit_for_bit(name):
    p = gc.problem(name, 4)
    n, nnz, B = p["n"], p["Q"].nnz, p["B"]
    mu1 = np.ascontiguousarray(p["mu"][:, 0])                       # smu = 0: one mean for all
    host = _run(p, mean=mu1)
    bb = _batch(p)
    dev = torch.device("cuda:0")
    sx = n + 5                                                      # sx > n
    Xs = np.full((sx, B), np.nan, order="F")
    Xs[:n] = p["X"]
    for off in (0, 1, 3):           # doubles: offsets 1 and 3 are 8-byte aligned only
        lens = (sx * B, n, n * B, nnz * B, nnz * B, n * B, n * B)
        bufs = [torch.full((k + 8,), float("nan"), dtype=torch.float64, device=dev) for k in lens]
        dx, dm, db, dq, oq, om, ol = (b[off:off + k] for b, k in zip(bufs, lens))
        for t, a in ((dx, Xs), (dm, mu1), (db, p["mubar"]), (dq, p["Gv"])):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a.reshape(-1, order="F"))))
        torch.cuda.synchronize()
        par, chk, info = bb.ga_pullback_dev(_dev(dx), sx, _dev(dm), 0, _dev(db), _dev(dq), _dev(oq), _dev(om), _dev(ol), refactorize=True)
        torch.cuda.synchronize()
        assert (info == 0).all() and same_bits(par, host[3]) and same_bits(chk, host[4])
        for t, a in ((oq, host[0]), (om, host[1]), (ol, host[2])):
            assert same_bits(t.cpu().numpy(), a.reshape(-1, order="F"))
        for b, k in zip(bufs[4:], lens[4:]):        # nothing is written outside the window
            assert bool(torch.isnan(torch.cat([b[:off], b[off + k:]])).all())
        # Qbar_prior written over Qbar
        par2, chk2, _ = bb.ga_pullback_dev(_dev(dx), sx, _dev(dm), 0, _dev(db), _dev(dq), _dev(dq), 0, 0)
        torch.cuda.synchronize()
        assert same_bits(par2, host[3]) and same_bits(chk2, host[4]) and same_bits(dq.cpu().numpy(), host[0].reshape(-1, order="F"))


# ---- 6. each nullable argument on its own -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_each_nullable_argument_on_its_own(name):
    p = gc.problem(name, 5)
    full = _run(p)
    bb = _batch(p)
    for want in ((True, False, False), (False, True, False), (False, False, True)):
        got = bb.ga_pullback(p["X"], mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"], want_Qbar_prior=want[0], want_mubar_prior=want[1],
                             want_lambda=want[2])
        for w, a, b in zip(want, got[:3], full[:3]):
            assert (a is None) if not w else same_bits(a, b)
        assert same_bits(got[3], full[3]) and same_bits(got[4], full[4])
    noG = bb.ga_pullback(p["X"], mean=p["mu"], mubar=p["mubar"], Qbar=None)
    noM = bb.ga_pullback(p["X"], mean=p["mu"], mubar=None, Qbar=p["Gv"])
    for k in range(p["B"]):
        _restated(f"{name} no Qbar member {k}", p, k, _member(noG, k), G=False)
        _restated(f"{name} no mubar member {k}", p, k, _member(noM, k), mubar=False)
    noMu = bb.ga_pullback(p["X"], mean=None, mubar=p["mubar"], Qbar=p["Gv"], refactorize=True)
    for k in range(p["B"]):
        _restated(f"{name} no mu member {k}", p, k, _member(noMu, k), mu=False)
        assert _same(_member(noMu, k), _plain(p, k, mean=None)), k


# ---- 7. projection -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_projection_with_a_sum_to_zero_batch_constraint(name):
    p = gc.problem(name, 1)
    n, B = p["n"], p["B"]
    free = _run(p)
    bb = _batch(p, fresh=True)
    Cm = sp.csr_matrix(np.ones((1, n)))
    try:
        bb.set_constraints(Cm, np.zeros(1))
        plain = bb.ga_pullback(p["X"], mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"], refactorize=True)       # held, bit 0 clear: the plain solve
        assert all(_same(_member(plain, k), _member(free, k)) for k in range(B))
        proj = bb.ga_pullback(p["X"], mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"], project=True)
        assert (proj[5] == 0).all()
        for k in range(B):
            At, _ = bb.constraint_fields(k)
            c = cref.prepare(Cm, np.zeros(1), At)
            rr = cref.correct(c, plain[2][:, k])
            err = np.abs(np.asarray(proj[2][:, k], LD) - rr["Xc"][:, 0])
            bound = cref.bound_X(c, rr)[:, 0]
            ratio = cref.residual_ratio(Cm, np.zeros(1), proj[2][:, k])
            print(f"{name} member {k}: projected lam err/bound {float((err / bound).max()):.3f} residual ratio {float(ratio):.3f}")
            assert (err <= bound).all() and ratio <= 1.0
    finally:
        bb.close()


# ---- 8. freshness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_read_outs_are_fresh_after_flag_bit_1(name):
    p = gc.problem(name, 1)
    bb = _batch(p)
    B, NZ = p["B"], bc.values(p["Qs"])
    bb.ga_pullback(p["X"] + 0.25, mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"], refactorize=True)       # another point first: nothing of it may survive
    bb.ga_pullback(p["X"], mean=p["mu"], mubar=p["mubar"], Qbar=p["Gv"], refactorize=True)
    _, H, _, _ = bb.fisher_eval(p["X"], mean=p["mu"], want_score=False)
    pos = diag_positions(p["Q"]) if p["A"] is None else bb.observations_hess_map()
    NZpost = NZ.copy(order="F")
    NZpost[pos, :] -= H
    fresh = gmrfx.MI355XBatchBackend(p["Q"], B, device=0, uplo=p["uplo"])
    try:
        assert (fresh.refactorize_values(NZpost) == 0).all()
        assert same_bits(bb.logdet(), fresh.logdet()) and same_bits(bb.selinv_diag(), fresh.selinv_diag())
    finally:
        fresh.close()


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "mesh"])
def test_end_to_end_gradient_of_the_laplace_objective_per_member(name):
    """theta_k scales member k's prior: batch loop (flag bit 3) -> logpdf_grad_dev(ybar = -1) -> ga_pullback_dev in place ->
    pattern_dot_dev gives dL/dtheta_k of -logpdf(posterior_k, x*_k) for all k. Bits: the plain chain per member. Member 0 also within the
    summed bound of tests/test_gpu_ga_pullback.py::test_end_to_end_gradient_of_the_laplace_objective, built the same way."""
    p = gc.problem(name, 1)
    Q, n, nnz, B = p["Q"], p["n"], p["Q"].nnz, p["B"]
    thetas = [1.3, 0.6, 2.1]
    p = dict(p, Qs=[gc.dc.shifted(Q, t, 0.0) for t in thetas])
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.reshape(-1, order="F"))).to(dev)
    bb = _batch(p)
    d_mu, d_x = up(p["mu"]), torch.empty(n * B, dtype=torch.float64, device=dev)
    d_G, d_J = torch.empty(nnz * B, dtype=torch.float64, device=dev), up(np.repeat(Q.data[:, None], B, axis=1))
    d_lam = torch.empty(n * B, dtype=torch.float64, device=dev)
    info = bb.gaussian_approximation_dev(d_x.data_ptr(), n, d_mu=d_mu.data_ptr(), smu=n, refactorize_final=True)
    assert info["converged"].all()
    assert (bb.logpdf_grad_dev(d_x.data_ptr(), n, -1.0, d_Qbar=d_G.data_ptr(), d_mu=d_x.data_ptr()) == 0).all()
    torch.cuda.synchronize()
    Gv = d_G.cpu().numpy().reshape(nnz, B, order="F")
    _, _, pinfo = bb.ga_pullback_dev(d_x.data_ptr(), n, d_mu.data_ptr(), n, 0, d_G.data_ptr(), d_G.data_ptr(), 0, d_lam.data_ptr())
    assert (pinfo == 0).all()
    got = bb.pattern_dot_dev(d_G.data_ptr(), d_J.data_ptr(), nnz, nnz, 1)[0]
    X, lam = (t.cpu().numpy().reshape(n, B, order="F") for t in (d_x, d_lam))
    # the plain chain, member by member
    be = _PLAIN.get(name) or _PLAIN.setdefault(name, gmrfx.MI355XBackend(Q, device=0, uplo=p["uplo"], factorize=False))
    for k in range(B):
        _set_obs(be, p, 0.0)
        Qk = p["Qs"][k]
        be.set_prior(Qk.data, diag_positions(Qk) if p["A"] is None else be.observations_hess_map())
        mu_k, x_k, G_k, J_k = up(p["mu"][:, k]), torch.empty(n, dtype=torch.float64, device=dev), torch.empty(nnz, dtype=torch.float64, device=dev), up(Q.data)
        assert be.gaussian_approximation_dev(x_k.data_ptr(), d_mu=mu_k.data_ptr(), refactorize_final=True)["converged"]
        be.logpdf_grad_dev(x_k.data_ptr(), d_Qbar=G_k.data_ptr(), d_mu=x_k.data_ptr(), ybar=-1.0)
        be.ga_pullback_dev(x_k.data_ptr(), mu_k.data_ptr(), 0, G_k.data_ptr(), G_k.data_ptr(), 0, 0)
        want = be.pattern_dot_dev(G_k.data_ptr(), J_k.data_ptr(), nnz, 1)[0]
        assert same_bits(np.array([got[k]]), np.array([want])), (k, got[k], want)
    # member 0 against the restatement at the handle's x*, fed the handle's Qbar and lam
    rows, cols = gref.pattern_rc(Q)
    Gd = np.zeros((n, n))
    Gd[rows, cols] = Gv[:, 0]
    S = LD(thetas[0]) * gref._sym(Q, p["uplo"])
    o = gc.member_obs(p, 0)
    r = gref.restate(S, p["mu"][:, 0], p["Ad"], p["b"], o, X[:, 0], None, Gd, lam=lam[:, 0])
    bd = gref.bounds(S, p["Ad"], p["b"], o, X[:, 0], None, Gd, r, lam[:, 0], krow=ref.symmetric_coo(Q, p["uplo"])[3])
    upper = p["uplo"] == "U"
    wgt = np.where(rows == cols, 1.0, np.where((rows < cols) == upper, 2.0, 0.0))
    J = np.asarray(Q.data, LD)
    terms = wgt * gref.to_pattern(Q, r["Qbar_prior"]) * J
    want = terms.sum()
    bound = (wgt * np.abs(J) * gref.to_pattern(Q, bd["Qbar_prior"])).sum() + gref.FACTOR * (nnz // 4096 + 22) * gref.EPS * np.abs(terms).sum()
    print(f"{name} end to end: dL/dtheta_0 {got[0]:.12e} restatement {float(want):.12e} err/bound {float(abs(got[0] - want) / bound):.3f}")
    assert abs(got[0] - want) <= bound
    resid = r["Qpost"] @ np.asarray(lam[:, 0], LD) - r["xbar"]
    assert float(np.sqrt((resid * resid).sum() / (r["xbar"] * r["xbar"]).sum())) < gref.SOLVE_RESIDUAL
