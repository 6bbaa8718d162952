"""gmrfx_batch_constrained_gaussian_approximation on the device against the restatement of the reference's projected loop
(tests/fisher_ref.py / tests/fisher_design_ref.py: newton_loop(..., A=...)), member by member, on the cases of
tests/batch_con_laplace_cases.py.

Per member: counts, flags and the alpha trace EXACTLY those of the float64 restatement of that member alone; mode and H within 64 x
max(the float64 restatement's own error against long double, eps x scale), the rule of tests/test_gpu_batch_laplace.py;
residual[k] <= 64 eps (iters_k + 1) max_r (|A| |x_k|)_r. Independence: a member has the same bits in a batch of copies of itself, beside
a member whose factorisation fails, and beside members that stopped earlier (the mask check: the forest-wide projection of a later
iterate must not touch a stopped member's step, iterate or operands). The host and _dev forms agree bit for bit; strided, NaN-framed
buffers keep their frame.

A W failure of ONE member alone can only arise from rounding: A is shared and W_k = A Q_k^-1 A' is positive definite whenever Q_k is.
It is therefore exercised through the case where every member fails (two equal rows of A: cinfo = 2 for all, x_k = x0_k) and through
the mask logic (a member stopping alone for another reason, the others going on), not forced. No test provokes a device fault:
non-positive pivots are reported status words."""
import numpy as np
import pytest
import torch

import batch_con_laplace_cases as cc
import batch_laplace_cases as bc
import fisher_ref as ref
import gmrfx
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
CASES = cc.cases()
LOOP = ["rw1_B1", "rw1_B2", "rw1_B3", "besag", "m13_m4", "m13_m5", "m16_m5", "m16_m64", "design"]
DEV = "cuda:0"


def _batch(c, Qs=None, params=None, constrain=True):
    Qs = c["Qs"] if Qs is None else Qs
    o, d = c["obs"], c["design"]
    p = c["params"] if params is None else params
    bb = gmrfx.MI355XBatchLaplace(Qs[0], len(Qs), device=0, uplo=d["uplo"] if d else "U")
    if d:
        bb.set_design_observations(o.family, o.y, d["A"], d["b"], o.aux, p)
    else:
        bb.set_observations(o.family, o.y, o.idx, o.aux, p)
    if constrain:
        bb.set_constraints(c["A"], np.zeros(c["A"].shape[0]))
    bb.set_prior(bc.values(Qs))          # (with the constraint held: gmrfx_batch_set_prior accepts it)
    return bb


def _run(c, **kw):
    bb = _batch(c)
    try:
        return bb.gaussian_approximation(x0=c["x0"], **{**c["kw"], **kw})
    finally:
        bb.close()


@pytest.fixture(scope="module")
def runs():
    """name -> (X, H, info) of the case's loop, computed once and left unchanged"""
    return {name: _run(CASES[name]) for name in LOOP + ["besag50", "one_fails"]}


@pytest.fixture(scope="module")
def restated():
    memo = {}

    def get(name, k, dtype):
        if (name, k, dtype) not in memo:
            memo[(name, k, dtype)] = cc.restate(CASES[name], k, dtype)
        return memo[(name, k, dtype)]
    return get


def _hess_ref(c, r, hmap):
    """the restatement's H in the order the device returns it"""
    if not c["design"]:
        return np.asarray(r["hess"], ref.LD)
    Q = c["Qs"][0]
    col = np.searchsorted(Q.indptr, hmap, side="right") - 1
    return np.asarray(r["hess_dense"], ref.LD)[Q.indices[hmap], col]


@pytest.mark.parametrize("name", LOOP)
def test_every_member_follows_its_own_projected_loop(runs, restated, name):
    c = CASES[name]
    X, H, info = runs[name]
    assert info["posdef"] and (info["info"] == 0).all() and (info["cinfo"] == 0).all()
    hmap = None
    if c["design"]:
        bb = _batch(c)
        hmap = bb.observations_hess_map()
        bb.close()
    for k in range(len(c["Qs"])):
        a, b = restated(name, k, np.float64), restated(name, k, ref.LD)
        assert info["iterations"][k] == a["iterations"] and info["converged"][k] == a["converged"] and info["frozen_finish"][k] == a["frozen"]
        assert np.array_equal(info["alpha_trace"][k], a["alpha_trace"]), (k, info["alpha_trace"][k], a["alpha_trace"])
        assert (info["factorizations"][k], info["solves"][k], info["merit_evaluations"][k]) == (
            a["factorizations"], a["solves"], a["merit_evaluations"]), k
        hb = _hess_ref(c, b, hmap)
        own_x = float(np.abs(np.asarray(a["x"], ref.LD) - b["x"]).max())
        own_h = float(np.abs(_hess_ref(c, a, hmap) - hb).max())
        tol_x = 64 * max(own_x, ref.EPS * float(np.abs(b["x"]).max()))
        tol_h = 64 * max(own_h, ref.EPS * float(np.abs(hb).max()))
        err_x, err_h = float(np.abs(X[:, k] - b["x"]).max()), float(np.abs(H[:, k] - hb).max())
        bound = cc.residual_bound(c, X[:, k], int(info["iterations"][k]))
        print(f"{name}[{k}]: restatement f64-vs-ld x {own_x:.2e} H {own_h:.2e}; device-vs-ld x {err_x:.2e} H {err_h:.2e}; "
              f"residual {info['residual'][k]:.2e} bound {bound:.2e}")
        assert err_x <= tol_x and err_h <= tol_h, k
        assert info["residual"][k] <= bound, k
    assert info["totals"]["factorizations"] == info["factorizations"].max()


def test_fifty_members_in_one_call(runs, restated):
    c = CASES["besag50"]
    X, H, info = runs["besag50"]
    assert info["posdef"] and info["converged"].all() and (info["cinfo"] == 0).all()
    assert len(set(info["iterations"].tolist())) >= 2
    for k in (0, 17, 33, 49):
        a = restated("besag50", k, np.float64)
        assert info["iterations"][k] == a["iterations"] and np.array_equal(info["alpha_trace"][k], a["alpha_trace"]), k
    for k in range(50):
        assert info["residual"][k] <= cc.residual_bound(c, X[:, k], int(info["iterations"][k])), k


@pytest.mark.parametrize("name", ["besag", "m16_m5", "one_fails"])
def test_a_member_does_not_depend_on_the_others(runs, name):
    """besag: members stop at iterates 7, 8, 9, 7, 5, so every member but the last to stop has sat beside running ones, masked out of
    their projections -- and in the batch of copies everybody stops together: the same bits either way is the mask check. one_fails: the
    same beside a member whose factorisation failed (cinfo = -1, its operands NaN)."""
    c = CASES[name]
    X, H, info = runs[name]
    B = len(c["Qs"])
    for k in range(B):
        if info["info"][k] != 0:
            continue
        bb = _batch(c, [c["Qs"][k]] * B, np.full(B, c["params"][k]))
        try:
            Xc, Hc, ic = bb.gaussian_approximation(x0=np.repeat(c["x0"][:, k:k + 1], B, axis=1), **c["kw"])
        finally:
            bb.close()
        for j in range(B):
            assert same_bits(Xc[:, j], X[:, k]) and same_bits(Hc[:, j], H[:, k]) and same_bits(ic["dec_trace"][j], info["dec_trace"][k]), (k, j)
            assert ic["residual"][j] == info["residual"][k]


def test_one_failing_factorisation_stops_alone(runs, restated):
    c = CASES["one_fails"]
    X, H, info = runs["one_fails"]
    assert not info["posdef"]
    assert info["info"][1] > 0 and info["cinfo"].tolist() == [0, -1, 0] and info["info"][0] == 0 and info["info"][2] == 0
    assert np.array_equal(X[:, 1], c["x0"][:, 1]) and info["iterations"][1] == 0 and np.isnan(H[:, 1]).all() and np.isnan(info["residual"][1])
    for k in (0, 2):
        a = restated("one_fails", k, np.float64)
        assert info["converged"][k] and info["iterations"][k] == a["iterations"] and np.array_equal(info["alpha_trace"][k], a["alpha_trace"])
        assert info["residual"][k] <= cc.residual_bound(c, X[:, k], int(info["iterations"][k]))


def test_equal_rows_fail_every_member_and_leave_the_handle_usable():
    c = CASES["equal_rows"]
    bb = _batch(c)
    try:
        X, H, info = bb.gaussian_approximation(x0=c["x0"])
        assert not info["posdef"] and info["cinfo"].tolist() == [2, 2, 2] and (info["info"] == 0).all()
        assert np.array_equal(X, c["x0"]) and (info["iterations"] == 0).all() and not info["converged"].any() and np.isnan(info["residual"]).all()
        bb.clear_constraints()
        X2, _, i2 = bb.gaussian_approximation(x0=c["x0"])
        assert i2["posdef"] and i2["converged"].all() and "cinfo" not in i2
        bb.set_constraints(c["A"][:1], np.zeros(1))
        X3, _, i3 = bb.gaussian_approximation(x0=c["x0"])
        assert i3["posdef"] and i3["converged"].all() and (i3["cinfo"] == 0).all()
        ref3 = _run(CASES["rw1_B3"])
        assert same_bits(X3, ref3[0])
    finally:
        bb.close()


@pytest.mark.parametrize("name", ["besag", "m13_m5", "design"])
def test_host_and_dev_forms_agree_and_strided_buffers_keep_their_frame(runs, name):
    c = CASES[name]
    X, H, info = runs[name]
    n, B = X.shape
    hl = H.shape[0]
    sx, sh, s0 = n + 3, hl + 5, n + 1
    dx, dh = (torch.full((B * s + 2,), float("nan"), dtype=torch.float64, device=DEV) for s in (sx, sh))
    d0 = torch.full((B * s0 + 1,), float("nan"), dtype=torch.float64, device=DEV)
    for k in range(B):
        d0[1 + k * s0:1 + k * s0 + n] = torch.from_numpy(c["x0"][:, k].copy()).to(DEV)
    torch.cuda.synchronize()
    bb = _batch(c)
    try:
        idev = bb.gaussian_approximation_dev(dx.data_ptr() + 8, sx, d_hess=dh.data_ptr() + 8, sh=sh, d_x0=d0.data_ptr() + 8, sx0=s0, **c["kw"])
    finally:
        bb.close()
    torch.cuda.synchronize()
    gx, gh = dx.cpu().numpy(), dh.cpu().numpy()
    inx, inh = np.zeros(gx.size, bool), np.zeros(gh.size, bool)
    for k in range(B):
        assert same_bits(gx[1 + k * sx:1 + k * sx + n], X[:, k]) and same_bits(gh[1 + k * sh:1 + k * sh + hl], H[:, k]), k
        inx[1 + k * sx:1 + k * sx + n] = True
        inh[1 + k * sh:1 + k * sh + hl] = True
    assert np.isnan(gx[~inx]).all() and np.isnan(gh[~inh]).all()
    for key in ("iterations", "alpha", "decrement", "energy", "loglik", "residual", "cinfo"):
        assert same_bits(np.asarray(idev[key], float), np.asarray(info[key], float)), key


@pytest.mark.parametrize("name", ["besag", "m16_m64"])
def test_refactorize_final_leaves_fresh_constrained_readouts(name):
    c = CASES[name]
    B, n = len(c["Qs"]), c["M"].shape[0]
    NZ = bc.values(c["Qs"])
    dpos = diag_positions(c["Qs"][0])
    z = np.asfortranarray(np.random.default_rng(2).standard_normal((n, B)))
    bb, fresh = _batch(c), gmrfx.MI355XBatchBackend(c["Qs"][0], B, device=0)
    try:
        X, H, info = bb.gaussian_approximation(x0=c["x0"], refactorize_final=True, **c["kw"])
        assert info["posdef"]
        NZpost = NZ.copy(order="F")
        NZpost[dpos, :] -= H
        fresh.set_constraints(c["A"], np.zeros(c["A"].shape[0]))
        assert (fresh.refactorize_values(NZpost) == 0).all()
        assert same_bits(bb.logdet(), fresh.logdet()) and same_bits(bb.selinv_diag(), fresh.selinv_diag())
        assert same_bits(bb.constrained_var(), fresh.constrained_var())
        assert same_bits(bb.constraint_info()["logdet_W"], fresh.constraint_info()["logdet_W"])
        assert same_bits(bb.sample(z), fresh.sample(z))
        t = bb.laplace_terms()
        assert same_bits(t["logdet_W"], fresh.constraint_info()["logdet_W"]) and same_bits(t["logdet"], fresh.logdet())
        assert same_bits(t["energy"], info["energy"]) and same_bits(t["loglik"], info["loglik"])
    finally:
        bb.close()
        fresh.close()


def _chol_ld(P):
    """lower Cholesky factor in long double, column by column"""
    L = np.tril(np.asarray(P, ref.LD))
    for j in range(L.shape[0]):
        L[j, j] = np.sqrt(L[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _terms_ld(c, k, x):
    """name -> (value, scale) in long double at the point x: energy and loglik (fisher_ref.eval_ref, the sums of absolute terms as
    scales), log det(Q_p,k - H(x)) (scale: the sum of the absolute log pivots) and log det W_k(x)"""
    o = cc.member_obs(c, k)
    r = ref.eval_ref(c["Qs"][k], "U", np.asarray(x, ref.LD), None, o)
    P = np.asarray(cc.dense(c, k), ref.LD) - np.diag(np.asarray(r["hess"], ref.LD))
    lp = 2 * np.log(np.diag(_chol_ld(P)))
    A = np.asarray(c["A"].toarray(), ref.LD)
    lw = 2 * np.log(np.diag(_chol_ld(A @ ref._solve(P, np.ascontiguousarray(A.T)))))
    return {"energy": (r["energy"], r["en_abs"]), "loglik": (r["loglik"], r["ll_abs"]), "logdet": (lp.sum(), np.abs(lp).sum()),
            "logdet_W": (lw.sum(), max(np.abs(lw).sum(), ref.LD(1)))}


def test_laplace_terms_against_the_plain_constrained_loop(runs, restated):
    """laplace_terms() of the batched constrained call and the same numbers of the plain constrained loop (ONE plain handle under
    gmrfx_constraints_set, member by member: its mode, fisher_eval at its mode, its log det and log det W). The two routes prepare W_k
    by different arithmetic (a forest solve and k_batch_con_chol against one solve and the host's Cholesky), so they are not compared
    bit for bit: each route is held to the long-double restatement under the rule of this file, 64 x max(the float64 restatement's
    own error, eps x scale) -- for a term, the own error is its long-double value at the float64 restatement's mode against that at
    the long-double one, and the scale the sum of the absolute terms it is made of. Counts and alpha trace agree exactly."""
    c = CASES["besag"]
    B = len(c["Qs"])
    bb = _batch(c)
    o = c["obs"]
    try:
        X, H, info = bb.gaussian_approximation(x0=c["x0"], refactorize_final=True)
        t = bb.laplace_terms()
    finally:
        bb.close()
    dpos = diag_positions(c["Qs"][0])
    plain = gmrfx.MI355XBackend(c["Qs"][0], device=0, factorize=False)
    try:
        plain.set_constraints(c["A"], np.zeros(1))
        for k in range(B):
            plain.set_prior(c["Qs"][k].data, dpos)
            plain.set_observations(o.family, o.y, o.idx, o.aux, float(c["params"][k]))
            xp, hp, ip = plain.gaussian_approximation(x0=c["x0"][:, k], refactorize_final=True)
            assert ip["iterations"] == info["iterations"][k] and np.array_equal(ip["alpha_trace"], info["alpha_trace"][k]), k
            _, _, en, ll = plain.fisher_eval(xp, want_score=False, want_hess=False)
            got = {"batched": dict(x=X[:, k], energy=t["energy"][k], loglik=t["loglik"][k], logdet=t["logdet"][k], logdet_W=t["logdet_W"][k]),
                   "plain": dict(x=xp, energy=en, loglik=ll, logdet=plain.compute_logdet(), logdet_W=plain.constraint_info()["logdet_W"])}
            ra, rb = restated("besag", k, np.float64), restated("besag", k, ref.LD)
            own_x = float(np.abs(np.asarray(ra["x"], ref.LD) - rb["x"]).max())
            tol_x = 64 * max(own_x, ref.EPS * float(np.abs(rb["x"]).max()))
            ta, tb = _terms_ld(c, k, ra["x"]), _terms_ld(c, k, rb["x"])
            for route, g in got.items():
                err_x = float(np.abs(np.asarray(g["x"], ref.LD) - rb["x"]).max())
                line = [f"x {err_x:.2e} (tol {tol_x:.2e})"]
                bad = [] if err_x <= tol_x else ["x"]
                for nm in ("energy", "loglik", "logdet", "logdet_W"):
                    tol = 64 * max(float(abs(ta[nm][0] - tb[nm][0])), ref.EPS * float(tb[nm][1]))
                    err = float(abs(ref.LD(g[nm]) - tb[nm][0]))
                    line.append(f"{nm} {err:.2e} (tol {tol:.2e})")
                    if not err <= tol:
                        bad.append(nm)
                print(f"besag[{k}] {route}: " + " ".join(line))
                assert not bad, (k, route, bad)
    finally:
        plain.close()


@pytest.mark.parametrize("name", ["besag", "design"])
def test_set_param_has_the_bits_of_a_full_set_observations(name):
    c = CASES[name]
    B, n = len(c["Qs"]), c["Qs"][0].shape[0]
    o = c["obs"]
    fam, y = 4, o.y                      # negative binomial: r enters the kernels (param and its log) and loglik_const
    p0, p1 = np.linspace(0.6, 3.1, B), np.linspace(5.0, 0.7, B)
    X = np.asfortranarray(np.random.default_rng(5).uniform(-0.5, 0.5, (n, B)))
    c4 = dict(c, obs=ref.Obs(fam, o.idx, y, o.aux, 1.0))
    a, b = _batch(c4, params=p0), _batch(c4, params=p1, constrain=False)
    try:
        a.set_param(p1)                   # with the constraint held
        assert same_bits(a.observations_info()["loglik_const"], b.observations_info()["loglik_const"])
        a.clear_constraints()
        for u, v in zip(a.fisher_eval(X), b.fisher_eval(X)):
            assert same_bits(u, v)
    finally:
        a.close()
        b.close()
