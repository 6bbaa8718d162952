"""gmrfx_batch_fisher_eval in design form (gmrfx_batch_obs_set_design) on the device: member k's score, hess, energy and loglik are, bit for
bit, MI355XBackend.fisher_eval in design form on a plain handle holding Q_p,k and param[k] (whose own test,
tests/test_gpu_fisher_design.py, bounds it against the long-double restatement: the bound carries over through the equality; one case
is checked against dref.eval_ref directly).

Cases of tests/fisher_design_ref.py: mesh (n = 37, an empty row, a node observed twice, offset), rows (row lengths 0, 1, 3, 16, 17, 33),
cols (column and term-list lengths 0, 1, 15, 16, 17, 511, 512, 513), intercept (nobs = 1537 > n = 30, four chunks, the last of one
entry), one (one observation, n = 17); B = 1, 2, 3 on each and B = 50 on mesh; all six families with a distinct parameter per member.
Forms of the call: a shared against a per-member mean, want_score / want_hess off, host against _dev bit for bit, NaN-framed device
buffers at offsets of 0, 1 and 3 doubles with strides above n and above cnt. Masks: inactive members keep the caller's bytes and
their out pairs; nobody active; only the last member. A selection matrix gives the bits of the batched node form. A map installed for
the other form is refused with the call to make named."""
import numpy as np
import pytest
import torch

import batch_design_cases as dc
import batch_laplace_cases as bc
import fisher_design_ref as dref
import gmrfx
from layout_buffers import diag_positions, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = dref.eval_cases()
COMBOS = [(name, B) for name in CASES for B in (1, 2, 3)] + [("mesh", 50)]


def _batch(c, Qs, obs, params):
    bb = gmrfx.MI355XBatchLaplace(Qs[0], len(Qs), device=0, uplo=c["uplo"])
    bb.set_design_observations(obs.family, obs.y, c["A"], c["b"], obs.aux, params)
    bb.set_prior(bc.values(Qs))
    return bb


def _point(c, B, rng, family):
    n = c["Q"].shape[0]
    X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, B)))
    shared = family < 3
    mean = rng.standard_normal(n) if shared else np.asfortranarray(rng.standard_normal((n, B)))
    return X, mean, shared


@pytest.mark.parametrize("name,B", COMBOS, ids=[f"{s}-B{b}" for s, b in COMBOS])
def test_every_member_has_the_bits_of_its_plain_design_handle(name, B):
    c = CASES[name]
    n, nobs = c["Q"].shape[0], c["A"].shape[0]
    Qs = dc.eval_members(c["Q"], B)
    rng = np.random.default_rng(n + B)
    plain = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=False)
    bb = gmrfx.MI355XBatchLaplace(Qs[0], B, device=0, uplo=c["uplo"])
    try:
        for family in range(6):
            obs = dref.make_obs(family, nobs, seed=family)
            params = bc.family_params(family, B)
            bb.set_design_observations(obs.family, obs.y, c["A"], c["b"], obs.aux, params)
            if family == 0:
                bb.set_prior(bc.values(Qs))          # (the map belongs to A: the later families keep it)
            m = bb.observations_hess_map()
            cnt = len(m)
            X, mean, shared = _point(c, B, rng, family)
            S, H, en, ll = bb.fisher_eval(X, mean)
            assert S.shape == (n, B) and H.shape == (cnt, B)
            S2, H2, en2, ll2 = bb.fisher_eval(X, mean)
            assert same_bits(S, S2) and same_bits(H, H2) and same_bits(en, en2) and same_bits(ll, ll2)
            for k in range(B):
                plain.set_design_observations(obs.family, obs.y, c["A"], c["b"], obs.aux, float(params[k]))
                assert np.array_equal(plain.observations_hess_map(), m)
                plain.set_prior(Qs[k].data, m)
                ps, ph, pe, pl = plain.fisher_eval(X[:, k], mean if shared else mean[:, k])
                assert same_bits(ps, S[:, k]) and same_bits(ph, H[:, k]), (family, k)
                assert pe == en[k] and pl == ll[k], (family, k, pe, en[k], pl, ll[k])
            assert np.isfinite(S).all() and np.isfinite(H).all() and np.isfinite(en).all() and np.isfinite(ll).all()
            # either output off: the other and the pair keep their bits
            S3, H3, en3, ll3 = bb.fisher_eval(X, mean, want_hess=False)
            assert H3 is None and same_bits(S3, S) and same_bits(en3, en) and same_bits(ll3, ll)
            S3, H3, en3, ll3 = bb.fisher_eval(X, mean, want_score=False)
            assert S3 is None and same_bits(H3, H) and same_bits(en3, en) and same_bits(ll3, ll)
            S3, H3, en3, ll3 = bb.fisher_eval(X, mean, want_score=False, want_hess=False)
            assert S3 is None and H3 is None and same_bits(en3, en) and same_bits(ll3, ll)
            # device form: the base pointer off by 0, 1 and 3 doubles, a stride above n and above cnt, inside NaN-filled buffers
            off = (0, 1, 3)[family % 3]
            ss = max(n, cnt) + 2 + family
            bx = torch.full((B * ss + off,), float("nan"), dtype=torch.float64, device=DEV)
            bs, bh = (torch.full((B * ss + off,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
            for k in range(B):
                bx[off + k * ss:off + k * ss + n] = torch.from_numpy(X[:, k].copy()).to(DEV)
            dm = torch.from_numpy(np.ascontiguousarray(mean.T if not shared else mean).reshape(-1).copy()).to(DEV)
            torch.cuda.synchronize()
            en4, ll4 = bb.fisher_eval_dev(bx.data_ptr() + 8 * off, ss, dm.data_ptr(), 0 if shared else n, None, bs.data_ptr() + 8 * off,
                                          bh.data_ptr() + 8 * off, ss)
            torch.cuda.synchronize()
            hs, hh = bs.cpu().numpy(), bh.cpu().numpy()
            assert np.isnan(hs[:off]).all() and np.isnan(hh[:off]).all()
            for k in range(B):
                a = off + k * ss
                assert same_bits(hs[a:a + n], S[:, k]) and same_bits(hh[a:a + cnt], H[:, k]), (family, k)
                assert np.isnan(hs[a + n:a + ss]).all() and np.isnan(hh[a + cnt:a + ss]).all()
            assert same_bits(en4, en) and same_bits(ll4, ll)
    finally:
        bb.close()
        plain.close()


@pytest.mark.parametrize("name,B", [("mesh", 3), ("intercept", 2), ("cols", 50)])
def test_masked_members_keep_the_callers_bytes(name, B):
    c = CASES[name]
    n, nobs = c["Q"].shape[0], c["A"].shape[0]
    rng = np.random.default_rng(3)
    obs = dref.make_obs(4, nobs, seed=4)
    bb = _batch(c, dc.eval_members(c["Q"], B), obs, bc.family_params(4, B))
    try:
        cnt = len(bb.observations_hess_map())
        ld = max(n, cnt)
        X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, B)))
        S, H, en, ll = bb.fisher_eval(X)
        masks = [np.arange(B) % 2 == 0 if B > 2 else np.array([False, True]), np.zeros(B, bool), np.arange(B) == B - 1]
        for active in masks:
            # the caller's arrays hold a pattern of their own: the inactive members' columns come back as they went in
            given_s, given_h = (np.asfortranarray(rng.standard_normal((ld, B))) for _ in range(2))
            keep_s, keep_h = given_s.copy(order="F"), given_h.copy(order="F")
            S2, H2, en2, ll2 = bb.fisher_eval(X, active=active, score=given_s, hess=given_h)
            assert same_bits(S2[:, active], S[:, active]) and same_bits(H2[:, active], H[:, active])
            assert same_bits(en2[active], en[active]) and same_bits(ll2[active], ll[active])
            assert same_bits(given_s[:, ~active], keep_s[:, ~active]) and same_bits(given_h[:, ~active], keep_h[:, ~active])
            assert same_bits(given_s[n:, :], keep_s[n:, :]) and same_bits(given_h[cnt:, :], keep_h[cnt:, :])         # (the rows past n / cnt)
            assert np.isnan(en2[~active]).all() and np.isnan(ll2[~active]).all()
            # the device form: out pairs given by the caller stay put for inactive members
            out = np.asfortranarray(np.full((2, B), 7.25))
            dx = torch.from_numpy(np.ascontiguousarray(X.T).reshape(-1).copy()).to(DEV)
            ds = torch.full((B * ld,), -3.5, dtype=torch.float64, device=DEV)
            dh = torch.full((B * ld,), -4.5, dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            bb.fisher_eval_dev(dx.data_ptr(), n, 0, 0, active, ds.data_ptr(), dh.data_ptr(), ld, out=out)
            torch.cuda.synchronize()
            hs, hh = ds.cpu().numpy().reshape(B, ld).T, dh.cpu().numpy().reshape(B, ld).T
            assert (out[:, ~active] == 7.25).all() and same_bits(out[0, active], en[active]) and same_bits(out[1, active], ll[active])
            assert (hs[:, ~active] == -3.5).all() and (hh[:, ~active] == -4.5).all()
            assert same_bits(np.ascontiguousarray(hs[:n, active]), np.ascontiguousarray(S[:, active]))
            assert same_bits(np.ascontiguousarray(hh[:cnt, active]), np.ascontiguousarray(H[:, active]))
    finally:
        bb.close()


@pytest.mark.parametrize("B", [1, 3])
def test_a_selection_matrix_has_the_bits_of_the_batched_node_form(B):
    Q, idx, A = dc.selection_case()
    n = Q.shape[0]
    Qs = dc.eval_members(Q, B, seed=2)
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, B)))
    mean = np.asfortranarray(rng.standard_normal((n, B)))
    bd, bn = gmrfx.MI355XBatchLaplace(Q, B, device=0), gmrfx.MI355XBatchLaplace(Q, B, device=0)
    try:
        bn.set_prior(bc.values(Qs))
        for family in range(6):
            obs = dref.make_obs(family, len(idx), seed=10 + family)
            params = bc.family_params(family, B)
            bd.set_design_observations(obs.family, obs.y, A, None, obs.aux, params)
            bd.set_prior(bc.values(Qs))
            bn.set_observations(obs.family, obs.y, idx, obs.aux, params)
            Sd, Hd, ed, ld = bd.fisher_eval(X, mean)
            Sn, Hn, en, ln = bn.fisher_eval(X, mean)
            m = bd.observations_hess_map()
            diag = diag_positions(Q)
            assert np.array_equal(m, np.sort(diag[idx]))           # the observed nodes' diagonal positions
            order = np.argsort(diag[idx])                          # map order -> the node it belongs to
            assert same_bits(Sd, Sn) and same_bits(ed, en), family
            assert same_bits(np.ascontiguousarray(Hd), np.ascontiguousarray(Hn[idx[order], :])), family
            # (loglik adds the same terms by observation instead of by node: another order, so no bits are claimed; the plain-handle
            # equality above covers it)
    finally:
        bd.close()
        bn.close()


def test_one_case_against_the_long_double_restatement():
    c = CASES["cols"]
    n, nobs, B = c["Q"].shape[0], c["A"].shape[0], 3
    Qs = dc.eval_members(c["Q"], B, seed=4)
    obs = dref.make_obs(1, nobs, seed=1)
    rng = np.random.default_rng(9)
    X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, B)))
    mean = np.asfortranarray(rng.standard_normal((n, B)))
    bb = _batch(c, Qs, obs, np.zeros(B))
    try:
        S, H, en, ll = bb.fisher_eval(X, mean)
        for k in range(B):
            ck = dc.member_case(c, Qs[k])
            r = dref.eval_ref(ck, obs, X[:, k], mean[:, k])
            bs, bh, be, bl = dref.bounds(r, 16)[:4]
            errs = (np.abs(S[:, k] - r["score"]), np.abs(H[:, k] - r["hess"]), abs(en[k] - r["energy"]), abs(ll[k] - r["loglik"]))
            print(f"member {k}: score {float(errs[0].max()):.2e} (bound {float(bs.max()):.2e}) hess {float(errs[1].max()):.2e} "
                  f"({float(bh.max()):.2e}) energy {float(errs[2]):.2e} ({float(be):.2e}) loglik {float(errs[3]):.2e} ({float(bl):.2e})")
            assert (errs[0] <= bs).all() and (errs[1] <= bh).all() and errs[2] <= be and errs[3] <= bl
    finally:
        bb.close()


def test_a_stale_map_is_refused_and_names_the_call_to_make():
    c = CASES["mesh"]
    n, nobs, B = c["Q"].shape[0], c["A"].shape[0], 3
    Qs = dc.eval_members(c["Q"], B)
    obs = dref.make_obs(1, nobs, seed=1)
    X = np.zeros((n, B))
    bb = gmrfx.MI355XBatchLaplace(Qs[0], B, device=0, uplo=c["uplo"])
    try:
        bb.set_prior(bc.values(Qs))                                   # no likelihood yet: the node-form map
        bb.set_design_observations(obs.family, obs.y, c["A"], c["b"], obs.aux, np.zeros(B))
        with pytest.raises(ValueError, match="gmrfx_batch_set_prior"):
            bb.fisher_eval(X)
        with pytest.raises(ValueError, match="gmrfx_batch_set_prior"):
            bb.gaussian_approximation(x0=X)
        bb.set_prior(bc.values(Qs))
        S, H, en, ll = bb.fisher_eval(X)
        # and the other way round: the design map under a node-form likelihood
        bb.set_observations(1, np.ones(n))
        with pytest.raises(ValueError, match="gmrfx_batch_set_prior"):
            bb.fisher_eval(X)
        bb.set_prior(bc.values(Qs))
        bb.fisher_eval(X)
        # the existing sequences: node form and set_prior in either order, then back to the design form with the same bits
        bb.set_design_observations(obs.family, obs.y, c["A"], c["b"], obs.aux, np.zeros(B))
        bb.set_prior(bc.values(Qs))
        S2, H2, en2, ll2 = bb.fisher_eval(X)
        assert same_bits(S, S2) and same_bits(H, H2) and same_bits(en, en2) and same_bits(ll, ll2)
    finally:
        bb.close()
