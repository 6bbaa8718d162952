"""Composite likelihoods on the device (gmrfx_obs_set_composite; csrc/fisher_design.hip: k_design_eta_comp, csrc/predictive.hip:
k_pred_design_comp, k_pred_scores_comp) against tests/composite_ref.py.

1. One component has the bits of the same handle under gmrfx_obs_set_design: evaluation, loop, marginals and scores; host and _dev agree.
2. Pure positions: a node whose column of A touches rows of one component only, and a Hessian position whose term list lies in one
   component only, have the bits of the single-family design-form run of that component's family on the same stacked A.
3. Every entry and the two scalars lie within bounds(r, 16) of the long-double restatement (the derivation of
   tests/test_gpu_fisher_design.py: a row's g, d and l carry the error of their own family). The ratios are printed.
4. The loop on a Normal + Poisson + Bernoulli joint model, with and without a sum-to-zero constraint: counters and alpha trace of the
   float64 restatement, the mode within the distance tests/test_gpu_fisher_design_loop.py allows (64 cond(Q_k) eps max|x|).
5. set_param then an evaluation has the bits of a fresh handle set with those parameters.
6. gmrfx_ga_pullback is refused and the handle stays usable."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import composite_ref as cref
import fisher_design_ref as dref
import fisher_ref as ref
import gmrfx

pytestmark = pytest.mark.gpu

CASES = cref.eval_cases()
DEV = "cuda:0"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _composite(c, factorize=False):
    o = c["obs"]
    comp = gmrfx.CompositeObservations(c["Q"].shape[0])
    A = sp.csr_matrix(c["A"])
    for k in range(o.ncomp):
        r0, r1 = int(o.rowptr[k]), int(o.rowptr[k + 1])
        comp.add(o.families[k], o.y[r0:r1], A=A[r0:r1], offset=None if c["b"] is None else c["b"][r0:r1],
                 aux=None if o.aux is None else o.aux[r0:r1], param=o.params[k])
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=factorize)
    gmrfx.set_composite_observations(be, comp)
    be.set_prior(c["Q"].data, be.observations_hess_map())
    return be


def _single(c, family, param, y=None, aux=None, factorize=False):
    o = c["obs"]
    be = gmrfx.MI355XBackend(c["Q"], device=0, uplo=c["uplo"], factorize=factorize)
    be.set_design_observations(family, o.y if y is None else y, c["A"], c["b"], aux, param)
    be.set_prior(c["Q"].data, be.observations_hess_map())
    return be


def test_one_component_has_the_bits_of_the_design_form():
    c = CASES["one"]
    o = c["obs"]
    n = c["Q"].shape[0]
    a, b = _composite(c, True), _single(c, o.families[0], o.params[0], aux=o.aux, factorize=True)
    try:
        ra, rb = a.fisher_eval(c["x"], c["mu"]), b.fisher_eval(c["x"], c["mu"])
        assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1]) and ra[2:] == rb[2:]
        dx, dm = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["mu"]).to(DEV)
        ds, dh = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(len(ra[1]), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        e2 = a.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())
        torch.cuda.synchronize()
        assert tuple(e2) == tuple(ra[2:]) and same_bits(ds.cpu().numpy(), ra[0]) and same_bits(dh.cpu().numpy(), ra[1])
        xa, ha, ia = a.gaussian_approximation(mean=c["mu"], refactorize_final=True)
        xb, hb, ib = b.gaussian_approximation(mean=c["mu"], refactorize_final=True)
        assert same_bits(xa, xb) and same_bits(ha, hb)
        for k in ia:
            assert same_bits(ia[k], ib[k]) if isinstance(ia[k], np.ndarray) else ia[k] == ib[k], k
        # gmrfx_gaussian_approximation_dev and the plan's transposed term table (gmrfx_obs_design_rows) on the composite
        dxo, dho = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(len(ha), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        id_ = a.gaussian_approximation_dev(dxo.data_ptr(), dho.data_ptr(), d_mu=dm.data_ptr(), refactorize_final=True)
        torch.cuda.synchronize()
        assert same_bits(dxo.cpu().numpy(), xa) and same_bits(dho.cpu().numpy(), ha) and same_bits(id_["dec_trace"], ia["dec_trace"])
        assert id_["iterations"] == ia["iterations"] and np.array_equal(id_["alpha_trace"], ia["alpha_trace"])
        assert all(np.array_equal(u, v) for u, v in zip(a.observations_design_rows(), b.observations_design_rows()))
        ma, mb = a.predictor_marginals(xa), b.predictor_marginals(xb)
        assert all(same_bits(u, v) for u, v in zip(ma, mb))
        z, w = a.gauss_hermite(17)
        (sa, ta), (sb, tb) = a.predictive_scores(ma[0], ma[1], z, w), b.predictive_scores(mb[0], mb[1], z, w)
        assert all(same_bits(u, v) for u, v in zip(sa, sb)) and ta == tb
        # the _dev forms of the predictive calls
        dxa = torch.from_numpy(xa).to(DEV)
        outs = [torch.empty(len(o.y), dtype=torch.float64, device=DEV) for _ in range(7)]
        torch.cuda.synchronize()
        a.predictor_marginals_dev(dxa.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
        td = a.predictive_scores_dev(outs[0].data_ptr(), outs[1].data_ptr(), z, w, *(t.data_ptr() for t in outs[3:]))
        torch.cuda.synchronize()
        assert all(same_bits(outs[k].cpu().numpy(), ma[k]) for k in range(3)) and all(same_bits(outs[3 + k].cpu().numpy(), sa[k]) for k in range(4))
        assert td == ta
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", [k for k in sorted(CASES) if CASES[k]["pure"]])
def test_pure_positions_have_the_bits_of_their_components_single_family_run(name):
    c = CASES[name]
    o = c["obs"]
    node_comp, pos_comp = cref.purity(c)
    be = _composite(c)
    try:
        score, hess, _, _ = be.fisher_eval(c["x"], c["mu"])
        seen = set()
        for k in range(o.ncomp):
            f, p = o.families[k], o.params[k]
            # the whole stacked A under family f: rows outside component k get values family f accepts (they do not reach pure positions)
            y, aux = o.y.copy(), None
            rows = np.arange(int(o.rowptr[k]), int(o.rowptr[k + 1]))
            other = np.setdiff1d(np.arange(len(y)), rows)
            y[other] = 1.0
            if f in cref.READS_AUX:
                aux = np.ones(len(y))
                aux[rows] = o.aux[rows]
            one = _single(c, f, p, y=y, aux=aux)
            try:
                s1, h1, _, _ = one.fisher_eval(c["x"], c["mu"])
            finally:
                one.close()
            assert (node_comp == k).any() and (pos_comp == k).any()
            assert same_bits(score[node_comp == k], s1[node_comp == k]) and same_bits(hess[pos_comp == k], h1[pos_comp == k])
            seen.add(k)
        assert len(seen) == o.ncomp
    finally:
        be.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_entry_is_within_the_bounds_of_the_restatement(name):
    c = CASES[name]
    tm = dref.hess_map(c["Q"], c["uplo"], c["A"])
    r = cref.eval_ref(c, c["x"], c["mu"], tm)
    be = _composite(c)
    try:
        score, hess, en, ll = be.fisher_eval(c["x"], c["mu"])
        bs, bh, b_en, b_ll = dref.bounds(r, 16)[:4]
        tiny = ref.LD(1e-300)
        es, eh = np.abs(score - r["score"]), np.abs(hess - r["hess"])
        print(f"{name}: score err/bound {float(np.max(es / (bs + tiny))):.3f} hess {float(np.max(eh / (bh + tiny))):.3f} "
              f"energy {float(abs(en - r['energy']) / b_en):.3f} loglik {float(abs(ll - r['loglik']) / b_ll):.3f}")
        assert (es <= bs).all() and (eh <= bh).all() and abs(en - r["energy"]) <= b_en and abs(ll - r["loglik"]) <= b_ll
        score2, hess2, en2, ll2 = be.fisher_eval(c["x"], c["mu"])
        assert same_bits(score, score2) and same_bits(hess, hess2) and (en, ll) == (en2, ll2)
    finally:
        be.close()


@pytest.mark.parametrize("name", sorted(cref.loop_cases()))
def test_whole_loop_on_a_joint_model(name):
    c = cref.loop_cases()[name]
    a, b = cref.newton_loop(c, np.float64), cref.newton_loop(c, ref.LD)
    assert dref.far_from_thresholds(a["margins"])
    be = _composite(c)
    try:
        if c["C"] is not None:
            be.set_constraints(sp.csr_matrix(c["C"]), np.zeros(c["C"].shape[0]))
        x, hess, info = be.gaussian_approximation(x0=c["x0"])
        assert info["iterations"] == a["iterations"] and info["converged"] == a["converged"] and info["frozen_finish"] == a["frozen"]
        assert np.array_equal(info["alpha_trace"], a["alpha_trace"]), (info["alpha_trace"], a["alpha_trace"])
        assert (info["factorizations"], info["solves"], info["merit_evaluations"]) == (a["factorizations"], a["solves"], a["merit_evaluations"])
        cond = float(np.linalg.cond(np.asarray(b["Qk"], np.float64)))
        tol_x = 64 * cond * ref.EPS * float(np.abs(b["x"]).max())
        err_x = float(np.abs(x - b["x"]).max())
        print(f"{name}: cond(Q_k) {cond:.2e} device vs long double {err_x:.2e}, bound {tol_x:.2e}")
        assert err_x <= tol_x
        # the _dev form on the joint model: the bits of the host form
        m = c["Q"].shape[0]
        dxo, dho = torch.empty(m, dtype=torch.float64, device=DEV), torch.empty(len(hess), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        i2 = be.gaussian_approximation_dev(dxo.data_ptr(), dho.data_ptr())
        torch.cuda.synchronize()
        assert same_bits(dxo.cpu().numpy(), x) and same_bits(dho.cpu().numpy(), hess) and same_bits(i2["dec_trace"], info["dec_trace"])
        if c["C"] is not None:
            assert np.abs(c["C"] @ x).max() <= 64 * info["solves"] * ref.EPS * np.abs(c["C"]).sum() * max(np.abs(x).max(), 1.0)
    finally:
        be.close()


def test_set_param_then_an_evaluation_has_the_bits_of_a_fresh_handle():
    c = CASES["six"]
    p = [1.3, 0.0, 0.0, 0.0, 4.0, 0.5]
    fresh_case = dict(c, obs=cref.CompObs(c["obs"].families, p, c["obs"].rowptr, c["obs"].y, c["obs"].aux))
    a, b = _composite(c, True), _composite(fresh_case, True)
    try:
        before = a.fisher_eval(c["x"], c["mu"])
        a.predictor_marginals(c["x"])                    # (the cached pointwise constants exist before the parameters change)
        m0 = a.observations_hess_map()
        gmrfx.set_composite_param(a, p)
        assert np.array_equal(a.observations_hess_map(), m0) and gmrfx.composite_info(a)["param"].tolist() == p
        ra, rb = a.fisher_eval(c["x"], c["mu"]), b.fisher_eval(c["x"], c["mu"])
        assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1]) and ra[2:] == rb[2:]
        assert not same_bits(ra[0], before[0]) and ra[3] != before[3]
        ma, mb = a.predictor_marginals(c["x"]), b.predictor_marginals(c["x"])
        assert all(same_bits(u, v) for u, v in zip(ma, mb))
        z, w = a.gauss_hermite(16)
        (sa, ta), (sb, tb) = a.predictive_scores(ma[0], ma[1], z, w), b.predictive_scores(mb[0], mb[1], z, w)
        assert all(same_bits(u, v) for u, v in zip(sa, sb)) and ta == tb
        # pll = l_i(mu_eta_i) + c_i under the row's own component, against the restatement
        want = cref.pointwise(fresh_case["obs"], np.asarray(ma[0], ref.LD))[2] + cref.pointwise_const(fresh_case["obs"])
        scale = np.abs(want) + np.abs(np.asarray(c["obs"].y)) * (1 + np.abs(ma[0])) + 64
        assert np.all(np.abs(ma[2] - want) <= 64 * ref.EPS * scale), float(np.max(np.abs(ma[2] - want) / scale))
    finally:
        a.close()
        b.close()


def test_the_pullback_is_refused_and_the_handle_stays_usable():
    c = CASES["six"]
    be = _composite(c, True)
    try:
        before = be.fisher_eval(c["x"], c["mu"])
        with pytest.raises(ValueError, match="ga_pullback: composite likelihoods are not supported"):
            be.ga_pullback(c["x"], mean=c["mu"], mubar=np.ones(c["Q"].shape[0]))
        after = be.fisher_eval(c["x"], c["mu"])
        assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2:] == after[2:]
    finally:
        be.close()
