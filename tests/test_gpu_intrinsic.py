"""Near-singular precisions against exact answers (run with -m gpu on an MI355X).

The intrinsic models of the reference package (RW1, RW2, Besag, separable RW1 x Besag: a singular structure matrix plus
eps I, eps = 1e-5 .. 1e-10) have cond(Q) from 1e5 to 1e11. There a correct float64 implementation is far from the truth
(the oracle's Sigma_ii is off by ~4e-6 at eps = 1e-10), so a fixed tolerance against the oracle cannot tell a correct kernel
from a wrong one. The criteria here are relative to what float64 can do:

- forward errors against the truth (closed forms of tests/intrinsic_models.py, or extended-precision refinement) of log det,
  Sigma_ii, Sigma between lattice neighbours, solves and the energy identity of backward solves (x' Q x = z' z for
  x = P' L^-T z): err_gpu <= 10 err_oracle + 1e-14, err_oracle the largest of the oracle in the handle's order and in two
  other nested-dissection orders (near the null space each is one rounding amplified by 1 / eps: see _oracles);
- normwise backward errors of solves and of the backward solve's substitution, and the factor residual
  ||P Q P' - L L'||_F / ||Q||_F: <= 1e-14 and <= 10 x the oracle's + the unit roundoff;
- tr(Sigma Q) = n through selinv_dot, within 10 x the oracle's error + 1e-12 n.

Every case prints its GPU / oracle errors (pytest -rP shows them)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import orc
import intrinsic_models as im
from gmrfx import spde

pytestmark = pytest.mark.gpu

EPS = (1e-5, 1e-8, 1e-10)


def _closed_cases():
    for eps in EPS:
        yield im.rw1_cycle(100, eps), (1,)
        yield im.rw2_cycle(2000, eps), (1,)
        yield im.besag_torus((64, 64), eps), (1, 0)
        yield im.besag_torus((256, 256), eps), (0, 1)
        yield im.besag_torus((20, 20, 20), eps), (0, 0, 1)
        yield im.separable_rw1_besag(6, 24, eps), (1, 0, 0)
    yield im.separable_rw1_besag(6, 24, 1e-5, rejoin=False), (0, 1, 0)


CLOSED = list(_closed_cases())

# Findings these tests made that this change does not fix, criterion by criterion (measured on an MI355X; GPU / oracle).
# Every other criterion of these cases is enforced; test_known_deviations holds each of these as a strict xfail, so that a fix
# (or a change of the numbers) shows up as a failure that asks for this table to be updated.
_SMALL_FRONT_INVERSES = ("the sweeps multiply by explicit inverses of the <= 16-column diagonal blocks of small fronts (sweep "
                         "chunks): backward error 6.2e-15 vs 2.3e-16 (solve) and 3.9e-15 vs 7.4e-17 (backward solve's "
                         "substitution), both under 1e-14")
_SELINV_INVERSES = ("the selected inversion multiplies by the full explicit inverse L11^-1 of every big front, whatever the "
                    "inverse cap: tr(Sigma Q) - n is 10x (Besag 64^2, eps = 1e-10, host contraction) to 60x (Matern range 20) "
                    "the oracle's")
KNOWN = {"rw2_cycle2000-eps1e-10": {"solve_bwd": _SMALL_FRONT_INVERSES, "bsolve_subst": _SMALL_FRONT_INVERSES},
         "besag64x64-eps1e-10": {"trace_host": _SELINV_INVERSES},
         "matern_range20_alpha2": {"trace_host": _SELINV_INVERSES, "trace_device": _SELINV_INVERSES}}
_FAILED = {}        # case id -> the criteria that failed in this session


def _open_cases():
    for eps in EPS:
        yield f"rw2_chain3000_eps{eps:g}", im.rw2_chain(3000, eps), {}
    m = spde.grid_mesh_2d(60, 60, jitter=0.2, seed=4)
    yield "matern_range20_alpha2", sp.csc_matrix(spde.matern_precision(m, 1, 20.0)), {"coords": m.points}


OPEN = list(_open_cases())


U = 2.0 ** -53


def _ok(e_gpu, e_orc, floor=1e-14):
    return e_gpu <= 10.0 * e_orc + floor


def _oracles(Q, perm):
    """The oracle in the handle's order, then in two other nested-dissection orders of Q. Near the null space an error is
    one rounding amplified by 1 / eps (the last pivots), so one order gives one random draw of it; the largest of three sets
    the bar, and one lucky rounding of the oracle does not."""
    Fs = [orc.OracleFactor(Q, perm)]
    for leaf in (16, 24):
        p = gmrfx.MI355XBackend(Q, symbolic_only=True, nd_leaf=leaf).ordering_permutation()
        Fs.append(orc.OracleFactor(Q, p))
    return Fs


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check_solves(tag, Q, be, Fs, perm, rng, report):
    n = Q.shape[0]
    F = Fs[0]
    B = rng.standard_normal((n, 2))
    T = im.refined_solve(Q, F, B)
    Xg = be.backend_solve(B)
    fg, fo = im.rel_fwd(Xg, T), max(im.rel_fwd(G.solve(B), T) for G in Fs)
    bg, bo = im.backward_error(Q, Xg, B), max(im.backward_error(Q, G.solve(B), B) for G in Fs)
    report.update(solve_fwd=(fg, fo), solve_bwd=(bg, bo))
    _expect(report, "solve_fwd", _ok(fg, fo), f"{tag}: solve forward error {fg:.3e} vs oracle {fo:.3e}")
    _expect(report, "solve_bwd", bg <= 1e-14 and bg <= 10 * bo + U, f"{tag}: solve backward error {bg:.3e} vs oracle {bo:.3e}")
    # backward solve x = P' L^-T z: the energy identity x' Q x = z' z (independent of which L) and the substitution's own
    # backward error L' (P x) = z with the handle's factor
    z = rng.standard_normal(n)
    Ql = sp.csr_matrix(Q).astype(np.longdouble)
    zz = np.dot(z.astype(np.longdouble), z)

    def energy(x):
        xl = x.astype(np.longdouble)
        return float(abs(np.dot(xl, Ql @ xl) - zz) / zz)

    def substitution(x, L):
        xl = x.astype(np.longdouble)
        L = sp.tril(L)
        r = np.abs(sp.csr_matrix(L.T).astype(np.longdouble) @ xl[perm] - z).max()
        return float(r / (float(abs(L).sum(axis=0).max()) * np.abs(xl).max() + np.abs(z).max()))

    xg = be.backend_backward_solve(z)
    out = {"gpu": (energy(xg), substitution(xg, be.factor_csc())),
           "orc": (max(energy(G.backward_solve(z)) for G in Fs), substitution(F.backward_solve(z), F.L()))}
    report.update(bsolve_energy=(out["gpu"][0], out["orc"][0]), bsolve_subst=(out["gpu"][1], out["orc"][1]))
    _expect(report, "bsolve_energy", _ok(out["gpu"][0], out["orc"][0]), f"{tag}: backward solve energy {out['gpu'][0]:.3e} vs {out['orc'][0]:.3e}")
    _expect(report, "bsolve_subst", out["gpu"][1] <= 1e-14 and out["gpu"][1] <= 10 * out["orc"][1] + U,
            f"{tag}: substitution {out['gpu'][1]:.3e} vs {out['orc'][1]:.3e}")


def _check_factor(tag, Q, be, Fs, perm, report):
    if Q.shape[0] > 70000:
        return
    rg, ro = im.factor_residual(Q, perm, be.factor_csc()), im.factor_residual(Q, perm, Fs[0].L())
    report.update(factor_res=(rg, ro))
    _expect(report, "factor_res", rg <= 1e-14 and rg <= 10 * ro + U, f"{tag}: factor residual {rg:.3e} vs oracle {ro:.3e}")


def _check_trace(tag, Q, be, Fs, report):
    n = Q.shape[0]
    eo = max(abs(orc.selinv_dot(F, Q) - n) for F in Fs)
    for who, v in (("host", be.selinv_dot(Q)), ("device", be.selinv_dot_device(Q))):
        report[f"trace_{who}"] = (abs(v - n) / n, eo / n)
        _expect(report, f"trace_{who}", abs(v - n) <= 10 * eo + 1e-12 * n, f"{tag}: tr(Sigma Q) ({who}) = {v!r}, oracle off by {eo:.3e}")


def _expect(report, key, ok, msg):
    """criteria are collected, not raised one by one, so that every case reports all of its errors"""
    if not ok:
        report.setdefault("_failed", {})[key] = msg


def _finish(case_id, tag, report):
    """print the GPU / oracle errors and their ratios; remember which criteria failed (test_known_deviations reads it) and fail
    with every one that is not a known deviation of this case"""
    failed = report.pop("_failed", {})
    _FAILED[case_id] = set(failed)
    print(tag + " " + " ".join(f"{k}={g:.2e}/{o:.2e}({g / max(o, 1e-300):.2f})" for k, (g, o) in report.items()))
    unexpected = [m for k, m in failed.items() if k not in KNOWN.get(case_id, {})]
    assert not unexpected, "; ".join(unexpected)


def _closed_form_checks(model, offset, be, Fs, report):
    tag = f"{model.name} eps={model.eps:g}"
    n = model.n
    ld = model.logdet()
    eg, eo = _rel(be.compute_logdet(), ld), max(_rel(F.logdet(), ld) for F in Fs)
    report.update(logdet=(eg, eo))
    _expect(report, "logdet", _ok(eg, eo), f"{tag}: logdet error {eg:.3e} vs oracle {eo:.3e}")
    s = model.sigma_diag()
    eg, eo = np.abs(be.get_selinv_diag() - s).max() / s, max(np.abs(F.selinv_diag() - s).max() / s for F in Fs)
    report.update(sigma_ii=(eg, eo))
    _expect(report, "sigma_ii", _ok(eg, eo), f"{tag}: Sigma_ii error {eg:.3e} vs oracle {eo:.3e}")
    i, j = model.offset_pairs(offset)
    so = model.sigma_offset(offset)
    P = sp.csc_matrix((np.ones(2 * n), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n))
    P.sum_duplicates()
    P.sort_indices()
    Pc = P.tocoo()
    vg = be.selinv_extract_at(P).tocoo()
    assert np.array_equal(vg.row, Pc.row) and np.array_equal(vg.col, Pc.col)
    eg = np.abs(vg.data - so).max() / s
    eo = max(np.abs(np.asarray(F.selinv().tocsr()[Pc.row, Pc.col]).ravel() - so).max() / s for F in Fs)
    report.update(sigma_ij=(eg, eo))
    _expect(report, "sigma_ij", _ok(eg, eo), f"{tag}: Sigma_ij error {eg:.3e} vs oracle {eo:.3e}")
    # a mode of moderate eigenvalue: for the smallest ones x' Q x cancels in any float64 evaluation
    x, lam = model.mode(tuple(max(1, m // 8) for m in model.dims))
    qt = lam * math.fsum(x * x)
    eg, eo = _rel(be.sqmahal(x), qt), _rel(orc.sqmahal(model.Q, x), qt)
    report.update(mode_quad=(eg, eo))
    _expect(report, "mode_quad", _ok(eg, eo), f"{tag}: quadratic form of a Fourier mode {eg:.3e} vs oracle {eo:.3e}")


def _closed_id(model):
    return f"{model.name}-eps{model.eps:g}"


def _run_closed(model, offset):
    Q = model.Q
    be = gmrfx.MI355XBackend(Q)
    assert be.last_info == 0
    if model.name.startswith("besag"):
        assert be.stats()["inv_cap"] == 2048          # pivot growth <= ~3e3 on these tori: the explicit inverses stay
    perm = be.ordering_permutation()
    Fs = _oracles(Q, perm)
    report = {}
    rng = np.random.default_rng(model.n)
    tag = f"{model.name} eps={model.eps:g}"
    _closed_form_checks(model, offset, be, Fs, report)
    _check_solves(tag, Q, be, Fs, perm, rng, report)
    _check_factor(tag, Q, be, Fs, perm, report)
    _check_trace(tag, Q, be, Fs, report)
    be.close()
    _finish(_closed_id(model), tag, report)


@pytest.mark.parametrize("model,offset", CLOSED, ids=[_closed_id(m) for m, _ in CLOSED])
def test_intrinsic_model_against_closed_forms(model, offset):
    _run_closed(model, offset)


def _run_open(name, Q, kw):
    be = gmrfx.MI355XBackend(Q, **kw)
    assert be.last_info == 0
    perm = be.ordering_permutation()
    Fs = _oracles(Q, perm)
    report = {}
    rng = np.random.default_rng(7)
    _check_solves(name, Q, be, Fs, perm, rng, report)
    _check_factor(name, Q, be, Fs, perm, report)
    _check_trace(name, Q, be, Fs, report)
    be.close()
    _finish(name, name, report)


@pytest.mark.parametrize("name,Q,kw", OPEN, ids=[c[0] for c in OPEN])
def test_near_singular_without_closed_form(name, Q, kw):
    _run_open(name, Q, kw)


@pytest.mark.parametrize("case_id,criterion", [pytest.param(c, k, id=f"{c}-{k}", marks=pytest.mark.xfail(reason=r, strict=True))
                                               for c, ks in KNOWN.items() for k, r in ks.items()])
def test_known_deviations(case_id, criterion):
    """Each known deviation alone, as a strict xfail: it must still fail (XFAIL); if it holds, this test fails (XPASS strict)."""
    if case_id not in _FAILED:                    # the case has not run in this session (a -k selection): run it now
        closed = {_closed_id(m): (m, o) for m, o in CLOSED}
        try:
            if case_id in closed:
                _run_closed(*closed[case_id])
            else:
                _run_open(*next(c for c in OPEN if c[0] == case_id))
        except AssertionError:
            pass                                  # other criteria of the case fail the case's own test, not this one
    assert criterion not in _FAILED[case_id], f"{case_id}: {criterion}"


def test_besag_torus_with_blocked_substitution(monkeypatch):
    """GMRFX_INV_CAP=256: the two-ring top separators (~512 columns) hold only 256-column inverses, the sweeps substitute
    block by block and the selected inversion completes the inverses, on a near-singular front."""
    monkeypatch.setenv("GMRFX_INV_CAP", "256")
    model = im.besag_torus((256, 256), 1e-10)
    be = gmrfx.MI355XBackend(model.Q)
    assert be.stats()["max_cols"] > 256
    perm = be.ordering_permutation()
    Fs = _oracles(model.Q, perm)
    report = {}
    tag = "besag256x256 eps=1e-10 cap=256"
    _closed_form_checks(model, (1, 0), be, Fs, report)
    _check_solves(tag, model.Q, be, Fs, perm, np.random.default_rng(3), report)
    _check_trace(tag, model.Q, be, Fs, report)
    _finish("besag256x256-eps1e-10-cap256", tag, report)
    be.close()


def test_besag_512_torus_fixed_bounds():
    """n = 262144 at eps = 1e-5, no oracle: log det to 1e-13, Sigma_ii to 1e-10, backward error of solves 1e-14."""
    model = im.besag_torus((512, 512), 1e-5)
    be = gmrfx.MI355XBackend(model.Q)
    assert be.last_info == 0
    ld = model.logdet()
    el = _rel(be.compute_logdet(), ld)
    s = model.sigma_diag()
    es = np.abs(be.get_selinv_diag() - s).max() / s
    B = np.random.default_rng(5).standard_normal((model.n, 2))
    eb = im.backward_error(model.Q, be.backend_solve(B), B)
    x, lam = model.mode((0, 3))
    X = be.backend_solve(x)
    ef = im.rel_fwd(X, np.asarray(x, np.longdouble) / np.longdouble(lam))
    print(f"besag512x512 eps=1e-5 logdet={el:.2e} sigma_ii={es:.2e} solve_bwd={eb:.2e} mode_solve_fwd={ef:.2e}")
    assert el <= 1e-13 and es <= 1e-10 and eb <= 1e-14
    assert ef <= 1e-9                  # cond ~ 8e5: a Fourier mode's exact solve x / lam_k, to what float64 allows
    be.close()


def test_batched_besag_members_differing_in_eps():
    """B = 32 Besag members on one 40 x 40 torus, eps from 1e-10 to 1e-2: each member against its own closed forms (log det,
    Sigma_ii, solve against its refined truth) by the oracle-ratio criteria, and with the bits of the plain handle of that member
    (factor, Sigma_ii, solve; the log-determinant to rounding, since the batch reduces it in its own kernel).

    The members form a smooth family in eps, and near the null space the oracle's error at one eps is one rounding of the last
    pivots: at eps = 1.1e-9 its log det error is 5e-13 - 5e-12 in each of five nested-dissection orders, at the neighbouring eps
    1.2e-10 - 1.6e-10 in all of them.
    So a member's bar is the largest oracle error (three orders) over the member and its two neighbours in eps."""
    eps = np.logspace(-10, -2, 32)
    models = [im.besag_torus((40, 40), float(e)) for e in eps]
    Q0 = models[0].Q
    n = Q0.shape[0]
    for mdl in models:
        assert np.array_equal(mdl.Q.indices, Q0.indices) and np.array_equal(mdl.Q.indptr, Q0.indptr)
    NZ = np.asfortranarray(np.stack([mdl.Q.data for mdl in models], axis=1))
    bb = gmrfx.MI355XBatchBackend(Q0, len(models))
    assert np.all(bb.refactorize_values(NZ) == 0)
    perm = bb.ordering_permutation()
    ld, sd = bb.logdet(), bb.selinv_diag()
    rng = np.random.default_rng(11)
    R = rng.standard_normal((n, len(models)))
    X = bb.solve(R)
    gpu, orc_err = [], []
    for k, mdl in enumerate(models):
        Fs = _oracles(mdl.Q, perm)
        lt, st = mdl.logdet(), mdl.sigma_diag()
        T = im.refined_solve(mdl.Q, Fs[0], R[:, k])
        gpu.append((_rel(ld[k], lt), np.abs(sd[:, k] - st).max() / st, im.rel_fwd(X[:, k], T)))
        orc_err.append((max(_rel(F.logdet(), lt) for F in Fs), max(np.abs(F.selinv_diag() - st).max() / st for F in Fs),
                        max(im.rel_fwd(F.solve(R[:, k]), T) for F in Fs)))
    gpu, orc_err = np.array(gpu), np.array(orc_err)
    bar = np.array([orc_err[max(k - 1, 0):k + 2].max(axis=0) for k in range(len(models))])
    failed = []
    for k, mdl in enumerate(models):
        print(f"batch member {k} eps={mdl.eps:.2e} " + " ".join(
            f"{nm}={g:.2e}/{o:.2e}({g / max(o, 1e-300):.2f})" for nm, g, o in zip(("logdet", "sigma_ii", "solve_fwd"), gpu[k], bar[k])))
        for nm, g, o in zip(("logdet", "sigma_ii", "solve_fwd"), gpu[k], bar[k]):
            if not _ok(g, o):
                failed.append(f"member {k} eps={mdl.eps:.2e}: {nm} {g:.3e} vs oracle {o:.3e}")
        if im.backward_error(mdl.Q, X[:, k], R[:, k]) > 1e-14:
            failed.append(f"member {k}: solve backward error")
        p = gmrfx.MI355XBackend(mdl.Q)
        tag = f"batch member {k}"
        assert np.array_equal(p.ordering_permutation(), perm)
        # the batch sums its members' log-pivots in its own kernel (batch.hip), the plain handle in another order: rounding apart
        assert abs(p.compute_logdet() - ld[k]) <= 4 * np.spacing(abs(ld[k])), tag
        assert np.array_equal(p.get_selinv_diag(), sd[:, k]), tag
        assert np.array_equal(p.backend_solve(R[:, k]), X[:, k]), tag
        p.close()
    bb.close()
    assert not failed, "; ".join(failed)


def test_ill_conditioned_fronts_keep_pipelined_and_separate_calls_identical():
    """The Matern precision of range 20 has cond(L11) ~ 2.5e7 at its top front: the handle's first factorisation drops the
    inverse cap to 64 columns (Device::decide_inverse_cap), which brings the solve's backward error to the substitution's level.
    A fresh handle's first pipelined call takes the plain sequence until the cap is decided, so pipelined and separate calls,
    first or later, and a clone give the same bits."""
    import torch
    m = spde.grid_mesh_2d(60, 60, jitter=0.2, seed=4)
    Q = sp.csc_matrix(spde.matern_precision(m, 1, 20.0))
    n = Q.shape[0]
    dev = torch.device("cuda", 0)
    a = gmrfx.MI355XBackend(Q, coords=m.points, factorize=False)
    b = gmrfx.MI355XBackend(Q, coords=m.points, factorize=False)
    rng = np.random.default_rng(2)
    for rep, nrhs in enumerate((64, 3, 64)):
        nz = Q.data * (1.0 + 0.5 * rep)
        d_nz = torch.from_numpy(np.ascontiguousarray(nz)).to(dev)
        Bh = rng.standard_normal((nrhs, n))
        d_B = torch.from_numpy(Bh).to(dev)
        d_Xa, d_Xb = torch.zeros_like(d_B), torch.zeros_like(d_B)
        torch.cuda.synchronize()
        assert a.refactorize_solve_dev(d_nz.data_ptr(), d_B.data_ptr(), n, nrhs, d_Xa.data_ptr(), n) == 0
        assert b.refactorize_dev(d_nz.data_ptr()) == 0
        b.solve_dev(d_B.data_ptr(), n, nrhs, d_Xb.data_ptr(), n)
        torch.cuda.synchronize()
        assert torch.equal(d_Xa, d_Xb), f"call {rep}"
        Qk = sp.csc_matrix((nz, Q.indices, Q.indptr), shape=Q.shape)
        assert im.backward_error(Qk, d_Xa.cpu().numpy().T, Bh.T) <= 1e-15, f"call {rep}"
    for h in (a, b):
        st = h.stats()
        assert st["inv_cap"] == 64 and st["ms_inv_decide"] > 0
    c = a.clone()
    assert c.stats()["inv_cap"] == 64
    Bh = rng.standard_normal((n, 5))
    assert np.array_equal(c.backend_solve(Bh), b.backend_solve(Bh))
    assert np.array_equal(a.get_selinv_diag(), b.get_selinv_diag())
    a.close(); b.close(); c.close()
