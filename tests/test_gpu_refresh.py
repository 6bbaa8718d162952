"""Every read-out is fresh after every way of refactorising (the protocol, the tables and the problems: tests/refresh_cases.py; what
they rest on is verified without a device by tests/test_refresh_host.py).

A handle is factorised at A and every read-out is run, so that every lazily built piece holds A's state; it is brought to B by the
route under test; every read-out is run again, in the table's order or reversed. A fresh handle factorised once at B by the plain
call must give the same bits, read-out by read-out and for what the route itself returned -- no tolerance anywhere. The only other
assertions are the documented refusals (no held values, a failed factorisation) and that the results differ from A's."""
import numpy as np
import pytest

import gmrfx
import refresh_cases as rc
from gmrfx._lib import lib, ptr

pytestmark = pytest.mark.gpu
ORDERS = ("table", "reverse")


def _env(monkeypatch, p):
    monkeypatch.delenv("GMRFX_INV_CAP", raising=False)
    for k, v in p.env.items():
        monkeypatch.setenv(k, v)


def _same_cap(be, fresh):
    assert be.stats()["inv_cap"] == fresh.stats()["inv_cap"]


def _plain(p, route, order, form="node", con="con1", make=None):
    tab = rc.table(con=bool(con))
    return rc.protocol(make or (lambda: p.make(form, con)), p.A, lambda be: route(be, p), lambda be, o, nz: rc.run_readouts(be, p, tab, o, nz),
                       order, refusals=lambda be: rc.refused(be, p, tab), invariant=_same_cap)


def _assert_equal(got, want, what):
    bad = [k for k in got if not rc.bits_equal(got[k], want[k])]
    assert not bad, f"{what}: {bad}"


# ---- routes of a plain handle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("route", [r for r in rc.ROUTES if r != "gaussian_approximation"])
def test_route_on_p_small(route, order, monkeypatch):
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    _plain(p, rc.ROUTES[route][0], order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("form", ["node", "design"])
def test_gaussian_approximation_leaves_the_final_factor(form, order, monkeypatch):
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    _plain(p, rc.ROUTES["gaussian_approximation"][0], order, form=form)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("route", ["refactorize_values", "refactorize_dev", "refactorize_solve[1]", "refactorize_solve[17]", "refactorize_solve[65]",
                                   "refactorize_solve_dev[17]", "refactorize_logpdf_dev", "refactorize_update_solve[17]", "gaussian_approximation"])
def test_route_on_p_cap(route, order, monkeypatch):
    """fronts wider than the inverse cap: the sweeps substitute block by block, the selected inversion adds the doubling stages"""
    p = rc.problem("P_cap")
    _env(monkeypatch, p)
    _plain(p, rc.ROUTES[route][0], order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("route", ["refactorize_dev", "refactorize_solve[65]", "refactorize_solve_dev[17]", "refactorize_logpdf_dev",
                                   "refactorize_update", "ga_pullback"])
def test_route_without_a_constraint(route, order, monkeypatch):
    """the constraint read-outs leave, the RBMC variances (refused with a constraint set) join"""
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    _plain(p, rc.ROUTES[route][0], order, con=None)


def test_selinv_solve_pipelined_selinv_solve_under_the_cap(monkeypatch):
    """selinv (completes the dense inverses: inverse_full_) -> solve -> pipelined refactorize_solve (inverses of the cap only, built
    level by level) -> selinv (must complete them again) -> solve"""
    p = rc.problem("P_cap")
    _env(monkeypatch, p)
    be, fresh = p.make(), None
    try:
        be.refactorize_values(p.A)
        s0, x0 = be.get_selinv_diag().copy(), be.backend_solve(p.R[:, :17])
        X = be.refactorize_solve(p.B, p.R[:, :65])
        s1, e1, x1 = be.get_selinv_diag().copy(), be.selinv_extract_at(p.Q).data, be.backend_solve(p.R[:, :17])
        fresh = p.make()
        fresh.refactorize_values(p.B)
        _same_cap(be, fresh)
        assert fresh.stats()["inv_cap"] == 64
        assert rc.same_bits(X, fresh.backend_solve(p.R[:, :65]))
        assert rc.same_bits(s1, fresh.get_selinv_diag()) and rc.same_bits(e1, fresh.selinv_extract_at(p.Q).data)
        assert rc.same_bits(x1, fresh.backend_solve(p.R[:, :17]))
        assert not rc.same_bits(s1, s0) and not rc.same_bits(x1, x0)
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


# ---- a failed factorisation in between --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_a_failed_factorisation_in_between_leaves_nothing_behind(order, monkeypatch):
    p = rc.problem("P_small")
    _env(monkeypatch, p)

    def route(be, p):
        be.refactorize_values(p.bad_values())          # check_posdef off: reported through last_info
        assert be.last_info > 0
        be.refactorize_values(p.B)
        assert be.last_info == 0
        return rc.RouteResult(p.B, True)

    _plain(p, route, order)


def test_a_failed_handle_refuses_the_gradient(monkeypatch):
    """include/gmrfx.h: gmrfx_logpdf_grad returns GMRFX_ERR_NOT_POSDEF when the last factorisation reported one"""
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    be = p.make()
    try:
        be.refactorize_values(p.A)
        rc.run_readouts(be, p, rc.table())
        be.refactorize_values(p.bad_values())
        assert be.last_info > 0
        with pytest.raises(gmrfx._lib.PosDefException):
            be.logpdf_grad(p.x, mean=p.mu)
        chk = p.make(check_posdef=True)
        try:
            chk.refactorize_values(p.A)
            with pytest.raises(gmrfx._lib.PosDefException):
                chk.refactorize_values(p.bad_values())
            with pytest.raises(gmrfx._lib.PosDefException):
                chk.logpdf_grad(p.x, mean=p.mu)
        finally:
            chk.close()
    finally:
        be.close()


# ---- a clone ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_a_clone_refactorises_without_touching_its_source(order, monkeypatch):
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    tab = rc.table()
    be, cl, fresh = p.make(), None, None
    try:
        be.refactorize_values(p.A)
        stale = rc.run_readouts(be, p, tab)
        cl = be.clone()
        wrong = rc.refused(cl, p, tab)                 # a clone does not hold Q's values
        assert not wrong, wrong
        _assert_equal(rc.run_readouts(cl, p, tab, order, p.A), stale, "the clone at A")
        cl.refactorize_values(p.B)
        got = rc.run_readouts(cl, p, tab, order)
        fresh = p.make()
        fresh.refactorize_values(p.B)
        _same_cap(cl, fresh)
        _assert_equal(got, rc.run_readouts(fresh, p, tab, order), "the clone at B against the fresh handle")
        assert not [k for k in got if rc.bits_equal(got[k], stale[k])]
        _assert_equal(rc.run_readouts(be, p, tab, order), stale, "the source after its clone's factorisation")
    finally:
        for h in (be, cl, fresh):
            if h is not None:
                h.close()


# ---- becoming a batch of one ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_becoming_a_batch_of_one_changes_nothing_a_plain_call_sees(order, monkeypatch):
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    tab = rc.table()

    def route(be, p):
        stale = rc.run_readouts(be, p, tab)
        obs_before = _obs_readouts(be, p, "node")
        qb, mb, info, yb = np.empty(p.nnz), np.empty(p.n), np.zeros(1, np.int64), np.array([-1.3])
        assert lib().gmrfx_batch_logpdf_grad(be._h, None, ptr(p.x), p.n, ptr(p.mu), ptr(yb), ptr(qb), ptr(mb), ptr(info)) == 0 and info[0] == 0
        assert rc.bits_equal((qb, mb), stale["logpdf_grad"])
        J = np.asfortranarray(np.random.default_rng(1).standard_normal((p.nnz, 2)))
        out = np.empty(2)
        assert lib().gmrfx_batch_pattern_dot(be._h, ptr(qb), ptr(J), p.nnz, 2 * p.nnz, 2, ptr(out)) == 0
        assert rc.same_bits(out, be.pattern_dot(qb, J))
        _assert_equal(rc.run_readouts(be, p, tab, order), stale, "after the handle became a batch of one")
        p.set_obs(be, "node")           # the likelihood's setter and the calls that read it still take the handle for a plain one
        _assert_equal(_obs_readouts(be, p, "node"), obs_before, "the likelihood's calls after the handle became a batch of one")
        return rc.ROUTES["refactorize_solve[17]"][0](be, p)

    _plain(p, route, order)


# ---- state a setter drops ----------------------------------------------------------------------------------------------------------------
CON_READOUTS = ("constraint_fields", "constraint_info", "constrained_mean", "constrained_var", "constraint_correct", "sample", "logpdf_grad",
                "predictor_marginals")


def _con_table(con):
    return {k: v for k, v in rc.table(con=bool(con)).items() if k in CON_READOUTS}


def test_constraint_change(monkeypatch):
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    be = p.make(con=None)
    try:
        be.refactorize_values(p.A)
        seen = []
        for vals, con in ((p.A, "con1"), (p.A, "con2"), (p.A, None), (p.A, "con1"), (p.B, "con1")):
            if con:
                be.set_constraints(*getattr(p, con))
            else:
                be.clear_constraints()
            if vals is p.B:          # across a refactorisation: read at A with con1 (the previous stage), pipelined route to B, read
                be.refactorize_solve(p.B, p.R[:, :17])
            got = rc.run_readouts(be, p, _con_table(con))
            fresh = p.make(con=con)
            try:
                fresh.refactorize_values(vals)
                _same_cap(be, fresh)
                _assert_equal(got, rc.run_readouts(fresh, p, _con_table(con)), f"constraint {con}")
            finally:
                fresh.close()
            seen.append(got)
        assert not rc.bits_equal(seen[0]["logpdf_grad"], seen[1]["logpdf_grad"]) and not rc.bits_equal(seen[1]["sample"], seen[2]["sample"])
        _assert_equal(seen[3], seen[0], "con1 again")
        assert not [k for k in seen[4] if rc.bits_equal(seen[4][k], seen[3][k])]
    finally:
        be.close()


def _obs_readouts(be, p, form):
    hmap = p.dpos if form == "node" else be.observations_hess_map()
    be.set_prior(p.prior, hmap)
    out = {"predictor_marginals": rc._arr(*be.predictor_marginals(p.x, constraint_correction=be._con_m() > 0)),
           "fisher_eval": rc._arr(*be.fisher_eval(p.x, mean=p.mu))}
    qp, mp, lam, par, chk = be.ga_pullback(p.x, mean=p.mu, mubar=p.mu, Qbar=p.Bm.data)
    out["ga_pullback"] = rc._arr(qp, mp, lam, par, chk)
    return out


def test_observation_change(monkeypatch):
    """gap_, pred_, prior_diag_ and prior_design_: node form, design form with another nobs and the new map, node form again"""
    p = rc.problem("P_small")
    _env(monkeypatch, p)
    be = p.make()
    try:
        be.refactorize_values(p.B)
        seen = []
        for form in ("node", "design", "node"):
            p.set_obs(be, form)
            got = _obs_readouts(be, p, form)
            fresh = p.make(form=form)
            try:
                fresh.refactorize_values(p.B)
                _assert_equal(got, _obs_readouts(fresh, p, form), f"{form} form")
            finally:
                fresh.close()
            seen.append(got)
        assert seen[0]["predictor_marginals"][0].shape != seen[1]["predictor_marginals"][0].shape
        _assert_equal(seen[2], seen[0], "node form again")
    finally:
        be.close()


# ---- batched handles ---------------------------------------------------------------------------------------------------------------------
_BP = []


def _bp():
    if not _BP:
        _BP.append(rc.BatchProblem())
    return _BP[0]


def _batch(route, VA, VB, order, con=True):
    p = _bp()
    tab = rc.batch_table(con)

    def refusals(bb):
        wrong = []
        for name in (k for k in rc.BATCH_NEEDS_VALUES if k in tab):
            try:
                tab[name](bb, p, None)
                wrong.append(name + ": returned numbers")
            except ValueError as ex:
                if rc.REFUSAL not in str(ex):
                    wrong.append(f"{name}: {ex}")
        return wrong

    return rc.protocol(lambda: p.make(con), VA, lambda bb: rc.BATCH_ROUTES[route][0](bb, p, VB), lambda bb, o, nz: rc.run_batch_readouts(bb, p, tab, o, nz),
                       order, refusals=refusals, may_stay=("info",))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("route", list(rc.BATCH_ROUTES))
def test_batch_route(route, order):
    p = _bp()
    _batch(route, p.A, p.B, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("route", ["refactorize_values", "refactorize_dev", "refactorize_logpdf_dev"])
def test_batch_route_without_a_constraint(route, order):
    """with the RBMC variances, which a handle with a constraint set refuses"""
    p = _bp()
    _batch(route, p.A, p.B, order, con=False)


@pytest.mark.parametrize("route", list(rc.BATCH_ROUTES))
def test_batch_member_bad_in_a_and_good_in_b(route):
    p = _bp()
    stale, got, want = _batch(route, p.bad(p.A), p.B, "table")
    assert stale["info"][0][1] > 0
    assert (got["info"][0] == 0).all() and (got["constraint_info"][3] == 0).all()
    assert all(np.isfinite(a).all() for v in got.values() for a in v)


@pytest.mark.parametrize("route", list(rc.BATCH_ROUTES))
def test_batch_member_good_in_a_and_bad_in_b(route):
    p = _bp()
    _, got, want = _batch(route, p.A, p.bad(p.B), "table")
    _, good, _ = _batch(route, p.A, p.B, "table")
    assert got["info"][0][1] > 0 and got["info"][0][0] == 0 and got["info"][0][2] == 0
    assert list(got["constraint_info"][3]) == [0, -1, 0]
    qb, mb, ginfo = got["logpdf_grad"]
    assert list(ginfo) == [0, -1, 0] and np.isnan(qb[:, 1]).all() and np.isnan(mb[:, 1]).all()
    for name in ("logdet", "solve", "backward_solve", "selinv_diag", "constrained_mean", "constrained_var", "sample", "logpdf_grad"):
        for a, g in zip(got[name], good[name]):
            if a.ndim >= 2:         # members along the last axis
                assert rc.same_bits(a[..., 0], g[..., 0]) and rc.same_bits(a[..., 2], g[..., 2]), name
            else:
                assert rc.same_bits(a[[0, 2]], g[[0, 2]]), name
