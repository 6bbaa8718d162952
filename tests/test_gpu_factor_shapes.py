"""The numeric factorisation ENTRY BY ENTRY on fronts of prescribed shape, per front and per launch path (run with -m gpu on
an MI355X).

tests/factor_shapes.py has the cases and the knob settings of every run (runs(); test_factor_shapes_host.py checks without a
device that they reach every row of its coverage table) and the reference. For every case one handle per setting is built
(the knobs are read at creation) and every stored entry of every panel's lower trapezoid (factor_values(), located through
symbolic()) is compared with the np.longdouble Cholesky factor of Q[perm][:, perm], in the measure

    err[i, j] = |Lg[i, j] - Lref[i, j]| / max_i |Lref[i, j]|

A failure names the setting, the front's (c, m, level, children), the row and the column inside the front. A second
factorisation must give the same bits, the log-determinant must agree with 2 sum log diag(Lref), stored entries outside the
pattern of the true factor (the padding of amalgamated fronts) must be exactly 0.0, and a planted non-positive pivot must be
reported at its column from inside every kernel class.

BOUND = 16 x the largest err of the two float64 witnesses against the same reference over every case of runs(), measured on
CPUs: LAPACK's np.linalg.cholesky and the CPU oracle (orc.OracleFactor(Q, perm).L(), the same recursion in float64, sums of
up to c + m terms in another order than the device's MFMA blocks). Measured witness err per group (LAPACK / oracle):
    chains       2.82e-16 / 2.14e-15     children     2.80e-16 / 9.69e-16     records      2.79e-16 / 1.88e-15
    bwd classes  2.42e-16 / 1.44e-15     wide         2.62e-16 / 2.10e-15     widths       2.34e-16 / 1.56e-15
    narrow       2.39e-16 / 1.33e-15     trsm         2.80e-16 / 1.38e-15     gemm         2.50e-16 / 1.90e-15
    dense        2.44e-16 / 2.93e-15     blocking     3.39e-16 / 2.12e-15     two chains   2.27e-16 / 2.08e-15
    syrk         2.77e-16 / 2.21e-15     small        2.23e-16 / 1.06e-15     small path   2.68e-16 / 3.00e-15
    amalgamated  2.22e-16 / 8.84e-16
WITNESS_ERR_MAX is the maximum (small path, the oracle), BOUND = 4.8e-14. (The reference's own residual max |A - L L'| / max |A|, in np.longdouble: <= 1.9e-19.)
The device is never the source of the bound. Device err per group, as printed by this test on an MI355X:
    chains       8.87e-16     children     6.53e-16     records      7.31e-16     bwd classes  8.11e-16
    wide         7.51e-16     widths       6.29e-16     narrow       8.60e-16     trsm         7.45e-16
    gemm         7.42e-16     dense        6.96e-16     blocking     7.10e-16     two chains   5.97e-16
    syrk         8.16e-16     small        8.18e-16     small path   1.16e-15     amalgamated  5.21e-16
    batched      6.62e-16
(the largest over every setting of the group).
"""
import numpy as np
import pytest

import gmrfx
import orc
import selinv_shapes as ss
import sweep_shapes as ws
import factor_shapes as fs

pytestmark = pytest.mark.gpu

WITNESS_ERR_MAX = 3.00e-15
BOUND = 16 * WITNESS_ERR_MAX

_ref_cache = {}


def _reference(case, perm):
    """Q, blocks, the reference factor (hi, lo) and its log-determinant: once per case, shared by its settings and tests."""
    hit = _ref_cache.get(case["name"])
    if hit is None or not np.array_equal(hit["perm"], perm):
        Q, blocks = ss.make(case)
        hi, lo, _ = fs.reference_factor(Q, perm)
        res = fs.residual(Q, perm, hi, lo)
        assert res <= BOUND / 100, f"{case['name']}: the reference's own residual {res:.2e}"
        Lo = np.tril(orc.OracleFactor(Q, perm).L().toarray())
        eo = fs.errors(Lo, np.ones(hi.shape, dtype=bool), hi, lo).max()
        assert eo <= WITNESS_ERR_MAX, f"{case['name']}: the CPU oracle's factor against the reference: {eo:.3e}"
        _ref_cache.clear()          # cases come grouped by name: keep one
        _ref_cache[case["name"]] = hit = {"perm": perm.copy(), "Q": Q, "blocks": blocks, "hi": hi, "lo": lo, "oracle": Lo, "logdet": fs.logdet_ref(hi, lo)}
    return hit


def _matrix(case):
    hit = _ref_cache.get(case["name"])
    return (hit["Q"], hit["blocks"]) if hit else ss.make(case)


def _logdet_tolerance(hi):
    """2 sum_j log L[j, j]: an entry's err e moves log L[j, j] by at most e max_i |L[i, j]| / L[j, j]; the sum of n terms in
    float64, in any order, adds at most n eps sum |2 log L[j, j]|."""
    d = np.diag(hi)
    return 2 * BOUND * float((np.abs(hi).max(axis=0) / d).sum()) + len(d) * np.finfo(float).eps * float(np.abs(2 * np.log(d)).sum())


def _check_factor(be, ref, tag):
    """Every stored entry against the reference and the oracle, the padding, the log-determinant. -> (values, err, padding entries)"""
    n = be.n
    vals = be.factor_values()
    Lg, stored = fs.panels(be.symbolic(), vals, n)
    e, where = fs.describe(fs.per_front(be, fs.errors(Lg, stored, ref["hi"], ref["lo"])))
    assert e <= BOUND, f"{tag}: {where} (bound {BOUND:.2e})"
    sc = np.abs(ref["hi"]).max(axis=0)
    assert (np.where(stored, np.abs(Lg - ref["oracle"]), 0.0) / sc).max() <= BOUND + WITNESS_ERR_MAX, f"{tag}: against the CPU oracle's factor"
    pad = fs.padding(stored, ref["hi"])
    assert not Lg[pad].any(), f"{tag}: {int((Lg[pad] != 0).sum())} of {int(pad.sum())} padding entries are not 0.0, the largest {np.abs(Lg[pad]).max():.3e}"
    ld = be.compute_logdet()
    assert abs(ld - ref["logdet"]) <= _logdet_tolerance(ref["hi"]), f"{tag}: logdet {ld!r} against {ref['logdet']!r}"
    return vals, e, int(pad.sum())


def _run_case(case, settings, monkeypatch):
    worst = 0.0
    for setting in settings:
        fs.apply_setting(monkeypatch, setting)
        Q, blocks = _matrix(case)
        be = gmrfx.MI355XBackend(Q, device=0, **ss.KW)
        tag = f"{case['name']}[{fs.label(setting)}]"
        assert be.last_info == 0, tag
        if "merged" not in case:
            ss.check_shapes(be, blocks)
        ref = _reference(case, be.ordering_permutation())
        vals, e, npad = _check_factor(be, ref, tag)
        if "merged" in case:
            assert npad > 0, f"{tag}: the merged front holds no padding"
        be.refactorize_values(Q.data)
        assert be.last_info == 0 and np.array_equal(be.factor_values(), vals), f"{tag}: a second factorisation gives other bits"
        worst = max(worst, e)
        be.close()
    print(f"{case['name']}: n={Q.shape[0]} gpu_err={worst:.3e}")
    return worst


RUNS = [(group, case, settings) for group, cases, settings in fs.runs() for case in cases]


@pytest.mark.parametrize("group,case,settings", RUNS, ids=[f"{g}-{c['name']}" for g, c, _ in RUNS])
def test_every_stored_entry_of_the_factor_per_front_and_path(group, case, settings, monkeypatch):
    _run_case(case, settings, monkeypatch)


# ---- pivot reports ----------------------------------------------------------------------------------------------------------
def _case(name):
    return next(c for c in fs.new_cases() if c["name"] == name)


def _plan(be, setting):
    fr = ws.fronts(be)
    levels, subs = fs.factor_levels(fr, fs.knobs(setting))
    return fr, levels, subs, be.symbolic().super_first


def _front(fr, c, m=None, nch=None):
    return next(f for f in fr if f[1] == c and (m is None or f[2] == m) and (nch is None or f[4] == nch))


def _in_small_class(q):
    def pick(fr, levels, subs, first):
        c, m = fs.SMALL_PARENTS[q]
        f = _front(fr, c, m, 3)
        assert any(f in L.small[q] for L in levels.values())
        return int(first[f[0]]) + c // 2
    return pick


def _in_subtree(fr, levels, subs, first):
    root = _front(fr, *fs.SMALL_PARENTS[1], 3)           # the 64-row parent and its three children: one subtree task
    assert subs[root[0]] == (root[0] - 3, 1)
    return int(first[root[0] - 2]) + 1                   # a column of a child


def _at_block0(c, shape):
    def pick(fr, levels, subs, first):
        f = _front(fr, c)
        L = levels[f[3]]
        assert any(v == shape + ":cut" and f in fl and b == 0 for v, fl, b in fs.panel_launches(L))
        return int(first[f[0]]) + c - 1
    return pick


def _at_block(c, b, j, shape):
    def pick(fr, levels, subs, first):
        f = _front(fr, c)
        assert any(v.startswith(shape) and f in fl and bb == b for v, fl, bb in fs.panel_launches(levels[f[3]]))
        assert b * 64 + j < c
        return int(first[f[0]]) + b * 64 + j
    return pick


def _on_second_chain(fr, levels, subs, first):
    f = _front(fr, 200)
    L = levels[f[3]]
    assert fs.two_chains(L) and L.big.index(f) % 2 == 1
    return int(first[f[0]]) + 150


PIVOTS = [
    ("small_kids3", fs.LEVEL128, _in_small_class(0), "k_factor_small<48>"),
    ("small_kids3", fs.LEVEL128, _in_small_class(1), "k_factor_small<64>"),
    ("small_kids3", fs.LEVEL128, _in_small_class(2), "k_factor_small<96>"),
    ("small_kids3", fs.LEVEL128, _in_small_class(3), "k_factor_small<128>"),
    ("small_kids3", fs.SUBTREE, _in_subtree, "k_factor_subtree<64>"),
    ("widths", fs.LEVEL0, _at_block0(15, "k_potrf64_b<1,1>"), "potrf<1,1>-block0"),
    ("widths", fs.LEVEL0, _at_block0(31, "k_potrf64_b<2,2>"), "potrf<2,2>-block0"),
    ("widths", fs.LEVEL0, _at_block0(47, "k_potrf64_b<4,3>"), "potrf<4,3>-block0"),
    ("widths", fs.LEVEL0, _at_block0(63, "k_potrf64_b<8,4>"), "potrf<8,4>-block0"),
    ("widths", fs.LEVEL0, _at_block(110, 1, 45, "k_potrf64_b<4,3>"), "potrf<4,3>-block1"),
    ("pair3", fs.DEFAULTS, _on_second_chain, "second-chain"),
    ("block_chain1", fs.DEFAULTS, _at_block(513, 2, 7, "k_potrf64_b<8,4>:arg"), "later-block"),
    ("block_chain1", fs.DEFAULTS, _at_block(577, 9, 0, "k_potrf64_b<1,1>:arg"), "partial-last-block"),
]


def _pivot_round(be, ref, Q, ks, tag):
    """Plant the pivots ks, expect the smallest reported; then the good values again: info 0 and the bits from before."""
    vals = be.factor_values()
    be.refactorize(fs.plant_pivot(Q, ref["perm"], ref["hi"], ref["lo"], ks))
    assert be.last_info == min(ks) + 1, f"{tag}: pivots planted in columns {ks}, info {be.last_info}"
    be.refactorize(Q)
    assert be.last_info == 0 and np.array_equal(be.factor_values(), vals), f"{tag}: the factorisation after a failed one"


@pytest.mark.parametrize("name,setting,pick,what", PIVOTS, ids=[p[3] for p in PIVOTS])
def test_a_planted_pivot_is_reported_from_inside_every_kernel_class(name, setting, pick, what, monkeypatch):
    case = _case(name)
    fs.apply_setting(monkeypatch, setting)
    Q, _ = _matrix(case)
    be = gmrfx.MI355XBackend(Q, device=0, **ss.KW)
    assert be.last_info == 0
    ref = _reference(case, be.ordering_permutation())
    k = pick(*_plan(be, setting))
    _pivot_round(be, ref, Q, [k], f"{name}[{fs.label(setting)}] {what}")
    be.close()


def test_of_two_failed_pivots_the_smaller_column_is_reported(monkeypatch):
    """Two independent fronts fail in one factorisation: on one level in different launches (the <1,1> and the <8,4> piece of
    block 0), and on different levels (a front of the lower level and a leaf of the level above it that is not its ancestor)."""
    case = _case("widths")
    fs.apply_setting(monkeypatch, fs.LEVEL0)
    Q, _ = _matrix(case)
    be = gmrfx.MI355XBackend(Q, device=0, **ss.KW)
    ref = _reference(case, be.ordering_permutation())
    fr, levels, subs, first = _plan(be, fs.LEVEL0)
    a, b = _front(fr, 15), _front(fr, 63)
    assert a[3] == b[3]
    _pivot_round(be, ref, Q, [int(first[a[0]]) + 7, int(first[b[0]]) + 40], "widths: one level, two launches")
    low = _front(fr, 5, 64)                                   # under the 110-column front
    par = _front(fr, 110)
    assert low[5] == par[0] and low[3] == par[3] - 1
    leaves = [f for f in fr if f[3] == par[3] and f[4] == 0]
    for leaf in (min(leaves), max(leaves)):                    # one numbered before the lower front, one after it
        _pivot_round(be, ref, Q, [int(first[low[0]]) + 2, int(first[leaf[0]]) + leaf[1] // 2], "widths: two levels")
    assert min(leaves)[0] < low[0] < max(leaves)[0]
    be.close()


# ---- batched handle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,setting", [("widths", fs.LEVEL0), ("syrk_kids3", fs.DEFAULTS)], ids=["widths", "syrk_kids3"])
def test_batched_handle_factors_every_member_entry_by_entry(name, setting, monkeypatch):
    """Three members of one pattern with different values: every member's slice of factor_values() against that member's
    reference; a pivot planted in the middle member is reported for it alone and its neighbours keep their bits."""
    fs.apply_setting(monkeypatch, setting)
    Q0, _ = ss.make(_case(name))
    members = [Q0, ss.with_values(Q0, 81), ss.with_values(Q0, 82)]
    n = Q0.shape[0]
    bb = gmrfx.MI355XBatchBackend(Q0, 3, ordering="natural", device=0)
    NZ = np.stack([q.data for q in members], axis=1)
    assert not bb.refactorize_values(NZ).any()
    perm = bb.ordering_permutation()
    sym = gmrfx.MI355XBackend.symbolic(bb)
    Lg, stored = fs.panels(sym, bb.factor_values(), 3 * n)
    refs = []
    for k, q in enumerate(members):
        hi, lo, _ = fs.reference_factor(q, perm)
        assert fs.residual(q, perm, hi, lo) <= BOUND / 100
        refs.append((hi, lo))
        sl = slice(k * n, (k + 1) * n)
        assert not stored[sl, :k * n].any() and not stored[sl, (k + 1) * n:].any()
        E = fs.errors(Lg[sl, sl], stored[sl, sl], hi, lo)
        i, j = np.unravel_index(int(E.argmax()), E.shape)
        print(f"batched {name} member {k}: gpu_err={E.max():.3e}")
        assert E.max() <= BOUND, f"member {k}: entry (row {i}, column {j}) in elimination order, err {E.max():.3e} (bound {BOUND:.2e})"
        assert not Lg[sl, sl][fs.padding(stored[sl, sl], hi)].any(), f"member {k}: padding that is not 0.0"
    ld = bb.logdet()
    for k, (hi, lo) in enumerate(refs):
        assert abs(ld[k] - fs.logdet_ref(hi, lo)) <= _logdet_tolerance(hi), f"member {k}: logdet"
    # a pivot planted in member 1
    kbad = n // 2
    bad = NZ.copy()
    bad[:, 1] = fs.plant_pivot(members[1], perm, *refs[1], [kbad]).data
    assert list(bb.refactorize_values(bad)) == [0, kbad + 1, 0]
    Lb, _ = fs.panels(sym, bb.factor_values(), 3 * n)
    for k in (0, 2):
        sl = slice(k * n, (k + 1) * n)
        assert np.array_equal(Lb[sl, sl], Lg[sl, sl]), f"member {k} lost its bits to its neighbour's failed pivot"
    assert not bb.refactorize_values(NZ).any()
    assert np.array_equal(fs.panels(sym, bb.factor_values(), 3 * n)[0], Lg)
    bb.close()
