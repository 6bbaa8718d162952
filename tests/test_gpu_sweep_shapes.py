"""The triangular sweeps ENTRY BY ENTRY on fronts of prescribed shape, per front and per path (run with -m gpu on an MI355X).

tests/sweep_shapes.py has the cases, the knob settings and widths of every run (runs(); test_sweep_shapes_host.py checks
without a device that they reach every class of its coverage table) and the references. For every case one handle per
knob setting is built (the knobs are read at creation), and for every listed width the full solve (backend_solve) and the
backward-only solve (backend_backward_solve) are compared with an extended-precision reference that is independent of
the library, in the measure

    err[i, j] = |X[i, j] - ref[i, j]| / max_i |ref[i, j]|

with the rows mapped to the front that owns them: a failure names the setting, the width, the front's (c, m, level,
children), the row inside the front and the column; a second call must give the same bits. The CPU oracle is a second
witness. Widths per setting: sweep_shapes.runs() (WIDTHS = 1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 37, 63, 64, 65 under the
defaults and wherever a setting changes the narrow kernels; W_WIDE = 17 .. 65 where it only changes the front kernels;
W_EDGE / W_FEW, one width per class, under the small-front and plain-grid settings).

BOUND = 16 x the largest err of the float64 CPU oracle (orc.OracleFactor.solve / .backward_solve on the handle's
permutation) against the same references over the same cases and all 65 columns, measured on CPUs: the same recursion in
float64 with sums of up to c + m terms in another order. Measured oracle err per case group (full solve / backward-only):
    chains       3.15e-15 / 2.70e-15     lone fronts  2.72e-15 / 2.19e-15     small-path sets  1.64e-15 / 1.33e-15
    mixed+gather 1.37e-15 / 1.48e-15     records      1.34e-15 / 1.11e-15     children         2.23e-15 / 1.87e-15
    bwd classes  6.68e-16 / 4.87e-16     wide         3.01e-15 / 2.96e-15     tasks            9.06e-16 / 7.98e-16
    split-K      3.63e-15 / 2.28e-15: the maximum, ORACLE_ERR_MAX
(The references' own residuals: <= 1e-19 for the full solve, <= 2.3e-17 for the backward-only solve.)
The device is never the source of the bound. Device err per group, as printed by this test on an MI355X:
    chains       3.45e-15     lone fronts  3.97e-15     small-path sets  3.19e-15     mixed+gather  2.33e-15
    records      2.01e-15     children     3.76e-15     bwd classes      3.11e-15     wide          4.07e-15
    split-K      2.47e-15     tasks        9.77e-16     batched handle   3.48e-15
(the larger of the two solves over every setting and width of the group; BOUND = 5.8e-14).
"""
import numpy as np
import pytest

import gmrfx
import orc
import selinv_shapes as ss
import sweep_shapes as ws

pytestmark = pytest.mark.gpu

ORACLE_ERR_MAX = 3.64e-15
BOUND = 16 * ORACLE_ERR_MAX

_ref_cache = {}


def _reference(case, perm):
    """(Q, blocks, B, (X, dX), (Xb, dXb), oracle results): once per case, shared by its settings (one permutation)."""
    hit = _ref_cache.get(case["name"])
    if hit is None or not np.array_equal(hit["perm"], perm):
        Q, blocks = ss.make(case)
        B = ws.rhs(Q.shape[0], case["seed"] if "seed" in case else 7)
        X, dX, res = ws.reference_solve(Q, B)
        Xb, dXb, resb = ws.reference_backward(Q, perm, B, B, X, dX)
        assert res.max() <= BOUND / 100 and resb.max() <= BOUND / 100, f"reference residuals {res.max():.2e}, {resb.max():.2e}"
        F = orc.OracleFactor(Q, perm)
        Xo, Xbo = F.solve(B), F.backward_solve(B)
        assert ws.errors(Xo, X, dX).max() <= ORACLE_ERR_MAX and ws.errors(Xbo, Xb, dXb).max() <= ORACLE_ERR_MAX
        _ref_cache.clear()          # cases come grouped by name: keep one
        _ref_cache[case["name"]] = hit = {"perm": perm.copy(), "Q": Q, "blocks": blocks, "B": B, "full": (X, dX), "bwd": (Xb, dXb), "oracle": (Xo, Xbo)}
    return hit


def _run_case(case, settings, monkeypatch):
    worst = 0.0
    for setting, widths in settings:
        ws.apply_setting(monkeypatch, setting)
        Q, blocks = ss.make(case) if case["name"] not in _ref_cache else (_ref_cache[case["name"]]["Q"], _ref_cache[case["name"]]["blocks"])
        be = gmrfx.MI355XBackend(Q, device=0, **ss.KW)
        assert be.last_info == 0
        ss.check_shapes(be, blocks)
        ref = _reference(case, be.ordering_permutation())
        B = ref["B"]
        tag = f"{case['name']}[{ws.label(setting)}]"
        for w in widths:
            Bw = B[:, 0] if w == 1 else B[:, :w]
            G = be.backend_solve(Bw).reshape(len(B), -1)
            Gb = be.backend_backward_solve(Bw).reshape(len(B), -1)
            assert np.array_equal(G, be.backend_solve(Bw).reshape(len(B), -1)), f"{tag} nr={w}: a second full solve gives other bits"
            assert np.array_equal(Gb, be.backend_backward_solve(Bw).reshape(len(B), -1)), f"{tag} nr={w}: a second backward-only solve gives other bits"
            e, where = ws.describe(ws.per_front(be, ws.errors(G, ref["full"][0][:, :w], ref["full"][1][:, :w])))
            eb, whereb = ws.describe(ws.per_front(be, ws.errors(Gb, ref["bwd"][0][:, :w], ref["bwd"][1][:, :w])))
            worst = max(worst, e, eb)
            assert eb <= BOUND, f"{tag} nr={w}, backward-only solve: {whereb} (bound {BOUND:.2e})"
            assert e <= BOUND, f"{tag} nr={w}, full solve: {where} (bound {BOUND:.2e}); the backward-only solve is clean ({eb:.2e}): the forward sweep is the suspect"
            # second witness: the float64 oracle on the same permutation
            sc = np.abs(ref["full"][0][:, :w]).max(axis=0)
            scb = np.abs(ref["bwd"][0][:, :w]).max(axis=0)
            assert (np.abs(G - ref["oracle"][0][:, :w]) / sc).max() <= BOUND + ORACLE_ERR_MAX, f"{tag} nr={w}: full solve against the CPU oracle"
            assert (np.abs(Gb - ref["oracle"][1][:, :w]) / scb).max() <= BOUND + ORACLE_ERR_MAX, f"{tag} nr={w}: backward-only solve against the CPU oracle"
        be.close()
    print(f"{case['name']}: n={len(B)} gpu_err={worst:.3e}")
    return worst


RUNS = [(group, case, settings) for group, cases, settings in ws.runs() for case in cases]


@pytest.mark.parametrize("group,case,settings", RUNS, ids=[f"{g}-{c['name']}" for g, c, _ in RUNS])
def test_every_entry_of_both_solves_per_front_and_path(group, case, settings, monkeypatch):
    _run_case(case, settings, monkeypatch)


def test_batched_handle_runs_the_same_kernels():
    """Three members of the 3-children pattern with different values in one batched handle: solve / backward_solve per member
    at the widths on both sides of the narrow kernels' limits, each member held to the same bound."""
    Q0, _ = ss.make(ws.children_cases()[6])
    members = [Q0, ss.with_values(Q0, 71), ss.with_values(Q0, 72)]
    n = Q0.shape[0]
    bb = gmrfx.MI355XBatchBackend(Q0, 3, ordering="natural", device=0)
    assert not bb.refactorize_values(np.stack([q.data for q in members], axis=1)).any()
    perm = bb.ordering_permutation()
    B = ws.rhs(n, 3)
    refs = []
    for q in members:
        X, dX, res = ws.reference_solve(q, B)
        Xb, dXb, resb = ws.reference_backward(q, perm, B, B, X, dX)
        assert res.max() <= BOUND / 100 and resb.max() <= BOUND / 100
        refs.append((X, dX, Xb, dXb))
    for w in (1, 9, 16, 17, 33, 64):
        R = np.repeat(B[:, :w, None], 3, axis=2)
        G = bb.solve(R[:, 0, :] if w == 1 else R).reshape(n, w, 3)
        Gb = bb.backward_solve(R[:, 0, :] if w == 1 else R).reshape(n, w, 3)
        for k, (X, dX, Xb, dXb) in enumerate(refs):
            e, eb = ws.errors(G[:, :, k], X[:, :w], dX[:, :w]), ws.errors(Gb[:, :, k], Xb[:, :w], dXb[:, :w])
            print(f"batched member {k} nr={w}: gpu_err={max(e.max(), eb.max()):.3e}")
            assert eb.max() <= BOUND, f"member {k} nr={w}, backward-only: entry {np.unravel_index(int(eb.argmax()), eb.shape)}, err {eb.max():.3e}"
            assert e.max() <= BOUND, f"member {k} nr={w}, full solve: entry {np.unravel_index(int(e.argmax()), e.shape)}, err {e.max():.3e}"
    bb.close()
