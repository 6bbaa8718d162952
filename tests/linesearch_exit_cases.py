"""The line-search exits of the Newton loop that no other case reaches (csrc/device_fisher.cpp, csrc/device_batch_fisher.cpp): an
exhausted search (max_linesearch_iter probes without an acceptance: the loop takes x - alpha step with the alpha it ended on, by a
candidate launch of its own), the tiny-step exit (alpha |step|_inf < newton_dec_tol / 1000 after a backtrack: the REJECTED candidate is
kept) and max_linesearch_iter = 0 (the search body never runs). Chosen on the CPU with the restatements (fisher_ref.newton_loop,
fisher_design_ref.newton_loop) on the problems the other loop tests use; each case names the events its float64 trace must contain, per
member for a batch. tests/test_linesearch_exits_host.py asserts them and the selection rule (selected()): the float64 and long-double
restatements take the same alpha trace and the same events, every merit lies fisher_design_ref.MERIT_MARGIN noise floors from its
threshold, every tiny-step comparison a factor 1 +- TINY_MARGIN from its own.

The tiny-step cases set newton_dec_tol = 1000 * 0.1 * |step_1|_inf * 1.5, with |step_1|_inf of the member that is to leave read from the
float64 restatement: the exit then fires after the first backtrack, a factor 1.5 from its threshold. The loop keeps the rejected full
step, so these cases stop after one or two iterates, before the numbers grow (mesh_tiny after one: its second iterate overflows). With
max_linesearch_iter = 0 from x0 = 0 the full step is taken unchecked: matern_ls0 and members 0 and 1 of mixed_ls0 go through x of 2e2
and 8e1, decrements of 1e90 and 1e39; their tolerances follow the scale, as everywhere.

Measured on the CPU, float64 against long-double restatement, max over the decrement trace / over the mode (batches: member by member):
  matern_ls0 2.9e+76 / 1.6e-13   matern_ls1 2.7e-5 / 1.8e-14   matern_ls2 4.7e-10 / 4.9e-16   matern200_tiny 8.5e-5 / 4.5e-14
  matern_sqrt_ls1 3.5e-5 / 2.1e-14   besag9x7_sum0_ls1 9.9e-10 / 1.5e-13   mesh_ls1 9.2e-5 / 1.2e-10   mesh_tiny 1.1e-9 / 2.2e-13
  mixed_ls0 2.9e+76 / 1.6e-13, 3.6e+25 / 1.9e-13, 8.1e-12 / 9.8e-16, 8.5e-5 / 4.6e-14, 1.1e-11 / 1.3e-15
  mixed_ls1 2.7e-5 / 1.8e-14, 1.5e-9 / 6.4e-16, 8.1e-12 / 9.8e-16, 2.6e-10 / 1.5e-15, 1.1e-11 / 1.3e-15
  mixed_ls2 4.7e-10 / 4.9e-16, 1.5e-9 / 6.4e-16, 8.1e-12 / 9.8e-16, 2.6e-10 / 2.3e-15, 1.1e-11 / 1.3e-15
  mixed_three_exits 2.7e-5 / 1.8e-14, 1.5e-9 / 1.4e-14, 8.1e-12 / 6.9e-16, 8.5e-5 / 4.5e-14, 1.1e-11 / 1.4e-15
  mesh_ls2 1.1e-9 / 7.3e-15, 6.0e-10 / 2.2e-15, 8.6e-12 / 1.3e-15, 2.6e-11 / 1.1e-15
  besag_ls2 5.7e-9 / 1.6e-15, 2.1e-9 / 3.3e-15, 2.4e-9 / 7.4e-16, 2.8e-10 / 3.4e-15, 3.1e-11 / 1.7e-15
(the large absolute figures belong to decrements of 1e10 and more: relative to the trace's largest entry none exceeds 2e-14)"""
import numpy as np

import batch_con_laplace_cases as bcl
import batch_design_cases as bdc
import batch_laplace_cases as bc
import fisher_design_ref as dref
import fisher_loop_cases as lc
import fisher_ref as ref

TINY_MARGIN = 1e-6
EXITS = {"linesearch_exhausted", "tiny_step_exit"}


def tiny_tol(step_inf):
    """newton_dec_tol at which a member of that full-step norm leaves after its first backtrack, a factor 1.5 inside the threshold"""
    return 1000 * 0.1 * step_inf * 1.5


ONE_FULL_STEP = dict(max_iter=1, adaptive=False, predictive=False, mean_tol=0.0, dec_tol=0.0)       # from x0 = 0: x_1 = -step_1


def plain_cases():
    """name -> dict(form 'node' | 'design', Q, obs, x0, A (constraint or None), base (the design case) or None, kw (the restatement's
    keywords), events)"""
    base = lc.cases()
    mat, besag = base["matern_far0"], base["besag9x7_sum0"]
    out = {}
    for ls, ev in ((0, {"linesearch_exhausted"}), (1, {"backtrack", "linesearch_exhausted"}), (2, {"backtrack", "linesearch_exhausted"})):
        out[f"matern_ls{ls}"] = dict(form="node", Q=mat["Q"], obs=mat["obs"], x0=None, A=None, kw=dict(max_iter=7, max_ls=ls), events=ev)
    # member 3 of batch_laplace_cases' mixed: 200 M, |step_1|_inf = 20.5
    Q3 = bc.shifted(mat["Q"], *bc.MIXED_SC[3])
    s3 = float(np.abs(ref.newton_loop(lc.dense(Q3), None, mat["obs"], **ONE_FULL_STEP)["x"]).max())
    out["matern200_tiny"] = dict(form="node", Q=Q3, obs=mat["obs"], x0=None, A=None, kw=dict(max_iter=2, dec_tol=tiny_tol(s3)),
                                 events={"backtrack", "tiny_step_exit"})
    out["matern_sqrt_ls1"] = dict(form="node", Q=mat["Q"], obs=mat["obs"], x0=None, A=None, kw=dict(max_iter=7, max_ls=1, retry_full=False),
                                  events={"backtrack", "linesearch_exhausted"})
    out["besag9x7_sum0_ls1"] = dict(form="node", Q=besag["Q"], obs=besag["obs"], x0=None, A=besag["A"], kw=dict(max_iter=7, max_ls=1),
                                    events={"backtrack", "linesearch_exhausted"})
    mesh = dref.loop_cases()["mesh_far0"]
    out["mesh_ls1"] = dict(form="design", base=mesh, Q=mesh["Q"], obs=mesh["obs"], x0=None, A=None, kw=dict(max_iter=7, max_ls=1),
                           events={"backtrack", "linesearch_exhausted"})
    sm = float(np.abs(_restate_design(mesh, np.float64, ONE_FULL_STEP)["x"]).max())
    out["mesh_tiny"] = dict(form="design", base=mesh, Q=mesh["Q"], obs=mesh["obs"], x0=None, A=None, kw=dict(max_iter=1, dec_tol=tiny_tol(sm)),
                            events={"backtrack", "tiny_step_exit"})
    return out


def _restate_design(base, dtype, kw):
    D = base["Q"].toarray()
    S = np.triu(D) + np.triu(D, 1).T
    return dref.newton_loop(S, None, base["obs"], base["A"].toarray(), b=base["b"], x0=base["x0"], A=base["C"], dtype=dtype, **kw)


def restate_plain(c, dtype):
    if c["form"] == "design":
        return _restate_design(c["base"], dtype, c["kw"])
    return ref.newton_loop(lc.dense(c["Q"]), None, c["obs"], x0=c["x0"], A=c["A"], dtype=dtype, **c["kw"])


def batch_cases():
    """name -> dict(kind 'node' | 'design' | 'con', c (a case of the kind's module with this case's kw), events (one set per member))"""
    mixed = bc.loop_cases()["mixed"]
    ex, bt, tiny = "linesearch_exhausted", "backtrack", "tiny_step_exit"
    out = {
        "mixed_ls0": dict(kind="node", c=dict(mixed, kw=dict(max_iter=7, max_ls=0)), events=[{ex}, {ex}, {ex, "frozen_return"}, {ex}, {ex, "lookahead_reject"}]),
        "mixed_ls1": dict(kind="node", c=dict(mixed, kw=dict(max_iter=7, max_ls=1)),
                          events=[{bt, ex}, {bt, ex}, set(), {bt, ex, "retry_full_reject"}, set()]),
        "mixed_ls2": dict(kind="node", c=dict(mixed, kw=dict(max_iter=7, max_ls=2)), events=[{bt, ex}, {bt}, set(), {bt}, set()]),
    }
    # one iterate, three exits: member 3 (|step_1|_inf = 20.5) leaves by the tiny-step test after its first backtrack, members 0 and 1
    # (207.8, 89.9) are above it and exhaust max_linesearch_iter = 1, members 2 and 4 accept the full step
    s3 = float(np.abs(bc.restate(dict(mixed, kw=ONE_FULL_STEP), 3, np.float64)["x"]).max())
    out["mixed_three_exits"] = dict(kind="node", c=dict(mixed, kw=dict(max_iter=2, max_ls=1, dec_tol=tiny_tol(s3))),
                                    events=[{bt, ex}, {bt, ex}, set(), {bt, tiny}, set()])
    mesh = bdc.loop_cases()["mesh_far0"]
    out["mesh_ls2"] = dict(kind="design", c=dict(mesh, kw=dict(max_iter=7, max_ls=2)), events=[{bt, ex}, {bt}, set(), {bt}])
    besag = bcl.cases()["besag"]
    out["besag_ls2"] = dict(kind="con", c=dict(besag, kw=dict(max_iter=7, max_ls=2)), events=[{bt, ex}, {bt, ex}, {bt, ex}, {bt}, set()])
    return out


_RESTATE = {"node": bc.restate, "design": bdc.restate, "con": bcl.restate}


def restate_member(case, k, dtype):
    return _RESTATE[case["kind"]](case["c"], k, dtype)


_RUNS = {}


def restated(name):
    """[(float64 run, long-double run)] of the case of that name, one pair per member (a plain case: one pair); computed once"""
    if name not in _RUNS:
        P, B = plain_cases(), batch_cases()
        if name in P:
            _RUNS[name] = [(restate_plain(P[name], np.float64), restate_plain(P[name], ref.LD))]
        else:
            _RUNS[name] = [(restate_member(B[name], k, np.float64), restate_member(B[name], k, ref.LD)) for k in range(len(B[name]["events"]))]
    return _RUNS[name]


def selected(a, b):
    """the selection rule on the float64 run a and the long-double run b of one loop"""
    same = np.array_equal(a["alpha_trace"], b["alpha_trace"]) and a["events"] == b["events"] and a["iterations"] == b["iterations"]
    merit = all(dist >= dref.MERIT_MARGIN * scale for r in (a, b) for kind, dist, scale in r["margins"] if kind == "merit")
    tiny = all(v < t * (1 - TINY_MARGIN) or v > t * (1 + TINY_MARGIN) for r in (a, b) for v, t in r["tiny"])
    return same and merit and tiny


def forest_totals(runs):
    """(factorisations, solves, evaluations) of the lockstep loop over the members whose restatement runs are given: an iterate is one
    evaluation and one factorise-and-solve for everybody still running, one round for the full-step retry if anybody takes it, as
    many search rounds as the longest search, and the chord steps of the look-ahead (an evaluation and a solve each: three if any
    member's is accepted, one if all are rejected); one evaluation at the modes ends the call"""
    fact = max(len(r["rounds"]) for r in runs)
    solves = evals = 0
    for i in range(fact):
        rd = [r["rounds"][i] for r in runs if len(r["rounds"]) > i]
        chord = max(c for _, _, c in rd)
        solves += 1 + chord
        evals += 1 + max(f for f, _, _ in rd) + max(p for _, p, _ in rd) + chord
    return fact, solves, evals + 1


def gaps(a, b):
    """(decrement trace, mode): the float64 run's largest distance from the long-double run"""
    return (float(np.abs(np.asarray(a["dec_trace"], ref.LD) - b["dec_trace"]).max()) if len(a["dec_trace"]) else 0.0,
            float(np.abs(np.asarray(a["x"], ref.LD) - b["x"]).max()))
