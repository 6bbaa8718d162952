"""The cases of tests/linesearch_exit_cases.py do what their names say, on the CPU: every case (every member of a batch) reaches the
events it names in its float64 restatement and keeps the selection rule; together they reach both exits in every form of the loop; the
counts the issue's table gives for the `mixed` batch hold; and no case the other loop tests use reaches either exit (which is why
these exist)."""
import numpy as np
import pytest

import batch_laplace_cases as bc
import fisher_loop_cases as lc
import linesearch_exit_cases as le

PLAIN, BATCH = le.plain_cases(), le.batch_cases()
EX, TINY, BT = "linesearch_exhausted", "tiny_step_exit", "backtrack"


@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_cases_reach_their_events_and_keep_the_margins(name):
    (a, b), = le.restated(name)
    assert PLAIN[name]["events"] <= set(a["events"]), a["events"]
    assert le.EXITS & set(a["events"])
    assert le.selected(a, b)
    gd, gx = le.gaps(a, b)
    print(f"{name}: float64-vs-long-double dec {gd:.1e} x {gx:.1e}; events {a['events']}")


@pytest.mark.parametrize("name", list(BATCH))
def test_batch_cases_reach_their_events_and_keep_the_margins(name):
    c = BATCH[name]
    assert len(c["events"]) == len(c["c"]["Qs"])
    for k, (a, b) in enumerate(le.restated(name)):
        assert c["events"][k] <= set(a["events"]), (k, a["events"])
        assert le.selected(a, b), k
        gd, gx = le.gaps(a, b)
        print(f"{name}[{k}]: float64-vs-long-double dec {gd:.1e} x {gx:.1e}; events {a['events']}")
    first = [a["alpha_trace"][0] for a, _ in le.restated(name)]
    exits = [le.EXITS & set(a["events"]) for a, _ in le.restated(name)]
    # a member that exhausts (or leaves by the tiny-step test) sits beside one that accepts, in iterate 1
    if c["c"]["kw"].get("max_ls") != 0:
        assert any(exits) and any(not e and f == 1.0 for e, f in zip(exits, first))


def test_every_form_reaches_what_the_issue_asks_for():
    ev = {n: set(le.restated(n)[0][0]["events"]) for n in PLAIN}
    node = [n for n in PLAIN if PLAIN[n]["form"] == "node"]
    design = [n for n in PLAIN if PLAIN[n]["form"] == "design"]
    for names in (node, design):
        assert any(EX in ev[n] for n in names) and any(TINY in ev[n] for n in names)
    assert {PLAIN[f"matern_ls{k}"]["kw"]["max_ls"] for k in (0, 1, 2)} == {0, 1, 2}
    assert PLAIN["matern_sqrt_ls1"]["kw"]["retry_full"] is False and EX in ev["matern_sqrt_ls1"]
    assert PLAIN["besag9x7_sum0_ls1"]["A"] is not None and EX in ev["besag9x7_sum0_ls1"]
    assert {BATCH[n]["kind"] for n in BATCH} == {"node", "design", "con"}
    # max_linesearch_iter = 0: no merit is ever evaluated, every iterate ends exhausted
    a = le.restated("matern_ls0")[0][0]
    assert a["merit_evaluations"] == 0 and a["events"].count(EX) == a["iterations"] and (a["alpha_trace"] == 1.0).all()
    # the tiny-step cases keep the REJECTED full step: alpha = 0.1 is recorded, x_1 = x0 - step
    for n in ("matern200_tiny", "mesh_tiny"):
        a = le.restated(n)[0][0]
        assert a["events"][:2] == [BT, TINY] and a["alpha_trace"][0] == 0.1 and len(a["tiny"]) >= 1
        v, t = a["tiny"][0]
        assert abs(v / t - 1 / 1.5) < 1e-12


def test_the_mixed_batch_does_what_the_table_says():
    r0, r1, r2 = (le.restated(f"mixed_ls{k}") for k in (0, 1, 2))
    # 0: every member exhausts at every iterate without a merit evaluation; member 2 ends in a frozen finish, member 4's look-ahead is rejected
    for a, _ in r0:
        searched = a["iterations"] - (1 if a["frozen"] else 0)
        assert a["merit_evaluations"] == 0 and a["events"].count(EX) == searched
    assert r0[2][0]["frozen"] and "lookahead_reject" in r0[4][0]["events"]
    # 1: members 0, 1 and 3 backtrack once and exhaust in iterate 1, members 2 and 4 accept; member 3 then sees retry_full_reject twice
    for k in (0, 1, 3):
        assert r1[k][0]["events"][:2] == [BT, EX] and r1[k][0]["alpha_trace"][0] == 0.1
    for k in (2, 4):
        assert not le.EXITS & set(r1[k][0]["events"]) and r1[k][0]["alpha_trace"][0] == 1.0
    assert r1[3][0]["events"].count("retry_full_reject") == 2
    # 2: member 0 exhausts after two backtracks, members 1 and 3 accept after one
    assert r2[0][0]["events"][:3] == [BT, BT, EX] and r2[0][0]["alpha_trace"][0] == 0.1 * 0.1
    for k in (1, 3):
        assert r2[k][0]["events"][0] == BT and EX not in r2[k][0]["events"] and r2[k][0]["alpha_trace"][0] == np.sqrt(0.1)


def test_three_exits_in_one_iterate():
    runs = [a for a, _ in le.restated("mixed_three_exits")]
    assert runs[3]["events"][:2] == [BT, TINY] and runs[3]["alpha_trace"][0] == 0.1
    for k in (0, 1):
        assert runs[k]["events"][:2] == [BT, EX] and runs[k]["alpha_trace"][0] == 0.1
        assert runs[k]["tiny"][0][0] > runs[k]["tiny"][0][1]          # above the threshold member 3 is under: their steps are longer
    for k in (2, 4):
        assert runs[k]["alpha_trace"][0] == 1.0 and not le.EXITS & set(runs[k]["events"])


def test_no_existing_node_form_case_reaches_either_exit():
    for name, c in lc.cases().items():
        assert not le.EXITS & set(lc.restate(c, np.float64)["events"]), name
    mixed = bc.loop_cases()["mixed"]
    for k in range(5):
        assert not le.EXITS & set(bc.restate(mixed, k, np.float64)["events"]), k
