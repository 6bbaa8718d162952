"""The SYRK time of a factorisation comes from device wall-clock stamps of the SYRK kernels' own workgroups, not from events on the
factorisation's stream (run with -m gpu on an MI355X).

That does not change what is computed: the factor, the solutions and the log-determinant keep their bits from step to step and
between the pipelined call (refactorize_solve_dev) and the separate calls (refactorize_dev + solve_dev), and agree with the CPU
oracle to 1e-10. Two meshes: a jittered 70 x 70 2-D grid created under GMRFX_SYRK_PIPED=48 (seven levels of big fronts with
trailing rows, three on k_syrk_cb_rec<false>, four on k_syrk_cb_rec<true>) and a 14^3 3-D grid at the defaults (six such levels,
both instantiations, the two fronts below the root on two panel chains); test_the_meshes_reach_what_they_are_for checks that
against the restated plan of tests/factor_shapes.py.

gmrfx_stats.ms_syrk stays a time: positive, at most ms_factor (the first stamp is taken behind the factorisation's first event,
the last one before its last), reset by every factorisation (a value that survived from the factorisation before would span the
host time between the two and exceed ms_factor), per handle, 0 where there is nothing to time, the same when read twice.
"""
import functools

import numpy as np
import pytest

import gmrfx
import orc
from gmrfx import spde
import sweep_shapes as ws
import factor_shapes as fs

pytestmark = pytest.mark.gpu

TOL = 1e-10
NRHS = 7
CASES = {"2d": {"GMRFX_SYRK_PIPED": "48"}, "3d": {}}


@functools.lru_cache(maxsize=None)
def _problem(name):
    if name == "2d":
        mesh = spde.grid_mesh_2d(70, 70, jitter=0.25, seed=3)
        Q = spde.matern_precision(mesh, smoothness=0, range_=0.3)
    elif name == "3d":
        mesh = spde.grid_mesh_3d(14, 14, 14)
        Q = spde.matern_precision(mesh, 0, 0.4)
    elif name == "small":         # big fronts, far fewer of them
        mesh = spde.grid_mesh_2d(24, 24, jitter=0.25, seed=5)
        Q = spde.matern_precision(mesh, smoothness=0, range_=0.3)
    else:                         # "tiny": no big front at all
        mesh = spde.grid_mesh_2d(8, 8, jitter=0.25, seed=3)
        Q = spde.matern_precision(mesh, smoothness=0, range_=0.3)
    B = np.random.default_rng(11).standard_normal((NRHS, Q.shape[0]))      # row j = column j of the n x NRHS right-hand sides
    return mesh, Q, B


_oracle_cache = {}


def _oracle(name, perm):
    """The CPU oracle's factor, solutions and log-determinant of a case: computed once, shared, never changed."""
    hit = _oracle_cache.get(name)
    if hit is None:
        _, Q, B = _problem(name)
        F = orc.OracleFactor(Q, perm)
        hit = _oracle_cache[name] = {"perm": perm.copy(), "L": F.L().tocsc(), "X": F.solve(B.T.copy()), "logdet": F.logdet()}
    assert np.array_equal(hit["perm"], perm)
    return hit


def _handle(name, monkeypatch, **kw):
    for k, v in CASES.get(name, {}).items():
        monkeypatch.setenv(k, v)
    mesh, Q, _ = _problem(name)
    return gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, **kw)


def _levels(be, name):
    """the levels of the restated plan that launch a SYRK: big fronts with trailing rows"""
    k = fs.knobs(CASES.get(name, {}))
    lv, _ = fs.factor_levels(ws.fronts(be), k)
    return [L for _, L in sorted(lv.items()) if L.big and L.max_trail > 0], k


def _device_arrays(name):
    import torch
    _, Q, B = _problem(name)
    dev = torch.device("cuda", 0)
    d_nz = torch.from_numpy(np.ascontiguousarray(Q.data)).to(dev)
    d_B = torch.from_numpy(B).to(dev)
    d_X = torch.zeros_like(d_B)
    torch.cuda.synchronize()
    return d_nz, d_B, d_X


@pytest.mark.parametrize("name", list(CASES))
def test_the_meshes_reach_what_they_are_for(name, monkeypatch):
    be = _handle(name, monkeypatch, symbolic_only=True)
    lv, k = _levels(be, name)
    kernels = {v for L in lv for v in fs.choose_syrk(L, k)}
    assert {"k_syrk_cb_rec<true>", "k_syrk_cb_rec<false>"} <= kernels and len(lv) >= 6, (len(lv), kernels)
    if name == "3d":
        assert any(fs.two_chains(L) for L in lv)
    be.close()


@pytest.mark.parametrize("name", list(CASES))
def test_bits_are_unchanged(name, monkeypatch):
    """factor, X and logdet: the same bits on two consecutive pipelined steps, on two consecutive separate steps and between the
    two forms; each against the oracle"""
    import torch
    be = _handle(name, monkeypatch)             # (the first factorisation decides the inverse cap: the pipelined call pipelines from now on)
    assert be.last_info == 0
    n = be.n
    d_nz, d_B, d_X = _device_arrays(name)
    got = []
    for form in ("pipelined", "pipelined", "separate", "separate"):
        d_X.zero_()
        torch.cuda.synchronize()
        if form == "pipelined":
            assert be.refactorize_solve_dev(d_nz.data_ptr(), d_B.data_ptr(), n, NRHS, d_X.data_ptr(), n) == 0
        else:
            assert be.refactorize_dev(d_nz.data_ptr()) == 0
            be.solve_dev(d_B.data_ptr(), n, NRHS, d_X.data_ptr(), n)
        torch.cuda.synchronize()
        got.append((form, be.factor_values(), d_X.cpu().numpy().copy(), be.compute_logdet()))
    form0, L0, X0, ld0 = got[0]
    for form, L, X, ld in got[1:]:
        assert np.array_equal(L, L0), f"{name}: the factor of a {form} step differs from the first {form0} step's"
        assert np.array_equal(X, X0), f"{name}: X of a {form} step differs from the first {form0} step's"
        assert ld == ld0, f"{name}: logdet of a {form} step differs from the first {form0} step's"
    ref = _oracle(name, be.ordering_permutation())
    eL = abs(be.factor_csc() - ref["L"]).max() / abs(ref["L"]).max()
    eX = np.abs(X0.T - ref["X"]).max() / np.abs(ref["X"]).max()
    eld = abs(ld0 - ref["logdet"]) / abs(ref["logdet"])
    print(f"{name}: n={n} factor_err={eL:.2e} solve_err={eX:.2e} logdet_err={eld:.2e}")
    assert eL <= TOL and eX <= TOL and eld <= TOL
    be.close()


def _check_time(st, launches, tag):
    print(f"{tag}: ms_syrk={st['ms_syrk']:.4f} ms_factor={st['ms_factor']:.4f} syrk_launches={st['syrk_launches']}")
    assert st["syrk_launches"] == launches, tag
    assert 0 < st["ms_syrk"] <= st["ms_factor"], tag


@pytest.mark.parametrize("name", list(CASES))
def test_ms_syrk_is_a_time_reset_by_every_factorisation(name, monkeypatch):
    be = _handle(name, monkeypatch, factorize=False)
    st = be.stats()
    assert st["ms_syrk"] == 0 and st["syrk_launches"] == 0, "before the first factorisation"
    launches = len(_levels(be, name)[0])
    _, Q, _ = _problem(name)
    be.refactorize_values(Q.data)
    first = be.stats()
    _check_time(first, launches, f"{name}: first factorisation")
    assert be.stats()["ms_syrk"] == first["ms_syrk"], "read twice without a factorisation in between"
    # a much smaller handle in between: a time of its own, and nothing of it shows in the first handle
    small = _handle("small", monkeypatch)
    ss_ = small.stats()
    _check_time(ss_, len(_levels(small, "small")[0]), "small handle")
    assert be.stats()["ms_syrk"] == first["ms_syrk"], "the other handle's factorisation changed this handle's value"
    be.refactorize_values(Q.data)
    _check_time(be.stats(), launches, f"{name}: second factorisation")
    assert small.stats()["ms_syrk"] == ss_["ms_syrk"]
    # the pipelined call times its launches the same way
    import torch
    d_nz, d_B, d_X = _device_arrays(name)
    assert be.refactorize_solve_dev(d_nz.data_ptr(), d_B.data_ptr(), be.n, NRHS, d_X.data_ptr(), be.n) == 0
    _check_time(be.stats(), launches, f"{name}: pipelined step")
    torch.cuda.synchronize()
    small.close()
    be.close()


def test_no_big_front_no_time(monkeypatch):
    be = _handle("tiny", monkeypatch)
    assert be.last_info == 0 and not _levels(be, "tiny")[0]
    st = be.stats()
    assert st["ms_syrk"] == 0 and st["syrk_launches"] == 0 and st["ms_factor"] > 0
    be.close()


def test_one_rank_sharded_handle_times_its_phases(monkeypatch):
    """shard_world = 1 with a forced top: the phase entry points; the slots accumulate over the phases"""
    import torch
    be = _handle("2d", monkeypatch, factorize=False, shard_rank=0, shard_world=1, shard_min_top=3)
    info = be.shard_info()
    assert info["n_top_levels"] >= 2
    d_nz, _, _ = _device_arrays("2d")
    seen = []
    for _ in range(2):
        for phase in range(1 + info["n_top_levels"]):
            be.refactorize_phase_dev(d_nz.data_ptr(), phase)
        st = be.stats()
        assert st["fail_col"] == -1
        print(f"sharded: ms_syrk={st['ms_syrk']:.4f} ms_factor={st['ms_factor']:.4f} syrk_launches={st['syrk_launches']}")
        assert st["syrk_launches"] > 0 and 0 < st["ms_syrk"] <= st["ms_factor"]
        assert be.stats()["ms_syrk"] == st["ms_syrk"]
        seen.append(st["syrk_launches"])
    assert seen[0] == seen[1]
    torch.cuda.synchronize()
    be.close()


def test_batched_handle_times_its_launches():
    _, Q, _ = _problem("small")
    bb = gmrfx.MI355XBatchBackend(Q, 3, device=0)
    assert bb.stats()["ms_syrk"] == 0
    NZ = np.stack([Q.data, 1.5 * Q.data, 2.0 * Q.data], axis=1)
    for _ in range(2):
        assert not bb.refactorize_values(NZ).any()
        st = bb.stats()
        print(f"batched: ms_syrk={st['ms_syrk']:.4f} ms_factor={st['ms_factor']:.4f} syrk_launches={st['syrk_launches']}")
        assert st["syrk_launches"] > 0 and 0 < st["ms_syrk"] <= st["ms_factor"]
    bb.close()
