#!/usr/bin/env python3
"""A/B of the Laplace path between two builds of the library, alternating in ONE process (gmrfx/_lib.py: load_from / use): the sweeps of
tools/batch_ga_bench.py -- node form, --design and --constraint, the batched route and the plain route on one handle -- and one plain
evaluation (gmrfx_fisher_eval_dev) at n = nobs = --eval-grid^2 in node and design form. `--rounds` medians per side and call, each the
median of `--reps` synchronised calls after `--warmup`, the sides in alternating order. The rule the result is read by: every new
median lies inside the old build's own min .. max. Also compared: the bits of the modes (loops) and of score and Hessian (evaluations).

ONE FORM PER PROCESS (--forms), and both orders of creation (--old-first), for figures that are meant to be compared. Measured with this
tool: from the second form of a process on, the side whose handles are created first runs its plain sweeps 1.75
times slower and its batched ones 5 - 19 % slower, whichever build it is (the new build against a copy of itself in a fresh process
shows no difference); a single evaluation is 0.4 - 3.5 % slower for the side created second, even in a fresh process.

usage: tools/laplace_ab.py --old PATH/TO/libgmrfx.so [--what loops|evals|all] [--forms node,design,constraint] [--old-first] [--grid 100]
                           [--batch 50] [--eval-grid 1000] [--rounds 4] [--reps 9] [--warmup 2] [--out profiles/laplace_refactor_ab.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

import batch_ga_bench as bg  # noqa: E402
import gmrfx  # noqa: E402
from gmrfx import _lib, spde  # noqa: E402


def loop_problem(form, g, B):
    """(first member, values (nnz, B), coords, batched-handle keywords, set-up of either kind of handle, per-member set-up of the plain one)"""
    rng = np.random.default_rng(g)
    if form == "design":
        Qs, pts, A, y = bg.design_problem(g, B, rng)
        return Qs, pts, dict(ordering=gmrfx.PinDenseColumns()), lambda h: h.set_design_observations("poisson", y, A), None
    if form == "constraint":
        M = bg.torus_besag(g)
        n = M.shape[0]
        taus = np.exp(rng.uniform(np.log(0.2), np.log(20.0), B))
        z = rng.standard_normal(n)
        y, aux = rng.poisson(20.0 * np.exp(z - z.mean())).astype(float), np.full(n, np.log(20.0))
        pts = np.stack(np.meshgrid(np.arange(g, dtype=float), np.arange(g, dtype=float), indexing="ij"), axis=-1).reshape(n, 2)

        def setup(h):
            h.set_observations("poisson", y, aux=aux)
            h.set_constraints(sp.csr_matrix(np.ones((1, n))), np.zeros(1))
        return [sp.csc_matrix((t * M.data, M.indices, M.indptr), shape=M.shape) for t in taus], pts, {}, setup, None
    Qs, pts = bg.members(g, B, rng)
    y = np.random.default_rng(1).poisson(20.0, Qs[0].shape[0]).astype(float)
    return Qs, pts, {}, lambda h: h.set_observations("poisson", y), lambda h: h.set_observations("poisson", y)


def loop_calls(form, a, libs):
    """per side: {call name: closure}, the closures' output arrays, the handles to close"""
    B = a.batch
    Qs, pts, bkw, setup, per_member = loop_problem(form, a.grid, B)
    n = Qs[0].shape[0]
    NZ = np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))
    dX0 = torch.zeros(n * B, dtype=torch.float64, device="cuda:0")
    calls, outs, handles = {}, {}, {}
    for tag, L in libs.items():
        _lib.use(L)
        bb = gmrfx.MI355XBatchLaplace(Qs[0], B, coords=pts, device=0, **bkw)
        setup(bb)
        plain = gmrfx.MI355XBackend(Qs[0], ordering=bb.ordering_permutation(), device=0, factorize=False)
        setup(plain)
        hmap = plain.observations_hess_map() if form == "design" else bg.diag_positions(Qs[0])
        dXb = torch.empty(n * B, dtype=torch.float64, device="cuda:0")
        dXs = torch.empty(n * B, dtype=torch.float64, device="cuda:0")

        def batched(bb=bb, dXb=dXb):
            bb.set_prior(NZ)
            bb.gaussian_approximation_dev(dXb.data_ptr(), n, d_x0=dX0.data_ptr(), sx0=n, refactorize_final=True)

        def sequential(plain=plain, dXs=dXs, hmap=hmap):
            for k in range(B):
                plain.set_prior(NZ[:, k], hmap)
                if per_member:
                    per_member(plain)
                plain.gaussian_approximation_dev(dXs.data_ptr() + 8 * k * n, d_x0=dX0.data_ptr(), refactorize_final=True)
        calls[tag] = {f"{form}: batched sweep": batched, f"{form}: plain handle, sequential sweep": sequential}
        outs[tag] = [dXb, dXs]
        handles[tag] = [bb, plain]
    return calls, outs, handles


def eval_calls(form, a, libs):
    g = a.eval_grid
    rng = np.random.default_rng(0)
    mesh = spde.grid_mesh_2d(g, g, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.3))
    Q.sort_indices()
    n = Q.shape[0]
    y, aux = rng.poisson(3.0, n).astype(float), rng.uniform(-0.5, 0.5, n)
    if form == "design":
        cells = np.asarray(mesh.cells)
        tri = cells[rng.integers(0, cells.shape[0], n)]
        A = sp.csr_matrix((rng.dirichlet(np.ones(3), n).ravel(), (np.repeat(np.arange(n), 3), tri.ravel())), shape=(n, n))
        A.sum_duplicates()
    dev = torch.device("cuda:0")
    dx, dm = torch.from_numpy(0.3 * rng.standard_normal(n)).to(dev), torch.from_numpy(0.1 * rng.standard_normal(n)).to(dev)
    calls, outs, handles = {}, {}, {}
    for tag, L in libs.items():
        _lib.use(L)
        be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
        if form == "design":
            be.set_design_observations("poisson", y, A, aux=aux)
            hmap = be.observations_hess_map()
        else:
            be.set_observations("poisson", y, aux=aux)
            hmap = bg.diag_positions(Q)
        be.set_prior(Q.data, hmap)
        ds = torch.empty(n, dtype=torch.float64, device=dev)
        dh = torch.empty(len(hmap), dtype=torch.float64, device=dev)
        pair = torch.empty(2, dtype=torch.float64)      # (energy, loglik) of the last call, on the host: nothing else is timed

        def call(be=be, ds=ds, dh=dh, pair=pair):
            pair[0], pair[1] = be.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())
        calls[tag] = {f"{form}: gmrfx_fisher_eval_dev, n = nobs = {n}": call}
        outs[tag] = [ds, dh, pair]
        handles[tag] = [be]
    return calls, outs, handles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True)
    ap.add_argument("--what", default="all", choices=["loops", "evals", "all"])
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--eval-grid", type=int, default=1000)
    ap.add_argument("--forms", default="node,design,constraint")
    ap.add_argument("--old-first", action="store_true", help="create the old build's handles first (the order of creation is part of what a handle's time depends on)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laplace_refactor_ab.json"))
    a = ap.parse_args()
    libs = {"new": _lib.lib(), "old": _lib.load_from(a.old)}
    if a.old_first:
        libs = {"old": libs["old"], "new": libs["new"]}
    forms = a.forms.split(",")
    groups = [(loop_calls, f) for f in forms] if a.what != "evals" else []
    groups += [(eval_calls, f) for f in forms if f != "constraint"] if a.what != "loops" else []
    rows = []
    for build, form in groups:
        calls, outs, handles = build(form, a, libs)
        medians = {name: {"old": [], "new": []} for name in calls["new"]}
        for r in range(a.rounds):
            for tag in (("old", "new") if r % 2 == 0 else ("new", "old")):
                _lib.use(libs[tag])
                for name, fn in calls[tag].items():
                    medians[name][tag].append(bg.timed(fn, a.reps, a.warmup)["median_ms"])
        same = all(np.array_equal(p.cpu().numpy().view(np.int64), q.cpu().numpy().view(np.int64)) for p, q in zip(outs["old"], outs["new"]))
        for name, md in medians.items():
            old, new = md["old"], md["new"]
            rows.append({"call": name, "old_median_ms": old, "new_median_ms": new, "old_min_ms": min(old), "old_max_ms": max(old),
                         "inside_old_min_max": bool(min(old) <= min(new) and max(new) <= max(old)),
                         "not_above_old_max": bool(max(new) <= max(old)), "same_bits": bool(same)})
            print(json.dumps(rows[-1]), flush=True)
        for tag, hs in handles.items():
            _lib.use(libs[tag])
            for h in hs:
                h.close()
    _lib.use(libs["new"])
    res = {"tool": "tools/laplace_ab.py --old", "device": torch.cuda.get_device_name(0), "source_tree_hash": _lib.source_tree_hash(),
           "created_first": "old" if a.old_first else "new", "grid": a.grid, "B": a.batch, "eval_grid": a.eval_grid, "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
