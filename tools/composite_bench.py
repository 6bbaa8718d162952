#!/usr/bin/env python3
"""The evaluation of a Fisher-scoring iterate for a composite likelihood (gmrfx_obs_set_composite) beside the single-family design form
on the same design matrix, and the whole loop.

Problem: the benchmark's cfg 2 (a --grid x --grid jittered 2-D Matern mesh, default 1000: n = 10^6), every node observed once through a
selection row (n = nobs), the first half of the rows a Normal component (sigma 1), the second half a Poisson component with log
exposure. Reported, milliseconds, median (and minimum, and the spread max - min) over --reps repetitions after --warmup, wall clock
with the GPU synchronised around the timed region:
  eval_composite    one gmrfx_fisher_eval_dev of the composite (k_design_eta_comp: one byte per row and the component table beside
                    what the single-family row pass reads)
  eval_single       one gmrfx_fisher_eval_dev of the design form on the same A, every row Poisson (k_design_eta)
  loop_composite    one gmrfx_gaussian_approximation_dev of the composite from x0 = 0, with its iteration count
The two evaluations run in this order and then once more in the other order (eval_single_2, eval_composite_2): a difference that
changes sign with the order is the run's noise. No time is a pass criterion.
usage: tools/composite_bench.py [--grid 1000] [--reps 15] [--warmup 3] [--out profiles/composite_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

import gmrfx  # noqa: E402
from gmrfx import _lib, spde  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = 1e3 * np.asarray(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "spread_ms": float(ts.max() - ts.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_bench.json"))
    a = ap.parse_args()
    mesh = spde.grid_mesh_2d(a.grid, a.grid, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.2))
    Q = sp.csc_matrix((Q + Q.T) * 0.5)
    Q.sort_indices()
    n = Q.shape[0]
    half = n // 2
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    y = np.r_[rng.standard_normal(half), rng.poisson(3.0, n - half).astype(float)]
    aux = rng.uniform(-0.5, 0.5, n)
    A = sp.identity(n, format="csr")
    x, mu = 0.3 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    dx, dm = torch.from_numpy(x).to(dev), torch.from_numpy(mu).to(dev)
    ds, dxo = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    res = {"n": n, "nobs": n, "components": ["normal", "poisson"], "rows": [half, n - half], "reps": a.reps, "warmup": a.warmup,
           "source_tree_hash": _lib.source_tree_hash()}

    def backend(composite):
        be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
        if composite:
            comp = gmrfx.CompositeObservations(n)
            comp.add("normal", y[:half], indices=np.arange(half), param=1.0)
            comp.add("poisson", y[half:], indices=np.arange(half, n), aux=aux[half:])
            gmrfx.set_composite_observations(be, comp)
        else:
            be.set_design_observations("poisson", np.abs(np.rint(y)), A, aux=aux)
        be.set_prior(Q.data, be.observations_hess_map())
        return be

    bc, bs = backend(True), backend(False)
    cnt = bc.observations_design_info()["cnt"]
    assert cnt == bs.observations_design_info()["cnt"]
    dh = torch.empty(cnt, dtype=torch.float64, device=dev)

    def eval_composite():
        bc.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())

    def eval_single():
        bs.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())

    info = {}

    def loop_composite():
        info.update(bc.gaussian_approximation_dev(dxo.data_ptr(), dh.data_ptr()))

    for name, fn in (("eval_composite", eval_composite), ("eval_single", eval_single), ("eval_single_2", eval_single),
                     ("eval_composite_2", eval_composite), ("loop_composite", loop_composite)):
        res[name] = timed(fn, a.reps, a.warmup)
    res["loop_iterations"] = int(info["iterations"])
    res["loop_converged"] = bool(info["converged"])
    res["loop_factorizations"] = int(info["factorizations"])
    res["composite_over_single"] = res["eval_composite"]["median_ms"] / res["eval_single"]["median_ms"]
    res["composite_over_single_2"] = res["eval_composite_2"]["median_ms"] / res["eval_single_2"]["median_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
