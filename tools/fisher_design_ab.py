"""A/B of the plain design-form evaluation between two builds of the library, alternating in ONE process (the method behind
profiles/fisher_kernels_ab.json): gmrfx_fisher_eval_dev in design form at the design configuration of tools/fisher_bench.py (a
grid x grid mesh, --nobs point observations with three barycentric weights each, Poisson), `--rounds` medians per side, each the median
of `--reps` synchronised calls after `--warmup`. Writes both sets of medians to profiles/fisher_design_kernels_ab.json.

usage: tools/fisher_design_ab.py --old PATH/TO/libgmrfx.so [--grid 1000] [--nobs 1000000] [--rounds 4] [--reps 15] [--warmup 3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--nobs", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisher_design_kernels_ab.json"))
    a = ap.parse_args()
    libs = {"new": _lib.lib(), "old": _lib.load_from(a.old)}
    rng = np.random.default_rng(0)
    mesh = spde.grid_mesh_2d(a.grid, a.grid, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.3))
    Q.sort_indices()
    n, nobs = Q.shape[0], a.nobs
    cells = np.asarray(mesh.cells)
    tri = cells[rng.integers(0, cells.shape[0], nobs)]
    A = sp.csr_matrix((rng.dirichlet(np.ones(3), nobs).ravel(), (np.repeat(np.arange(nobs), 3), tri.ravel())), shape=(nobs, n))
    A.sum_duplicates()
    y, aux = rng.poisson(3.0, nobs).astype(float), rng.uniform(-0.5, 0.5, nobs)
    dev = torch.device("cuda:0")
    dx, dm = torch.from_numpy(0.3 * rng.standard_normal(n)).to(dev), torch.from_numpy(0.1 * rng.standard_normal(n)).to(dev)
    ds = torch.empty(n, dtype=torch.float64, device=dev)
    side = {}
    for tag, L in libs.items():          # one handle per build, the same problem
        _lib.use(L)
        be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
        be.set_design_observations("poisson", y, A, aux=aux)
        be.set_prior(Q.data, be.observations_hess_map())
        dh = torch.empty(be.observations_design_info()["cnt"], dtype=torch.float64, device=dev)
        side[tag] = (be, dh)
    bits = {}
    medians = {"old": [], "new": []}
    for r in range(a.rounds):
        for tag in (("old", "new") if r % 2 == 0 else ("new", "old")):
            _lib.use(libs[tag])
            be, dh = side[tag]

            def call():
                return be.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())
            for _ in range(a.warmup):
                call()
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e = call()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            medians[tag].append(float(np.median(1e3 * np.asarray(ts))))
            bits[tag] = (e, ds.cpu().numpy().copy(), dh.cpu().numpy().copy())
    same = bits["old"][0] == bits["new"][0] and all(np.array_equal(p.view(np.int64), q.view(np.int64)) for p, q in zip(bits["old"][1:], bits["new"][1:]))
    old, new = medians["old"], medians["new"]
    res = {"call": "gmrfx_fisher_eval_dev, design form", "n": n, "nobs": nobs, "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup,
           "old_median_ms": old, "new_median_ms": new, "old_spread_ms": max(old) - min(old), "new_max_above_old_max_ms": max(new) - max(old),
           "inside_old_spread": max(new) - max(old) <= max(old) - min(old), "same_bits": bool(same), "source_tree_hash": _lib.source_tree_hash()}
    print(json.dumps(res))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    for tag in side:
        _lib.use(libs[tag])
        side[tag][0].close()
    _lib.use(libs["new"])


if __name__ == "__main__":
    main()
