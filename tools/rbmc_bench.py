#!/usr/bin/env python3
"""Rao-Blackwellised Monte Carlo marginal variances (gmrfx_rbmc_var_dev) beside selected inversion (gmrfx_selinv_diag) on one handle.

Problems: 2-D Matern (smoothness 0) grids of 250^2 and 1000^2 nodes with enclosure_size -1 (RBMCStrategy), 0 and 1
(BlockRBMCStrategy), a 3-D 40^3 grid with -1 and 0; k = 64 and 256 samples, Z in HBM. Reported per cell: milliseconds of one
gmrfx_rbmc_var_dev call -- median (and minimum) over --reps timed repetitions after --warmup, the GPU synchronised around each
timed region --, the same for the k-column backward sweep alone (gmrfx_backward_solve_dev: its share of the estimator), the same
handle's selected inversion (gmrfx_stats.ms_selinv after a fresh refactorisation; the first call's host analysis of the block
plan is reported apart as plan_ms), the relative error of the estimate against selinv_diag, and the source tree hash. No time
is a pass criterion.
usage: tools/rbmc_bench.py [--cases 2d:250,2d:1000,3d:40] [--samples 64,256] [--reps 25] [--warmup 3] [--out profiles/rbmc_bench.json]"""
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
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2d:250,2d:1000,3d:40")
    ap.add_argument("--samples", default="64,256")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbmc_bench.json"))
    a = ap.parse_args()
    tree = _lib.source_tree_hash()
    ks = [int(x) for x in a.samples.split(",")]
    rows = []
    for case in a.cases.split(","):
        dim, g = case.split(":")
        g = int(g)
        mesh = spde.grid_mesh_2d(g, g, jitter=0.25, seed=0) if dim == "2d" else spde.grid_mesh_3d(g, g, g)
        Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.2 if dim == "2d" else 0.6))
        n = Q.shape[0]
        be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0)
        truth = be.get_selinv_diag().copy()
        sel = []
        for _ in range(3):                      # selected inversion of a fresh factorisation, GPU time
            be.refactorize_values(Q.data)
            be.get_selinv_diag()
            sel.append(be.stats()["ms_selinv"])
        be.refactorize_values(Q.data)           # the handle holds Q's values: nzval = NULL below
        d_Z = torch.randn((max(ks), n), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        d_X = torch.empty_like(d_Z)
        d_out = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for enc in ((-1, 0, 1) if dim == "2d" else (-1, 0)):
            t0 = time.perf_counter()
            plan = be.rbmc_plan(enc) if enc >= 0 else None
            plan_ms = 1e3 * (time.perf_counter() - t0)
            for k in ks:
                t_bs, _ = timed(lambda: be.backward_solve_dev(d_Z.data_ptr(), n, k, d_X.data_ptr(), n), a.reps, a.warmup)
                t_rb, t_rb_min = timed(lambda: be.rbmc_var_dev(d_Z.data_ptr(), n, k, d_out.data_ptr(), enc), a.reps, a.warmup)
                v = d_out.cpu().numpy()
                row = {"case": case, "n": n, "nnz": int(Q.nnz), "enclosure_size": enc, "k": k, "ms_rbmc": t_rb, "ms_rbmc_min": t_rb_min,
                       "ms_rbmc_gpu": be.stats()["ms_rbmc"], "ms_backward_solve": t_bs, "backward_share": t_bs / t_rb,
                       "ms_selinv": float(np.median(sel)), "rel_err_vs_selinv_diag": float(np.linalg.norm(v - truth) / np.linalg.norm(truth)),
                       "blocks": None if plan is None else int(len(plan["n_interior"])), "max_block": None if plan is None else plan["max_block"],
                       "plan_ms": plan_ms, "reps": a.reps, "warmup": a.warmup, "source_tree_hash": tree}
                print(json.dumps(row), flush=True)
                rows.append(row)
        be.close()
        del d_Z, d_X, d_out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/rbmc_bench.py", "device": torch.cuda.get_device_name(0), "source_tree_hash": tree, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
