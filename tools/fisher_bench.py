#!/usr/bin/env python3
"""The fused evaluation of a Fisher-scoring iterate (gmrfx_fisher_eval_dev) and one whole iterate, beside the route the library
offered before it.

Problem: the benchmark's cfg 2 (a --grid x --grid jittered 2-D Matern mesh, default 1000: n = 10^6), a Poisson observation on every
node. Reported, milliseconds, median (and minimum, and the spread max - min) over --reps repetitions after --warmup, wall clock with
the GPU synchronised around the timed region:
  eval_dev          one gmrfx_fisher_eval_dev (score, hess, energy, loglik), and the bytes it must move over HBM by the model
                        16 B per entry of Symmetric(Q) (value 8, column 4, position 4) + 8 (n + 1) row pointers
                        + n (8 x + 8 mu + 8 y + 8 aux + 1 mask + 8 score + 8 hess)            (x and mu gathered through L2)
                    as a fraction of --peak-gbs (8000: the figure BASELINE.md divides by); the bytes are MODELLED, the time is measured
  solve_dev         gmrfx_refactorize_update_solve_dev with nrhs = 1 alone: the part of an iterate that was on the device already
  iterate_dev       eval_dev + solve_dev on the evaluation's own outputs: nothing but two numbers leaves HBM
  iterate_host      the same iterate through the older entry points: x on the host, gradient, Hessian, Q x - Q mu and the merit in
                    numpy / scipy, then gmrfx_refactorize_update_solve with host arrays
The figure to read is iterate_dev - solve_dev (the cost of an iterate above its factorisation and solve) against
iterate_host - solve_dev. No time is a pass criterion.

--design: the same mesh observed through a design matrix (gmrfx_obs_set_design): --nobs (default 10^6) point observations, each inside a
triangle of the mesh chosen at random, three barycentric weights per row of A, Poisson with log exposure; pattern(A'A) lies inside the
19-point pattern of Q by construction. Reported with the same protocol, in the same run:
  eval_node         one node-form gmrfx_fisher_eval_dev on the same mesh (a Poisson observation on every node), for comparison
  eval_design       one design-form gmrfx_fisher_eval_dev (score n, hess cnt), with its MODELLED bytes
                        eta    12 nnz(A) + 8 (nobs + 1) + nobs (8 y + 8 aux + 8 g + 8 d) + 8 n (x, gathered)
                        score  16 nnz(Symmetric(Q)) + 8 (n + 1) + 12 nnz(A) + 12 (n + 1) + n (8 x + 8 mu + 8 score) + 8 nobs (g, gathered)
                        hess   12 terms + 12 (cnt + 1) + 8 cnt + 8 nobs (d, gathered)
  solve_dev         gmrfx_refactorize_update_solve_dev, nrhs = 1, under the design map
  iterate_dev       eval_design + solve_dev on the evaluation's outputs
  iterate_host      x to the host, eta = A x + aux, g and d in numpy, score = Q x - Q mu - A' g, scipy A.T @ (D @ A), its values in map
                    order (through an index computed once, untimed), then gmrfx_refactorize_update_solve with host arrays
The one condition: iterate_dev must not be slower than iterate_host of the same run ("device_not_slower" in the output).
usage: tools/fisher_bench.py [--design [--nobs 1000000]] [--grid 1000] [--reps 15] [--warmup 3] [--out profiles/fisher_bench[_design].json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

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


def design(a, mesh, Q, be, rng):
    n, nobs = Q.shape[0], a.nobs
    dev = torch.device("cuda:0")
    cells = np.asarray(mesh.cells)
    tri = cells[rng.integers(0, cells.shape[0], nobs)]
    w = rng.dirichlet(np.ones(3), nobs)
    A = sp.csr_matrix((w.ravel(), (np.repeat(np.arange(nobs), 3), tri.ravel())), shape=(nobs, n))
    A.sum_duplicates()
    At = sp.csr_matrix(A.T)
    y = rng.poisson(3.0, nobs).astype(float)
    aux = rng.uniform(-0.5, 0.5, nobs)
    x, mu = 0.3 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    dx, dm = torch.from_numpy(x).to(dev), torch.from_numpy(mu).to(dev)
    ds, dstep = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    S = sp.csr_matrix(sp.triu(Q) + sp.triu(Q, 1).T)
    nsym = int(S.nnz)
    res = {"n": n, "nobs": nobs, "nnz_symmetric": nsym, "reps": a.reps, "warmup": a.warmup, "source_tree_hash": _lib.source_tree_hash()}
    # the node form on the same mesh, for comparison (needs nobs >= n observations' worth of y: its own draw)
    cols = np.repeat(np.arange(n), np.diff(Q.indptr))
    be.set_prior(Q.data, np.flatnonzero(Q.indices == cols).astype(np.int64))
    be.set_observations("poisson", rng.poisson(3.0, n).astype(float), aux=rng.uniform(-0.5, 0.5, n))
    dhn = torch.empty(n, dtype=torch.float64, device=dev)
    res["eval_node"] = timed(lambda: be.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dhn.data_ptr()), a.reps, a.warmup)
    res["model_bytes_eval_node"] = 16 * nsym + 8 * (n + 1) + n * (8 * 6 + 1)
    # the design form
    t0 = time.perf_counter()
    be.set_design_observations("poisson", y, A, aux=aux)
    res["set_design_s"] = time.perf_counter() - t0
    hmap = be.observations_hess_map()
    info = be.observations_design_info()
    cnt, terms, nnza = info["cnt"], info["terms"], info["nnz"]
    res.update({"nnz_A": nnza, "cnt": cnt, "terms": terms})
    be.set_prior(Q.data, hmap)
    dh = torch.empty(cnt, dtype=torch.float64, device=dev)
    model = (12 * nnza + 8 * (nobs + 1) + 32 * nobs + 8 * n) + (16 * nsym + 8 * (n + 1) + 12 * nnza + 12 * (n + 1) + 24 * n + 8 * nobs) \
        + (12 * terms + 12 * (cnt + 1) + 8 * cnt + 8 * nobs)
    res["model_bytes_eval_design"] = model
    # host route: the values of scipy's A' D A in map order, through an index computed once
    H0 = sp.csc_matrix(At @ sp.diags(np.ones(nobs)) @ A)
    H0.sort_indices()
    hcols = np.repeat(np.arange(n, dtype=np.int64), np.diff(H0.indptr))
    hkeys = hcols * n + H0.indices
    qcols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Q.indptr))
    hidx = np.searchsorted(hkeys, qcols[hmap] * n + Q.indices[hmap])
    assert np.array_equal(hkeys[hidx], qcols[hmap] * n + Q.indices[hmap])

    def eval_design():
        be.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())

    def solve_dev():
        be.refactorize_update_solve_dev(dh.data_ptr(), ds.data_ptr(), n, 1, dstep.data_ptr(), n)

    def iterate_dev():
        eval_design()
        solve_dev()

    def iterate_host():
        xh = dx.cpu().numpy()
        e = A @ xh + aux
        m = np.exp(e)
        Qx, h = S @ xh, S @ mu
        score = (Qx - h) - At @ (y - m)
        H = sp.csc_matrix(At @ (sp.diags(-m) @ A))
        H.sort_indices()
        merit = (0.5 * xh @ Qx - xh @ h) - float(np.sum(y * e - m))
        return be.refactorize_update_solve(H.data[hidx], score), merit

    eval_design()
    for name, fn in (("eval_design", eval_design), ("solve_dev", solve_dev), ("iterate_dev", iterate_dev), ("iterate_host", iterate_host)):
        res[name] = timed(fn, a.reps, a.warmup)
    ev = res["eval_design"]["median_ms"]
    res["eval_design_gbs_modelled_bytes"] = model / ev / 1e6
    res["eval_design_fraction_of_peak"] = res["eval_design_gbs_modelled_bytes"] / a.peak_gbs
    res["eval_node_gbs_modelled_bytes"] = res["model_bytes_eval_node"] / res["eval_node"]["median_ms"] / 1e6
    res["iterate_above_solve_dev_ms"] = res["iterate_dev"]["median_ms"] - res["solve_dev"]["median_ms"]
    res["iterate_above_solve_host_ms"] = res["iterate_host"]["median_ms"] - res["solve_dev"]["median_ms"]
    res["device_not_slower"] = bool(res["iterate_dev"]["median_ms"] <= res["iterate_host"]["median_ms"])
    iterate_dev()
    step_dev = dstep.cpu().numpy()
    step_host = iterate_host()[0]
    res["step_max_rel_diff"] = float(np.abs(step_dev - step_host).max() / np.abs(step_host).max())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--peak-gbs", type=float, default=8000.0)
    ap.add_argument("--design", action="store_true")
    ap.add_argument("--nobs", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "fisher_bench_design.json" if a.design else "fisher_bench.json")
    mesh = spde.grid_mesh_2d(a.grid, a.grid, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.2))
    Q = sp.csc_matrix((Q + Q.T) * 0.5)
    Q.sort_indices()
    n = Q.shape[0]
    rng = np.random.default_rng(0)
    be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
    if a.design:
        return design(a, mesh, Q, be, rng)
    cols = np.repeat(np.arange(n), np.diff(Q.indptr))
    dpos = np.flatnonzero(Q.indices == cols).astype(np.int64)
    be.set_prior(Q.data, dpos)
    y = rng.poisson(3.0, n).astype(float)
    aux = rng.uniform(-0.5, 0.5, n)
    be.set_observations("poisson", y, aux=aux)
    x, mu = 0.3 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    dev = torch.device("cuda:0")
    dx, dm = torch.from_numpy(x).to(dev), torch.from_numpy(mu).to(dev)
    ds, dh, dstep = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    S = sp.csr_matrix(sp.triu(Q) + sp.triu(Q, 1).T)
    nsym = int(S.nnz)
    model_bytes = 16 * nsym + 8 * (n + 1) + n * (8 * 6 + 1)

    def eval_dev():
        be.fisher_eval_dev(dx.data_ptr(), dm.data_ptr(), ds.data_ptr(), dh.data_ptr())

    def solve_dev():
        be.refactorize_update_solve_dev(dh.data_ptr(), ds.data_ptr(), n, 1, dstep.data_ptr(), n)

    def iterate_dev():
        eval_dev()
        solve_dev()

    def iterate_host():
        xh = dx.cpu().numpy()
        e = xh + aux
        m = np.exp(e)
        Qx, h = S @ xh, S @ mu
        score, hess = (Qx - h) - (y - m), -m
        merit = (0.5 * xh @ Qx - xh @ h) - float(np.sum(y * e - m))
        return be.refactorize_update_solve(hess, score), merit

    eval_dev()
    res = {"n": n, "nnz_symmetric": nsym, "reps": a.reps, "warmup": a.warmup, "source_tree_hash": _lib.source_tree_hash(),
           "model_bytes_eval": model_bytes}
    for name, fn in (("eval_dev", eval_dev), ("solve_dev", solve_dev), ("iterate_dev", iterate_dev), ("iterate_host", iterate_host)):
        res[name] = timed(fn, a.reps, a.warmup)
    ev = res["eval_dev"]["median_ms"]
    res["eval_gbs_modelled_bytes"] = model_bytes / ev / 1e6
    res["eval_fraction_of_peak"] = res["eval_gbs_modelled_bytes"] / a.peak_gbs
    res["iterate_above_solve_dev_ms"] = res["iterate_dev"]["median_ms"] - res["solve_dev"]["median_ms"]
    res["iterate_above_solve_host_ms"] = res["iterate_host"]["median_ms"] - res["solve_dev"]["median_ms"]
    # the two routes agree on the step
    step_dev = dstep.cpu().numpy()
    step_host = iterate_host()[0]
    res["step_max_rel_diff"] = float(np.abs(step_dev - step_host).max() / np.abs(step_host).max())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
