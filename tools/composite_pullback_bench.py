#!/usr/bin/env python3
"""The pullback of gaussian_approximation for a composite likelihood (gmrfx_ga_pullback_composite_dev) beside the single-family
design-form pullback on the same A, and beside the route a user of a joint model had before it.

Problem: the benchmark's cfg 2 (a --grid x --grid jittered 2-D Matern mesh, default 1000: n = 10^6), every node observed once through a
selection row (n = nobs), the first half of the rows a Normal component (sigma 1), the second half a Gamma component (phi 2). Each
handle holds the factor of Q_prior - H(x) (one call with the refactorisation bit, untimed). Protocol of tools/ga_pullback_bench.py: wall
clock, the GPU synchronised around the timed region, median (minimum, spread max - min) of --reps after --warmup. Routes, same run:
  composite_dev   gmrfx_ga_pullback_composite_dev: Qbar, mubar, x, mu resident; Qbar_prior and mubar_prior written in HBM; ncomp + 1
                  numbers come back
  single_dev      gmrfx_ga_pullback_dev on a handle with the same A under gmrfx_obs_set_design, every row Gamma
  host            x and Qbar down; d3, gp, dp per component in numpy; c_i the diagonal of Qbar; xbar; the solve through the host entry
                  point; the symmetrised outer product on the pattern and Q_p lam in numpy / scipy; the two sums per component;
                  Qbar_prior and mubar_prior up
composite_dev and single_dev run in this order and then once more in the other order (single_dev_2, composite_dev_2): a difference
that changes sign with the order is the run's noise; it is reported, not gated. The one condition: composite_dev is not slower than
host of the same run ("device_not_slower").
usage: tools/composite_pullback_bench.py [--grid 1000] [--reps 15] [--warmup 3] [--out profiles/composite_pullback_bench.json]"""
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

import gmrfx  # noqa: E402
from gmrfx import _lib, composite, spde  # noqa: E402
from fisher_bench import timed  # noqa: E402

SIGMA, PHI = 1.0, 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_pullback_bench.json"))
    a = ap.parse_args()
    mesh = spde.grid_mesh_2d(a.grid, a.grid, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.2))
    Q = sp.csc_matrix((Q + Q.T) * 0.5)
    Q.sort_indices()
    n, nnz = Q.shape[0], Q.nnz
    half = n // 2
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    y = rng.gamma(2.0, 1.0, n) + 0.05           # positive: the Gamma family accepts every row
    A = sp.identity(n, format="csr")
    cols = np.repeat(np.arange(n), np.diff(Q.indptr))
    diag = np.flatnonzero(Q.indices == cols)
    S = sp.csr_matrix(sp.triu(Q) + sp.triu(Q, 1).T)
    res = {"n": n, "nobs": n, "nnz": int(nnz), "components": ["normal", "gamma"], "rows": [half, n - half], "reps": a.reps, "warmup": a.warmup,
           "source_tree_hash": _lib.source_tree_hash()}

    def backend(comp):
        be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
        if comp:
            co = gmrfx.CompositeObservations(n)
            co.add("normal", y[:half], indices=np.arange(half), param=SIGMA)
            co.add("gamma", y[half:], indices=np.arange(half, n), param=PHI)
            gmrfx.set_composite_observations(be, co)
        else:
            be.set_design_observations("gamma", y, A, param=PHI)
        be.set_prior(Q.data, be.observations_hess_map())
        return be

    bc, bs = backend(True), backend(False)
    x, mu = 0.3 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    mubar = rng.standard_normal(n)
    Gs = sp.csc_matrix((rng.standard_normal(nnz), Q.indices, Q.indptr), shape=Q.shape)
    Gs = sp.csc_matrix((Gs + Gs.T) * 0.5)              # a symmetric cotangent on the pattern
    Gs.sort_indices()
    G = np.ascontiguousarray(Gs.data)
    assert Gs.nnz == nnz
    dx, dm, db, dG = (torch.from_numpy(v).to(dev) for v in (x, mu, mubar, G))
    oq, om, ol = (torch.empty(k, dtype=torch.float64, device=dev) for k in (nnz, n, n))
    ptrs = (dx.data_ptr(), dm.data_ptr(), db.data_ptr(), dG.data_ptr(), oq.data_ptr(), om.data_ptr())
    composite.ga_pullback_dev(bc, *ptrs, ol.data_ptr(), refactorize=True)
    bs.ga_pullback_dev(*ptrs, ol.data_ptr(), refactorize=True)
    out = {}

    def composite_dev():
        out["dev"] = composite.ga_pullback_dev(bc, *ptrs, 0)

    def single_dev():
        bs.ga_pullback_dev(*ptrs, 0)

    def host():
        xh, Gh = dx.cpu().numpy(), dG.cpu().numpy()
        c = Gh[diag]
        d3, gp, dp = np.zeros(n), np.empty(n), np.empty(n)
        gp[:half], dp[:half] = -2.0 * (y[:half] - xh[:half]) / SIGMA ** 3, 2.0 / SIGMA ** 3
        w = y[half:] * np.exp(-xh[half:])
        d3[half:], gp[half:], dp[half:] = PHI * w, w - 1.0, -w
        lam = bc.backend_solve(mubar - c * d3)
        r = xh - mu
        qp = Gh - 0.5 * (lam[Q.indices] * r[cols] + lam[cols] * r[Q.indices])
        mp = S @ lam
        par = [float((lam[s] * gp[s]).sum() - (c[s] * dp[s]).sum()) for s in (slice(0, half), slice(half, n))]
        return torch.from_numpy(qp).to(dev), torch.from_numpy(mp).to(dev), par

    for name, fn in (("composite_dev", composite_dev), ("single_dev", single_dev), ("single_dev_2", single_dev), ("composite_dev_2", composite_dev),
                     ("host", host)):
        res[name] = timed(fn, a.reps, a.warmup)
    res["device_not_slower"] = bool(res["composite_dev"]["median_ms"] <= res["host"]["median_ms"])
    res["composite_over_single"] = res["composite_dev"]["median_ms"] / res["single_dev"]["median_ms"]
    res["composite_over_single_2"] = res["composite_dev_2"]["median_ms"] / res["single_dev_2"]["median_ms"]
    # the two routes agree
    composite_dev()
    hq, hm, hpar = host()
    res["param_bar"] = [float(v) for v in out["dev"][0]]
    res["param_bar_host"] = hpar
    res["Qbar_prior_max_rel_diff"] = float((oq - hq).abs().max() / hq.abs().max())
    res["mubar_prior_max_rel_diff"] = float((om - hm).abs().max() / hm.abs().max())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
