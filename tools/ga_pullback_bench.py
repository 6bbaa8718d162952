#!/usr/bin/env python3
"""The pullback of gaussian_approximation (gmrfx_ga_pullback_dev) beside the route a user had before it.

Problem: the benchmark's cfg 2 (a --grid x --grid jittered 2-D Matern mesh, default 1000: n = 10^6) with a Poisson likelihood, by node
or (--design) through --nobs point observations with three barycentric weights per row, as tools/fisher_bench.py builds them. The
handle holds the factor of Q_prior - H(x) (one call with the refactorisation bit, untimed). Protocol of tools/fisher_bench.py: wall
clock, the GPU synchronised around the timed region, median (minimum, spread max - min) of --reps after --warmup. Routes, same run:
  pullback_dev    gmrfx_ga_pullback_dev: Qbar, mubar, x, mu resident; Qbar_prior and mubar_prior written in HBM; two numbers come back
  solve_dev       gmrfx_solve_dev with one right-hand side: the part of either route that was on the device already
  pullback_host   x and Qbar down; d3 in numpy; c_i = a_i' Qbar a_i (node form: the diagonal; design form: the scipy triple product
                  rowsum((A Qbar_sym) . A)); xbar; the solve through the host entry point; the symmetrised outer product on the pattern
                  and Q_p lam in numpy / scipy; Qbar_prior and mubar_prior up
The one condition: pullback_dev is not slower than pullback_host of the same run ("device_not_slower"). MODELLED bytes of the kernels
around the solve (the time is measured, the bytes are not):
  node    point 8 n (map) + n (8 G + 8 x + 8 y + 8 aux + 1 mask + 8 mubar + 8 xbar);  pattern 12 nnz + 8 (n + 1) + 16 nnz (G, out)
          + 24 n (lam, x, mu gathered);  mean 16 nnz_sym + 8 (n + 1) + 16 n
  design  point 12 nnz(A) + 12 terms + 8 terms (G gathered through the map) + 16 (nobs + 1) + nobs (8 y + 8 aux + 8 t) + 8 n;
          gather 12 nnz(A) + 12 (n + 1) + 8 nobs + 16 n;  pattern and mean as above
--old PATH/TO/libgmrfx.so: an A/B of gmrfx_ga_pullback_dev between this build and another one (the parent commit's), alternating in
ONE process, each with its own handle on the same problem: --rounds medians per side. The rule, set beforehand: the new median lies
inside the other build's min .. max; the outputs must have its bits. --first: whose handle is created first (it is part of the
measurement: DESIGN.md section 6m). Written to profiles/ga_pullback_ab[_design].json.
usage: tools/ga_pullback_bench.py [--design [--nobs 1000000]] [--grid 1000] [--reps 15] [--warmup 3] [--old LIB [--rounds 4] [--first old|new]]
                                  [--out profiles/ga_pullback_bench[_design].json]"""
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
from gmrfx import _lib, spde  # noqa: E402
from fisher_bench import timed  # noqa: E402


def ab(a, libs, handles, A, y, aux, Q, cols, ins, outs, res):
    """the plain call on both builds, alternating; the old build's handle gets the likelihood and prior the new one has"""
    dx, dm, db, dG = ins
    oq, om, ol = outs
    _lib.use(libs["old"])
    bo = handles["old"]
    if a.design:
        bo.set_design_observations("poisson", y, A, aux=aux)
        bo.set_prior(Q.data, bo.observations_hess_map())
    else:
        bo.set_observations("poisson", y, aux=aux)
        bo.set_prior(Q.data, np.flatnonzero(Q.indices == cols).astype(np.int64))
    medians, bits, results = {"old": [], "new": []}, {}, {}
    for tag in ("old", "new"):
        _lib.use(libs[tag])
        results[tag] = handles[tag].ga_pullback_dev(dx.data_ptr(), dm.data_ptr(), db.data_ptr(), dG.data_ptr(), oq.data_ptr(), om.data_ptr(),
                                                    ol.data_ptr(), refactorize=True)
        torch.cuda.synchronize()
        bits[tag] = [t.cpu().numpy().copy() for t in (oq, om, ol)]
    for r in range(a.rounds):
        for tag in (("old", "new") if r % 2 == 0 else ("new", "old")):
            _lib.use(libs[tag])
            be = handles[tag]
            t = timed(lambda: be.ga_pullback_dev(dx.data_ptr(), dm.data_ptr(), db.data_ptr(), dG.data_ptr(), oq.data_ptr(), om.data_ptr(), 0),
                      a.reps, a.warmup)
            medians[tag].append(t["median_ms"])
    for tag in ("old", "new"):          # every handle is destroyed by the library that made it (close() goes to the library in use)
        _lib.use(libs[tag])
        handles[tag].close()
    _lib.use(libs["new"])
    old, new = medians["old"], medians["new"]
    res.update({"tool": "tools/ga_pullback_bench.py --old", "rounds": a.rounds, "handle_created_first": a.first, "old_median_ms": old, "new_median_ms": new,
                "new_inside_old_min_max": bool(min(old) <= float(np.median(new)) <= max(old)),
                "new_median_above_old_max_ms": float(np.median(new)) - max(old),
                "same_bits": bool(all(np.array_equal(u.view(np.int64), v.view(np.int64)) for u, v in zip(bits["old"], bits["new"]))
                                  and results["old"] == results["new"])})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--design", action="store_true")
    ap.add_argument("--nobs", type=int, default=1000000)
    ap.add_argument("--old", default=None, help="another build of libgmrfx.so: A/B of gmrfx_ga_pullback_dev against it")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--first", choices=("old", "new"), default="old", help="whose handle is created first (DESIGN.md 6m: it is part of the measurement)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        stem = "ga_pullback_ab" if a.old else "ga_pullback_bench"
        a.out = os.path.join(ROOT, "profiles", stem + ("_design.json" if a.design else ".json"))
    mesh = spde.grid_mesh_2d(a.grid, a.grid, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.2))
    Q = sp.csc_matrix((Q + Q.T) * 0.5)
    Q.sort_indices()
    n, nnz = Q.shape[0], Q.nnz
    rng = np.random.default_rng(0)
    libs = {"new": _lib.lib()}
    if a.old:
        libs["old"] = _lib.load_from(a.old)
    if a.old and a.first == "old":
        _lib.use(libs["old"])
        be_old = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
        _lib.use(libs["new"])
    be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
    if a.old and a.first == "new":
        _lib.use(libs["old"])
        be_old = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0, factorize=False)
        _lib.use(libs["new"])
    dev = torch.device("cuda:0")
    cols = np.repeat(np.arange(n), np.diff(Q.indptr))
    S = sp.csr_matrix(sp.triu(Q) + sp.triu(Q, 1).T)
    res = {"n": n, "nnz": int(nnz), "nnz_symmetric": int(S.nnz), "reps": a.reps, "warmup": a.warmup, "design": bool(a.design),
           "source_tree_hash": _lib.source_tree_hash()}
    if a.design:
        nobs = a.nobs
        cells = np.asarray(mesh.cells)
        tri = cells[rng.integers(0, cells.shape[0], nobs)]
        A = sp.csr_matrix((rng.dirichlet(np.ones(3), nobs).ravel(), (np.repeat(np.arange(nobs), 3), tri.ravel())), shape=(nobs, n))
        A.sum_duplicates()
        At = sp.csr_matrix(A.T)
        y, aux = rng.poisson(3.0, nobs).astype(float), rng.uniform(-0.5, 0.5, nobs)
        be.set_design_observations("poisson", y, A, aux=aux)
        be.set_prior(Q.data, be.observations_hess_map())
        info = be.observations_design_info()
        res.update({"nobs": nobs, "nnz_A": info["nnz"], "terms": info["terms"]})
        model = (12 * info["nnz"] + 20 * info["terms"] + 16 * (nobs + 1) + 24 * nobs + 8 * n) + (12 * info["nnz"] + 12 * (n + 1) + 8 * nobs + 16 * n)
    else:
        A = At = None
        y, aux = rng.poisson(3.0, n).astype(float), rng.uniform(-0.5, 0.5, n)
        be.set_observations("poisson", y, aux=aux)
        be.set_prior(Q.data, np.flatnonzero(Q.indices == cols).astype(np.int64))
        model = 8 * n + n * 49
    model += (12 * nnz + 8 * (n + 1) + 16 * nnz + 24 * n) + (16 * int(S.nnz) + 8 * (n + 1) + 16 * n)
    res["model_bytes_kernels"] = int(model)
    x, mu = 0.3 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    mubar = rng.standard_normal(n)
    G = rng.standard_normal(nnz)
    Gs = sp.csc_matrix((G, Q.indices, Q.indptr), shape=Q.shape)
    Gs = sp.csc_matrix((Gs + Gs.T) * 0.5)              # a symmetric cotangent on the pattern
    Gs.sort_indices()
    G = np.ascontiguousarray(Gs.data)
    assert Gs.nnz == nnz
    dx, dm, db, dG = (torch.from_numpy(v).to(dev) for v in (x, mu, mubar, G))
    oq, om, ol, dl = (torch.empty(k, dtype=torch.float64, device=dev) for k in (nnz, n, n, n))
    if a.old:
        return ab(a, libs, {"new": be, "old": be_old}, A, y, aux, Q, cols, (dx, dm, db, dG), (oq, om, ol), res)
    be.ga_pullback_dev(dx.data_ptr(), dm.data_ptr(), db.data_ptr(), dG.data_ptr(), oq.data_ptr(), om.data_ptr(), ol.data_ptr(), refactorize=True)
    diag = np.flatnonzero(Q.indices == cols)

    def pullback_dev():
        be.ga_pullback_dev(dx.data_ptr(), dm.data_ptr(), db.data_ptr(), dG.data_ptr(), oq.data_ptr(), om.data_ptr(), 0)

    def solve_dev():
        be.solve_dev(db.data_ptr(), n, 1, dl.data_ptr(), n)

    def pullback_host():
        xh, Gh = dx.cpu().numpy(), dG.cpu().numpy()
        if a.design:
            Gm = sp.csr_matrix(sp.csc_matrix((Gh, Q.indices, Q.indptr), shape=Q.shape))
            c = np.asarray((A @ Gm).multiply(A).sum(axis=1)).ravel()
            d3 = -np.exp(A @ xh + aux)
            xbar = mubar - At @ (c * d3)
        else:
            xbar = mubar + Gh[diag] * np.exp(xh + aux)
        lam = be.backend_solve(xbar)
        r = xh - mu
        qp = Gh - 0.5 * (lam[Q.indices] * r[cols] + lam[cols] * r[Q.indices])
        mp = S @ lam
        return torch.from_numpy(qp).to(dev), torch.from_numpy(mp).to(dev), lam

    for name, fn in (("pullback_dev", pullback_dev), ("solve_dev", solve_dev), ("pullback_host", pullback_host)):
        res[name] = timed(fn, a.reps, a.warmup)
    res["device_not_slower"] = bool(res["pullback_dev"]["median_ms"] <= res["pullback_host"]["median_ms"])
    res["kernels_above_solve_ms"] = res["pullback_dev"]["median_ms"] - res["solve_dev"]["median_ms"]
    # the two routes agree
    pullback_dev()
    hq, hm, _ = pullback_host()
    res["Qbar_prior_max_rel_diff"] = float((oq - hq).abs().max() / hq.abs().max())
    res["mubar_prior_max_rel_diff"] = float((om - hm).abs().max() / hm.abs().max())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
