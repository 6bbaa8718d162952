#!/usr/bin/env python3
"""The linear predictor's marginals and the predictive scores on the device (gmrfx_predictor_marginals_dev,
gmrfx_predictive_scores_dev), beside the route through the entry points the library offered before them.

Problem: the benchmark's cfg 2 (a --grid x --grid jittered 2-D Matern mesh, default 1000: n = 10^6), Poisson with log exposure; node
form (an observation on every node, shuffled order) or, with --design, --nobs (default 10^6) point observations inside random triangles
of the mesh, three barycentric weights per row of A and an offset. K = --nodes (32) Gauss-Hermite nodes. Reported, milliseconds, median
(and minimum, and the spread max - min) over --reps repetitions after --warmup, wall clock with the GPU synchronised around the timed
region, all in one run:
  refactorize        gmrfx_refactorize alone
  refactorize_selinv gmrfx_refactorize + gmrfx_selinv_compute; selinv_compute_ms = the difference of the two medians
  marginals_dev      gmrfx_predictor_marginals_dev (mu_eta, v_eta, pll) on a computed selected inverse
  scores_dev         gmrfx_predictive_scores_dev on its outputs (four arrays and the totals)
  host_route         x to the host; node form: gmrfx_selinv_diag and a gather; design form: gmrfx_selinv_row_diag_apply on a plan built
                     once (untimed) and A x + b by scipy; then the nobs x K log densities, lpd, lcpo, elp, vlp and their totals in numpy
The workload sets no constraint: neither route forms the constraint's correction and clamp (the host route would add
gmrfx_constraints_get, a product with B and a maximum in numpy), so the host route timed here is the lighter one -- conservative for the
condition below; the corrected path is not timed.
The one condition: marginals_dev + scores_dev must not be slower than host_route of the same run ("device_not_slower").
A byte MODEL (not a measurement; the kernels are not timed apart from their calls):
  marginals, node form    nobs (4 idx + 8 x + 4 dpos + 8 zoff + 8 Z + 8 y + 8 aux + 8 c + 24 out)      (gathers through L2)
  marginals, design form  12 nnz(A) + 8 (nobs + 1) + 8 nnz(A) (x) + terms (12 + 8 hmap + 8 zoff + 8 Z) + 8 (nobs + 1) + nobs (8 b + 8 y + 8 aux + 8 c + 24 out)
  scores                  nobs (8 mu + 8 v + 8 y + 8 aux + 8 c + 32 out) (+ 4 nobs idx in node form); K exponentials and logarithms per observation
--old PATH/TO/libgmrfx.so: an A/B of gmrfx_predictor_marginals_dev and gmrfx_predictive_scores_dev between this build and another one
(the parent commit's), alternating in one process on the same operands: --rounds (4) medians of --reps per side and call, the order
within a round alternating; --first old|new: whose handle is created first (it is part of the measurement). Reported per
call: both sides' medians, whether the new median lies inside the old min .. max, and whether the seven output arrays and the four
totals of both builds have the same bits. Output: profiles/predictive_ab[_design].json.
usage: tools/predictive_bench.py [--design [--nobs 1000000]] [--grid 1000] [--nodes 32] [--reps 15] [--warmup 3]
                                 [--old LIB [--rounds 4] [--first old|new]] [--out profiles/predictive_bench[_design].json]"""
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
from scipy.special import gammaln  # noqa: E402

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


def host_scores(mu, v, y, aux, c, z, w):
    s = np.sqrt(v)
    e = (mu[:, None] + s[:, None] * z[None, :]) + aux[:, None]
    lk = y[:, None] * e - np.exp(e) + c[:, None]
    M = lk.max(axis=1)
    lpd = M + np.log((w * np.exp(lk - M[:, None])).sum(axis=1))
    Mn = (-lk).max(axis=1)
    lcpo = -(Mn + np.log((w * np.exp(-lk - Mn[:, None])).sum(axis=1)))
    elp = (w * lk).sum(axis=1)
    vlp = (w * (lk - elp[:, None]) ** 2).sum(axis=1)
    return lpd, lcpo, elp, vlp, (lpd.sum(), lcpo.sum(), elp.sum(), vlp.sum())


def ab(a, libs, handles, setup, Q, ptrs, z, w, res):
    """the two plain calls on both builds, alternating; each handle is set up, factorised and inverted by the library that made it"""
    dx, outs = ptrs
    p = [t.data_ptr() for t in outs]
    calls = {"marginals_dev": lambda be: be.predictor_marginals_dev(dx.data_ptr(), p[0], p[1], p[2]),
             "scores_dev": lambda be: be.predictive_scores_dev(p[0], p[1], z, w, p[3], p[4], p[5], p[6])}
    medians = {c: {"old": [], "new": []} for c in calls}
    bits, totals = {}, {}
    for tag in ("old", "new"):
        _lib.use(libs[tag])
        be = handles[tag]
        setup(be)
        be.refactorize_values(Q.data)
        be.selinv_compute_dev()
        calls["marginals_dev"](be)
        totals[tag] = calls["scores_dev"](be)
        torch.cuda.synchronize()
        bits[tag] = [t.cpu().numpy().copy() for t in outs]
    same = True
    for r in range(a.rounds):
        for tag in (("old", "new") if r % 2 == 0 else ("new", "old")):
            _lib.use(libs[tag])
            be = handles[tag]
            for c, fn in calls.items():
                medians[c][tag].append(timed(lambda: fn(be), a.reps, a.warmup)["median_ms"])
            torch.cuda.synchronize()       # the parent's bits in every run: the arrays the timed calls left
            same = same and all(np.array_equal(t.cpu().numpy().view(np.int64), u.view(np.int64)) for t, u in zip(outs, bits["old"]))
    for tag in ("old", "new"):          # every handle is destroyed by the library that made it (close() goes to the library in use)
        _lib.use(libs[tag])
        handles[tag].close()
    _lib.use(libs["new"])
    res.update({"tool": "tools/predictive_bench.py --old", "rounds": a.rounds, "handle_created_first": a.first})
    for c in calls:
        old, new = medians[c]["old"], medians[c]["new"]
        res[c] = {"old_median_ms": old, "new_median_ms": new, "new_inside_old_min_max": bool(min(old) <= float(np.median(new)) <= max(old)),
                  "new_median_above_old_max_ms": float(np.median(new)) - max(old)}
    res["same_bits"] = bool(same and all(np.array_equal(u.view(np.int64), v.view(np.int64)) for u, v in zip(bits["old"], bits["new"]))
                            and totals["old"] == totals["new"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=32)
    ap.add_argument("--design", action="store_true")
    ap.add_argument("--nobs", type=int, default=1000000)
    ap.add_argument("--old", default=None, help="another build of libgmrfx.so: A/B of the two plain calls against it")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--first", choices=("old", "new"), default="old", help="whose handle is created first (DESIGN.md 6m: it is part of the measurement)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        stem = "predictive_ab" if a.old else "predictive_bench"
        a.out = os.path.join(ROOT, "profiles", stem + ("_design.json" if a.design else ".json"))
    mesh = spde.grid_mesh_2d(a.grid, a.grid, jitter=0.25, seed=0)
    Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.2))
    Q = sp.csc_matrix((Q + Q.T) * 0.5)
    Q.sort_indices()
    n = Q.shape[0]
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    libs = {"new": _lib.lib()}
    be_old = None
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
    z, w = be.gauss_hermite(a.nodes)
    x = 0.3 * rng.standard_normal(n)
    if a.design:
        nobs = a.nobs
        cells = np.asarray(mesh.cells)
        tri = cells[rng.integers(0, cells.shape[0], nobs)]
        A = sp.csr_matrix((rng.dirichlet(np.ones(3), nobs).ravel(), (np.repeat(np.arange(nobs), 3), tri.ravel())), shape=(nobs, n))
        A.sum_duplicates()
        b = rng.uniform(-0.2, 0.2, nobs)
        idx = None
    else:
        nobs, A, b = n, None, None
        idx = rng.permutation(n)
    y = rng.poisson(3.0, nobs).astype(float)
    aux = rng.uniform(-0.5, 0.5, nobs)
    def setup(h):
        if a.design:
            h.set_design_observations("poisson", y, A, offset=b, aux=aux)
        else:
            h.set_observations("poisson", y, indices=idx, aux=aux)
    if not a.old:
        setup(be)
    res = {"n": n, "nobs": nobs, "K": a.nodes, "design": bool(a.design), "reps": a.reps, "warmup": a.warmup,
           "source_tree_hash": _lib.source_tree_hash()}
    if a.old:
        dx = torch.from_numpy(x).to(dev)
        outs = [torch.empty(nobs, dtype=torch.float64, device=dev) for _ in range(7)]
        return ab(a, libs, {"new": be, "old": be_old}, setup, Q, (dx, outs), z, w, res)
    if a.design:
        info = be.observations_design_info()
        res.update({"nnz_A": info["nnz"], "terms": info["terms"]})
        res["model_bytes_marginals"] = 20 * info["nnz"] + 16 * (nobs + 1) + 36 * info["terms"] + 56 * nobs
    else:
        res["model_bytes_marginals"] = 80 * nobs
    res["model_bytes_scores"] = (72 if a.design else 76) * nobs
    dx = torch.from_numpy(x).to(dev)
    dm, dv, dp, o0, o1, o2, o3 = (torch.empty(nobs, dtype=torch.float64, device=dev) for _ in range(7))

    def refactorize():
        be.refactorize_values(Q.data)

    def refactorize_selinv():
        be.refactorize_values(Q.data)
        be.selinv_compute_dev()

    def marginals_dev():
        be.predictor_marginals_dev(dx.data_ptr(), dm.data_ptr(), dv.data_ptr(), dp.data_ptr())

    def scores_dev():
        return be.predictive_scores_dev(dm.data_ptr(), dv.data_ptr(), z, w, o0.data_ptr(), o1.data_ptr(), o2.data_ptr(), o3.data_ptr())

    c = -gammaln(y + 1.0)

    def host_route():
        xh = dx.cpu().numpy()
        if a.design:
            mu = A @ xh + b
            v = be.row_diag_ASigmaAt(A)
        else:
            be._selinv_diag_cache = None
            mu, v = xh[idx], be.get_selinv_diag()[idx]
        return mu, v, host_scores(mu, v, y, aux, c, z, w)

    res["refactorize"] = timed(refactorize, a.reps, a.warmup)
    res["refactorize_selinv"] = timed(refactorize_selinv, a.reps, a.warmup)
    res["selinv_compute_ms"] = res["refactorize_selinv"]["median_ms"] - res["refactorize"]["median_ms"]
    if a.design:
        be.row_diag_ASigmaAt(A)          # the host route's pair plan, built once
    for name, fn in (("marginals_dev", marginals_dev), ("scores_dev", scores_dev), ("host_route", host_route)):
        res[name] = timed(fn, a.reps, a.warmup)
    res["device_route_ms"] = res["marginals_dev"]["median_ms"] + res["scores_dev"]["median_ms"]
    res["device_not_slower"] = bool(res["device_route_ms"] <= res["host_route"]["median_ms"])
    res["marginals_gbs_modelled_bytes"] = res["model_bytes_marginals"] / res["marginals_dev"]["median_ms"] / 1e6
    # the two routes agree
    tot = scores_dev()
    mu, v, hs = host_route()
    res["v_eta_max_rel_diff"] = float(np.abs(dv.cpu().numpy() - v).max() / np.abs(v).max())
    res["lpd_total_rel_diff"] = float(abs(tot["lpd"] - hs[4][0]) / abs(hs[4][0]))
    res["totals"] = tot
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
