#!/usr/bin/env python3
"""What follows the fit, for every member of a sweep: selected inversion + gmrfx_batch_predictor_marginals_dev +
gmrfx_batch_predictive_scores_dev + gmrfx_batch_predictive_mixture_dev on a batched handle held at its modes, against the same
read-outs taken B times on ONE plain handle (gmrfx_predictor_marginals_dev, which computes the selected inverse, +
gmrfx_predictive_scores_dev per member, the mixture formed on the host from the downloaded arrays), in the same process and run.

Problem: the cases of tools/batch_ga_bench.py -- B = 50 Matern precisions on a 100 x 100 mesh (n = 10 000), Poisson counts on every
node, K = 32 Gauss-Hermite nodes; --design: 30 000 point observations plus an intercept. The batch is fitted once
(gmrfx_batch_gaussian_approximation, flag bit 3); Q_post,k = Q_p,k - H_k is kept on the device. Every repetition refactorises at those
values first (untimed: a fresh factor has no selected inverse), then times the read-outs, the GPU synchronised around the timed region;
the plain route refactorises member by member (untimed) and sums the B timed read-outs; it is reported
with the download and the host mixture ("one_plain_handle_sequential") and without them ("one_plain_handle_readouts_only": the B pairs of
device calls alone, against a batched route that includes its mixture). Protocol of tools/fisher_bench.py: median of
--reps 15 after --warmup 3, with min .. max. Whether member k's arrays of both routes agree bit for bit is reported.
usage: tools/batch_predictive_bench.py [--design] [--grid 100] [--batch 50] [--K 32] [--reps 15] [--warmup 3] [--out profiles/...json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gmrfx  # noqa: E402
from batch_ga_bench import design_problem, diag_positions, members  # noqa: E402
from gmrfx import _lib  # noqa: E402


def summary(ts):
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return {"median_ms": float(q[2]), "min_ms": float(q[0]), "q25_ms": float(q[1]), "q75_ms": float(q[3]), "max_ms": float(q[4])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--design", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, g, dev = a.batch, a.grid, "cuda:0"
    if a.design:
        Qs, pts, A, y = design_problem(g, B, np.random.default_rng(g))
        order = dict(ordering=gmrfx.PinDenseColumns())
    else:
        Qs, pts = members(g, B, np.random.default_rng(g))
        A, y, order = None, np.random.default_rng(1).poisson(20.0, Qs[0].shape[0]).astype(float), {}
    n, nobs = Qs[0].shape[0], len(y)
    NZ = np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))
    z, w = gmrfx.MI355XBackend.gauss_hermite(a.K)
    logw = np.random.default_rng(2).uniform(-3.0, 0.0, B)

    bb = gmrfx.MI355XBatchLaplace(Qs[0], B, coords=pts, device=0, **order)
    if a.design:
        bb.set_design_observations("poisson", y, A, param=0.0)
    else:
        bb.set_observations("poisson", y, param=0.0)
    bb.set_prior(NZ)
    X, H, info = bb.gaussian_approximation(refactorize_final=True)
    assert info["converged"].all()
    pos = bb.observations_hess_map() if a.design else diag_positions(Qs[0])
    POST = NZ.copy(order="F")
    POST[pos, :] -= H
    perm = bb.ordering_permutation()
    f64 = dict(dtype=torch.float64, device=dev)
    dP = torch.from_numpy(np.ascontiguousarray(POST.T).reshape(-1)).to(dev)
    dX = torch.from_numpy(np.ascontiguousarray(X.T).reshape(-1)).to(dev)
    dM, dV, dL = (torch.empty(nobs * B, **f64) for _ in range(3))
    mix = [torch.empty(nobs, **f64) for _ in range(3)]
    nnz = Qs[0].nnz
    tb, ts, tr = [], [], []      # batched route; plain route with the host mixture; the plain read-outs alone
    for r in range(a.warmup + a.reps):
        bb.refactorize_dev(dP.data_ptr())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        i1 = bb.predictor_marginals_dev(dX.data_ptr(), n, dM.data_ptr(), dV.data_ptr())
        tot, i2 = bb.predictive_scores_dev(dM.data_ptr(), dV.data_ptr(), a.K, d_lpd=dL.data_ptr())
        total = bb.predictive_mixture_dev(logw, dM.data_ptr(), dV.data_ptr(), dL.data_ptr(), *(t.data_ptr() for t in mix))
        torch.cuda.synchronize()
        if r >= a.warmup:
            tb.append(1e3 * (time.perf_counter() - t0))
    assert (i1 == 0).all() and (i2 == 0).all()
    batch_arrays = [t.cpu().numpy().reshape(B, nobs).copy() for t in (dM, dV, dL)]
    batch_mix = [t.cpu().numpy().copy() for t in mix]
    bb.close()

    plain = gmrfx.MI355XBackend(Qs[0], ordering=perm, device=0, factorize=False)
    if a.design:
        plain.set_design_observations("poisson", y, A)
    else:
        plain.set_observations("poisson", y)
    pM, pV, pL = (torch.empty(nobs * B, **f64) for _ in range(3))
    om = np.exp(logw - logw.max())
    om /= om.sum()
    for r in range(a.warmup + a.reps):
        t = 0.0
        for k in range(B):
            plain.refactorize_dev(dP.data_ptr() + 8 * k * nnz)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = 8 * k * nobs
            plain.predictor_marginals_dev(dX.data_ptr() + 8 * k * n, pM.data_ptr() + o, pV.data_ptr() + o)
            plain.predictive_scores_dev(pM.data_ptr() + o, pV.data_ptr() + o, z, w, pL.data_ptr() + o)
            torch.cuda.synchronize()
            t += time.perf_counter() - t0
        t_read = t
        t0 = time.perf_counter()        # the mixture on the host, from the downloaded arrays
        hM, hV, hL = (x.cpu().numpy().reshape(B, nobs) for x in (pM, pV, pL))
        mm = om @ hM
        mv = om @ (hV + (hM - mm) ** 2)
        al = np.log(om)[:, None] + hL
        ml = al.max(axis=0) + np.log(np.exp(al - al.max(axis=0)).sum(axis=0))
        t += time.perf_counter() - t0
        if r >= a.warmup:
            ts.append(1e3 * t)
            tr.append(1e3 * t_read)
    plain_arrays = [x.cpu().numpy().reshape(B, nobs) for x in (pM, pV, pL)]
    plain.close()
    same = all(np.array_equal(u.view(np.int64), v.view(np.int64)) for u, v in zip(batch_arrays, plain_arrays))
    sb, sp_, sr = summary(tb), summary(ts), summary(tr)
    row = {"tool": "tools/batch_predictive_bench.py" + (" --design" if a.design else ""), "device": torch.cuda.get_device_name(0),
           "source_tree_hash": _lib.source_tree_hash(), "n": n, "nobs": nobs, "grid": g, "B": B, "K": a.K, "family": "poisson", "reps": a.reps,
           "warmup": a.warmup, "batched": sb, "one_plain_handle_sequential": sp_, "one_plain_handle_readouts_only": sr,
           "speedup_vs_readouts_only": sr["median_ms"] / sb["median_ms"], "speedup_vs_sequential": sp_["median_ms"] / sb["median_ms"],
           "batched_not_slower": sb["median_ms"] <= sr["median_ms"], "members_same_bits": bool(same), "mixture_total": total,
           "max_abs_mixture_diff": float(max(np.abs(batch_mix[0] - mm).max(), np.abs(batch_mix[1] - mv).max(), np.abs(batch_mix[2] - ml).max()))}
    print(json.dumps(row), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "batch_predictive_bench_design.json" if a.design else "batch_predictive_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
