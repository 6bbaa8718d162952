#!/usr/bin/env python3
"""The log-density gradient on Q's pattern (gmrfx_logpdf_grad / gmrfx_batch_logpdf_grad) beside the two routes the library offered
before it: (a) gmrfx_selinv_csc, the whole selected inverse over PCIe, + numpy; (b) gmrfx_selinv_extract on pattern(Q) + numpy.

Problems: 2-D Matern (smoothness 0) grids of 250^2 and 1000^2 nodes on a plain handle, and B = 50 members of 100^2 nodes on a batched
handle (routes (a) / (b) there: a plain handle on one member, timed, times B -- a batched handle offers no other way). The selected
inversion is computed once per factorisation and cached, so it is reported apart (gmrfx_stats.ms_selinv of a fresh factorisation) and
every timed call below finds it done. Reported per case: milliseconds -- median (and minimum) over --reps repetitions after --warmup,
wall clock around the call -- of the host form (Qbar and mubar arrive in host memory), of the _dev form (operands in HBM, GPU
synchronised around the timed region), of gmrfx_pattern_dot_dev with p = 4, of the two old routes (Qbar = ybar/2 (Sigma - r r') on the
pattern and mubar = ybar Q r in numpy), the bytes each route moves over PCIe, and the source tree hash. No time is a pass criterion.
usage: tools/grad_bench.py [--cases 2d:250,2d:1000,batch:50x100] [--reps 15] [--warmup 2] [--out profiles/grad_bench.json]"""
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


def old_routes(be, Q, z, ybar):
    """(a) the whole selected inverse, (b) the extraction on pattern(Q); both finish in numpy"""
    cols = np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))
    rr = z[Q.indices] * z[cols]

    def a():
        be._selinv_cache = None
        S = be.get_selinv()
        sig = np.asarray(S[Q.indices, cols]).ravel()
        return 0.5 * ybar * (sig - rr), ybar * (Q @ z)

    def b():
        sig = be.selinv_extract_at(Q).data
        return 0.5 * ybar * (sig - rr), ybar * (Q @ z)

    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2d:250,2d:1000,batch:50x100")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_bench.json"))
    a = ap.parse_args()
    tree = _lib.source_tree_hash()
    rows = []
    for case in a.cases.split(","):
        kind, spec = case.split(":")
        B, g = (int(x) for x in spec.split("x")) if kind == "batch" else (1, int(spec))
        mesh = spde.grid_mesh_2d(g, g, jitter=0.25, seed=0)
        Q = sp.csc_matrix(spde.matern_precision(mesh, smoothness=0, range_=0.2))
        Q = sp.csc_matrix((Q + Q.T) * 0.5)
        Q.sort_indices()
        n, nnz = Q.shape[0], Q.nnz
        rng = np.random.default_rng(0)
        ybar = 1.0
        row = {"case": case, "n": n, "nnz": int(nnz), "nbatch": B, "reps": a.reps, "warmup": a.warmup, "source_tree_hash": tree}
        be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0)
        sel = []
        for _ in range(3):
            be.refactorize_values(Q.data)
            be.get_selinv_diag()
            sel.append(be.stats()["ms_selinv"])
            be._selinv_diag_cache = None
        row["ms_selinv_member"] = float(np.median(sel))
        C_nnz = int(be.get_selinv().nnz)
        row["pcie_bytes_selinv_csc"] = 8 * C_nnz + 8 * C_nnz + 8 * (n + 1)
        row["pcie_bytes_selinv_extract"] = 8 * nnz
        row["pcie_bytes_logpdf_grad_host"] = 8 * (nnz + 2 * n)
        row["nnz_selinv_over_nnz_q"] = C_nnz / nnz
        z = rng.standard_normal(n)
        ra, rb = old_routes(be, Q, z, ybar)
        big = n > 200000                         # the whole selected inverse of the 1000^2 mesh is 4 10^8 values: one repetition
        ta, ta_min = timed(ra, 1 if big else max(3, a.reps // 3), 0 if big else 1)
        tb, tb_min = timed(rb, a.reps, a.warmup)
        row.update(ms_route_selinv_csc=ta * B, ms_route_selinv_csc_min=ta_min * B, ms_route_selinv_extract=tb * B, ms_route_selinv_extract_min=tb_min * B)
        if kind != "batch":
            th, th_min = timed(lambda: be.logpdf_grad(z, ybar=ybar), a.reps, a.warmup)
            dz = torch.from_numpy(z).cuda()
            dq = torch.empty(nnz, dtype=torch.float64, device="cuda")
            dm = torch.empty(n, dtype=torch.float64, device="cuda")
            dJ = torch.randn((4, nnz), dtype=torch.float64, device="cuda")
            td, td_min = timed(lambda: be.logpdf_grad_dev(dz.data_ptr(), dq.data_ptr(), dm.data_ptr()), a.reps, a.warmup)
            tp, tp_min = timed(lambda: be.pattern_dot_dev(dq.data_ptr(), dJ.data_ptr(), nnz, 4), a.reps, a.warmup)
            want = rb()
            row["max_abs_diff_vs_extract_route"] = float(np.abs(dq.cpu().numpy() - want[0]).max())
        else:
            bb = gmrfx.MI355XBatchBackend(Q, B, coords=mesh.points, device=0)
            NZ = np.asfortranarray(np.stack([(1.0 + 0.01 * k) * Q.data for k in range(B)], axis=1))
            bb.refactorize_values(NZ)
            Z = np.asfortranarray(rng.standard_normal((n, B)))
            bb.selinv_diag()
            row["ms_selinv"] = bb.stats()["ms_selinv"]
            th, th_min = timed(lambda: bb.logpdf_grad(Z, ybar=ybar), a.reps, a.warmup)
            dz = torch.from_numpy(Z.ravel(order="F").copy()).cuda()
            dq = torch.empty(nnz * B, dtype=torch.float64, device="cuda")
            dm = torch.empty(n * B, dtype=torch.float64, device="cuda")
            dJ = torch.randn((B * 4, nnz), dtype=torch.float64, device="cuda")
            td, td_min = timed(lambda: bb.logpdf_grad_dev(dz.data_ptr(), n, ybar, dq.data_ptr(), dm.data_ptr()), a.reps, a.warmup)
            tp, tp_min = timed(lambda: bb.pattern_dot_dev(dq.data_ptr(), dJ.data_ptr(), nnz, 4 * nnz, 4), a.reps, a.warmup)
            bb.close()
        row.update(ms_logpdf_grad_host=th, ms_logpdf_grad_host_min=th_min, ms_logpdf_grad_dev=td, ms_logpdf_grad_dev_min=td_min,
                   ms_pattern_dot_dev_p4=tp, ms_pattern_dot_dev_p4_min=tp_min)
        print(json.dumps(row), flush=True)
        rows.append(row)
        be.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/grad_bench.py", "device": torch.cuda.get_device_name(0), "source_tree_hash": tree, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
