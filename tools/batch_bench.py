#!/usr/bin/env python3
"""Batched handles against one handle called B times: the hyper-parameter loop of the reference's tutorial
(docs/src/literate-tutorials/workspace_factorization_reuse.jl: logpdf at many hyper-parameter values with one pattern).

Problems: 2-D Matern (alpha = 2) on jittered n = 40^2, 100^2, 250^2 meshes; member k has its own tau and kappa (range), the
pattern is the same. For B in {1, 8, 50, 128}:
  (a) B sequential gmrfx_refactorize_logpdf_dev calls on one plain handle (member values, z, all in HBM);
  (b) one gmrfx_batch_refactorize_logpdf_dev on a batched handle of B members.
Reported: microseconds PER EVALUATION (= per member), median over --reps timed repetitions after --warmup, the GPU synchronised
around each timed region; ms_symbolic and bytes_device_total of both handles; the source tree hash.
usage: tools/batch_bench.py [--grids 40,100,250] [--batches 1,8,50,128] [--reps 25] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gmrfx  # noqa: E402
from gmrfx import _lib, spde  # noqa: E402


def member_values(mesh, B, rng):
    """Q_k = matern(tau_k, range_k) on one pattern: (pattern of member 0, nnz x B values)"""
    Qs = []
    for k in range(B):
        Qs.append(spde.matern_precision(mesh, 0, float(rng.uniform(0.15, 0.4)), tau=float(rng.uniform(0.5, 2.0))).tocsc())
    Q0 = Qs[0]
    for Q in Qs[1:]:
        assert np.array_equal(Q.indptr, Q0.indptr) and np.array_equal(Q.indices, Q0.indices), "pattern changed with the values"
    return Q0, np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))


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
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="40,100,250")
    ap.add_argument("--batches", default="1,8,50,128")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = _lib.source_tree_hash()
    rows = []
    for g in (int(x) for x in a.grids.split(",")):
        mesh = spde.grid_mesh_2d(g, g, jitter=0.25, seed=0)
        Bmax = max(int(x) for x in a.batches.split(","))
        Q, NZall = member_values(mesh, Bmax, np.random.default_rng(g))
        n, nnz = Q.shape[0], Q.nnz
        plain = gmrfx.MI355XBackend(Q, coords=mesh.points, device=0)
        perm = plain.ordering_permutation()
        st_plain = plain.stats()
        z = np.random.default_rng(1).standard_normal((n, Bmax))
        for B in (int(x) for x in a.batches.split(",")):
            d_nz = torch.from_numpy(np.ascontiguousarray(NZall[:, :B].T).reshape(-1)).cuda()     # nnz x B column-major
            d_z = torch.from_numpy(np.ascontiguousarray(z[:, :B].T).reshape(-1)).cuda()         # n x B column-major
            torch.cuda.synchronize()
            ptr_nz, ptr_z = d_nz.data_ptr(), d_z.data_ptr()

            def seq():
                for k in range(B):
                    plain.refactorize_logpdf_dev(ptr_nz + 8 * k * nnz, ptr_z + 8 * k * n, n, 1)
            t_seq, t_seq_min = timed(seq, a.reps, a.warmup)
            bb = gmrfx.MI355XBatchBackend(Q, B, ordering=perm, device=0)
            st_b = bb.stats()

            def bat():
                bb.refactorize_logpdf_dev(ptr_nz, ptr_z, n, n, 1)
            t_bat, t_bat_min = timed(bat, a.reps, a.warmup)
            # the two agree (member by member: logdet and quadratic form)
            ld_b, q_b, info_b = bb.refactorize_logpdf_dev(ptr_nz, ptr_z, n, n, 1)
            q_p, ld_p = plain.refactorize_logpdf_dev(ptr_nz + 8 * (B - 1) * nnz, ptr_z + 8 * (B - 1) * n, n, 1)
            agree = max(abs(ld_b[-1] - ld_p) / abs(ld_p), abs(q_b[0, -1] - q_p[0]) / abs(q_p[0]))
            row = {"n": n, "grid": g, "B": B, "us_per_eval_sequential": 1e6 * t_seq / B, "us_per_eval_batched": 1e6 * t_bat / B,
                   "speedup": t_seq / t_bat, "us_per_eval_sequential_min": 1e6 * t_seq_min / B, "us_per_eval_batched_min": 1e6 * t_bat_min / B,
                   "ms_symbolic_plain": st_plain["ms_symbolic"], "ms_symbolic_batched": st_b["ms_symbolic"],
                   "bytes_device_total_plain": st_plain["bytes_device_total"], "bytes_device_total_batched": st_b["bytes_device_total"],
                   "nlevels": st_b["nlevels"], "max_rel_diff_last_member": agree, "info_max": int(np.max(info_b)),
                   "reps": a.reps, "warmup": a.warmup, "source_tree_hash": tree}
            print(json.dumps(row), flush=True)
            rows.append(row)
            bb.close()
            del d_nz, d_z
        plain.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/batch_bench.py", "device": torch.cuda.get_device_name(0), "source_tree_hash": tree, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
