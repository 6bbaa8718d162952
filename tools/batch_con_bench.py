#!/usr/bin/env python3
"""One constrained logpdf evaluation per member: a batched handle with a batch constraint against what had to be done without it.

Problems: a 2-D Matern (alpha = 2) precision on a jittered g x g mesh and a Besag lattice (graph Laplacian of the g x g grid
+ 1e-5 I), g = 40 and 100 (n = 1 600, 10 000); member k has its own tau (and range, for the Matern), the pattern is the same.
Constraint: m = 1 (sum to zero) or m = 16 (that row + 15 sparse rows of 7 entries), the same for all members.
For B in {1, 8, 50}:
  (a) B plain handles, each with the constraint set, each evaluated by gmrfx_refactorize_logpdf_dev + gmrfx_constraints_mean
      (log_correction only) -- the only way before batch constraints existed;
  (b) one gmrfx_batch_constrained_logpdf_dev on a batched handle of B members.
Member values and z live in HBM. Reported: microseconds PER EVALUATION (= per member), median (and minimum) over --reps timed
repetitions after --warmup, the GPU synchronised around each timed region; the largest relative difference of the two paths'
log det, quadratic form and log_correction; the source tree hash.
usage: tools/batch_con_bench.py [--grids 40,100] [--batches 1,8,50] [--rows 1,16] [--reps 25] [--warmup 3] [--out FILE]"""
import argparse
import ctypes as C
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


def matern_members(g, B, rng):
    mesh = spde.grid_mesh_2d(g, g, jitter=0.25, seed=0)
    Qs = [spde.matern_precision(mesh, 0, float(rng.uniform(0.15, 0.4)), tau=float(rng.uniform(0.5, 2.0))).tocsc() for _ in range(B)]
    return Qs, mesh.points


def besag_members(g, B, rng):
    path = sp.diags([-np.ones(g - 1), -np.ones(g - 1)], [-1, 1])
    adj = sp.kron(sp.identity(g), path) + sp.kron(path, sp.identity(g))
    lap = sp.diags(-np.asarray(adj.sum(axis=1)).ravel()) + adj + 1e-5 * sp.identity(g * g)
    pts = np.stack(np.meshgrid(np.arange(g, dtype=float), np.arange(g, dtype=float), indexing="ij"), axis=-1).reshape(-1, 2)
    return [sp.csc_matrix(float(rng.uniform(0.5, 2.0)) * lap) for _ in range(B)], pts


def values(Qs):
    for Q in Qs:
        Q.sort_indices()
        assert np.array_equal(Q.indptr, Qs[0].indptr) and np.array_equal(Q.indices, Qs[0].indices), "pattern changed with the values"
    return np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))


def constraint(n, m, rng):
    A = sp.lil_matrix((m, n))
    A[0, :] = 1.0
    for r in range(1, m):
        A[r, rng.choice(n, size=7, replace=False)] = rng.standard_normal(7)
    e = np.zeros(m)
    e[1:] = rng.standard_normal(m - 1)
    return sp.csr_matrix(A), e


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
    ap.add_argument("--grids", default="40,100")
    ap.add_argument("--batches", default="1,8,50")
    ap.add_argument("--rows", default="1,16")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = _lib.source_tree_hash()
    L = _lib.lib()
    batches = [int(x) for x in a.batches.split(",")]
    rows = []
    for model, make in (("matern", matern_members), ("besag", besag_members)):
        for g in (int(x) for x in a.grids.split(",")):
            Qs, pts = make(g, max(batches), np.random.default_rng(g))
            NZall = values(Qs)
            n, nnz = Qs[0].shape
            nnz = Qs[0].nnz
            z = np.random.default_rng(1).standard_normal((n, max(batches)))
            for m in (int(x) for x in a.rows.split(",")):
                A, e = constraint(n, m, np.random.default_rng(100 + m))
                for B in batches:
                    d_nz = torch.from_numpy(np.ascontiguousarray(NZall[:, :B].T).reshape(-1)).cuda()     # nnz x B column-major
                    d_z = torch.from_numpy(np.ascontiguousarray(z[:, :B].T).reshape(-1)).cuda()         # n x B column-major
                    torch.cuda.synchronize()
                    ptr_nz, ptr_z = d_nz.data_ptr(), d_z.data_ptr()
                    bb = gmrfx.MI355XBatchBackend(Qs[0], B, coords=pts, device=0)
                    bb.set_constraints(A, e)
                    perm = bb.ordering_permutation()
                    plain = [gmrfx.MI355XBackend(Qs[0], ordering=perm, device=0, factorize=False) for _ in range(B)]
                    for p in plain:
                        p.set_constraints(A, e)
                    lc_seq, ld_seq, q_seq = np.zeros(B), np.zeros(B), np.zeros(B)

                    def seq():
                        lc = C.c_double(0.0)
                        for k, p in enumerate(plain):
                            q, ld = p.refactorize_logpdf_dev(ptr_nz + 8 * k * nnz, ptr_z + 8 * k * n, n, 1)
                            _lib.check(L.gmrfx_constraints_mean(p._h, None, None, C.byref(lc)), p._h)
                            lc_seq[k], ld_seq[k], q_seq[k] = lc.value, ld, q[0]
                    t_seq, t_seq_min = timed(seq, a.reps, a.warmup)
                    out = []

                    def bat():
                        out[:] = bb.constrained_logpdf_dev(ptr_nz, ptr_z, n, n, 1)
                    t_bat, t_bat_min = timed(bat, a.reps, a.warmup)
                    ld_b, q_b, lc_b, info_b, cinfo_b = out
                    agree = float(max(np.abs(ld_b / ld_seq - 1).max(), np.abs(q_b[0] / q_seq - 1).max(), np.abs(lc_b / lc_seq - 1).max()))
                    row = {"model": model, "n": n, "grid": g, "m": m, "B": B, "us_per_eval_plain_handles": 1e6 * t_seq / B,
                           "us_per_eval_batched": 1e6 * t_bat / B, "speedup": t_seq / t_bat, "us_per_eval_plain_handles_min": 1e6 * t_seq_min / B,
                           "us_per_eval_batched_min": 1e6 * t_bat_min / B, "prepare_ms_batched": bb.constraint_info()["ms"],
                           "max_rel_diff": agree, "info_max": int(np.max(info_b)), "cinfo_max": int(np.max(np.abs(cinfo_b))),
                           "reps": a.reps, "warmup": a.warmup, "source_tree_hash": tree}
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                    bb.close()
                    for p in plain:
                        p.close()
                    del d_nz, d_z
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/batch_con_bench.py", "device": torch.cuda.get_device_name(0), "source_tree_hash": tree, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
