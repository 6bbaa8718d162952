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
--old PATH/TO/libgmrfx.so: an A/B of the existing constrained calls between this build and another one, alternating in one process
(see ab(); profiles/batch_con_mask_ab.json).
usage: tools/batch_con_bench.py [--old PATH [--rounds 4]] [--grids 40,100] [--batches 1,8,50] [--rows 1,16] [--reps 25] [--warmup 3] [--out FILE]"""
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


def ab(a):
    """--old PATH: the same calls on this build and on another one (the parent commit's), alternating in ONE process: `--rounds`
    medians per side, each the median of `--reps` synchronised calls after `--warmup`. Besag, g = 100 (n = 10 000), B = 50, m = 16:
    gmrfx_batch_constrained_logpdf_dev (prepare + the reduction A x), gmrfx_batch_sample_dev with 64 columns (the reduction and the
    MFMA correction kernel) and the same two on a plain handle (one member, gmrfx_refactorize_logpdf_dev + gmrfx_constraints_mean;
    gmrfx_sample_dev). Also the widths of one forest solve on the new build's factor: 1, m and m + 1 columns for m = 1 and 16."""
    libs = {"new": _lib.lib(), "old": _lib.load_from(a.old)}
    g, B, m, nvec = 100, 50, 16, 64
    Qs, pts = besag_members(g, B, np.random.default_rng(g))
    NZ = values(Qs)
    n, nnz = Qs[0].shape[0], Qs[0].nnz
    A, e = constraint(n, m, np.random.default_rng(100 + m))
    rng = np.random.default_rng(1)
    d_nz = torch.from_numpy(np.ascontiguousarray(NZ.T).reshape(-1)).cuda()
    d_z = torch.from_numpy(rng.standard_normal(n * B)).cuda()
    d_Z = torch.from_numpy(rng.standard_normal(n * nvec * B)).cuda()
    d_X = torch.empty(n * nvec * B, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    side = {}
    for tag, L in libs.items():
        _lib.use(L)
        bb = gmrfx.MI355XBatchBackend(Qs[0], B, coords=pts, device=0)
        bb.set_constraints(A, e)
        p = gmrfx.MI355XBackend(Qs[0], ordering=bb.ordering_permutation(), device=0, factorize=False)
        p.set_constraints(A, e)
        side[tag] = (bb, p)
    lc = C.c_double(0.0)

    def calls(tag):
        bb, p = side[tag]
        L = libs[tag]

        def plain_logpdf():
            p.refactorize_logpdf_dev(d_nz.data_ptr(), d_z.data_ptr(), n, 1)
            _lib.check(L.gmrfx_constraints_mean(p._h, None, None, C.byref(lc)), p._h)
        return {"batch_constrained_logpdf_dev": lambda: bb.constrained_logpdf_dev(d_nz.data_ptr(), d_z.data_ptr(), n, n, 1),
                "batch_sample_dev_64": lambda: bb.sample_dev(d_Z.data_ptr(), n, n * nvec, nvec, d_X.data_ptr(), n, n * nvec),
                "plain_logpdf_dev": plain_logpdf,
                "plain_sample_dev_64": lambda: p.sample_dev(d_Z.data_ptr(), n, nvec, d_X.data_ptr(), n)}
    names = list(calls("new"))
    medians = {nm: {"old": [], "new": []} for nm in names}
    bits = {nm: {} for nm in names}
    for nm in names:
        for r in range(a.rounds):
            for tag in (("old", "new") if r % 2 == 0 else ("new", "old")):
                _lib.use(libs[tag])
                fn = calls(tag)[nm]
                t, _ = timed(fn, a.reps, a.warmup)
                medians[nm][tag].append(1e3 * t)
                if "sample" in nm:
                    bits[nm][tag] = d_X[:n * nvec * (B if "batch" in nm else 1)].cpu().numpy().copy()
    rows = []
    for nm in names:
        old, new = medians[nm]["old"], medians[nm]["new"]
        row = {"call": nm, "old_median_ms": old, "new_median_ms": new, "old_spread_ms": max(old) - min(old),
               "new_max_above_old_max_ms": max(new) - max(old), "inside_old_spread": max(new) - max(old) <= max(old) - min(old)}
        if bits[nm]:
            row["same_bits"] = bool(np.array_equal(bits[nm]["old"].view(np.int64), bits[nm]["new"].view(np.int64)))
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the widths of one forest solve (B = 50 members) on the factor in hand: what a fused [score, A'] pass would have to beat
    _lib.use(libs["new"])
    bb = side["new"][0]
    widths = {}
    for w in (1, 2, 16, 17):
        t, tmin = timed(lambda: bb.solve_dev(d_Z.data_ptr(), n, n * nvec, w, d_X.data_ptr(), n, n * nvec), a.reps, a.warmup)
        widths[str(w)] = {"median_ms": 1e3 * t, "min_ms": 1e3 * tmin}
    print(json.dumps({"forest_solve_width_ms": widths}), flush=True)
    res = {"tool": "tools/batch_con_bench.py --old", "device": torch.cuda.get_device_name(0), "source_tree_hash": _lib.source_tree_hash(),
           "model": "besag", "n": n, "B": B, "m": m, "nvec": nvec, "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup, "rows": rows,
           "forest_solve_width_ms": widths}
    for tag in side:
        _lib.use(libs[tag])
        for h in side[tag]:
            h.close()
    _lib.use(libs["new"])
    out = a.out or os.path.join(ROOT, "profiles", "batch_con_mask_ab.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="another build of libgmrfx.so: A/B of the existing constrained calls against it")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--grids", default="40,100")
    ap.add_argument("--batches", default="1,8,50")
    ap.add_argument("--rows", default="1,16")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.old:
        if a.reps == 25:
            a.reps = 15
        return ab(a)
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
