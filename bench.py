#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path on MI355X.

Metric (BASELINE.json): factor + solve(64 RHS) throughput in DoF/s on the 1M-node 2-D Matérn
(nu=1 => smoothness=0, alpha=2) SPDE precision; a "step" = one numeric refactorisation on the
fixed pattern (update_precision_values! -> ensure_numeric!) followed by one 64-RHS solve
(workspace_solve(ws, B)), with nzval and B already resident in HBM. Symbolic analysis is
excluded from the step and reported separately.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--grid G] [--nrhs R] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line (headline, phases of the timed steps, logdet of the
last step). --full adds everything else the benchmark measures: the separate-call steps, logpdf, host I/O, cfg 3, the
rooflines, the CPU baseline and, for N > 1, the distributed-X step, the per-level probe and the cfg-4 line.
--dump-outputs DIR writes what the last timed step returned (a fixed sample of the rows of X, the column norms of X, logdet)
as DIR/<name>.npy in float64, so that two builds can be compared output for output; the inputs are seeded.

N > 1: one process per GPU (torch.distributed, backend nccl = RCCL). The headline is ONE
factorisation + 64-RHS solve SHARDED over the N GPUs (strong scaling: `value` = n / step time;
gmrfx/shard.py); the independent-replica throughput (one workspace per GPU, the reference's
WorkspacePool pattern, weak scaling) is reported beside it under "replicas", and becomes the
headline only if the sharded path fails or with --no-shard. Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

T_START = time.time()              # N > 1: the line must be out before the launcher's limit (see --deadline)
# the host driver of this pool only supports dmabuf IPC: without it RCCL across processes fails with `hipIpcGetMemHandle: invalid
# argument` (exported on the boxes already; kept here for any environment that is built from scratch -- before anything loads HIP)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def launch_time():
    """When the RUN started: the creation time of the launcher (`python -m torch.distributed.run` / torchrun, whose own first
    `import torch` on a fresh box can take a minute or two before any rank exists) when this process is one of its ranks, else the
    import time of this module."""
    try:
        import psutil
        p = psutil.Process(os.getppid())
        cmd = " ".join(p.cmdline())
        if "torch.distributed.run" in cmd or "torchrun" in cmd or "torch/distributed" in cmd:
            return min(T_START, p.create_time())
    except Exception:
        pass
    return T_START


ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SHARD_TIMEOUT_EXIT = 3     # the sharded (strong-scaling) run hung: replica line printed with the error, every rank exits 3
SHARD_FAILED_EXIT = 4      # the sharded run raised: replica line printed with the error, every rank exits 4
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable)
FP64_MFMA_PEAK_TF = 78.6   # datasheet FP64 matrix peak (32 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz)
FP64_MFMA_MEASURED_TF = 75.7   # sustained v_mfma_f64_16x16x4_f64 with >= 2 issuing waves per SIMD (tools/micro/mix64.hip);
                               # ONE wave per SIMD only issues one per ~138 cycles = 36.3 (tools/micro/mfma64.hip); an LDS-staged
                               # 128x128-tile DGEMM reaches 54 (tools/micro/dgemm_mfma.hip)


LAUNCH_FLOOR_US = 2.0      # what ONE dependent launch costs on the GPU side whatever it does: 0.9 us launch-to-launch boundary (a chain
                           # of dependent kernels that each spin 5 / 10 us costs 5.89 / 10.88 us per launch, stream or graph alike) +
                           # the ~1 us cold start of a one-round-trip kernel (tools/micro/launch_floor.hip, profiles/r04_barrier_lat.txt)
COPY_PEAK_GUIDE_GBS = 6290.0   # MI355X_MICROARCH.md: achievable HBM copy rate; the live figure of this box is measured below


def measure_copy_peak(dev, nbytes=1 << 30):
    """Device-to-device copy rate of this box, read + write bytes over HIP-event time (the sweep's roofline is quoted
    against peak AND against what a plain copy reaches here)."""
    import torch
    a = torch.empty(nbytes // 8, dtype=torch.float64, device=dev).normal_()
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(5):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    del a, b
    return 2.0 * nbytes / (ms * 1e-3) / 1e9


DUMP_X_BYTES = 32 << 20    # --dump-outputs: the rows of X written stay under this (the whole dump under 64 MB)


def output_rows(n, nrhs):
    """The rows of X that --dump-outputs writes: all of them when they fit DUMP_X_BYTES, else a fixed seeded sample (sorted)."""
    import numpy as np
    k = max(1, min(n, DUMP_X_BYTES // (8 * nrhs)))
    if k == n:
        return np.arange(n)
    return np.sort(np.random.default_rng(2024).choice(n, k, replace=False))


def dump_outputs(outdir, X_rows, rows, col_norms, logdet):
    """--dump-outputs: what the timed call returned, in float64 -- X at `rows` (len(rows) x nrhs), the indices `rows`, the 2-norm
    of every column of X over all n rows, and logdet"""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    for name, a in (("X_sample", X_rows), ("X_sample_rows", rows), ("X_column_norms", col_norms), ("logdet", [logdet])):
        np.save(os.path.join(outdir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def sweep_model_bound(be, nrhs, copy_gbs, floor_us=LAUNCH_FLOOR_US, small_rows=64):
    """A defensible CEILING for the multifrontal triangular sweeps as they are scheduled here -- the number that belongs next to the
    70 %-of-HBM-peak target of the north star. For the sweep-task launch and for every tree level, forward and backward:
        (algorithmic bytes + the W / x hand-off the level moves through HBM) / copy peak  +  launches x per-launch floor.
    Algorithmic bytes of a front: panel 8 r c, row list 4 r, own rows of X read and written 16 c nrhs. Hand-off: the
    update vector of a front, 8 nrhs (r - c) bytes, is written once by the front and read once by its parent's level in the forward
    sweep (fronts INSIDE a sweep task hand off in LDS: only task roots write); in the backward sweep a front gathers its r - c trailing
    rows of x. Launches per level as device.cpp enqueues them: forward = one per non-empty small-front class + assemble, triangular
    product, update for the big fronts; backward = small classes + one launch (k_bwd_front) or two. The bound concedes the hand-off
    (a supernodal sweep WITHOUT per-front update vectors would not move it) and the level-by-level launch structure; what is left
    between it and the measured time is the kernels'."""
    import numpy as np
    sy = be.symbolic()
    c = np.diff(sy.super_first).astype(np.float64)
    r = np.diff(sy.row_ptr).astype(np.float64)
    m = r - c
    lev = np.asarray(sy.level)
    par = np.asarray(sy.super_parent)
    _, tf, tl, _ = be.sweep_tasks()
    in_task = np.zeros(len(c), bool)
    for a, b in zip(tf, tl):
        in_task[a:b + 1] = True
    roots = np.zeros(len(c), bool)
    roots[np.asarray(tl, dtype=np.int64)] = True
    alg = 8 * r * c + 4 * r + 16 * c * nrhs
    hand = 8.0 * nrhs * m
    small = (c <= 64) & (r <= small_rows)
    cls48 = small & (r <= 48)
    fwd_b = bwd_b = 0.0
    fwd_l = bwd_l = 0
    rows = []
    if in_task.any():
        fb = float(alg[in_task].sum() + hand[roots].sum())          # task roots write their update vector
        bb = float(alg[in_task].sum() + hand[roots].sum())          # ... and gather their trailing x
        fwd_b += fb; bwd_b += bb; fwd_l += 1; bwd_l += 1
        rows.append({"level": -1, "fronts": int(in_task.sum()), "fwd_bytes": fb, "bwd_bytes": bb, "fwd_launches": 1, "bwd_launches": 1})
    for lv in range(int(lev.max()) + 1):
        sel = (~in_task) & (lev == lv)
        if not sel.any():
            continue
        kid = np.isin(par, np.nonzero(sel)[0]) & (par >= 0) & (~in_task | roots)
        fb = float(alg[sel].sum() + hand[sel].sum() + hand[kid].sum())
        bb = float(alg[sel].sum() + hand[sel].sum())
        ncls = int((sel & cls48).any()) + int((sel & small & ~cls48).any())
        big = sel & ~small
        # (round 6: k_fwd_front takes the fronts of at most 128 columns of a level that has at least 384 of them: one launch)
        ff = big & (c <= 128)
        fl = ncls + ((1 + (3 if (big & ~ff).any() else 0)) if ff.sum() >= 384 else (3 if big.any() else 0))
        bl = ncls + (0 if not big.any() else (1 if (c[big] <= 128).all() else 2))
        fwd_b += fb; bwd_b += bb; fwd_l += fl; bwd_l += bl
        rows.append({"level": lv, "fronts": int(sel.sum()), "fwd_bytes": fb, "bwd_bytes": bb, "fwd_launches": fl, "bwd_launches": bl})
    ms = lambda by, nl: by / (copy_gbs * 1e9) * 1e3 + nl * floor_us * 1e-3
    return {"fwd_ms": ms(fwd_b, fwd_l), "bwd_ms": ms(bwd_b, bwd_l), "fwd_bytes": fwd_b, "bwd_bytes": bwd_b, "fwd_launches": fwd_l,
            "bwd_launches": bwd_l, "handoff_bytes_fwd": float(fwd_b - alg.sum()), "handoff_bytes_bwd": float(bwd_b - alg.sum()),
            "levels": rows}


def cholmod_reference(Q, perm, Bn, workdir):
    """The reference's own CPU path (Julia + CHOLMOD) when a `julia` binary exists on this box: bench/cholmod_baseline.jl
    on the same Q / permutation / right-hand sides. Returns its JSON object, or a note that it is unavailable."""
    import shutil
    import subprocess
    import numpy as np
    jl = shutil.which("julia")
    if jl is None:
        return {"status": "CHOLMOD baseline unavailable on this box (no `julia` on PATH)"}
    try:
        os.makedirs(workdir, exist_ok=True)
        n = Q.shape[0]
        np.array([n, Q.nnz, Bn.shape[1]], dtype=np.int64).tofile(os.path.join(workdir, "meta.bin"))
        (Q.indptr.astype(np.int64) + 1).tofile(os.path.join(workdir, "colptr.bin"))
        (Q.indices.astype(np.int64) + 1).tofile(os.path.join(workdir, "rowval.bin"))
        Q.data.astype(np.float64).tofile(os.path.join(workdir, "nzval.bin"))
        (np.asarray(perm, dtype=np.int64) + 1).tofile(os.path.join(workdir, "perm.bin"))
        np.asfortranarray(Bn).T.copy().tofile(os.path.join(workdir, "B.bin"))       # column-major n x nrhs
        # second argument: the script also writes the parity vectors (logdet, F \ B, F.UP \ z, ...; tests/test_cholmod_parity.py);
        # under gpurun_out/ they travel back from a GPU box
        r = subprocess.run([jl, "-t", "auto", os.path.join(ROOT, "bench", "cholmod_baseline.jl"), workdir,
                            os.path.join(ROOT, "gpurun_out", "cholmod_out")],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"status": "julia found but the CHOLMOD script failed", "stderr": r.stderr[-400:]}
        return json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:          # the baseline must never break the bench line
        return {"status": "julia found but the CHOLMOD script failed", "error": repr(e)}


def cpu_baseline(Q, mesh, nrhs: int):
    """CPU stand-in for the reference's CHOLMOD path on the FULL workload of the bench line: oracle/supernodal_cpu.c, a
    multi-threaded supernodal multifrontal LL' + blocked multi-RHS solve on OpenBLAS kernels (kind "port"), same Q,
    same permutation, same supernode partition as the GPU path; steady-state numeric refactorisation (second of two)
    + one nrhs-column solve, like the GPU step. Julia/CHOLMOD itself is timed beside it when the box has Julia."""
    import numpy as np
    import gmrfx
    import sncpu
    n = Q.shape[0]
    cores = min(os.cpu_count() or 1, 16)                 # a one-GPU box's CPU share
    sym = gmrfx.MI355XBackend(Q, coords=mesh.points, symbolic_only=True)
    perm = sym.ordering_permutation()
    sn = sncpu.SupernodalCPU(sym.symbolic(), perm, n, nthreads=cores)
    B = np.random.default_rng(1).standard_normal((n, nrhs))
    tf = []
    for _ in range(2):                                   # first pass pays page faults / BLAS thread start-up
        t0 = time.perf_counter()
        fail = sn.factorize(Q.data)
        tf.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    X = sn.solve(B)
    ts = time.perf_counter() - t0
    resid = float(np.linalg.norm(Q @ X[:, :4] - B[:, :4]) / np.linalg.norm(B[:, :4]))
    out = {"value": n / (tf[1] + ts), "unit": "DoF/s", "cores": cores, "kind": "port",
           "sample": f"the full workload (n={n}, {nrhs} RHS), same Q / permutation / supernodes as the GPU path: supernodal "
                     f"multifrontal LL' on OpenBLAS (scipy wheel) {tf[1]:.2f}s (first pass {tf[0]:.2f}s) + blocked {nrhs}-RHS solve "
                     f"{ts:.2f}s, {cores} threads; residual {resid:.1e}; fail_col {fail}",
           "s_refactorize": tf[1], "s_solve": ts,
           "cholmod_reference": cholmod_reference(Q, perm, B, os.path.join(ROOT, "gpurun_out", "cholmod_in"))}
    return out


def probe_level_ms(Q, mesh, local_rank):
    """Per-level HIP-event times of ONE unsharded refactorise + 64-RHS solve on this GPU (a second handle created under
    GMRFX_LEVEL_MARK=1; the marks cost a few empty launches, so they are never on in a timed handle): the input of the time
    bounds of the sharding plan (gmrfx/shard.py plan_summary). None when the unsharded problem does not fit next to the
    sharded one."""
    import numpy as np
    import torch
    import gmrfx
    os.environ["GMRFX_LEVEL_MARK"] = "1"
    try:
        probe = gmrfx.MI355XBackend(Q, coords=mesh.points, device=local_rank, factorize=False)
    except Exception:
        return None
    finally:
        del os.environ["GMRFX_LEVEL_MARK"]
    try:
        dev = torch.device("cuda", local_rank)
        n = Q.shape[0]
        d_nz = torch.from_numpy(np.ascontiguousarray(Q.data)).to(dev)
        d_B = torch.randn((64, n), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float64).to(dev)
        d_X = torch.empty_like(d_B)
        torch.cuda.synchronize()
        for _ in range(2):
            probe.refactorize_dev(d_nz.data_ptr())
            probe.solve_dev(d_B.data_ptr(), n, 64, d_X.data_ptr(), n)
        return {"factor": probe.level_times(0).tolist(), "fwd": probe.level_times(1).tolist(), "bwd": probe.level_times(2).tolist()}
    except Exception:
        return None
    finally:
        probe.close()


def bench_sharded(args, Q, mesh, dist, rank, world, local_rank, steps=None, warmup=None, level_ms=None, probe=True, keep=None):
    """Strong scaling: ONE refactorisation + 64-RHS solve sharded over the ranks (gmrfx/shard.py): subtrees
    per rank, every top front on one rank of its group, contribution blocks / update vectors point-to-point along the
    owner-crossing tree edges (RCCL over xGMI), x of the top fronts broadcast by their owners. Returns the result dict
    on rank 0 (None elsewhere); timed exactly like the replica loop (barrier + sync on both sides, max over ranks).
    The distributed-X step and the per-level probe only run with --full. `keep` (rank 0): receives X and logdet."""
    import numpy as np
    import torch
    from gmrfx import shard
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    dev = torch.device("cuda", local_rank)
    n = Q.shape[0]
    d_nz = torch.from_numpy(np.ascontiguousarray(Q.data)).to(dev)
    Bh = torch.randn((args.nrhs, n), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float64)
    d_B = Bh.to(dev)
    d_X = torch.zeros_like(d_B)
    torch.cuda.synchronize()     # torch's fill runs on torch's stream; the library's streams do not wait for it
    sf = shard.ShardedFactor(Q, dist, device=local_rank, coords=mesh.points)
    # B is ROW-SHARDED: a rank only holds the rows it reads (shard.needed_rows(): its subtrees' and its own top fronts'; the masks
    # partition the rows), the rest of its buffer is zeroed -- nothing of B is replicated over the ranks
    need = torch.from_numpy(sf.needed_rows()).to(dev)
    d_B[:, ~need] = 0.0
    torch.cuda.synchronize()

    def step(gather):
        sf.refactorize_dev(d_nz.data_ptr(), check=False)                   # (the pivot report rides with logdet's host round trip)
        sf.solve_dev(d_B.data_ptr(), n, args.nrhs, d_X.data_ptr(), n, gather=gather)
        sf.logdet()                                                         # all-reduce of the ranks' partial sums (config 2: "+ logdet")
        return sf.last_info

    def timed(gather, k):
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            inf = step(gather)
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cpu" if args.rehearse else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t, inf

    # HEADLINE = the step that does the single-GPU step's work: refactorise + solve with ALL of X delivered on rank 0 + logdet
    # (round 5 timed the distributed-X form only: less work than the N = 1 line and than earlier rounds -- advisor finding). The
    # distributed-X form (every rank keeps the rows shard.valid_rows() names; the reference's callers reduce X further) is timed
    # right behind it and reported beside it, never as `value`. --gather-x is kept for compatibility (it is the default now).
    for _ in range(warmup):
        step(True)
    el, info = timed(True, steps)
    el_dist = None
    if args.full:
        for _ in range(min(warmup, 2)):
            step(False)
        el_dist, _ = timed(False, steps)
    sf.solve_dev(d_B.data_ptr(), n, args.nrhs, d_X.data_ptr(), n, gather=True)      # (untimed: all of X on rank 0 for the check)
    torch.cuda.synchronize()
    # how many ranks the collective library really spans: a device all-reduce of ones (RCCL unless --rehearse)
    ones = torch.ones(1, dtype=torch.float64, device="cpu" if args.rehearse else dev)
    dist.all_reduce(ones)
    rccl_ranks = int(round(float(ones.item())))
    ld = sf.logdet()
    st = sf.be.stats()
    mem = torch.tensor([st["bytes_device_total"], st["bytes_factor"]], dtype=torch.float64, device="cpu" if args.rehearse else dev)
    mem_max = mem.clone(); dist.all_reduce(mem_max, op=dist.ReduceOp.MAX)
    mem_sum = mem.clone(); dist.all_reduce(mem_sum, op=dist.ReduceOp.SUM)
    out = None
    if rank == 0:
        if level_ms is None and probe and args.full:
            level_ms = probe_level_ms(Q, mesh, local_rank)
        lstep = None if level_ms is None else (np.asarray(level_ms["factor"]) + np.asarray(level_ms["fwd"]) + np.asarray(level_ms["bwd"]))
        plan = shard.plan_summary(sf.be, lstep)
        X = d_X.cpu().numpy().T
        if keep is not None:
            keep.update(X=X, logdet=ld)
        resid = float(np.linalg.norm(Q @ X - Bh.numpy().T) / np.linalg.norm(Bh.numpy()))
        bounds = {"flop_bound_speedup": plan["flop_bound_speedup"]}
        if lstep is not None:
            bounds.update({k: plan[k] for k in ("time_bound_speedup_latency", "time_bound_speedup_share", "time_bound_ms_latency",
                                                "time_bound_ms_share", "measured_ms_one_gpu", "top_levels", "top_levels_ms")})
            bounds["note"] = ("time bounds from the per-level HIP-event times of one unsharded step on this GPU: subtree fronts cost "
                              "their flop share of their level; `latency` = every level holding a top front keeps its full time (the "
                              "potrf64 -> trsm -> gemm chains do not shorten), `share` = top fronts scale with the heaviest rank's share")
        out = {"value": n / (float(el.item()) / steps), "ms_per_step": 1e3 * float(el.item()) / steps,
               "plan": {"top_fronts": plan["top_fronts"], "cross_rank_edges": sf.info["n_edges"], "top_levels": sf.K, **bounds},
               "per_rank_hbm_bytes": {"max_total": float(mem_max[0]), "max_factor_panels": float(mem_max[1]), "sum_factor_panels": float(mem_sum[1])},
               "exchange": "gloo + host staging (rehearsal)" if args.rehearse else "RCCL point-to-point (batch_isend_irecv) + broadcast + all-reduce over xGMI, stream-ordered (no host synchronisation between phases)",
               "x": "gathered on rank 0 in every timed step (the headline: the same work as the N = 1 line)",
               "ms_per_step_x_distributed": 1e3 * float(el_dist.item()) / steps if el_dist is not None else None,
               "value_x_distributed": n / (float(el_dist.item()) / steps) if el_dist is not None else None,
               "b": "row-sharded: every rank holds the rows shard.needed_rows() names, zeros elsewhere",
               "rccl_ranks": rccl_ranks, "collective_backend": dist.get_backend(), "world_size": dist.get_world_size(),
               "check": {"logdet": ld, "rel_residual": resid, "info": info}}
    dist.barrier()
    sf.close()
    return out


def bench_cfg4_sharded(args, dist, rank, world, local_rank):
    """BASELINE cfg 4 -- the configuration whose flops can actually be shared: 3-D Matern SPDE (nu = 1/2, alpha = 2) on
    G^3 nodes (default 126^3 = 2 000 376), ONE factorisation sharded over the ranks, refactorise + 64-RHS solve. Every rank
    checks first that its part fits (sharded handles only store their own panels / arena); 1 warm-up + 2 timed steps."""
    import numpy as np
    import torch
    import gmrfx
    from gmrfx import spde
    G = args.cfg4_grid
    mesh = spde.grid_mesh_3d(G, G, G)
    Q = spde.matern_precision(mesh, 0, 0.4)          # range = 0.2 x domain width
    n = Q.shape[0]
    sym = gmrfx.MI355XBackend(Q, coords=mesh.points, symbolic_only=True, shard_rank=rank, shard_world=world)
    st = sym.stats()
    sym.close()
    need = st["bytes_factor"] + st["bytes_cb_arena"] + 8.0 * Q.nnz + 4 * 8.0 * 64 * n + 0.6 * st["bytes_factor"] / max(world, 1)
    free = torch.cuda.mem_get_info(local_rank)[0]
    if args.rehearse:
        free /= world                                  # the rehearsal's ranks share one GPU
    ok = torch.tensor([1 if need < 0.92 * free else 0], dtype=torch.int64, device="cpu" if args.rehearse else torch.device("cuda", local_rank))
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 0:
        return {"status": f"skipped: a rank's part ({need / 1e9:.0f} GB predicted on rank {rank}) does not fit its GPU ({free / 1e9:.0f} GB free)"} if rank == 0 else None
    level_ms = None
    try:
        import glob
        cand = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_level_ms_cfg4_{G}cubed.json")))     # newest round last
        with open(cand[-1]) as fh:
            level_ms = json.load(fh)                   # measured on one GPU (tools/level_times.py cfg4): the unsharded problem
    except Exception:                                  # needs 226 GB and cannot sit next to the sharded one
        level_ms = None
    r = bench_sharded(args, Q, mesh, dist, rank, world, local_rank, steps=2, warmup=1, level_ms=level_ms, probe=False)
    if r is not None:
        r["workload"] = f"cfg4: 3-D Matern SPDE nu=1/2 (alpha=2), {G}^3-node Kuhn mesh (n = {n}), refactorize + {args.nrhs}-RHS solve, sharded over {world} GPUs"
        r["n"] = int(n)
    return r


class _NoLock:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--grid", type=int, default=1000, help="nodes per side of the 2-D mesh (cfg 2: 1000)")
    ap.add_argument("--nrhs", type=int, default=64)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--separate-calls", action="store_true",
                    help="time gmrfx_refactorize_dev + gmrfx_solve_dev per step instead of the one pipelined call gmrfx_refactorize_solve_dev")
    ap.add_argument("--rehearse", action="store_true",
                    help="multi-process rehearsal on a box with ONE GPU: every rank uses cuda:0 and the "
                         "process group runs on gloo (RCCL refuses two ranks on one device)")
    ap.add_argument("--gather-x", action="store_true", help="sharded runs: gather X on rank 0 inside every timed step (default: X stays distributed)")
    ap.add_argument("--extras", action="store_true", help="also time predictor variances diag(A Sigma A') and the Newton iterate (f1, f4)")
    ap.add_argument("--shard-timeout", type=float, default=300.0,
                    help="N > 1: seconds the sharded strong-scaling run may take before the replica line is printed without it")
    ap.add_argument("--deadline", type=float, default=540.0,
                    help="N > 1: seconds after the start of the run (of the launcher, when there is one) by which rank 0's line must be out "
                         "(the driver gives a bench run 600 s): the watchdog of the sharded cfg-2 run is cut to fit, and the additional cfg-4 line is only started "
                         "when --cfg4-budget seconds of it are left")
    ap.add_argument("--cfg4-budget", type=float, default=300.0,
                    help="N > 1: what the cfg-4 sharded line needs at most (126^3 mesh + Q on the host 110-130 s per rank, two symbolic "
                         "analyses 50 s, allocation, 3 steps, the residual check): skipped, and said so, when less of --deadline is left")
    ap.add_argument("--no-shard", action="store_true",
                    help="N > 1: only time the independent replicas (weak scaling); by default the headline of an N > 1 run is "
                         "ONE factorisation sharded over the N GPUs (strong scaling, gmrfx/shard.py) and the replicas are reported beside it")
    ap.add_argument("--no-logpdf", action="store_true",
                    help="skip the (untimed) logpdf loop after the timed steps: keeps kernel traces / PMC passes to whole "
                         "refactorise+solve steps (tools/prof_summary.py, tools/pmc_traffic.py)")
    ap.add_argument("--no-host-io", action="store_true",
                    help="skip the (untimed) host-I/O block: the step through gmrfx_refactorize_solve with host B / X")
    ap.add_argument("--no-cfg3", action="store_true",
                    help="skip the (untimed) cfg-3 block after the timed steps: selected inverse + 256 samples on the same factor")
    ap.add_argument("--cfg4-grid", type=int, default=126,
                    help="N > 1: nodes per side of the 3-D mesh of the additional cfg-4 sharded line (126^3 = BASELINE cfg 4)")
    ap.add_argument("--no-cfg4", action="store_true", help="N > 1: skip the additional cfg-4 sharded line")
    ap.add_argument("--pool", type=int, default=0,
                    help="extra: throughput of P independent workspaces driven concurrently on this GPU "
                         "(the reference's WorkspacePool pattern; reported separately, never as `value`)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline (separate-call steps, logpdf, host I/O, cfg 3, rooflines, CPU "
                         "baseline; N > 1: distributed-X step, per-level probe, cfg-4 line); --extras and --pool imply it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (sampled rows of X, column norms of X, logdet) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.extras or args.pool > 1:
        args.full = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks as CHILD processes (one per GPU) before
        # anything in this process touches the GPU, and exit with their return code. Never an exec.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd).returncode)
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks")

    import numpy as np
    import torch
    import gmrfx
    from gmrfx import spde

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: libgmrfx has no CPU path")
    if args.rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        if args.rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    mesh = spde.grid_mesh_2d(args.grid, args.grid, jitter=0.25, seed=0)
    Q = spde.matern_precision(mesh, smoothness=0, range_=0.2)   # range = 0.1 * domain width (2.0)
    n = Q.shape[0]
    be = gmrfx.MI355XBackend(Q, coords=mesh.points, device=local_rank, factorize=False)
    st0 = be.stats()

    dev = torch.device("cuda", local_rank)
    d_nz = torch.from_numpy(np.ascontiguousarray(Q.data)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    Bh = torch.randn((args.nrhs, n), generator=g, dtype=torch.float64)   # row j = column j of the n x nrhs B
    d_B = Bh.to(dev)
    d_X = torch.empty_like(d_B)
    torch.cuda.synchronize()

    # BASELINE.json config 2: "factor Q + 64-RHS solve + logdet" -- the log-determinant (two small kernels on the factor's
    # diagonal + one scalar read back) is part of every timed step
    def step_separate():
        be.refactorize_dev(d_nz.data_ptr())
        be.solve_dev(d_B.data_ptr(), n, args.nrhs, d_X.data_ptr(), n)
        return be.compute_logdet()

    def step_pipelined():
        # workspace_solve on a workspace with new values (gmrf_workspace.jl:170-178 + 207-215) as ONE call: the forward sweep
        # follows the factorisation up the tree on a second stream; same bits as the two calls
        be.refactorize_solve_dev(d_nz.data_ptr(), d_B.data_ptr(), n, args.nrhs, d_X.data_ptr(), n)
        return be.compute_logdet()

    step = step_separate if args.separate_calls else step_pipelined
    for _ in range(args.warmup):
        step()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    t_factor, t_solve, t_fwd, t_bwd, t_perm, t_syrk = [], [], [], [], [], []
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        s = be.stats()
        t_factor.append(s["ms_factor"]); t_solve.append(s["ms_solve"])
        t_fwd.append(s["ms_solve_fwd"]); t_bwd.append(s["ms_solve_bwd"]); t_perm.append(s["ms_solve_perm"])
        t_syrk.append(s["ms_syrk"])
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if args.rehearse else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # The phases one after the other (the two separate calls), untimed by `value`: in the pipelined step the forward sweep runs
    # beside the factorisation, so the per-phase device times that the factor / sweep rooflines need only exist here. Same
    # kernels, same launches, same results.
    pipelined_phases = None
    ms_step_separate = None
    # the output of the call that was TIMED is kept before anything else writes d_X: the residual / logdet checks below and
    # the bit-for-bit comparison with the two separate calls are made on it
    d_X_timed = d_X.clone()
    logdet_timed = be.compute_logdet()
    fail_col_timed = be.stats()["fail_col"]
    pipelined_equals_separate = None
    # --dump-outputs: what the timed call returned (rank 0; an N > 1 run replaces it with the sharded X when that is the headline)
    X_out = None
    if args.dump_outputs and rank == 0:
        rows_out = output_rows(n, args.nrhs)
        X_out = (d_X_timed.index_select(1, torch.from_numpy(rows_out).to(dev)).T.cpu().numpy(), rows_out,
                 torch.linalg.vector_norm(d_X_timed, dim=1).cpu().numpy(), logdet_timed)
    if not args.separate_calls:
        pipelined_phases = {"factor": float(np.median(t_factor)), "behind_factor": float(np.median(t_solve)),
                            "forward_left_behind_factor": float(np.median(t_fwd)), "backward": float(np.median(t_bwd)),
                            "syrk_launches": float(np.median(t_syrk))}
    if args.full and not args.separate_calls:
        t_factor, t_solve, t_fwd, t_bwd, t_perm, t_syrk_sep = [], [], [], [], [], []
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step_separate()
            s = be.stats()
            t_factor.append(s["ms_factor"]); t_solve.append(s["ms_solve"])
            t_fwd.append(s["ms_solve_fwd"]); t_bwd.append(s["ms_solve_bwd"]); t_perm.append(s["ms_solve_perm"])
            t_syrk_sep.append(s["ms_syrk"])
        torch.cuda.synchronize()
        ms_step_separate = 1e3 * (time.perf_counter() - t1) / args.steps
        pipelined_phases["syrk_launches_separate"] = float(np.median(t_syrk_sep))
        pipelined_equals_separate = bool(torch.equal(d_X_timed, d_X)) and be.compute_logdet() == logdet_timed

    # hyper-parameter loop (docs/.../workspace_factorization_reuse.jl:94-102): new values -> numeric
    # factorisation -> logpdf(z) = -r'Qr/2 + logdet(Q)/2 - n log(2 pi)/2, Q's values and z resident in HBM.
    # Untimed by `value`; wall clock of 5 evaluations including the two scalar read-backs each. Runs right after the
    # timed steps, before the host-side checks below (their BLAS / sparse products leave busy host threads behind).
    logpdf_ms = ms_quadform = logpdf_relerr = None
    if args.full and rank == 0 and not args.no_logpdf:
        d_z = d_B[0]
        def logpdf_eval():
            # ONE call: factorisation, r'Qr beside it, logdet behind it, one synchronisation (gmrfx_refactorize_logpdf_dev)
            q, ld = be.refactorize_logpdf_dev(d_nz.data_ptr(), d_z.data_ptr(), n, 1)
            return -0.5 * q[0] + 0.5 * ld - 0.5 * n * np.log(2.0 * np.pi)
        lp = logpdf_eval(); torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(5):
            lp = logpdf_eval()
        torch.cuda.synchronize()
        logpdf_ms = 1e3 * (time.perf_counter() - t1) / 5
        be.quadform_dev(d_nz.data_ptr(), d_z.data_ptr(), n, 1)      # (the kernel alone, for its event time)
        ms_quadform = be.stats()["ms_quadform"]

    # ---- host I/O: the same step through the HOST entry point, gmrfx_refactorize_solve(nzval, B, X) with column-major host arrays --
    # what the reference's workspace_solve(ws, B::Matrix) hands over (src/workspace/gmrf_workspace.jl:170-178, 207-215, backend.jl:207-209).
    # The transfers are SERIAL: B goes up in front of the factorisation, X leaves in slices behind the backward sweep (Device::host_upload /
    # host_download); nothing is overlapped with the factorisation (a transfer beside it slows its launch chain by more than it hides).
    # Untimed by `value`; pageable arrays (a Julia Matrix) and page-locked ones.
    host_io = None
    if args.full and rank == 0 and not args.no_host_io:
        nzh = np.ascontiguousarray(Q.data)
        host_io = {}
        for kind in ("pageable", "pinned"):
            if kind == "pageable":
                Bf = np.asfortranarray(Bh.numpy().T)                      # n x nrhs, column-major
                Xf = np.zeros_like(Bf, order="F")                         # (touched: no page faults inside the timed calls)
                bp, xp = Bf.ctypes.data, Xf.ctypes.data
            else:
                Bp = Bh.clone().pin_memory()                              # row j of (nrhs, n) = column j of the column-major n x nrhs B
                Xp = torch.zeros_like(Bp).pin_memory()
                bp, xp = Bp.data_ptr(), Xp.data_ptr()
            be.refactorize_solve_ptr(nzh.ctypes.data, bp, n, args.nrhs, xp, n)          # warm-up: staging buffer, copy stream
            reps = max(3, min(args.steps, 10))
            t1 = time.perf_counter()
            for _ in range(reps):
                be.refactorize_solve_ptr(nzh.ctypes.data, bp, n, args.nrhs, xp, n)
            ms = 1e3 * (time.perf_counter() - t1) / reps
            Xh = torch.from_numpy(Xf.T) if kind == "pageable" else Xp
            host_io[kind] = {"ms_per_step": ms, "dof_per_s": n / (ms * 1e-3), "reps": reps,
                             "equals_device_resident_call": bool(torch.equal(Xh, d_X_timed.cpu()))}
        be.refactorize_dev(d_nz.data_ptr())

    # ---- untimed correctness evidence on this very run: the output of the TIMED call ---------
    resid = None
    if args.full:
        X = d_X_timed.cpu().numpy().T            # n x nrhs
        Bn = Bh.numpy().T
        resid = float(np.linalg.norm(Q @ X - Bn) / np.linalg.norm(Bn))
    logdet = logdet_timed
    st = be.stats()
    if logpdf_ms is not None:
        zz = Bh[0].numpy()
        qq = float(zz @ (Q @ zz))
        lp_host = -0.5 * qq + 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
        logpdf_relerr = abs(lp - lp_host) / abs(lp_host)

    extras = {}
    cfg3 = None
    if args.full and not args.no_cfg3 and rank == 0:
        # BASELINE cfg 3 on the same factor (untimed by `value`; median of 3 each): Takahashi selected inverse on pattern(L)
        # (compute_selinv!, backend.jl:226-257) and 256 samples P' L^-T z (backend_backward_solve, backend.jl:281-284)
        t_sel, t_rand = [], []
        d_Z = torch.randn((256, n), generator=torch.Generator(device="cpu").manual_seed(2), dtype=torch.float64).to(dev)
        d_S = torch.empty_like(d_Z)
        torch.cuda.synchronize()
        for _ in range(3):
            be.refactorize_dev(d_nz.data_ptr())          # (a refactorisation drops the selected-inverse cache)
            be.selinv_compute_dev()
            t_sel.append(be.stats()["ms_selinv"])
            be.backward_solve_dev(d_Z.data_ptr(), n, 256, d_S.data_ptr(), n)
            t_rand.append(be.stats()["ms_backward_solve"])
        extras["ms_selinv"] = float(np.median(t_sel))
        extras["ms_rand256"] = float(np.median(t_rand))
        # the same 256 samples the way the reference's rand(d, 256) reaches a backend WITHOUT the batched `_rand!` of julia/GMRFX.jl:
        # one single-RHS backward solve per sample (src/gmrf.jl:271-281 under Distributions' column loop), operands resident in
        # HBM (a host caller adds two PCIe round trips per sample); extrapolated from 16 calls
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for j in range(16):
            be.backward_solve_dev(d_Z.data_ptr() + 8 * n * j, n, 1, d_S.data_ptr() + 8 * n * j, n)
        torch.cuda.synchronize()
        extras["ms_rand256_single_calls"] = 1e3 * (time.perf_counter() - t1) * 256.0 / 16.0
        # one right-hand side and sixteen through the separate solve call (HIP-event time of the call, median of 5, inverses built):
        # what `mean` / a Newton step's solve / a narrow rand cost (the passes of at most 16 columns have kernels of their own)
        for k in (1, 16):
            ts = []
            for _ in range(6):
                be.solve_dev(d_Z.data_ptr(), n, k, d_S.data_ptr(), n)
                ts.append(be.stats()["ms_solve"])
            extras[f"ms_solve_{k}rhs"] = float(np.median(ts[1:]))
        sy = be.symbolic()
        cc = np.diff(sy.super_first).astype(np.float64)
        mm = np.diff(sy.row_ptr).astype(np.float64) - cc
        # per front: Y = L21 X (2 c^2 m), Z21 = -Z22 Y (2 c m^2), Z11 = X'X - Y'Z21 (c^3 / 3 + 2 c^2 m), X = L11^-1 (c^3 / 3)
        sel_flops = float((2.0 * cc * mm * mm + 4.0 * cc * cc * mm + 2.0 * cc ** 3 / 3.0).sum())
        cfg3 = {"sel_flops": sel_flops}

    if args.extras and rank == 0:
        # predictor marginal variances: diag(A Sigma A') for a P1 evaluation matrix with one random
        # point per node (3 weights per row), contracted on the device from the selected-inverse panels; wall clock
        # including the host-side pair planning and the transfers
        import scipy.sparse as sp
        rg = np.random.default_rng(4)
        cells = mesh.cells[rg.integers(0, len(mesh.cells), size=n)]
        A = sp.csr_matrix((rg.dirichlet(np.ones(3), size=n).ravel(), (np.repeat(np.arange(n), 3), cells.ravel())), shape=(n, n))
        t1 = time.perf_counter()
        vdiag = be.row_diag_ASigmaAt(A)
        extras["row_diag_ASigmaAt_wall_ms"] = 1e3 * (time.perf_counter() - t1)      # plans the pairs, then contracts
        t1 = time.perf_counter()
        vdiag = be.row_diag_ASigmaAt(A)
        extras["row_diag_ASigmaAt_planned_wall_ms"] = 1e3 * (time.perf_counter() - t1)   # plan resident on the device
        extras["row_diag_rows"] = int(n)
        extras["row_diag_min_max"] = [float(vdiag.min()), float(vdiag.max())]

    if args.extras and rank == 0:
        # Newton iterate: Q_k = Q_prior - diag(h_k), refactorise. Host path = update nzval on the
        # host and send all of it (what _update_hessian! + the CHOLMOD copy do); device path = send h only.
        coo = Q.tocoo()                                     # same entry order as Q.data
        diag_idx = np.flatnonzero(coo.row == coo.col)
        hvec = -np.random.default_rng(3).uniform(0.1, 1.0, n)
        be.set_prior(Q.data, diag_idx)
        tt = {}
        for name, fn in (("host_values", lambda: be.refactorize_values((lambda z: (z.__setitem__(diag_idx, z[diag_idx] - hvec), z)[1])(Q.data.copy()))),
                         ("device_update", lambda: be.refactorize_update(hvec))):
            fn(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            tt[name] = 1e3 * (time.perf_counter() - t1) / 3
        extras["newton_iterate_ms"] = tt
        be.refactorize_dev(d_nz.data_ptr())      # back to Q itself for the checks below

    if args.pool > 1 and rank == 0:
        # P independent handles (own HIP streams), one host thread each; ctypes drops the GIL in the calls
        import threading
        perm = be.ordering_permutation()
        pool = [be] + [gmrfx.MI355XBackend(Q, ordering=perm, device=local_rank, factorize=False) for _ in range(args.pool - 1)]
        bufs = [(d_B, d_X)] + [(d_B, torch.empty_like(d_B)) for _ in range(args.pool - 1)]
        torch.cuda.synchronize()

        def worker(b, bx, reps):
            for _ in range(reps):
                b.refactorize_dev(d_nz.data_ptr())
                b.solve_dev(bx[0].data_ptr(), n, args.nrhs, bx[1].data_ptr(), n)

        for reps in (1, args.steps):     # warm-up round, then the timed round
            th = [threading.Thread(target=worker, args=(pool[i], bufs[i], reps)) for i in range(args.pool)]
            torch.cuda.synchronize()
            tp0 = time.perf_counter()
            [t.start() for t in th]
            [t.join() for t in th]
            torch.cuda.synchronize()
            tp = time.perf_counter() - tp0
        extras["pool"] = {"workspaces": args.pool, "dof_per_s": args.pool * args.steps * n / tp,
                          "ms_per_step_per_workspace": 1e3 * tp / args.steps}
        for b in pool[1:]:
            b.close()

    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        nnzl = st["nnz_l_stored"]
        out = {
            "metric": "factor+solve(64 RHS) throughput", "value": world * n / (elapsed / args.steps), "unit": "DoF/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"cfg2: {args.grid}x{args.grid}-node jittered P1 mesh, 2-D Matern nu=1 (alpha=2), "
                                   f"refactorize + {args.nrhs}-RHS solve + logdet per step, inputs resident in HBM",
                       "n": n, "nnz_Q": int(Q.nnz), "nnz_L": int(st["nnz_l"]), "nnz_L_stored": int(nnzl),
                       "nrhs": args.nrhs, "parallelism": "1 workspace per GPU (replicas)" if world > 1 else "1 GPU",
                       "ordering": "own geometric nested dissection"},
            "step_call": "gmrfx_refactorize_dev + gmrfx_solve_dev" if args.separate_calls else
                         "gmrfx_refactorize_solve_dev (one pipelined call; include/gmrfx.h)",
            "pipelined_phases_ms": pipelined_phases,
            "check": {"logdet": logdet, "fail_col": fail_col_timed,
                      "of": "the output of the timed call (copied out before any other call wrote d_X)"},
            "supernodes": int(st["nsuper"]), "levels": int(st["nlevels"]),
            "hbm_bytes_allocated": st["bytes_device_total"], "full": args.full,
        }
        if args.full:
            med = lambda v: float(np.median(v))
            mf, ms_, mfw, mbw = med(t_factor), med(t_solve), med(t_fwd), med(t_bwd)
            # algorithmic bytes of one triangular sweep: 8 nnz(L) + 4 sum_s r_s + 2*8*n*nrhs
            # (round 6: the TRUE nnz(L) -- amalgamation zeros and panel padding are this implementation's bytes, not the algorithm's; the
            #  figure on the stored entries, which rounds 1-5 quoted, stays beside it as frac_on_stored_entries)
            bytes_sweep = 8.0 * st["nnz_l"] + 4.0 * st["sum_rows"] + 16.0 * n * args.nrhs
            bytes_sweep_stored = 8.0 * nnzl + 4.0 * st["sum_rows"] + 16.0 * n * args.nrhs
            sweep_ms = 0.5 * (mfw + mbw)
            sweep_gbs = bytes_sweep / (sweep_ms * 1e-3) / 1e9
            copy_gbs = measure_copy_peak(dev)
            try:
                smb = sweep_model_bound(be, args.nrhs, copy_gbs)
                smb_guide = sweep_model_bound(be, args.nrhs, COPY_PEAK_GUIDE_GBS)       # the same sum at the guide's achievable copy rate
            except Exception as ex:        # (the bound is a report, never a reason to lose the line)
                smb = {"error": repr(ex)}
            factor_tf = st["factor_flops"] / (mf * 1e-3) / 1e12
            # HBM traffic from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate
            # runs, gfx950 FETCH_SIZE x2 correction): only valid for the workload they were collected on
            # The counters cannot be read inside this process, so `traffic` is a COMMITTED counter pass (tools/pmc_traffic.py,
            # tools/cfg3_profile.py): each file names the source tree it was collected on (csrc_hash = gmrfx._lib.source_tree_hash()),
            # and its figures are quoted only while the tree being timed is that tree -- otherwise traffic is null.
            from gmrfx._lib import source_tree_hash
            tree_hash = source_tree_hash()
            pmc, pmc_note = None, "no counter pass for this workload under profiles/"
            try:
                with open(os.path.join(ROOT, "profiles", "r06_pmc_traffic.json")) as fh:
                    pj = json.load(fh)
                if pj["workload"] == {"grid": args.grid, "nrhs": args.nrhs}:
                    if pj.get("csrc_hash") == tree_hash:
                        pmc, pmc_note = pj, f"profiles/r06_pmc_traffic.json, collected on source tree {tree_hash} = the tree being timed"
                    else:
                        pmc_note = (f"null: profiles/r06_pmc_traffic.json belongs to source tree {pj.get('csrc_hash')}, the tree being timed is "
                                    f"{tree_hash} (re-run tools/final_profile.sh)")
            except Exception:
                pmc = None
            # ---- roofline of the DOMINANT KERNEL: k_syrk_cb_rec (contribution-block SYRK, ~18 % of the step) ----
            # algorithmic flops: sum over the big fronts of c m (m + 1) (lower triangle of the m x m block,
            # 2 c flops per entry), one launch per level; time: HIP events around every launch, recorded by
            # the library on the stream the kernel runs on (gmrfx_stats.ms_syrk), median over the timed steps
            ms_syrk = med(t_syrk)
            n_launch = max(int(st["syrk_launches"]), 1)
            syrk_tf = st["syrk_flops"] / (ms_syrk * 1e-3) / 1e12
            per_k = (pmc or {}).get("per_kernel_GB_per_step", {})
            # (round 6: two instantiations -- <true>: the software-pipelined product loop of the levels of wide fronts, <false>: the rest;
            #  one launch per level, either one or the other: their bytes and launches add up to the kernel's)
            inst = [v for k, v in per_k.items() if k == "k_syrk_cb_rec" or k.startswith("k_syrk_cb_rec<")]
            pk = ({"fetch_x2": sum(v["fetch_x2"] for v in inst), "write": sum(v["write"] for v in inst)} if inst else per_k.get("k_syrk_cb"))
            roof_kernel = {"bound": "mfma", "achieved": syrk_tf, "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s",
                           "frac": syrk_tf / FP64_MFMA_PEAK_TF,
                           "traffic": (1e9 * (pk["fetch_x2"] + pk["write"]) / n_launch) if pk else None,
                           "peak_measured": FP64_MFMA_MEASURED_TF, "frac_of_measured_peak": syrk_tf / FP64_MFMA_MEASURED_TF,
                           "kernel": "k_syrk_cb_rec", "instantiations": "k_syrk_cb_rec<true> (levels whose widest front has >= 128 columns: pipelined "
                                                                         "product loop) + k_syrk_cb_rec<false> (the levels below)",
                           "launches_per_step": n_launch, "avg_launch_ms": ms_syrk / n_launch,
                           "flops_per_launch": st["syrk_flops"] / n_launch, "ms_per_step": ms_syrk,
                           "note": "achieved = algorithmic flops of the launches of one step / their summed HIP-event time over the "
                                   "timed (pipelined) steps -- the forward sweep of the same step runs beside some of them; "
                                   "traffic = PMC HBM bytes per launch (" + pmc_note + ")"}
            if pipelined_phases is not None:
                alone = pipelined_phases["syrk_launches_separate"]
                roof_kernel.update({"ms_per_step_alone": alone, "achieved_alone": st["syrk_flops"] / (alone * 1e-3) / 1e12,
                                    "frac_alone": st["syrk_flops"] / (alone * 1e-3) / 1e12 / FP64_MFMA_PEAK_TF})
            roof_factor = {"bound": "mfma", "achieved": factor_tf, "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s",
                           "frac": factor_tf / FP64_MFMA_PEAK_TF, "traffic": pmc["factor"]["total_bytes"] if pmc else None,
                           "peak_measured": FP64_MFMA_MEASURED_TF, "frac_of_measured_peak": factor_tf / FP64_MFMA_MEASURED_TF,
                           "kernel": "numeric factorisation (all ~500 launches)", "ms": mf, "flops": st["factor_flops"], "note": "traffic: " + pmc_note}
            roof_sweep = {"bound": "hbm", "achieved": sweep_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "frac": sweep_gbs / HBM_PEAK_GBS,
                          "traffic": 0.5 * (pmc["sweep_forward"]["total_bytes"] + pmc["sweep_backward"]["total_bytes"]) if pmc else None,
                          "kernel": "triangular sweep (mean of forward and backward, all launches)", "ms": sweep_ms, "bytes": bytes_sweep,
                          "frac_on_stored_entries": bytes_sweep_stored / (sweep_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "copy_peak_measured": copy_gbs, "frac_of_copy_peak": sweep_gbs / copy_gbs,
                          "note": "bytes = 8 nnz(L) [true fill] + 4 sum r_s + 16 n nrhs (SURVEY 8d); traffic: " + pmc_note}
            if "error" not in smb:
                roof_sweep.update({
                    "model_bound_ms": {"fwd": smb["fwd_ms"], "bwd": smb["bwd_ms"], "mean": 0.5 * (smb["fwd_ms"] + smb["bwd_ms"])},
                    "model_bound_ms_at_guide_copy_peak": {"copy_peak_gbs": COPY_PEAK_GUIDE_GBS, "fwd": smb_guide["fwd_ms"], "bwd": smb_guide["bwd_ms"],
                                                          "mean": 0.5 * (smb_guide["fwd_ms"] + smb_guide["bwd_ms"]),
                                                          "frac_of_it": 0.5 * (smb_guide["fwd_ms"] + smb_guide["bwd_ms"]) / sweep_ms},
                    "frac_of_model_bound": 0.5 * (smb["fwd_ms"] + smb["bwd_ms"]) / sweep_ms,
                    "frac_of_model_bound_fwd": smb["fwd_ms"] / mfw, "frac_of_model_bound_bwd": smb["bwd_ms"] / mbw,
                    "model_bound": {"copy_peak_gbs": copy_gbs, "launch_floor_us": LAUNCH_FLOOR_US, "fwd_launches": smb["fwd_launches"],
                                    "bwd_launches": smb["bwd_launches"], "fwd_bytes": smb["fwd_bytes"], "bwd_bytes": smb["bwd_bytes"],
                                    "handoff_bytes_fwd": smb["handoff_bytes_fwd"], "handoff_bytes_bwd": smb["handoff_bytes_bwd"],
                                    # what the schedule itself forfeits of the 70 % target: the algorithmic bytes over the bound's time
                                    "ceiling_frac_of_hbm_peak": bytes_sweep / (0.5 * (smb["fwd_ms"] + smb["bwd_ms"]) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                    "note": "sum over the task launch and every level of (algorithmic + hand-off bytes) / measured copy peak "
                                            "+ launches x floor (bench.py sweep_model_bound); ceiling_frac = the roofline fraction a sweep "
                                            "running AT this bound would show"}})
            else:
                roof_sweep["model_bound_ms"] = None
                roof_sweep["model_bound_error"] = smb["error"]
            if roof_sweep["traffic"]:
                # the bytes the sweeps really move (PMC), W / x hand-off between the levels included, against the same peak
                roof_sweep["frac_of_peak_with_measured_traffic"] = roof_sweep["traffic"] / (sweep_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
            roof_cfg3 = {}
            pmc3, pmc3_note = None, "no counter pass for this workload under profiles/"
            try:
                with open(os.path.join(ROOT, "profiles", "r06_cfg3_pmc_traffic.json")) as fh:
                    p3 = json.load(fh)
                if p3["workload"]["grid"] == args.grid:
                    if p3.get("csrc_hash") == tree_hash:
                        pmc3, pmc3_note = p3, f"profiles/r06_cfg3_pmc_traffic.json, collected on source tree {tree_hash} = the tree being timed"
                    else:
                        pmc3_note = f"null: profiles/r06_cfg3_pmc_traffic.json belongs to source tree {p3.get('csrc_hash')}, the tree being timed is {tree_hash}"
            except Exception:
                pmc3 = None
            if cfg3 is not None:
                sel_tf = cfg3["sel_flops"] / (extras["ms_selinv"] * 1e-3) / 1e12
                roof_cfg3["roofline_selinv"] = {
                    "bound": "mfma", "achieved": sel_tf, "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": sel_tf / FP64_MFMA_PEAK_TF,
                    "traffic": pmc3["selinv"]["total_bytes"] if pmc3 else None,
                    "kernel": "selected inversion on pattern(L) (all launches; dominant: k_sel_dense, Z21 = -Z22 Y of the big fronts)",
                    "ms": extras["ms_selinv"], "flops": cfg3["sel_flops"], "flops_over_factor_flops": cfg3["sel_flops"] / st["factor_flops"],
                    "bytes_min": 16.0 * nnzl, "gbs_on_bytes_min": 16.0 * nnzl / (extras["ms_selinv"] * 1e-3) / 1e9,
                    "note": "cfg 3: flops = sum_s 2 c m^2 + 4 c^2 m + 2 c^3 / 3 (Takahashi recursion through the dense inverse of L11); "
                            "bytes_min = L read + Z written once; traffic: " + pmc3_note}
                # 256 samples = 4 passes of 64 columns, each one backward sweep + the transposes of its columns (SURVEY 8d:
                # bytes_backward_solve = bytes_sweep + 8 n nrhs)
                rb = 4.0 * (8.0 * nnzl + 4.0 * st["sum_rows"] + 16.0 * n * 64 + 8.0 * n * 64)
                roof_cfg3["roofline_rand256"] = {
                    "bound": "hbm", "achieved": rb / (extras["ms_rand256"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": rb / (extras["ms_rand256"] * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": pmc3["rand256"]["total_bytes"] if pmc3 else None,
                    "kernel": "256 samples P' L^-T z: 4 backward sweeps of 64 columns on two lanes", "ms": extras["ms_rand256"], "bytes": rb,
                    "note": "traffic: " + pmc3_note}
            out.update({
                "roofline": roof_kernel,
                "roofline_factor": roof_factor, "roofline_sweep": roof_sweep, **roof_cfg3,
                "ms_per_step_separate_calls": ms_step_separate,
                # the same step through the HOST entry point (what the reference's seam hands over): never `value`
                "ms_per_step_host_io": host_io["pageable"]["ms_per_step"] if host_io else None,
                "value_host_io": host_io["pageable"]["dof_per_s"] if host_io else None,
                "host_io": ({**host_io, "call": "gmrfx_refactorize_solve(nzval, B, X): column-major HOST arrays, n x nrhs doubles each way over PCIe "
                                                "inside the timed call; upload IN FRONT of the factorisation (staged by host threads when pageable), X out in slices behind the backward sweep"}
                            if host_io else None),
                "phases_ms": {"factor": mf, "solve": ms_, "solve_fwd": mfw, "solve_bwd": mbw, "solve_perm": med(t_perm),
                              "symbolic_host": st0["ms_symbolic"], **extras},
                "logpdf_per_s": (1e3 / logpdf_ms) if logpdf_ms else None, "logpdf_ms": logpdf_ms, "ms_quadform": ms_quadform,
                "logpdf_relerr_vs_host": logpdf_relerr,
            })
            out["check"].update({"rel_residual": resid, "pipelined_equals_separate": pipelined_equals_separate})
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(Q, mesh, args.nrhs)

    # ---- N > 1: ONE factorisation sharded over the ranks (the headline of a multi-GPU run), LAST and under a watchdog:
    # the replica line above is complete by now, and an exchange that never completes (the sharded path has not run on
    # a multi-GPU node yet) must not take it down. Every rank arms the same timer at the same barrier; when it fires,
    # rank 0 prints the replica line with the failure recorded and all ranks leave.
    sharded = None
    sharded_out = {}
    shard_raised = False
    printed = [False]
    out_lock = None
    watchdog = None
    stage = ["cfg2"]
    if dist is not None and not args.no_shard:
        import threading
        out_lock = threading.Lock()
        dist.barrier()

        def give_up():
            # The sharded run hangs or an exchange never completes: flush the line with the failure recorded, then leave
            # with a NON-ZERO code on every rank (a process that has touched the GPU and is killed by its watchdog has
            # failed; the launcher and the driver must see that).
            with out_lock:
                if rank == 0 and not printed[0]:
                    if stage[0] == "cfg2":
                        out["sharded"] = {"error": f"the sharded run did not finish within {args.shard_timeout} s"}
                        out["replicas"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "scaling": "weak"}
                    else:
                        out["cfg4_sharded"] = {"error": "the cfg-4 sharded run did not finish in time"}
                    print(json.dumps(out), flush=True)
                    printed[0] = True
            if rank != 0:
                time.sleep(1.0)     # the launcher ends all ranks when the first one fails: rank 0 prints first
            # (the cfg-4 leg is an extra: the cfg-2 headline of the line is complete and checked, its time-out is recorded in the
            #  line and does not fail the run)
            os._exit(SHARD_TIMEOUT_EXIT if stage[0] == "cfg2" else 0)
        t_launch = launch_time()
        remaining = lambda: args.deadline - (time.time() - t_launch)
        watchdog = threading.Timer(min(args.shard_timeout, max(30.0, remaining() - 15.0)), give_up)
        watchdog.daemon = True
        watchdog.start()
        try:
            sharded = bench_sharded(args, Q, mesh, dist, rank, world, local_rank, keep=sharded_out)
        except Exception as e:           # the replica line must survive a failure of the sharded path
            sharded = {"error": repr(e)} if rank == 0 else None
            shard_raised = True

    if rank == 0 and world > 1:
        replicas = {"value": out["value"], "ms_per_step": out["ms_per_step"], "scaling": "weak",
                    "note": "one independent workspace per GPU (the reference's WorkspacePool pattern), no data-path collective"}
        with out_lock if out_lock is not None else _NoLock():
            if sharded is not None and "error" not in sharded:
                # headline of an N > 1 run: ONE factorisation + 64-RHS solve over all N GPUs (north_star: strong scaling)
                out.update({"value": sharded["value"], "ms_per_step": sharded["ms_per_step"], "scaling": "strong"})
                out["config"]["parallelism"] = (f"ONE factorisation sharded over {world} GPUs: subtrees per rank, top fronts owned inside their "
                                                f"group, Schur-complement blocks point-to-point ({sharded['exchange']})")
                out["sharded"] = sharded
                out["check"] = {**out["check"], "sharded": sharded["check"]}
            else:
                out["sharded"] = sharded
            out["replicas"] = replicas

    if dist is not None and not args.no_shard and not args.no_cfg4 and args.full:
        # the configuration that CAN scale (3-D: the flops sit in a few huge fronts), next to the graded cfg-2 line; its
        # failure is recorded in the line but does not change the exit code (the headline is cfg 2)
        # every rank takes the same decision: 2 = the sharded cfg-2 run raised somewhere, 1 = some rank has less than --cfg4-budget
        # seconds of --deadline left (the line is printed AFTER this leg: a leg that outlives the launcher's limit would take the
        # cfg-2 headline down with it)
        flag = torch.tensor([2 if shard_raised else 1 if remaining() < args.cfg4_budget else 0], dtype=torch.int64,
                            device="cpu" if args.rehearse else dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if int(flag.item()) == 1 and rank == 0:
            with out_lock:
                out["cfg4_sharded"] = {"status": f"skipped: {remaining():.0f} s of --deadline {args.deadline:.0f} s left, the leg is given "
                                                 f"--cfg4-budget {args.cfg4_budget:.0f} s"}
        if int(flag.item()) == 0:
            stage[0] = "cfg4"
            watchdog.cancel()
            watchdog = threading.Timer(max(30.0, remaining() - 10.0), give_up)
            watchdog.daemon = True
            watchdog.start()
            try:
                cfg4 = bench_cfg4_sharded(args, dist, rank, world, local_rank)
            except Exception as e:
                cfg4 = {"error": repr(e)}
            if rank == 0:
                with out_lock:
                    out["cfg4_sharded"] = cfg4

    if rank == 0 and X_out is not None:
        if out["scaling"] == "strong" and "X" in sharded_out:          # the headline is the sharded step: its X and logdet
            Xs = sharded_out["X"]
            X_out = (Xs[X_out[1]], X_out[1], np.linalg.norm(Xs, axis=0), sharded_out["logdet"])
        dump_outputs(args.dump_outputs, *X_out)
    if rank == 0:
        if out_lock is not None:
            with out_lock:
                if not printed[0]:
                    print(json.dumps(out), flush=True)
                    printed[0] = True
        else:
            print(json.dumps(out), flush=True)
    failed = False
    if dist is not None:
        # did the sharded path fail on rank 0 (exception)? every rank leaves with the same code
        flag = torch.tensor([1 if (shard_raised or (rank == 0 and not args.no_shard and (sharded is None or "error" in sharded))) else 0],
                            dtype=torch.int64, device="cpu" if args.rehearse else dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        failed = bool(flag.item())
        dist.barrier()          # (still under the watchdog: a rank that failed alone would wait here for ever)
        if watchdog is not None:
            watchdog.cancel()
        dist.destroy_process_group()
    if failed:
        raise SystemExit(SHARD_FAILED_EXIT)     # the JSON line (replica headline + the error) is out; the exit code says so too


if __name__ == "__main__":
    main()
