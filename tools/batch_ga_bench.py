#!/usr/bin/env python3
"""B Gaussian approximations of one hyper-parameter sweep: gmrfx_batch_gaussian_approximation_dev on a batched handle against the same
B approximations on ONE plain handle, one after the other (gmrfx_set_prior + gmrfx_obs_set + gmrfx_gaussian_approximation_dev per
member), in the same process and run.

Problem (DESIGN.md section 6a's): a 2-D Matern (alpha = 2) precision on a jittered g x g mesh, g = 100 (n = 10 000), B = 50 values of
(range, tau) on one pattern, Poisson counts on every node (one data set), zero prior mean, x0 = 0, flag bit 3 (the handle is left
factorised at every mode). Operands live in HBM. Reported: milliseconds per sweep and per member, median / minimum / maximum / the
quartiles over --reps timed repetitions after --warmup, the GPU synchronised around each timed region; the per-member iteration
counts of both routes, ASSERTED equal; the largest difference of the modes; the forest-level totals; the source tree hash. The
plain route's per-member set_prior (nnz doubles over PCIe) and obs_set are part of what a sweep on one plain handle costs and are
timed with it; "plain_loop_only" times the plain loops alone on B handles prepared beforehand.

--design: the same sweep observed through a design matrix. 3 n point observations, each inside a random mesh
triangle with three barycentric weights, plus an intercept column: the latent vector is the field and one intercept node with a proper
N(0, 1 / 0.01) prior, every row of A observes it with weight 1 (n + 1 nodes; the members' pattern is united with pattern(A'A), explicit
zeros; the dense intercept column is pinned to the end of the elimination order, PinDenseColumns). gmrfx_batch_obs_set_design once, then
gmrfx_batch_set_prior + gmrfx_batch_gaussian_approximation_dev per sweep, against ONE plain handle whose design likelihood is set once
(the plan does not depend on theta) and which takes gmrfx_set_prior + gmrfx_gaussian_approximation_dev per member.
--constraint: a Besag model on a g x g torus plus 1e-6 I under a sum-to-zero constraint, Poisson counts on every
node, B = 50 precisions. gmrfx_batch_set_prior + gmrfx_batch_constrained_gaussian_approximation_dev per sweep on a batched handle holding
the constraint, against the same 50 approximations on ONE plain handle under gmrfx_constraints_set (gmrfx_set_prior +
gmrfx_gaussian_approximation_dev per member; the data set goes in once). Output: profiles/batch_ga_con_bench.json by default.
--pullback [--design]: the gradient chain of the sweep, dL/dtheta_k of -logpdf(posterior_k, x*_k) for every member with
theta_k scaling member k's prior: gmrfx_batch_set_prior + gmrfx_batch_gaussian_approximation_dev (flag bit 3) ->
gmrfx_batch_logpdf_grad_dev (ybar = -1) -> gmrfx_batch_ga_pullback_dev (Qbar_prior over Qbar) -> gmrfx_batch_pattern_dot_dev, against
the same chain run B times on ONE plain handle (gmrfx_set_prior + gmrfx_gaussian_approximation_dev -> gmrfx_logpdf_grad_dev ->
gmrfx_ga_pullback_dev -> gmrfx_pattern_dot_dev per member). Node case and, with --design, the design case above (3 n points and an
intercept). Whether the B gradients of both routes agree bit for bit is reported (gradients_same_bits). Output: profiles/batch_ga_pullback_bench[_design].json.
usage: tools/batch_ga_bench.py [--design | --constraint | --pullback [--design]] [--grid 100] [--batch 50] [--reps 15] [--warmup 3]
                               [--out profiles/batch_ga_bench.json]"""
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


def members(g, B, rng):
    mesh = spde.grid_mesh_2d(g, g, jitter=0.25, seed=0)
    Qs = [spde.matern_precision(mesh, 0, float(rng.uniform(0.15, 0.4)), tau=float(rng.uniform(0.5, 2.0))).tocsc() for _ in range(B)]
    for Q in Qs:
        Q.sort_indices()
        assert np.array_equal(Q.indptr, Qs[0].indptr) and np.array_equal(Q.indices, Qs[0].indices), "pattern changed with the values"
    return Qs, mesh.points


def design_problem(g, B, rng):
    """(members on n + 1 nodes with pattern(A'A) stored, coords, A (3 n x (n + 1)), y)"""
    mesh = spde.grid_mesh_2d(g, g, jitter=0.25, seed=0)
    n = mesh.points.shape[0]
    nobs = 3 * n
    cells = np.asarray(mesh.cells)
    tri = cells[rng.integers(0, cells.shape[0], nobs)]
    A = sp.csr_matrix((rng.dirichlet(np.ones(3), nobs).ravel(), (np.repeat(np.arange(nobs), 3), tri.ravel())), shape=(nobs, n))
    A.sum_duplicates()
    A = sp.hstack([A, sp.csr_matrix(np.ones((nobs, 1)))], format="csr")
    P = sp.csr_matrix(A, copy=True)
    P.data[:] = 1.0
    P = sp.coo_matrix(P.T @ P)
    Qs = []
    for _ in range(B):
        M = spde.matern_precision(mesh, 0, float(rng.uniform(0.15, 0.4)), tau=float(rng.uniform(0.5, 2.0)))
        C = sp.coo_matrix(sp.block_diag([M, sp.csc_matrix([[0.01]])]))
        Q = sp.csc_matrix((np.r_[C.data, np.zeros(P.nnz)], (np.r_[C.row, P.row], np.r_[C.col, P.col])), shape=(n + 1, n + 1))
        Q.sort_indices()
        Qs.append(Q)
        assert np.array_equal(Q.indptr, Qs[0].indptr) and np.array_equal(Q.indices, Qs[0].indices), "pattern changed with the values"
    pts = np.vstack([mesh.points, mesh.points.mean(axis=0)])
    return Qs, pts, A, rng.poisson(20.0, nobs).astype(float)


def design(a):
    B, g = a.batch, a.grid
    Qs, pts, A, y = design_problem(g, B, np.random.default_rng(g))
    n, nobs = Qs[0].shape[0], A.shape[0]
    NZ = np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))
    kw = dict(refactorize_final=True)
    bb = gmrfx.MI355XBatchLaplace(Qs[0], B, ordering=gmrfx.PinDenseColumns(), coords=pts, device=0)
    bb.set_design_observations("poisson", y, A, param=0.0)
    info = bb.observations_design_info()
    perm = bb.ordering_permutation()
    dX = torch.empty(n * B, dtype=torch.float64, device="cuda:0")
    dX0 = torch.zeros(n * B, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    res = {}

    def batched():
        bb.set_prior(NZ)
        res["b"] = bb.gaussian_approximation_dev(dX.data_ptr(), n, d_x0=dX0.data_ptr(), sx0=n, **kw)
    t_b = timed(batched, a.reps, a.warmup)
    Xb = dX.cpu().numpy().reshape(B, n).copy()

    plain = gmrfx.MI355XBackend(Qs[0], ordering=perm, device=0, factorize=False)
    plain.set_design_observations("poisson", y, A)
    hmap = plain.observations_hess_map()
    assert np.array_equal(hmap, bb.observations_hess_map())
    dx = torch.empty(n * B, dtype=torch.float64, device="cuda:0")
    its = np.zeros(B, np.int64)

    def sequential():
        for k in range(B):
            plain.set_prior(NZ[:, k], hmap)
            i = plain.gaussian_approximation_dev(dx.data_ptr() + 8 * k * n, d_x0=dX0.data_ptr(), **kw)
            its[k] = i["iterations"]
    t_s = timed(sequential, a.reps, a.warmup)
    Xs = dx.cpu().numpy().reshape(B, n).copy()
    plain.close()

    many = []
    for k in range(B):
        p = gmrfx.MI355XBackend(Qs[0], ordering=perm, device=0, factorize=False)
        p.set_design_observations("poisson", y, A)
        p.set_prior(NZ[:, k], hmap)
        many.append(p)

    def loops_only():
        for k, p in enumerate(many):
            p.gaussian_approximation_dev(dx.data_ptr() + 8 * k * n, d_x0=dX0.data_ptr(), **kw)
    t_l = timed(loops_only, a.reps, a.warmup)
    for p in many:
        p.close()

    ib = res["b"]
    assert np.array_equal(ib["iterations"], its), (ib["iterations"], its)
    row = {"tool": "tools/batch_ga_bench.py --design", "device": torch.cuda.get_device_name(0), "source_tree_hash": _lib.source_tree_hash(),
           "n": n, "nobs": nobs, "nnz_A": info["nnz"], "cnt": info["cnt"], "terms": info["terms"], "grid": g, "B": B, "family": "poisson",
           "reps": a.reps, "warmup": a.warmup, "batched": t_b, "one_plain_handle_sequential": t_s, "plain_loop_only": t_l,
           "ms_per_member_batched": t_b["median_ms"] / B, "ms_per_member_sequential": t_s["median_ms"] / B,
           "speedup_vs_sequential": t_s["median_ms"] / t_b["median_ms"], "speedup_vs_loops_only": t_l["median_ms"] / t_b["median_ms"],
           "iterations": ib["iterations"].tolist(), "iteration_counts_agree": True, "converged": bool(ib["converged"].all()), "totals": ib["totals"],
           "sum_member_factorizations": int(ib["factorizations"].sum()), "max_abs_mode_diff": float(np.abs(Xb - Xs).max())}
    print(json.dumps(row), flush=True)
    bb.close()
    return row


def pullback(a):
    """the batched gradient chain against the plain chain member by member (module docstring)"""
    B, g = a.batch, a.grid
    if a.design:
        Qs, pts, A, y = design_problem(g, B, np.random.default_rng(g))
        order = dict(ordering=gmrfx.PinDenseColumns())
    else:
        Qs, pts = members(g, B, np.random.default_rng(g))
        A, y, order = None, np.random.default_rng(1).poisson(20.0, Qs[0].shape[0]).astype(float), {}
    n, nnz = Qs[0].shape[0], Qs[0].nnz
    NZ = np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))
    dev = "cuda:0"
    kw = dict(refactorize_final=True)
    bb = gmrfx.MI355XBatchLaplace(Qs[0], B, coords=pts, device=0, **order)
    if a.design:
        bb.set_design_observations("poisson", y, A, param=0.0)
    else:
        bb.set_observations("poisson", y, param=0.0)
    perm = bb.ordering_permutation()
    dX, dX0 = torch.empty(n * B, dtype=torch.float64, device=dev), torch.zeros(n * B, dtype=torch.float64, device=dev)
    dG = torch.empty(nnz * B, dtype=torch.float64, device=dev)
    dJ = torch.from_numpy(np.ascontiguousarray(NZ.T).reshape(-1)).to(dev)          # dQ_k / dtheta_k at theta_k = 1: Q_k itself
    torch.cuda.synchronize()
    res = {}

    def batched():
        bb.set_prior(NZ)
        res["ga"] = bb.gaussian_approximation_dev(dX.data_ptr(), n, d_x0=dX0.data_ptr(), sx0=n, **kw)
        bb.logpdf_grad_dev(dX.data_ptr(), n, -1.0, d_Qbar=dG.data_ptr(), d_mu=dX.data_ptr())
        res["info"] = bb.ga_pullback_dev(dX.data_ptr(), n, 0, 0, 0, dG.data_ptr(), dG.data_ptr(), 0, 0)[2]
        res["grad"] = bb.pattern_dot_dev(dG.data_ptr(), dJ.data_ptr(), nnz, nnz, 1)[0].copy()
    t_b = timed(batched, a.reps, a.warmup)
    assert (res["info"] == 0).all() and res["ga"]["converged"].all()

    plain = gmrfx.MI355XBackend(Qs[0], ordering=perm, device=0, factorize=False)
    if a.design:
        plain.set_design_observations("poisson", y, A)
        hmap = plain.observations_hess_map()
    else:
        plain.set_observations("poisson", y)
        hmap = diag_positions(Qs[0])
    dx, dg = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(nnz, dtype=torch.float64, device=dev)
    grad = np.zeros(B)

    def sequential():
        for k in range(B):
            plain.set_prior(NZ[:, k], hmap)
            plain.gaussian_approximation_dev(dx.data_ptr(), d_x0=dX0.data_ptr(), **kw)
            plain.logpdf_grad_dev(dx.data_ptr(), d_Qbar=dg.data_ptr(), d_mu=dx.data_ptr(), ybar=-1.0)
            plain.ga_pullback_dev(dx.data_ptr(), 0, 0, dg.data_ptr(), dg.data_ptr(), 0, 0)
            grad[k] = plain.pattern_dot_dev(dg.data_ptr(), dJ.data_ptr() + 8 * k * nnz, nnz, 1)[0]
    t_s = timed(sequential, a.reps, a.warmup)
    plain.close()
    same = bool(np.array_equal(grad.view(np.int64), res["grad"].view(np.int64)))
    row = {"tool": "tools/batch_ga_bench.py --pullback" + (" --design" if a.design else ""), "device": torch.cuda.get_device_name(0),
           "source_tree_hash": _lib.source_tree_hash(), "n": n, "nnz": int(nnz), "nobs": int(len(y)), "grid": g, "B": B, "family": "poisson",
           "reps": a.reps, "warmup": a.warmup, "batched_chain": t_b, "one_plain_handle_chain_sequential": t_s,
           "ms_per_member_batched": t_b["median_ms"] / B, "ms_per_member_sequential": t_s["median_ms"] / B,
           "speedup_vs_sequential": t_s["median_ms"] / t_b["median_ms"], "gradients_same_bits": same,
           "gradients_max_rel_diff": float(np.max(np.abs(grad - res["grad"]) / np.abs(grad))), "iterations": res["ga"]["iterations"].tolist()}
    print(json.dumps(row), flush=True)
    bb.close()
    return row


def torus_besag(g, eps=1e-6):
    """graph Laplacian of the g x g periodic lattice + eps I (the intrinsic CAR model of the reference's besag.jl, regularised)"""
    idx = np.arange(g * g).reshape(g, g)
    r = np.concatenate([idx.ravel(), idx.ravel()])
    c = np.concatenate([np.roll(idx, -1, axis=0).ravel(), np.roll(idx, -1, axis=1).ravel()])
    W = sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(g * g, g * g))
    W = (W + W.T).tocsc()
    Q = sp.csc_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W + eps * sp.identity(g * g))
    Q.sort_indices()
    return Q


def constraint(a):
    B, g = a.batch, a.grid
    M = torus_besag(g)
    n = M.shape[0]
    rng = np.random.default_rng(g)
    taus = np.exp(rng.uniform(np.log(0.2), np.log(20.0), B))
    NZ = np.asfortranarray(np.stack([t * M.data for t in taus], axis=1))
    z = rng.standard_normal(n)
    rate = 20.0
    y = rng.poisson(rate * np.exp(z - z.mean())).astype(float)
    aux = np.full(n, np.log(rate))
    A, e = sp.csr_matrix(np.ones((1, n))), np.zeros(1)
    dpos = diag_positions(M)
    kw = dict(refactorize_final=True)
    pts = np.stack(np.meshgrid(np.arange(g, dtype=float), np.arange(g, dtype=float), indexing="ij"), axis=-1).reshape(n, 2)
    bb = gmrfx.MI355XBatchLaplace(M, B, coords=pts, device=0)
    bb.set_observations("poisson", y, aux=aux, param=0.0)
    bb.set_constraints(A, e)
    perm = bb.ordering_permutation()
    dX = torch.empty(n * B, dtype=torch.float64, device="cuda:0")
    dX0 = torch.zeros(n * B, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    res = {}

    def batched():
        bb.set_prior(NZ)
        res["b"] = bb.gaussian_approximation_dev(dX.data_ptr(), n, d_x0=dX0.data_ptr(), sx0=n, **kw)
    t_b = timed(batched, a.reps, a.warmup)
    Xb = dX.cpu().numpy().reshape(B, n).copy()

    plain = gmrfx.MI355XBackend(M, ordering=perm, device=0, factorize=False)
    plain.set_observations("poisson", y, aux=aux)
    plain.set_constraints(A, e)
    dx = torch.empty(n * B, dtype=torch.float64, device="cuda:0")
    its = np.zeros(B, np.int64)

    def sequential():
        for k in range(B):
            plain.set_prior(NZ[:, k], dpos)
            i = plain.gaussian_approximation_dev(dx.data_ptr() + 8 * k * n, d_x0=dX0.data_ptr(), **kw)
            its[k] = i["iterations"]
    t_s = timed(sequential, a.reps, a.warmup)
    Xs = dx.cpu().numpy().reshape(B, n).copy()
    plain.close()

    ib = res["b"]
    assert np.array_equal(ib["iterations"], its), (ib["iterations"], its)
    assert (ib["cinfo"] == 0).all() and (ib["info"] == 0).all()
    assert t_b["median_ms"] <= t_s["median_ms"], "the batched constrained route is slower than the plain route of the same run"
    row = {"tool": "tools/batch_ga_bench.py --constraint", "device": torch.cuda.get_device_name(0), "source_tree_hash": _lib.source_tree_hash(),
           "n": n, "grid": g, "B": B, "m": 1, "family": "poisson", "reps": a.reps, "warmup": a.warmup,
           "batched_constrained": t_b, "one_plain_handle_sequential": t_s,
           "ms_per_member_batched": t_b["median_ms"] / B, "ms_per_member_sequential": t_s["median_ms"] / B,
           "speedup_vs_sequential": t_s["median_ms"] / t_b["median_ms"],
           "iterations": ib["iterations"].tolist(), "iteration_counts_agree": True, "converged": bool(ib["converged"].all()), "totals": ib["totals"],
           "sum_member_factorizations": int(ib["factorizations"].sum()), "max_residual": float(np.nanmax(ib["residual"])),
           "max_abs_mode_diff": float(np.abs(Xb - Xs).max())}
    print(json.dumps(row), flush=True)
    bb.close()
    return row


def diag_positions(Q):
    out = np.empty(Q.shape[0], np.int64)
    for j in range(Q.shape[0]):
        r = Q.indices[Q.indptr[j]:Q.indptr[j + 1]]
        out[j] = Q.indptr[j] + int(np.searchsorted(r, j))
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return {"median_ms": float(q[2]), "min_ms": float(q[0]), "q25_ms": float(q[1]), "q75_ms": float(q[3]), "max_ms": float(q[4])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--design", action="store_true")
    ap.add_argument("--constraint", action="store_true")
    ap.add_argument("--pullback", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.pullback:
        row = pullback(a)
        out = a.out or os.path.join(ROOT, "profiles", "batch_ga_pullback_bench_design.json" if a.design else "batch_ga_pullback_bench.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(row, f, indent=1)
        return
    if a.design or a.constraint:
        row = constraint(a) if a.constraint else design(a)
        if a.constraint and a.out is None:
            a.out = os.path.join(ROOT, "profiles", "batch_ga_con_bench.json")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(row, f, indent=1)
        return
    B, g = a.batch, a.grid
    Qs, pts = members(g, B, np.random.default_rng(g))
    n = Qs[0].shape[0]
    NZ = np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1))
    y = np.random.default_rng(1).poisson(20.0, n).astype(float)
    dpos = diag_positions(Qs[0])
    kw = dict(refactorize_final=True)

    bb = gmrfx.MI355XBatchLaplace(Qs[0], B, coords=pts, device=0)
    bb.set_observations("poisson", y, param=0.0)
    perm = bb.ordering_permutation()
    dX = torch.empty(n * B, dtype=torch.float64, device="cuda:0")
    dX0 = torch.zeros(n * B, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    res = {}

    def batched():
        bb.set_prior(NZ)
        res["b"] = bb.gaussian_approximation_dev(dX.data_ptr(), n, d_x0=dX0.data_ptr(), sx0=n, **kw)
    t_b = timed(batched, a.reps, a.warmup)
    Xb = dX.cpu().numpy().reshape(B, n).copy()

    plain = gmrfx.MI355XBackend(Qs[0], ordering=perm, device=0, factorize=False)
    dx = torch.empty(n * B, dtype=torch.float64, device="cuda:0")
    its = np.zeros(B, np.int64)

    def sequential():
        for k in range(B):
            plain.set_prior(NZ[:, k], dpos)
            plain.set_observations("poisson", y)
            i = plain.gaussian_approximation_dev(dx.data_ptr() + 8 * k * n, d_x0=dX0.data_ptr(), **kw)
            its[k] = i["iterations"]
    t_s = timed(sequential, a.reps, a.warmup)
    Xs = dx.cpu().numpy().reshape(B, n).copy()
    plain.close()

    many = []
    for k in range(B):
        p = gmrfx.MI355XBackend(Qs[0], ordering=perm, device=0, factorize=False)
        p.set_prior(NZ[:, k], dpos)
        p.set_observations("poisson", y)
        many.append(p)

    def loops_only():
        for k, p in enumerate(many):
            p.gaussian_approximation_dev(dx.data_ptr() + 8 * k * n, d_x0=dX0.data_ptr(), **kw)
    t_l = timed(loops_only, a.reps, a.warmup)
    for p in many:
        p.close()

    ib = res["b"]
    assert np.array_equal(ib["iterations"], its), (ib["iterations"], its)
    row = {"tool": "tools/batch_ga_bench.py", "device": torch.cuda.get_device_name(0), "source_tree_hash": _lib.source_tree_hash(),
           "n": n, "grid": g, "B": B, "family": "poisson", "reps": a.reps, "warmup": a.warmup,
           "batched": t_b, "one_plain_handle_sequential": t_s, "plain_loop_only": t_l,
           "ms_per_member_batched": t_b["median_ms"] / B, "ms_per_member_sequential": t_s["median_ms"] / B,
           "speedup_vs_sequential": t_s["median_ms"] / t_b["median_ms"], "speedup_vs_loops_only": t_l["median_ms"] / t_b["median_ms"],
           "iterations": ib["iterations"].tolist(), "iteration_counts_agree": True, "totals": ib["totals"],
           "sum_member_factorizations": int(ib["factorizations"].sum()), "max_abs_mode_diff": float(np.abs(Xb - Xs).max())}
    print(json.dumps(row), flush=True)
    bb.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
