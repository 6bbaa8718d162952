"""The cases, the restatement and the bounds of tests/test_gpu_constraint_edges.py, verified WITHOUT a device (A~' = Q^-1 A' and
diag Q^-1 come from the CPU here): the long-double restatement agrees with the mirror and with the dense kriging formulas; every
case of tests/constraint_edges.py reaches the edge it names and has kappa(W) <= 1e3; the float64 restatement in numpy's own
summation order stays within the first-order bounds WITHOUT the factor 16 on every case and output (the control that justifies the
bounds; pytest -rP shows the ratios); and every named mutant exceeds the device bound on the case that names it."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import constraint_edges as ce
import constraint_ref as cr
import gmrfx
from mirror.workspace_gmrf import ConstraintInfo, WorkspaceGMRF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc")
LD = cr.LD
_FEED = {}


def tridiag_inverse_diag(Q):
    """diag(Q^-1) of a symmetric tridiagonal Q from the two pivot recursions"""
    n = Q.shape[0]
    d, a = Q.diagonal(), (Q.diagonal(1) if n > 1 else np.zeros(0))
    fwd, bwd = np.empty(n), np.empty(n)
    fwd[0] = d[0]
    for i in range(1, n):
        fwd[i] = d[i] - a[i - 1] ** 2 / fwd[i - 1]
    bwd[n - 1] = d[n - 1]
    for i in range(n - 2, -1, -1):
        bwd[i] = d[i] - a[i] ** 2 / bwd[i + 1]
    return 1.0 / (fwd + bwd - d)


def feed(case, member=0):
    """(A, e, A~', sigma) with the CPU in the handle's place"""
    key = (case.name, member)
    if key not in _FEED:
        Q = sp.csc_matrix(case.Q(member))
        A, e = case.A_e()
        At = spla.splu(Q).solve(A.T.toarray()) if case.m else np.zeros((case.n, 0))
        _FEED[key] = (A, e, At.reshape(case.n, case.m), tridiag_inverse_diag(Q))
    return _FEED[key]


def outputs(case, dtype, nvec, mutant=None, member=0, linv=None):
    """every output of the restatement in `dtype`"""
    A, e, At, sigma = feed(case, member)
    c = cr.prepare(A, e, At, dtype, mutant=mutant, linv=linv)
    Y, Z, mu = case.operands(nvec)
    return {"core": c, "Xc": cr.correct(c, Y), "Xc_mu": cr.correct(c, Y, mu), "var": cr.variance(c, sigma)}


def compare(case, got, ref, factor):
    """name -> error / bound of `got` (outputs()) against the long-double `ref`, the way the GPU test compares the device"""
    c = ref["core"]
    r = {"X": cr.ratio(got["Xc"]["Xc"], ref["Xc"]["Xc"], cr.bound_X(c, ref["Xc"], factor)),
         "X_mu": cr.ratio(got["Xc_mu"]["Xc"], ref["Xc_mu"]["Xc"], cr.bound_X(c, ref["Xc_mu"], factor))}
    if case.m:
        r["W"] = cr.ratio(got["core"]["W"], c["W"], cr.bound_W(c, factor))
        r["logdet"] = cr.ratio(got["core"]["logdet"], c["logdet"], cr.bound_logdet(c, factor))
        r["var"] = cr.ratio(got["var"]["var"], ref["var"]["var"], cr.bound_var(c, ref["var"], factor), nonnegative=True)
    return r


def test_constants_restate_the_source():
    h = open(os.path.join(CSRC, "kernels.h")).read()
    for name, val in (("kConChunk", cr.CHUNK), ("kConColTile", cr.COLTILE), ("kConApplyGroups", cr.GROUPS)):
        assert int(re.search(r"constexpr int " + name + r" = (\d+);", h).group(1)) == val, name
    d = open(os.path.join(CSRC, "device_constraint.cpp")).read()
    assert int(re.search(r"constexpr long long kConColBatch = (\d+);", d).group(1)) == cr.COLBATCH
    k = open(os.path.join(CSRC, "constraint.hip")).read()
    # the launch table of launch_con_apply and the tile sizes the cases are built around
    for m in (1, 2, 3):
        assert f"else if (m == {m}) GMRFX_CON_VEC({m});" in k
    assert "if (m <= 0) GMRFX_CON_VEC(0);" in k and "else GMRFX_CON_MFMA(16);" in k
    for m, q in ((4, 1), (8, 2), (16, 4), (32, 8)):
        assert f"else if (m <= {m}) GMRFX_CON_MFMA({q});" in k
    assert "((long long)n + 63) >> 6" in k and "((long long)n + 255) >> 8" in k and "const int jc0 = blockIdx.y * 64;" in k
    assert [cr.template(m) for m in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)] == \
        ["vec<1>", "vec<2>", "vec<3>", "mfma<1>", "mfma<2>", "mfma<2>", "mfma<4>", "mfma<4>", "mfma<8>", "mfma<8>", "mfma<16>", "mfma<16>", "mfma<16>"]
    assert cr.template(0, True) == "vec<0>" and cr.template(0) is None


@pytest.mark.parametrize("name", ["rows_n17_m3", "choice_m5", "pairs"])
def test_restatement_agrees_with_the_mirror_and_the_dense_formulas(name):
    case = ce.CASES[name]
    A, e, At, sigma = feed(case)
    Y, Z, mu = case.operands(4)
    c = cr.prepare(A, e, At, LD)
    r, v = cr.correct(c, Y, mu), cr.variance(c, sigma)
    Ad = A.toarray()
    Sigma = np.linalg.inv(case.Q().toarray())
    SAt = Sigma @ Ad.T
    W = Ad @ SAt
    X = Y + mu[:, None]
    dense = X - SAt @ np.linalg.solve(W, Ad @ X - e[:, None])
    var_c = np.diag(Sigma - SAt @ np.linalg.solve(W, SAt.T))

    def rel(a, b):
        return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())

    assert rel(c["W"], W) < 1e-12 and abs(float(c["logdet"]) - np.linalg.slogdet(W)[1]) < 1e-11
    assert rel(r["Xc"], dense) < 1e-12 and rel(v["var"], var_c) < 1e-11 and rel(sigma, np.diag(Sigma)) < 1e-12
    assert np.abs(Ad @ np.asarray(r["Xc"], np.float64) - e[:, None]).max() < 1e-12

    class _Ws:
        loaded_version = 0

        def selinv_diag(self):
            return sigma

        def backward_solve(self, Zz):
            return Zz

    ci = object.__new__(ConstraintInfo)
    ci.matrix, ci.vector, ci.A_tilde_T, ci.L_c = sp.csc_matrix(A), e, At, np.linalg.cholesky(np.asarray(A @ At))
    d = object.__new__(WorkspaceGMRF)
    d.mean_, d.workspace, d.version, d.constraints = mu, _Ws(), 0, ci
    assert rel(r["Xc"], d.rand_from(Y)) < 1e-12 and rel(v["var"], d.var()) < 1e-11
    assert rel(c["L"], ci.L_c) < 1e-12


def test_every_case_reaches_its_edge():
    by_group = {}
    for case in ce.cases():
        by_group.setdefault(case.group, []).append(case)
        A, e = case.A_e()
        assert A.shape == (case.m, case.n) and (np.diff(A.indptr) > 0).all() and case.m <= 64
        assert case.m == 0 or (np.abs(A.data).min() >= 0.5 and np.abs(A.data).max() <= 8.0), case.name
    # kernel choice: all nine templates, the masked k-step and its clamped read
    choice = by_group["choice"]
    assert sorted(c.m for c in choice) == [0] + list(ce.CHOICE_M) and all(c.n % 16 and c.nvecs == (17,) for c in choice)
    assert {cr.template(c.m, True) for c in choice} == {"vec<0>", "vec<1>", "vec<2>", "vec<3>", "mfma<1>", "mfma<2>", "mfma<4>", "mfma<8>", "mfma<16>"}
    assert {c.m for c in choice if c.m > 3 and cr.padded_m(c.m) - c.m in (1, 2, 3) + (7, 15, 31)} >= {5, 9, 17, 33, 63}
    assert all(any(cr.padded_m(c.m) == 4 * q and c.m == 4 * q for c in choice) for q in (1, 2, 4, 8, 16))       # and every template full
    # rows of X: one, partial and full wave / workgroup tiles of both templates
    rows = by_group["rows"]
    assert {(c.n, cr.template(c.m)[:3]) for c in rows} >= {(n, "vec") for n in ce.ROWS_N} | {(n, "mfm") for n in ce.ROWS_N if n >= 5}
    assert {c.n % 16 for c in rows} >= {0, 1, 15} and {c.n % 64 for c in rows} >= {0, 1, 63} and {c.n - 256 for c in rows} >= {-1, 0, 1}
    # columns
    cols = by_group["cols"]
    assert {(c.m, c.nvecs[0]) for c in cols} == {(m, k) for m in (2, 5) for k in ce.COLS_NVEC}
    ks = {c.nvecs[0] for c in cols}
    assert {k % cr.COLTILE for k in ks} >= {0, 1, 7} and {k - 64 for k in ks} >= {-1, 0, 1} and {k % 16 for k in ks if k < 64} >= {0, 1, 15}
    assert {len(cr.pieces(k)) for k in ks} == {1, 2, 3} and cr.pieces(1025) == [(0, 1024), (1024, 1)] and cr.pieces(2049)[2] == (2048, 1)
    # row length: every chunk count in one launch
    (rl,) = by_group["rowlen"]
    lens, nch, choff = cr.chunks(rl.A_e()[0])
    assert tuple(lens) == ce.ROWLEN and list(nch) == [1, 1, 1, 2, 2, 2, 3] and choff[-1] == 12 and rl.nvecs == (1, 9)
    assert {int(l) - 4096 for l in lens} >= {-1, 0, 1} and {int(l) - 8192 for l in lens} >= {-1, 0, 1}
    # pair loads: the census of each row on each layout
    (pr,) = by_group["pairs"]
    A = pr.A_e()[0]
    assert [int(p) % 2 for p in A.indptr[:4]] == [0, 0, 0, 1]
    for lay, (pad, off) in ce.LAYOUTS.items():
        cen = [cr.pair_census(A, r, pr.n + pad, off, 3) for r in range(4)]
        assert cen[0]["lone"] == 0 and cen[0]["vec16"] + cen[0]["two8"] == 15, lay
        assert (cen[0]["vec16"] > 0) == (off == 0 or (pr.n + pad) % 2 == 1), lay      # every column start odd: no aligned pair in row 0
        assert (cen[0]["two8"] > 0) == ((pr.n + pad) % 2 == 1 or off == 1), lay      # an odd column start: the pair is split
        assert cen[1] == {"vec16": 0, "two8": 15, "lone": 0}, lay
        assert cen[2]["lone"] == 3 and cen[2]["vec16"] + cen[2]["two8"] == 9, lay
        assert cen[3]["lone"] == 0 and cen[3]["vec16"] + cen[3]["two8"] == 6, lay
        assert sum(c["vec16"] for c in cen) > 0 and sum(c["two8"] for c in cen) > 0
    assert {((pr.n + pad) % 2, off) for pad, off in ce.LAYOUTS.values()} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    # in the contiguous host calls (ldx = n = 41, odd) rows 0 and 3 take both paths too
    assert all(0 < cr.pair_census(A, r, pr.n, 0, 3)["vec16"] < 3 * (len(ce.PAIR_COLS[r]) // 2) for r in (0, 3))
    # tile walk
    for c, (tile, tmpl) in zip(by_group["tiles"], ((64, "mfma<2>"), (256, "vec<2>"))):
        ntile = -(-c.n // tile)
        assert cr.template(c.m) == tmpl and ntile == cr.GROUPS + 1 and c.n % tile in (17, 3) and c.nvecs == (2,)
    assert all(-(-c.n // 64) <= cr.GROUPS for c in ce.cases() if c.group != "tiles")
    # batched
    assert sorted(c.m for c in by_group["batched"]) == list(ce.BATCH_M) and all(c.members == 2 for c in by_group["batched"])
    b = by_group["batched"][0]
    Q0, Q1 = b.Q(0), b.Q(1)
    assert np.array_equal(Q0.indices, Q1.indices) and np.array_equal(Q0.indptr, Q1.indptr) and (Q0.data != Q1.data).all()
    # every mutant has its case
    assert set(ce.MUTANT_CASE) == set(cr.MUTANTS) and all(n in ce.CASES for n, _ in ce.MUTANT_CASE.values())


def test_staged_forms_give_the_sorted_row():
    """on a symbolic handle: log det(A A') of the unsorted and the duplicated form has the bits of the sorted row's"""
    case = ce.CASES["pairs"]
    A, e = case.A_e()
    be = gmrfx.MI355XBackend(case.Q(), symbolic_only=True)
    be.set_constraints(A, e)
    want = be.constraint_info()
    forms = list(ce.staged_forms(A))
    assert [f[0] for f in forms] == ["unsorted", "duplicates"]
    for name, rp, ci, va in forms:
        assert not np.array_equal(ci[:len(A.indices)], A.indices) or len(ci) != len(A.indices), name
        B = cr.csr(sp.csr_matrix((va.copy(), ci.copy(), rp.copy()), shape=A.shape))
        assert np.array_equal(B.indices, A.indices) and np.array_equal(B.data, A.data), name
        be.set_constraints_csr(case.m, rp, ci, va, e)
        assert be.constraint_info() == want, name
    be.close()


@pytest.mark.parametrize("name", list(ce.CASES))
def test_conditioning_and_control(name):
    """kappa(W) <= 1e3, and the float64 restatement within the bounds WITHOUT the factor 16 (per output; the largest is printed)"""
    case = ce.CASES[name]
    worst = {}
    for member in range(case.members):
        for nvec in case.nvecs:
            ref = outputs(case, LD, nvec, member=member)
            if case.m:
                assert ref["core"]["kappa"] <= ce.KAPPA_MAX, (name, ref["core"]["kappa"])
            got = outputs(case, np.float64, nvec, member=member)
            for k, v in compare(case, got, ref, factor=1).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if case.m:
                for key in ("Xc", "Xc_mu"):
                    worst["residual"] = max(worst.get("residual", 0.0), cr.residual_ratio(ref["core"]["A"], ref["core"]["e"], got[key]["Xc"]))
    kap = f"kappa {ref['core']['kappa']:.3g} " if case.m else ""
    print(f"{name}: {kap}control/bound " + " ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_mutant_exceeds_the_device_bound(mutant):
    name, nvec = ce.MUTANT_CASE[mutant]
    case = ce.CASES[name]
    member = case.members - 1
    ref = outputs(case, LD, nvec, member=member)
    linv = None
    if mutant == "first_member_linv":
        A, e, At0, _ = feed(case, 0)
        linv = cr.prepare(A, e, At0, np.float64)["Linv"]
    got = outputs(case, np.float64, nvec, mutant=mutant, member=member, linv=linv)
    r = compare(case, got, ref, factor=cr.FACTOR)
    clean = compare(case, outputs(case, np.float64, nvec, member=member), ref, factor=cr.FACTOR)
    print(f"{mutant} on {name}: error/bound " + " ".join(f"{k} {v:.3g}" for k, v in sorted(r.items())))
    assert max(clean.values()) <= 1.0 / cr.FACTOR
    hit = {"drop_lone": ("W", "X"), "drop_last_chunk": ("W", "X"), "neighbour_chunks": ("W", "X"), "clamped_column": ("X",), "round_m_to_4": ("X",),
           "masked_reads_last": ("X",), "skip_second_piece": ("X",), "first_member_linv": ("X", "var"), "no_clamp": ("var",)}[mutant]
    for k in hit:
        assert r[k] > 1.0, (mutant, k, r[k])
