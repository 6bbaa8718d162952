"""The cases, the restatements and the bounds of tests/test_gpu_readout_edges.py, verified WITHOUT a device (the factor's diagonal
and Sigma come from the CPU here, pattern facts from symbolic_only handles): the launch constants restate the source; every case of
tests/readout_edges.py reaches the edge it names (nparts, per, nblk, lane passes, chunk, pair and tile counts recomputed with the
launch wrappers' formulas); the float64 restatement in numpy's own summation order stays within the first-order bounds WITHOUT the
factor 16 (the control that justifies the bounds; pytest -rP shows the ratios); every named mutant exceeds the device bound."""
import os
import re

import numpy as np
import pytest

import gmrfx
import readout_edges as re_
import readout_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc")
LD = rr.LD
_SIGMA = {}


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def sigma_feed(name):
    """(Q, Sigma dense, factor pattern dense, the value a clamped read of a masked entry would see) with the CPU in the handle's place"""
    if name not in _SIGMA:
        Q = re_.SIGMA_Q[name]()
        be = gmrfx.MI355XBackend(Q, symbolic_only=True)
        inpat = re_.factor_pattern(be)
        be.close()
        Sig = np.linalg.inv(Q.toarray())
        _SIGMA[name] = (Q, Sig, inpat, float(Sig.max()))
    return _SIGMA[name]


def _worst(tag, ratios):
    print(f"{tag}: control/bound " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def _ratio(got, ref, factor):
    return rr.ratio(got["value"], ref["value"], rr.bound_sum(ref, factor))


def test_constants_restate_the_source():
    u, q, b, d, a, dv = (_src(f) for f in ("util_kernels.hip", "quadform.hip", "batch.hip", "dense.hip", "api_selinv.cpp", "device.cpp"))
    assert f"constexpr int QF_COLS = {rr.QF_COLS};" in q and f"constexpr int QF_COLS = {rr.QF_COLS};" in b
    assert "const int g = tid >> 4, l = tid & 15;" in q and "p += 16" in q and "const int j = blockIdx.x * QF_COLS + t * 16 + g;" in q
    assert "for (int i = tid; i < nblk; i += 256) acc += p[i];" in q and "for (int i = tid; i < nblk; i += 256) acc += p[i];" in b
    assert f"constexpr int BD_COLS = {rr.BD_COLS};" in b and "const int c = c0 + tid + 256 * u;" in b
    assert "std::min<long long>(1024, std::max<long long>(1, (S_->n + 255) / 256))" in dv
    assert "const int per = (n + gridDim.x - 1) / gridDim.x;" in u and "for (int k = k0 + tid; k < k1; k += 256)" in u
    assert u.count("t < t1; t += 64") == 2 and u.count("for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh, 64);") == 2
    assert "(p == q ? 1.0 : 2.0) * vals[p] * vals[q] * src[o >= 0 ? o : 0] * (o >= 0 ? 1.0 : 0.0)" in u
    assert f"const i64 CH = {rr.DOT_CHUNK}" in a and "for (double v : part) acc += v;" in a and "seg[i + 1] = seg[i] + k * (k + 1) / 2;" in a
    assert "const int mt = (n1 + 63) / 64;" in d and "const long long groups = (nt + 7) / 8;" in d and "groups * mt * 8" in d
    assert "const int qpair = (n2 & 1) ? n1 - 1 : n1;" in d and "nvec > 65535" in dv
    assert re.search(r"q0 \+ 8 <= qhi; q0 \+= 8", _src("kernel_common.h"))
    assert rr.NVEC_MAX == 65535


# ---- every case reaches its edge ------------------------------------------------------------------------------------------------------------
def test_logdet_cases_reach_their_edges():
    launch = {n: rr.logdet_launch(n) for n in re_.LOGDET_CHAINS + tuple(n for n, _ in re_.LOGDET_BIG)}
    assert [launch[n] for n in re_.LOGDET_CHAINS] == [(1, 1), (1, 255), (1, 256), (2, 129), (2, 256), (3, 171)]
    assert launch[262144] == (1024, 256) and launch[262145] == (1024, 257)
    k0, k1 = rr.logdet_blocks(257)
    assert list(k1 - k0) == [129, 128]
    # a thread loops (a second pass) first at per = 257, and blocks past the end exist first there
    assert all(rr.logdet_launch(n)[1] <= 256 for n in (1, 2, 255, 256, 257, 65537, 262143, 262144))
    assert all(not (np.diff(np.stack(rr.logdet_blocks(n)), axis=0) <= 0).any() for n in (257, 513, 65281, 130817, 262144))
    k0, k1 = rr.logdet_blocks(262145)
    assert list(np.flatnonzero(k1 < k0)) == [1021, 1022, 1023] and k1[1020] - k0[1020] == 5 and k0[1020] + 4 == 262144
    assert rr.logdet_depth(262144) == 1 + 8 + 4 + 8 + 1 and rr.logdet_depth(262145) == 2 + 8 + 4 + 8 + 1 and rr.logdet_depth(513) == 19
    # spread: sum log cancels against sum |log|
    r = rr.logdet(re_.chain_factor_diag(re_.chain(513, "spread")))
    assert abs(r["value"]) < 0.2 * r["abs"] and r["abs"] > 2 * 513 * 2.0
    # batched
    assert [rr.batch_parts(nm) for nm in re_.BATCH_NM] == [1, 1, 1, 2, 3] and re_.BATCH_B == (1, 3)
    for nm in (1025, 2049):
        ca, cb = re_.failing_columns(nm)
        assert ca < cb < nm and ca // rr.BD_COLS != cb // rr.BD_COLS and (ca % rr.BD_COLS) % 256 != (cb % rr.BD_COLS) % 256
    d = np.ones(2049)
    d[[700, 1500]] = np.nan, -1.0
    assert rr.batch_info(d) == 701 and rr.batch_info(np.ones(5)) == 0


def test_quadform_cases_reach_their_edges():
    ns = set(re_.QUAD_N)
    assert {n % 16 for n in ns if n < 128} >= {0, 1, 15} and {n - 128 for n in ns} >= {-1, 0, 1} and {1, 257} <= ns
    assert rr.quadform_blocks(32768) == 256 and rr.quadform_blocks(32769) == 257 and rr.cdiv(257, 256) == 2 and rr.cdiv(256, 256) == 1
    assert re_.QUAD_NVEC == (1, 2, 7)
    for k in re_.HUB_ENTRIES:
        for hub in (0, re_.HUB_N - 1):
            Q = re_.arrowhead(k, hub)
            lens = np.diff(Q.indptr)
            assert lens[hub] == k and (np.delete(lens, hub) <= 2).all() and abs(Q - Q.T).max() == 0
            assert rr.cdiv(k, 16) == {1: 1, 16: 1, 17: 2, 33: 3}[k]
    # the 17th entry of the hub column: an off-diagonal of the lower triangle (hub first), the diagonal itself (hub last)
    Q0, Q1 = re_.arrowhead(17, 0), re_.arrowhead(17, re_.HUB_N - 1)
    assert Q0.indices[Q0.indptr[0] + 16] == 16 and Q1.indices[Q1.indptr[re_.HUB_N - 1] + 16] == re_.HUB_N - 1
    Q = re_.chain(129)
    for use_lower in (False, True):
        un = re_.unused_triangle(Q, use_lower)
        col = np.repeat(np.arange(129), np.diff(Q.indptr))
        assert len(un) == 128 and ((Q.indices[un] < col[un]) if use_lower else (Q.indices[un] > col[un])).all()
    z = re_.with_stored_zeros(Q)
    assert (z == 0).sum() >= 40 and (z[Q.indices == col] != 0).all()
    # the defining triangle alone gives the dense form
    X, mu = re_.quad_operands(129, 2)
    for use_lower in (False, True):
        v = Q.data.copy()
        v[re_.unused_triangle(Q, use_lower)] = 1e30
        r = rr.quadform(Q.indptr, Q.indices, v, X, mu, use_lower)
        R = X - mu[:, None]
        want = np.einsum("iv,ij,jv->v", R, Q.toarray(), R)
        assert np.abs(np.asarray(r["value"], np.float64) - want).max() <= 1e-12 * np.abs(want).max()


def test_sigma_cases_reach_their_edges():
    assert [len(rr.dot_chunks(c)) - 1 for c in re_.DOT_COUNTS] == [0, 1, 1, 1, 1, 1, 1, 2, 3]
    assert [rr.cdiv(c, 64) for c in (63, 64, 65)] == [1, 1, 2]
    assert tuple(k * (k + 1) // 2 for k in re_.ROW_ENTRIES) == re_.ROW_PAIRS
    assert [rr.cdiv(p, 64) for p in re_.ROW_PAIRS] == [0, 1, 1, 1, 2, 3, 9]           # on either side of one and two wave passes
    for name in re_.SIGMA_Q:
        Q, Sig, inpat, _ = sigma_feed(name)
        n = Q.shape[0]
        assert inpat[Q.nonzero()].all() and np.array_equal(inpat, inpat.T) and 0.05 < inpat.mean() < 0.6, (name, inpat.mean())
        for cnt in re_.DOT_COUNTS:
            if cnt > n * n:
                assert name == "chain70" and cnt == 8193
                continue
            B = re_.dot_pattern(Q, inpat, cnt)
            assert B.nnz == cnt and B.has_sorted_indices
            r, c = B.indices, np.repeat(np.arange(n), np.diff(B.indptr))
            outside = ~inpat[r, c]
            if cnt > 4000:
                assert outside.sum() > 100 and (B.data[outside] == re_.HUGE).sum() > 10 and (B.data[~outside] == 0).sum() > 10
                assert (np.abs(B.data[~outside]) < 1e4).all()
        A = rr.csr(re_.design(n))
        lens = np.diff(A.indptr)
        assert tuple(lens[:-1]) == re_.ROW_ENTRIES and lens[-1] == 3 and re_.design(n).nnz == sum(re_.ROW_ENTRIES) + 4
        assert A[len(re_.ROW_ENTRIES), 3] == 1.25 and (A.data < 0).any() and (A.data > 0).any()
        seg, pi, qi = rr.row_pairs(A)
        assert tuple(np.diff(seg)[:-1]) == re_.ROW_PAIRS and (qi <= pi).all()
        jp, jq = A.indices[pi], A.indices[qi]
        per_row_out = np.add.reduceat(~inpat[jp, jq], seg[:-1][np.diff(seg) > 0])
        assert (per_row_out > 0).any() and (per_row_out < np.diff(seg)[np.diff(seg) > 0]).all()         # rows PARTLY outside
        pats = [rr.csr(X) for X in re_.other_designs(n)]
        assert len({(tuple(P.indptr), tuple(P.indices)) for P in pats + [A]}) == 5


def test_dense_cases_reach_their_edges():
    sh = set(re_.DENSE_SHAPES)
    assert {(n1, n2) for n1 in range(1, 10) for n2 in (3, 66)} <= sh and set(re_.DENSE_EDGE) <= sh
    assert {(1, 1), (1, 65), (65, 1)} <= set(re_.TRANSPOSE_SHAPES)
    # the masked path alone (n1 < 8), the pair path alone (n1 = 8 k, n2 even), both; the last row of T masked for odd n2
    split = {s: rr.dense_k_split(*s) for s in sh}
    assert split[(7, 3)] == (0, 7) and split[(8, 66)] == (8, 0) and split[(8, 3)] == (0, 8) and split[(9, 3)] == (8, 1) and split[(9, 66)] == (8, 1)
    assert split[(32, 64)] == (32, 0) and split[(33, 65)] == (32, 1) and split[(64, 512)] == (64, 0) and split[(65, 513)] == (64, 1)
    assert split[(65, 511)] == (64, 1) and split[(130, 1025)] == (128, 2) and split[(31, 63)] == (24, 7) and split[(63, 1)] == (56, 7)
    # waves that leave early (m0 >= n1 or n0 >= n2), tiles dealt over 8 slots with empty workgroups, more than one group
    assert any(n1 <= 32 for n1, _ in sh) and any(n2 <= 32 for _, n2 in sh) and any(32 < n1 % 64 for n1, _ in sh)
    assert rr.dense_tiles(130, 1025) == (3, 17, 72, 21) and rr.dense_tiles(64, 512) == (1, 8, 8, 0) and rr.dense_tiles(65, 513) == (2, 9, 32, 14)
    assert rr.dense_tiles(1, 3) == (1, 1, 8, 7)
    assert {n2 - 512 for _, n2 in sh} >= {-1, 0, 1} and {n1 for n1, _ in sh} >= {31, 32, 33} and {n2 for _, n2 in sh} >= {1, 2, 3}
    for n1, n2 in ((5, 66), (65, 513)):
        D, T = re_.dense_operands(n1, n2)
        assert (D < 0).any() and (D > 0).any() and np.abs(T).max() / np.abs(T).min() > 1e4


def test_every_mutant_has_its_case():
    assert set(re_.MUTANT_CASE) == set(rr.MUTANTS) and len(rr.MUTANTS) == 14


# ---- the control -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(n, k) for n in re_.LOGDET_CHAINS for k in ("plain", "spread")] + list(re_.LOGDET_BIG))
def test_control_logdet(n, kind):
    d = re_.chain_factor_diag(re_.chain(n, kind))
    ref, got = rr.logdet(d, LD), rr.logdet(d, np.float64)
    _worst(f"logdet n={n} {kind}", {"logdet": _ratio(got, ref, 1)})


@pytest.mark.parametrize("nm", re_.BATCH_NM)
def test_control_batch_logdet(nm):
    d = re_.chain_factor_diag(re_.chain(nm, "spread" if nm > 1 else "plain"))
    _worst(f"batchdiag nm={nm}", {"logdet": _ratio(rr.batch_logdet(d, np.float64), rr.batch_logdet(d, LD), 1)})


def _quad_matrices():
    out = [(f"chain{n}", re_.chain(n)) for n in re_.QUAD_N]
    return out + [(f"hub{k}_at{hub}", re_.arrowhead(k, hub)) for k in re_.HUB_ENTRIES for hub in (0, re_.HUB_N - 1)]


@pytest.mark.parametrize("name,Q", _quad_matrices(), ids=[m[0] for m in _quad_matrices()])
def test_control_quadform(name, Q):
    n = Q.shape[0]
    worst = {}
    for use_lower in (False, True):
        for nvec in re_.QUAD_NVEC:
            X, mu = re_.quad_operands(n, nvec)
            for m in (mu, None):
                ref = rr.quadform(Q.indptr, Q.indices, Q.data, X, m, use_lower, LD)
                got = rr.quadform(Q.indptr, Q.indices, Q.data, X, m, use_lower, np.float64)
                worst["quad"] = max(worst.get("quad", 0.0), _ratio(got, ref, 1))
    X, mu = re_.quad_operands(n, 2)
    Xn = mu[:, None] * (1 + 1e-8 * X)                                  # x - mu of order 1e-8 |x|
    ref = rr.quadform(Q.indptr, Q.indices, re_.with_stored_zeros(Q), Xn, mu, True, LD)
    got = rr.quadform(Q.indptr, Q.indices, re_.with_stored_zeros(Q), Xn, mu, True, np.float64)
    worst["near_mean"] = _ratio(got, ref, 1)
    _worst(name, worst)


@pytest.mark.parametrize("name", list(re_.SIGMA_Q))
def test_control_sigma(name):
    Q, Sig, inpat, s0 = sigma_feed(name)
    n = Q.shape[0]
    worst = {"dot": 0.0}
    for cnt in re_.DOT_COUNTS:
        if cnt > n * n:
            continue
        B = re_.dot_pattern(Q, inpat, cnt)
        r, c = B.indices, np.repeat(np.arange(n), np.diff(B.indptr))
        ref = rr.selinv_dot(B.data, Sig[r, c], inpat[r, c], LD)
        got = rr.selinv_dot(B.data, Sig[r, c], inpat[r, c], np.float64)
        assert np.isfinite(float(ref["value"])) and (cnt > 0 or (ref["value"] == 0 and ref["abs"] == 0))
        worst["dot"] = max(worst["dot"], _ratio(got, ref, 1))
    A = re_.design(n)
    for products in (2, 3):
        worst[f"rows{products}"] = _ratio(rr.row_diag(A, Sig, inpat, np.float64, products), rr.row_diag(A, Sig, inpat, LD, products), 1)
    # with the whole pattern inside, the restatement is diag(A Sigma A')
    Ad = rr.csr(A).toarray()
    full = rr.row_diag(A, Sig, np.ones_like(inpat), LD)
    want = np.diag(Ad @ Sig @ Ad.T)
    assert np.abs(np.asarray(full["value"], np.float64) - want).max() <= 1e-12 * np.abs(want).max()
    _worst(name, worst)


@pytest.mark.parametrize("n1,n2", re_.DENSE_SHAPES)
def test_control_dense(n1, n2):
    D, T = re_.dense_operands(n1, n2)
    _worst(f"dense {n1}x{n2}", {"dense": _ratio(rr.dense_apply(D, T, np.float64), rr.dense_apply(D, T, LD), 1)})
    assert np.array_equal(rr.transpose(T), T.T)


# ---- the mutants ----------------------------------------------------------------------------------------------------------------------------
def _mutant_ratios(mutant):
    """(clean float64 ratio, mutant ratio) against the long-double reference with the DEVICE bound (F = 16)"""
    case = re_.MUTANT_CASE[mutant]
    if case[0] == "logdet":
        d = re_.chain_factor_diag(re_.chain(case[1], case[2]))
        ref = rr.logdet(d, LD)
        return _ratio(rr.logdet(d, np.float64), ref, rr.FACTOR), _ratio(rr.logdet(d, np.float64, mutant), ref, rr.FACTOR)
    if case[0] in ("quad", "hub"):
        clean = worst = 0.0
        for hub, use_lower in ((0, True), (re_.HUB_N - 1, False)):
            Q = re_.chain(case[1]) if case[0] == "quad" else re_.arrowhead(case[1], hub)
            X, mu = re_.quad_operands(Q.shape[0], 2)
            ref = rr.quadform(Q.indptr, Q.indices, Q.data, X, mu, use_lower, LD)
            clean = max(clean, _ratio(rr.quadform(Q.indptr, Q.indices, Q.data, X, mu, use_lower, np.float64), ref, rr.FACTOR))
            r = rr.ratio(rr.quadform(Q.indptr, Q.indices, Q.data, X, mu, use_lower, np.float64, mutant)["value"], ref["value"], rr.bound_sum(ref))
            worst = r if worst == 0.0 else min(worst, r)                # caught under BOTH uplo
        return clean, worst
    if case[0] in ("dot", "rows"):
        Q, Sig, inpat, s0 = sigma_feed(case[1])
        n = Q.shape[0]
        if case[0] == "dot":
            B = re_.dot_pattern(Q, inpat, case[2])
            r, c = B.indices, np.repeat(np.arange(n), np.diff(B.indptr))
            f = lambda dt, mu=None: rr.selinv_dot(B.data, Sig[r, c], inpat[r, c], dt, mu, s0)       # noqa: E731
        else:
            A = re_.design(n)
            f = lambda dt, mu=None: rr.row_diag(A, Sig, inpat, dt, 3, mu, s0)                       # noqa: E731
        ref = f(LD)
        return _ratio(f(np.float64), ref, rr.FACTOR), _ratio(f(np.float64, mutant), ref, rr.FACTOR)
    D, T = re_.dense_operands(case[1], case[2])
    if case[0] == "transpose":
        return 0.0, (0.0 if np.array_equal(rr.transpose(T, mutant), T.T) else float("inf"))
    ref = rr.dense_apply(D, T, LD)
    return _ratio(rr.dense_apply(D, T, np.float64), ref, rr.FACTOR), _ratio(rr.dense_apply(D, T, np.float64, mutant), ref, rr.FACTOR)


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_mutant_exceeds_the_device_bound(mutant):
    clean, bad = _mutant_ratios(mutant)
    print(f"{mutant} on {re_.MUTANT_CASE[mutant]}: error/bound clean {clean:.3g} mutant {bad:.3g}")
    assert clean <= 1.0 / rr.FACTOR and bad > 1.0, (mutant, clean, bad)


def test_segment_mutants_show_in_the_pair_form_too():
    """element 64 dropped and a masked entry counted, on the design matrix's rows (the kept plan's kernel)"""
    Q, Sig, inpat, s0 = sigma_feed("grid")
    A = re_.design(Q.shape[0])
    ref = rr.row_diag(A, Sig, inpat, LD)
    for mutant in ("drop_elem_64", "masked_counts_sigma0"):
        assert _ratio(rr.row_diag(A, Sig, inpat, np.float64, 3, mutant, s0), ref, rr.FACTOR) > 1.0, mutant
