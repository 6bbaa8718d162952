"""Log-density gradients on Q's pattern, host only.

1. The dense restatement (tests/logpdf_grad_ref.py) against central differences of a dense numpy logpdf (+ constraint correction)
   along a random direction (dQ on the pattern, dmu): differences at h and h / 2, and
       |analytic - FD(h/2)| <= 4 |FD(h) - FD(h/2)| + eps |f| / h
   (the truncation error of a central difference falls by four when h halves, so the difference of the two estimates bounds it; the
   second term is the roundoff of f in the quotient). This pins the signs, the factor 1/2 and the triangle weights of the contraction.
2. The C ABI on symbolic-only handles: every new entry point validates its arguments, then answers NO_DEVICE; the refusals are
   INVALID_ARG with a message."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import logpdf_grad_ref as ref
from gmrfx._lib import GmrfxOpts, lib, ptr

INVALID_ARG, NO_DEVICE = 1, 2


def _spd_pattern(n, seed):
    """a sparse symmetric positive definite matrix, both triangles stored, a few long-range entries"""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    for i in range(n - 1):
        D[i, i + 1] = D[i + 1, i] = -rng.uniform(0.2, 1.0)
    for _ in range(n // 3):
        i, j = rng.integers(0, n, 2)
        if i != j:
            D[i, j] = D[j, i] = -rng.uniform(0.1, 0.5)
    D += np.diag(np.abs(D).sum(1) + rng.uniform(0.5, 1.5, n))
    return sp.csc_matrix(D)


@pytest.mark.parametrize("mode", ["full", "L", "U"])
@pytest.mark.parametrize("n,m", [(n, m) for n in (1, 2, 7, 30) for m in (0, 1, 3) if m <= n])
def test_restatement_against_central_differences(n, m, mode):
    rng = np.random.default_rng(1000 * n + 10 * m + len(mode))
    Q = _spd_pattern(n, n + m)
    if mode != "full":          # the other triangle holds junk that must not matter
        junk = Q.copy()
        cols = np.repeat(np.arange(n), np.diff(Q.indptr))
        other = junk.indices < cols if mode == "L" else junk.indices > cols
        junk.data[other] = 1e3
        Q = junk
    A, e = (ref.sum_to_zero(n, m) if m else (None, None))
    if m:
        A = sp.csr_matrix(A.multiply(rng.uniform(0.5, 1.5, (1, n))))
    z, mu = rng.standard_normal(n), rng.standard_normal(n)
    ybar = 1.7
    dQ = rng.standard_normal(Q.nnz)
    if mode == "full":          # a symmetric direction
        S = sp.csc_matrix((dQ, Q.indices, Q.indptr), shape=Q.shape)
        dQ = ref.on_pattern(((S + S.T) / 2).toarray(), Q)
    dmu = rng.standard_normal(n)

    def f(t):
        Qt = sp.csc_matrix((Q.data + t * dQ, Q.indices, Q.indptr), shape=Q.shape)
        return ybar * ref.logpdf_dense(ref.symmetric_dense(Qt, mode), z, mu + t * dmu, A, e)

    Qbar, mubar = ref.grad_dense(ref.symmetric_dense(Q, mode), z, mu, ybar, A, e)
    analytic = ref.pattern_dot(Q, mode, ref.on_pattern(Qbar, Q), dQ[:, None])[0] + mubar @ dmu
    h = 1e-3
    fd1 = (f(h) - f(-h)) / (2 * h)
    fd2 = (f(h / 2) - f(-h / 2)) / h
    bound = 4 * abs(fd1 - fd2) + ref.EPS * abs(f(0.0)) / h
    print(f"n={n} m={m} {mode}: analytic {analytic:.12e} FD(h/2) {fd2:.12e} |diff| {abs(analytic - fd2):.2e} bound {bound:.2e}")
    assert abs(analytic - fd2) <= bound


def test_long_double_constraint_terms_agree_with_float64():
    n, m = 24, 3
    Q = _spd_pattern(n, 5).toarray()
    A, e = ref.sum_to_zero(n, m)
    At = np.linalg.solve(Q, A.toarray().T)
    mu = np.linspace(-1, 1, n)
    T64, abs64, a64, _ = ref.constraint_terms(At, A @ At, A, e, mu)
    Tld, _, ald, _ = ref.constraint_terms(At, A @ At, A, e, mu, np.longdouble)
    assert np.abs(T64 - Tld.astype(np.float64)).max() <= 64 * ref.EPS * abs64.max()
    assert np.abs(a64 - ald.astype(np.float64)).max() <= 64 * ref.EPS * np.abs(a64).max()


# ---- the C ABI on symbolic-only handles ----------------------------------------------------------------------------------------
N = 6


def _pattern():
    cp, ri = [0], []
    for j in range(N):
        ri += [i for i in (j - 1, j, j + 1) if 0 <= i < N]
        cp.append(len(ri))
    return np.array(cp, dtype=np.int64), np.array(ri, dtype=np.int64)


COLPTR, ROWVAL = _pattern()
NNZ = int(COLPTR[-1])


class _Handle:
    def __init__(self, nbatch=0, **opts):
        self.nbatch, self.opts = nbatch, opts

    def __enter__(self):
        self.h = C.c_void_p()
        o = GmrfxOpts()
        o.struct_size = C.sizeof(GmrfxOpts)
        o.symbolic_only = 1
        o.device = -1
        for k, v in self.opts.items():
            setattr(o, k, v)
        if self.nbatch:
            rc = lib().gmrfx_create_batched(N, ptr(COLPTR), ptr(ROWVAL), 0, None, self.nbatch, C.byref(o), C.byref(self.h))
        else:
            rc = lib().gmrfx_create(N, ptr(COLPTR), ptr(ROWVAL), 0, None, C.byref(o), C.byref(self.h))
        assert rc == 0 and self.h.value, lib().gmrfx_last_create_error()
        return self.h

    def __exit__(self, *exc):
        lib().gmrfx_destroy(self.h)


def _msg(h):
    return lib().gmrfx_last_error(h).decode()


def _calls(h, nb, z="ok", out="ok", G="ok", ldj=NNZ, p=2, ybar="ok"):
    """the eight entry points with host arrays of the right sizes (a "null" argument replaces one of them)"""
    L = lib()
    B = max(nb, 1)
    zz, mu, yb = np.zeros((N, B), order="F"), np.zeros((N, B), order="F"), np.ones(B)
    qb, mb, info = np.zeros((NNZ, B), order="F"), np.zeros((N, B), order="F"), np.zeros(B, np.int64)
    g, J, o = np.zeros((NNZ, B), order="F"), np.zeros((max(ldj, 1) * max(p, 1) * B,)), np.zeros(max(p, 1) * B)
    pz = None if z == "null" else ptr(zz)
    pq, pm = (None, None) if out == "null" else (ptr(qb), ptr(mb))
    pg = None if G == "null" else ptr(g)
    pyb = None if ybar == "null" else ptr(yb)
    res = {}
    if nb == 0:
        res["gmrfx_logpdf_grad"] = L.gmrfx_logpdf_grad(h, None, pz, ptr(mu), 1.0, pq, pm)
        res["gmrfx_logpdf_grad_dev"] = L.gmrfx_logpdf_grad_dev(h, None, pz, ptr(mu), 1.0, pq, pm)
        res["gmrfx_pattern_dot"] = L.gmrfx_pattern_dot(h, pg, ptr(J), ldj, p, ptr(o))
        res["gmrfx_pattern_dot_dev"] = L.gmrfx_pattern_dot_dev(h, pg, ptr(J), ldj, p, ptr(o))
    res["gmrfx_batch_logpdf_grad"] = L.gmrfx_batch_logpdf_grad(h, None, pz, N, ptr(mu), pyb, pq, pm, ptr(info))
    res["gmrfx_batch_logpdf_grad_dev"] = L.gmrfx_batch_logpdf_grad_dev(h, None, pz, N, ptr(mu), pyb, pq, pm, ptr(info))
    res["gmrfx_batch_pattern_dot"] = L.gmrfx_batch_pattern_dot(h, pg, ptr(J), ldj, max(ldj, 1) * max(p, 1), p, ptr(o))
    res["gmrfx_batch_pattern_dot_dev"] = L.gmrfx_batch_pattern_dot_dev(h, pg, ptr(J), ldj, max(ldj, 1) * max(p, 1), p, ptr(o))
    return res


@pytest.mark.parametrize("nbatch", [0, 3])
def test_valid_calls_on_symbolic_only_handles_answer_no_device(nbatch):
    with _Handle(nbatch) as h:
        res = _calls(h, nbatch)
        assert len(res) == (8 if nbatch == 0 else 4)
        for name, rc in res.items():
            assert rc == NO_DEVICE, (name, rc, _msg(h))
        assert "no device state" in _msg(h)


@pytest.mark.parametrize("nbatch", [0, 3])
@pytest.mark.parametrize("what,kw,only", [
    ("z is null", dict(z="null"), "logpdf_grad"),
    ("Qbar and mubar are both null", dict(out="null"), "logpdf_grad"),
    ("G / J / out is null", dict(G="null"), "pattern_dot"),
    ("p < 1", dict(p=0), "pattern_dot"),
    ("ldj < nnz", dict(ldj=NNZ - 1), "pattern_dot"),
])
def test_refused_arguments(nbatch, what, kw, only):
    with _Handle(nbatch) as h:
        for name, rc in _calls(h, nbatch, **kw).items():
            if only in name:
                assert rc == INVALID_ARG, (name, rc)
            else:
                assert rc == NO_DEVICE, (name, rc)
        # the message of the refusal itself (the last refusing call of its kind)
        L = lib()
        if only == "logpdf_grad":
            rc = L.gmrfx_batch_logpdf_grad(h, None, None if "z" in kw else ptr(np.zeros(N * 3)), N, None, ptr(np.ones(3)),
                                           None if "out" in kw else ptr(np.zeros(NNZ * 3)), None, None)
        else:
            rc = L.gmrfx_batch_pattern_dot(h, None if "G" in kw else ptr(np.zeros(NNZ * 3)), ptr(np.zeros(NNZ * 6)), kw.get("ldj", NNZ), NNZ * 2,
                                           kw.get("p", 2), ptr(np.zeros(6)))
        assert rc == INVALID_ARG and what in _msg(h), _msg(h)


def test_null_ybar_and_overlapping_members_are_refused():
    with _Handle(3) as h:
        res = _calls(h, 3, ybar="null")
        assert res["gmrfx_batch_logpdf_grad"] == INVALID_ARG and res["gmrfx_batch_logpdf_grad_dev"] == INVALID_ARG
        z, yb, q = np.zeros(3 * N), np.ones(3), np.zeros(3 * NNZ)
        assert lib().gmrfx_batch_logpdf_grad(h, None, ptr(z), N, None, None, ptr(q), None, None) == INVALID_ARG
        assert "ybar is null" in _msg(h)
        assert lib().gmrfx_batch_logpdf_grad(h, None, ptr(z), N - 1, None, ptr(yb), ptr(q), None, None) == INVALID_ARG
        assert "member stride" in _msg(h)
        assert lib().gmrfx_batch_pattern_dot(h, ptr(q), ptr(np.zeros(6 * NNZ)), NNZ, NNZ, 2, ptr(np.zeros(6))) == INVALID_ARG
        assert "member stride" in _msg(h)


def test_plain_forms_refuse_a_batched_handle():
    with _Handle(3) as h:
        z, q, o = np.zeros(N), np.zeros(NNZ), np.zeros(2)
        assert lib().gmrfx_logpdf_grad(h, None, ptr(z), None, 1.0, ptr(q), None) == INVALID_ARG
        assert "gmrfx_batch_logpdf_grad" in _msg(h)
        assert lib().gmrfx_pattern_dot(h, ptr(q), ptr(np.zeros(2 * NNZ)), NNZ, 2, ptr(o)) == INVALID_ARG
        assert "gmrfx_batch_pattern_dot" in _msg(h)


def test_sharded_handles_are_refused():
    with _Handle(0, shard_world=2, shard_rank=0) as h:
        for name, rc in _calls(h, 0).items():
            assert rc == INVALID_ARG, (name, rc)
            assert "sharded" in _msg(h)


@pytest.mark.parametrize("nbatch", [0, 3])
def test_pattern_nnz_is_the_members_stored_entries(nbatch):
    with _Handle(nbatch) as h:
        nnz = C.c_int64(-1)
        assert lib().gmrfx_pattern_nnz(h, C.byref(nnz)) == 0 and nnz.value == NNZ
        assert lib().gmrfx_pattern_nnz(h, None) == INVALID_ARG
