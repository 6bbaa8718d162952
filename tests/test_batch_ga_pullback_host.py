"""The batched pullback of gaussian_approximation, what needs no device (gmrfx_batch_ga_pullback[_dev] on symbolic_only handles; the
problems of tests/batch_ga_pullback_cases.py).

1. The header declares and the library exports both calls.
2. Every refusal of the C ABI on symbolic_only batched handles (B = 3 and B = 1), host and _dev form, with its message, in front of
   GMRFX_ERR_NO_DEVICE, and the likelihood in place is as it was afterwards. The plain call keeps refusing a batched handle.
3. The cases sit where the GPU tests claim: n > kGapNode, the chunk count of the intercept column, nobs of "rows" no multiple of 16,
   every healthy member's Q_p,k - H(x_k) positive definite with the margin the case file states, the failing member's lambda_min <= -1."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_ga_pullback_cases as gc
import fisher_ref as ref
from gmrfx._lib import lib, ptr
from test_ga_pullback_host import INVALID_ARG, _Handle, _msg

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gmrfx.h")


def test_header_declares_and_library_exports_both_calls():
    text = open(HEADER).read()
    for name in ("gmrfx_batch_ga_pullback", "gmrfx_batch_ga_pullback_dev"):
        assert re.search(r"int32_t\s+" + name + r"\s*\(", text), name
        assert callable(getattr(lib(), name))
        assert len(getattr(lib(), name).argtypes) == 13


def _call(h, n, nnz, B, x=True, sx=None, mu=False, smu=0, mubar=True, Qbar=True, flags=0, outs=(True, True, True), out=True, info=True, dev=False):
    a = lambda on, k: np.zeros(k) if on else None
    fn = lib().gmrfx_batch_ga_pullback_dev if dev else lib().gmrfx_batch_ga_pullback
    return fn(h, ptr(a(x, n * B)), n if sx is None else sx, ptr(a(mu, n * B)), smu, ptr(a(mubar, n * B)), ptr(a(Qbar, nnz * B)), flags,
              ptr(a(outs[0], nnz * B)), ptr(a(outs[1], n * B)), ptr(a(outs[2], n * B)), ptr(a(out, 2 * B)),
              ptr(np.zeros(B, np.int64)) if info else None)


def _obs_info(h, B):
    fam, nobs, c = C.c_int32(0), C.c_int64(0), np.zeros(B)
    assert lib().gmrfx_batch_obs_info(h, C.byref(fam), C.byref(nobs), ptr(c)) == 0
    return fam.value, nobs.value, c.tobytes()


@pytest.mark.parametrize("B", [3, 1])
def test_refusals_on_symbolic_only_batched_handles(B):
    Q = ref.banded(8, 1)
    n, nnz = 8, Q.nnz
    y = np.ones(n)
    with _Handle(Q, batched=B) as h:
        for dev in (False, True):
            assert _call(h, n, nnz, B, dev=dev) == INVALID_ARG and "no observation likelihood" in _msg(h)
        assert lib().gmrfx_batch_obs_set(h, 4, n, None, 0, ptr(y), None, ptr(np.linspace(1.0, 2.0, B))) == 0, _msg(h)
        before = _obs_info(h, B)
        no_device = lib().gmrfx_batch_fisher_eval(h, ptr(np.zeros(n * B)), n, None, 0, None, None, None, n, ptr(np.zeros(2 * B)))
        assert no_device not in (0, INVALID_ARG)
        refusals = [(dict(x=False), "x is null"), (dict(out=False), "out is null"), (dict(sx=n - 1), "x: member stride smaller than n"),
                    (dict(mu=True, smu=n - 1), "mu: member stride smaller than n"), (dict(mu=True, smu=-1), "mu: member stride smaller than n"),
                    (dict(flags=4), "unknown flag bits"), (dict(flags=-1), "unknown flag bits"), (dict(mubar=False, Qbar=False), "both null"),
                    (dict(outs=(False, False, False)), "every output is null"), (dict(flags=1), "needs a batch constraint"),
                    (dict(flags=3), "needs a batch constraint")]
        for kw, what in refusals:
            for dev in (False, True):
                assert _call(h, n, nnz, B, dev=dev, **kw) == INVALID_ARG, kw
                assert what in _msg(h), (kw, _msg(h))
        # behind the argument checks: no device, with or without the refactorisation bit, each nullable argument on its own
        for kw in (dict(), dict(flags=2), dict(mubar=False), dict(Qbar=False), dict(outs=(True, False, False)), dict(outs=(False, False, True)),
                   dict(mu=True, smu=0), dict(mu=True, smu=n), dict(sx=n + 3), dict(info=False)):
            for dev in (False, True):
                assert _call(h, n, nnz, B, dev=dev, **kw) == no_device, kw
        # with a batch constraint held: bit 0 passes the argument checks, and so does a call without the bit
        rp, ci, v, e = np.array([0, n], np.int64), np.arange(n, dtype=np.int64), np.ones(n), np.zeros(1)
        assert lib().gmrfx_batch_constraints_set(h, 1, ptr(rp), ptr(ci), ptr(v), 0, ptr(e)) == 0, _msg(h)
        assert _call(h, n, nnz, B, flags=1) == no_device and _call(h, n, nnz, B, flags=0) == no_device
        assert _obs_info(h, B) == before          # nothing of the handle's likelihood has changed
        # the plain call keeps refusing a batched handle (B = 1: its own likelihood is missing)
        rc = lib().gmrfx_ga_pullback(h, ptr(np.zeros(n * B)), None, ptr(np.zeros(n * B)), None, 0, None, None, ptr(np.zeros(n * B)), ptr(np.zeros(2)))
        assert rc == INVALID_ARG and ("batched" in _msg(h) if B > 1 else "no observation likelihood" in _msg(h))
    assert lib().gmrfx_batch_ga_pullback(None, None, 0, None, 0, None, None, 0, None, None, None, None, None) == INVALID_ARG


def test_a_plain_handle_without_a_batch_likelihood_is_refused():
    Q = ref.banded(8, 1)
    n, nnz = 8, Q.nnz
    with _Handle(Q) as h:
        assert lib().gmrfx_obs_set(h, 1, n, None, 0, ptr(np.ones(n)), None, 0.0) == 0          # (the plain likelihood is not the batch one)
        assert _call(h, n, nnz, 1) == INVALID_ARG and "no observation likelihood" in _msg(h)


def test_the_cases_sit_where_the_gpu_tests_claim():
    assert gc.case("grid")["Q"].shape[0] == 289 > gc.K_GAP_NODE
    assert gc.intercept_chunks() == (1537, 4)
    rows = gc.case("rows")["A"]
    assert rows.shape[0] % 16 != 0 and sorted(set(np.diff(rows.tocsr().indptr))) == [0, 1, 3, 16, 17, 33]
    for name in gc.NAMES:
        c = gc.case(name)
        if c["A"] is None:
            p = gc.problem(name, 1)
            assert 0 < len(p["obs"].idx) < p["n"] and len(set(p["obs"].idx)) == len(p["obs"].idx)          # a strict subset of the nodes
        for family in range(6):
            p = gc.problem(name, family)
            assert p["B"] == 3 and (len(set(p["params"])) == 3) == (family in (0, 4, 5))
            for k in range(3):
                lo = float(np.linalg.eigvalsh(gc.post_dense(p, k)).min())
                assert lo >= gc.MARGIN, (name, family, k, lo)
        f = gc.with_failing_member(gc.problem(name, 1))
        lo = float(np.linalg.eigvalsh(gc.post_dense(f, 1)).min())
        print(f"{name}: lambda_min of the failing member's Q_post {lo:.6f}")
        assert lo <= -1.0
        assert all(float(np.linalg.eigvalsh(gc.post_dense(f, k)).min()) >= gc.MARGIN for k in (0, 2))
