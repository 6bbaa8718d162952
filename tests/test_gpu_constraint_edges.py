"""The linear-constraint kernels (csrc/constraint.hip; drivers in csrc/device_constraint.cpp) entry by entry at every launch edge.

Cases: tests/constraint_edges.py (each names its edge; tests/test_constraint_edges_host.py checks without a device that it is
reached). Reference: tests/constraint_ref.py in np.longdouble, FED the handle's own A~' = constraint_fields()[0], its own selinv
diagonal and its own backward solve, so that the constraint kernels are judged on their own arithmetic. Bounds: the per-entry
first-order bounds derived in the docstring of tests/constraint_ref.py, times the project's factor 16; the control of the host test
holds them without that factor on the CPU.

Per case: every entry of W, of X_c from constraint_correct, constraint_correct_dev, sample and sample_dev without and with a mean, of
constrained_mean and of constrained_var within its bound; constrained_var never negative; log det W within its bound; the residual
|A X_c - e| <= 2 (24 + ceil(len_r / 4096)) eps (|A| |X_c| + |e|) per row and column; host and _dev forms, windows of larger NaN-filled
buffers (leading dimension above n, base aligned to 8 bytes only) and two runs agree bit for bit; nothing outside a window is written;
A~' has the bits of backend_solve of the dense A'. Batched cases: the same per member, against the restatement fed that member's
constraint_fields(k). Every case prints its largest error / bound ratio per output (pytest -rP)."""
import time

import numpy as np
import pytest
import torch

import constraint_edges as ce
import constraint_ref as cr
import gmrfx
import layout_buffers as lb
from layout_buffers import same_bits

pytestmark = pytest.mark.gpu
LD = cr.LD
_HANDLES = {}
DEFAULT_LAYOUTS = {"contiguous": (0, 0), "odd_ld_off1": (3, 1)}


def _handle(case):
    """one handle per distinct precision (n, members), built once per module"""
    key = (case.n, case.members)
    if key not in _HANDLES:
        t0 = time.perf_counter()
        if case.members == 1:
            be = gmrfx.MI355XBackend(case.Q(), device=0)
        else:
            Qs = [case.Q(k) for k in range(case.members)]
            be = gmrfx.MI355XBatchBackend(Qs[0], case.members, device=0)
            info = be.refactorize_values(np.asfortranarray(np.stack([Q.data for Q in Qs], axis=1)))
            assert not np.any(info)
        print(f"handle n={case.n} members={case.members}: built in {time.perf_counter() - t0:.2f} s")
        _HANDLES[key] = be
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for be in _HANDLES.values():
        be.close()
    _HANDLES.clear()


def _device(a):
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert d.data_ptr() % 16 == 0
    return d


def _correct_dev(be, Y, pad, off):
    """constraint_correct_dev on the window (leading dimension n + pad, offset off doubles) of a NaN-filled buffer"""
    n, k = Y.shape
    buf = _device(lb.input_buffer(Y, n + pad, off))
    torch.cuda.synchronize()
    be.constraint_correct_dev(buf.data_ptr() + 8 * off, n + pad, k)
    win, rest = lb.split(buf.cpu().numpy(), n, k, n + pad, off)
    assert np.isnan(rest).all(), "written outside the window"
    return win


def _sample_dev(be, Z, mu, pad, off):
    n, k = Z.shape
    dz, dmu = _device(Z.T), (None if mu is None else _device(mu))
    buf = _device(np.full(lb.buffer_len(k, n + pad, off), np.nan))
    torch.cuda.synchronize()
    be.sample_dev(dz.data_ptr(), n, k, buf.data_ptr() + 8 * off, n + pad, 0 if mu is None else dmu.data_ptr())
    win, rest = lb.split(buf.cpu().numpy(), n, k, n + pad, off)
    assert np.isnan(rest).all(), "written outside the window"
    return win


class _Worst(dict):
    def add(self, key, value):
        self[key] = max(self.get(key, 0.0), value)

    def report(self, case, extra=""):
        print(f"{case.name}: {extra}error/bound " + " ".join(f"{k} {v:.3g}" for k, v in sorted(self.items())))
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, (case.name, bad)


def _columns(worst, c, A, e, tag, got, X, mu=None):
    """every entry of a corrected block against the restatement on the same input, and its residual"""
    ref = cr.correct(c, X, mu)
    worst.add(tag, cr.ratio(got, ref["Xc"], cr.bound_X(c, ref)))
    if c["m"]:
        worst.add("residual", cr.residual_ratio(A, e, got))


def _plain(case):
    be = _handle(case)
    A, e = case.A_e()
    n, m = case.n, case.m
    layouts = ce.LAYOUTS if case.group == "pairs" else DEFAULT_LAYOUTS
    worst = _Worst()
    if m:
        be.set_constraints(A, e)
        At, W = be.constraint_fields()
        info = be.constraint_info()
        assert info["m"] == m
        assert same_bits(At, be.backend_solve(A.T.toarray()).reshape(n, m)), "A~' is not the blocked solve of the dense A'"
        assert same_bits(be.constraint_fields()[1], W)
    else:
        be.clear_constraints()
        At = np.zeros((n, 0))
    c = cr.prepare(A, e, At, LD)
    if m:
        worst.add("W", cr.ratio(W, c["W"], cr.bound_W(c)))
        worst.add("logdet", cr.ratio(info["logdet_W"], c["logdet"], cr.bound_logdet(c)))
        sigma = be.get_selinv_diag().copy()
        var = be.constrained_var()
        v = cr.variance(c, sigma)
        worst.add("var", cr.ratio(var, v["var"], cr.bound_var(c, v), nonnegative=True))
        assert same_bits(be.constrained_var(), var)
    for nvec in case.nvecs:
        Y, Z, mu = case.operands(nvec)
        X0 = be.backend_backward_solve(Z).reshape(n, nvec)
        Xc = be.constraint_correct(Y)
        Xs, Xm = be.sample(Z), be.sample(Z, mean=mu)
        _columns(worst, c, A, e, "correct", Xc, Y)
        _columns(worst, c, A, e, "sample", Xs, X0)
        _columns(worst, c, A, e, "sample_mu", Xm, X0, mu)
        for lay, (pad, off) in layouts.items():
            assert same_bits(_correct_dev(be, Y, pad, off), Xc), (case.name, nvec, lay, "constraint_correct_dev")
            assert same_bits(_sample_dev(be, Z, None, pad, off), Xs), (case.name, nvec, lay, "sample_dev")
            assert same_bits(_sample_dev(be, Z, mu, pad, off), Xm), (case.name, nvec, lay, "sample_dev with a mean")
        assert same_bits(be.constraint_correct(Y), Xc) and same_bits(be.sample(Z, mean=mu), Xm)          # run to run
    mc, _ = be.constrained_mean(mu)
    _columns(worst, c, A, e, "mean", mc.reshape(n, 1), mu.reshape(n, 1))
    worst.report(case, f"kappa {c['kappa']:.3g} " if m else "")
    return be, A, e, c


PLAIN = [c.name for c in ce.cases() if c.members == 1]
BATCHED = [c.name for c in ce.cases() if c.members > 1]


@pytest.mark.parametrize("name", PLAIN)
def test_plain_handle_entry_by_entry(name):
    _plain(ce.CASES[name])


def test_staged_rows_give_the_bits_of_the_sorted_row():
    """unsorted columns and duplicates with an exact sum through set_constraints_csr: the fields, the correction and the variance of
    the sorted, summed row, bit for bit"""
    case = ce.CASES["pairs"]
    be, A, e, c = _plain(case)
    Y, Z, mu = case.operands(3)

    def everything():
        At, W = be.constraint_fields()
        return [At, W, np.array([be.constraint_info()["logdet_W"]]), be.constraint_correct(Y), be.sample(Z, mean=mu), be.constrained_var()]

    want = everything()
    for name, rp, ci, va in ce.staged_forms(A):
        be.set_constraints_csr(case.m, rp, ci, va, e)
        for a, b in zip(everything(), want):
            assert same_bits(a, b), name


@pytest.mark.parametrize("name", BATCHED)
def test_batched_handle_per_member(name):
    case = ce.CASES[name]
    bb = _handle(case)
    A, e = case.A_e()
    n, m, nb = case.n, case.m, case.members
    bb.set_constraints(A, e)
    info = bb.constraint_info()
    assert info["m"] == m and np.array_equal(info["cinfo"], np.zeros(nb))
    sigma = bb.selinv_diag().copy()
    var = bb.constrained_var()
    assert same_bits(bb.constrained_var(), var)
    (nvec,) = case.nvecs
    Y, Z, mu = case.operands(nvec)
    Yb = np.stack([Y + 0.25 * k for k in range(nb)], axis=-1)
    Zb = np.stack([np.roll(Z, k, axis=0) for k in range(nb)], axis=-1)
    mub = np.stack([mu + 0.125 * k for k in range(nb)], axis=-1)
    X0 = bb.backward_solve(Zb)
    Xc, Xs, Xm = bb.constraint_correct(Yb), bb.sample(Zb), bb.sample(Zb, mean=mub)
    mc, _ = bb.constrained_mean(mub)
    worst = _Worst()
    kap = 0.0
    for k in range(nb):
        At, W = bb.constraint_fields(k)
        c = cr.prepare(A, e, At, LD)
        kap = max(kap, c["kappa"])
        worst.add("W", cr.ratio(W, c["W"], cr.bound_W(c)))
        worst.add("logdet", cr.ratio(info["logdet_W"][k], c["logdet"], cr.bound_logdet(c)))
        v = cr.variance(c, sigma[:, k])
        worst.add("var", cr.ratio(var[:, k], v["var"], cr.bound_var(c, v), nonnegative=True))
        _columns(worst, c, A, e, "correct", Xc[:, :, k], Yb[:, :, k])
        _columns(worst, c, A, e, "sample", Xs[:, :, k], X0[:, :, k])
        _columns(worst, c, A, e, "sample_mu", Xm[:, :, k], X0[:, :, k], mub[:, k])
        _columns(worst, c, A, e, "mean", mc[:, k].reshape(n, 1), mub[:, k].reshape(n, 1))
    # device-pointer forms on padded, offset member blocks of NaN-filled buffers = the host forms, bit for bit
    ldx, off = n + 3, 1
    sx = ldx * nvec + 5
    idx = off + np.arange(n)[:, None, None] + ldx * np.arange(nvec)[None, :, None] + sx * np.arange(nb)[None, None, :]
    host = np.full(off + sx * nb + ldx, np.nan)
    host[idx] = Yb
    buf = _device(host)
    torch.cuda.synchronize()
    bb.constraint_correct_dev(buf.data_ptr() + 8 * off, ldx, sx, nvec)
    out = buf.cpu().numpy()
    rest = np.ones(out.shape, bool)
    rest[idx] = False
    assert same_bits(out[idx], Xc) and np.isnan(out[rest]).all()
    dz, dmu = _device(np.transpose(Zb, (2, 1, 0))), _device(mub.T)
    buf = _device(np.full(off + sx * nb + ldx, np.nan))
    torch.cuda.synchronize()
    bb.sample_dev(dz.data_ptr(), n, n * nvec, nvec, buf.data_ptr() + 8 * off, ldx, sx, dmu.data_ptr())
    out = buf.cpu().numpy()
    assert same_bits(out[idx], Xm) and np.isnan(out[rest]).all()
    assert same_bits(bb.constraint_correct(Yb), Xc) and same_bits(bb.sample(Zb, mean=mub), Xm)          # run to run
    worst.report(case, f"kappa {kap:.3g} ")
