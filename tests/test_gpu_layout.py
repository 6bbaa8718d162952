"""The plain handle's device-pointer calls on strided, offset right-hand sides (include/gmrfx.h, "Layout of B, X and Z").

Every _dev entry point takes a leading dimension and promises a column-major n x nrhs window at ptr + j ld; the Julia extension
passes stride(B, 2) of a view straight through, so ld > n and a base pointer that is only 8-byte aligned are what a caller sends.
Here every such call is made on a window inside a larger buffer (layout_buffers.py: NaN around an input, a sentinel around an
output) and must

  * give, bit for bit, what the same handle gives for a contiguous call on fresh arrays,
  * leave every element outside the output window, the whole input buffer and the device array of values as they were,
  * and the contiguous result itself must match a dense float64 reference (numpy on Q.toarray()) to the tolerances of
    test_gpu_parity.py: 1e-10 relative for solves, 1e-11 for quadratic forms.

The problems are the smallest at which the caller-side kernels (k_permute: 64 rows per workgroup, passes of more than 8 columns;
k_permute_narrow: 256 rows, at most 8 columns) have a partial block, a block of one row, or only full blocks; the right-hand-side
counts put passes of both kinds on both lanes. The default ordering is used, so the permutation is not the identity."""
import itertools
import zlib

import numpy as np
import pytest

import gmrfx
from gmrfx._lib import lib
from layout_buffers import (LAYOUTS, NRHS, NVEC, PROBLEM_REMAINDERS, SENTINEL, X_LAYOUTS, diag_positions, input_buffer, output_buffer,
                            problems, same_bits, split)

pytestmark = pytest.mark.gpu

PROBLEMS = tuple(PROBLEM_REMAINDERS)
SOLVES = ("solve_dev", "backward_solve_dev", "refactorize_solve_dev", "refactorize_update_solve_dev")
QUADS = ("quadform_dev", "refactorize_logpdf_dev")
ALIAS_NRHS = (1, 9, 65, 129)
SCALE = {"1": 1.0, "a": 1.5, "b": 0.7}


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class Problem:
    """One problem: its handle (factorised once, here, on its own stream), a second handle for the separate-calls comparison, the
    value sets on the device with their host copies, and the dense references (computed once, never changed)."""

    def __init__(self, name, Q):
        import torch
        self.name, self.Q, self.n = name, Q, Q.shape[0]
        n = self.n
        assert (n, n % 64, n % 256) == PROBLEM_REMAINDERS[name], f"{name}: n = {n} does not leave the remainders the problem is there for"
        self.be = gmrfx.MI355XBackend(Q)
        self.be2 = gmrfx.MI355XBackend(Q, factorize=False)
        assert self.be.last_info == 0
        self.perm = self.be.ordering_permutation()
        assert n == 1 or not np.array_equal(self.perm, np.arange(n)), "the default ordering is the identity: the permutation is not tested"
        self.Qd = Q.toarray()
        self.dpos = diag_positions(Q)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.B = rng.standard_normal((n, max(NRHS)))
        self.mu = rng.standard_normal(n)
        # value sets: "1" Q itself, "a" / "b" two rescalings (refactorising calls alternate between them: new values on every call),
        # "ha" / "hb" two diagonal Hessians H of the Newton step Q = Q_prior - H (negative: Q stays positive definite)
        self.hvals = {k: -(0.1 + rng.random(n)) * f * Q.diagonal() for k, f in (("ha", 1.0), ("hb", 3.0))}
        self.qvals = {k: np.ascontiguousarray(Q.data * s) for k, s in SCALE.items()}
        for k, h in self.hvals.items():
            v = Q.data.copy()
            v[self.dpos] -= h
            self.qvals[k] = v
        self.h_vals = {**{k: self.qvals[k] for k in SCALE}, **self.hvals}      # what the calls are handed: Q's values, or H's
        self.d_vals = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.h_vals.items()}
        torch.cuda.synchronize()
        self._dense, self._ref = {}, {}
        self._prior_set = False

    def close(self):
        self.be.close()
        self.be2.close()

    # ---- dense float64 references ---------------------------------------------------------------------------------------------
    def dense(self, key):
        if key not in self._dense:
            D = self.Qd * SCALE[key] if key in SCALE else self.Qd - np.diag(self.hvals[key])
            D.setflags(write=False)
            self._dense[key] = D
        return self._dense[key]

    def ref(self, what, key):
        """the reference for all max(NRHS) columns of self.B: "solve": Q^-1 B, "backward": P' L^-T B"""
        if (what, key) not in self._ref:
            D, n, p = self.dense(key), self.n, self.perm
            if n == 1:
                R = self.B / D[0, 0] if what == "solve" else self.B / np.sqrt(D[0, 0])
            elif what == "solve":
                R = np.linalg.solve(D, self.B)
            else:
                L = np.linalg.cholesky(D[np.ix_(p, p)])
                R = np.empty_like(self.B)
                R[p] = np.linalg.solve(L.T, self.B)
            R.setflags(write=False)
            self._ref[(what, key)] = R
        return self._ref[(what, key)]

    # ---- the entry points ------------------------------------------------------------------------------------------------------
    def keys(self, entry):
        return {"solve_dev": ("1",), "backward_solve_dev": ("1",), "refactorize_solve_dev": ("a", "b"),
                "refactorize_update_solve_dev": ("ha", "hb"), "quadform_dev": ("a", "b"), "refactorize_logpdf_dev": ("a", "b")}[entry]

    def prepare(self, entry):
        """the handle is shared by the tests of a problem: put it into the state the entry point starts from"""
        if entry in ("solve_dev", "backward_solve_dev"):
            assert self.be.refactorize_dev(self.d_vals["1"].data_ptr()) == 0
        if entry == "refactorize_update_solve_dev" and not self._prior_set:
            self.be.set_prior(self.Q.data, self.dpos)
            self._prior_set = True

    def call(self, entry, key, pB, ldb, r, pX, ldx):
        be, v = self.be, self.d_vals[key].data_ptr()
        if entry == "solve_dev":
            be.solve_dev(pB, ldb, r, pX, ldx)
        elif entry == "backward_solve_dev":
            be.backward_solve_dev(pB, ldb, r, pX, ldx)
        elif entry == "refactorize_solve_dev":
            assert be.refactorize_solve_dev(v, pB, ldb, r, pX, ldx) == 0
        else:
            assert be.refactorize_update_solve_dev(v, pB, ldb, r, pX, ldx) == 0

    def run(self, entry, key, W, lay, msg, alias=False):
        """one call on the window W (n, r) laid out as lay = (ldb - n, ldx - n, offset of B, offset of X); with alias the output IS
        the input buffer. Checks everything outside the output window, the input and the values; returns the output window."""
        import torch
        n, r = W.shape
        ldb, ldx, ob, ox = n + lay[0], n + lay[1], lay[2], lay[3]
        hb = input_buffer(W, ldb, ob)
        d_B = torch.from_numpy(hb.copy()).cuda()
        if alias:
            assert (ldb, ob) == (ldx, ox)
            hx0, d_X = hb, d_B
        else:
            hx0 = output_buffer(r, ldx, ox)
            d_X = torch.from_numpy(hx0.copy()).cuda()
        torch.cuda.synchronize()
        assert d_B.data_ptr() % 16 == 0 and d_X.data_ptr() % 16 == 0      # the offsets decide the alignment
        self.call(entry, key, d_B.data_ptr() + 8 * ob, ldb, r, d_X.data_ptr() + 8 * ox, ldx)
        torch.cuda.synchronize()
        X, rest = split(d_X.cpu().numpy(), n, r, ldx, ox)
        assert same_bits(rest, split(hx0, n, r, ldx, ox)[1]), f"{msg}: wrote outside the n x nrhs window of X"
        if not alias:
            assert same_bits(d_B.cpu().numpy(), hb), f"{msg}: the input buffer changed"
        assert same_bits(self.d_vals[key].cpu().numpy(), self.h_vals[key]), f"{msg}: the device array of values changed"
        return X

    def separate(self, key, W):
        """the same step as two calls on the second handle: gmrfx_refactorize_dev + gmrfx_solve_dev, contiguous"""
        import torch
        n, r = W.shape
        d_nz = torch.from_numpy(self.qvals[key].copy()).cuda()
        d_B = torch.from_numpy(np.ascontiguousarray(W.T)).cuda()
        d_X = torch.zeros_like(d_B)
        torch.cuda.synchronize()
        assert self.be2.refactorize_dev(d_nz.data_ptr()) == 0
        self.be2.solve_dev(d_B.data_ptr(), n, r, d_X.data_ptr(), n)
        torch.cuda.synchronize()
        return d_X.cpu().numpy().T


@pytest.fixture(scope="module")
def probs():
    made, Qs = {}, problems()

    def get(name):
        if name not in made:
            made[name] = Problem(name, Qs[name])
        return made[name]

    yield get
    for P in made.values():
        P.close()


def test_problem_sizes_leave_the_stated_remainders():
    for name, Q in problems().items():
        n = Q.shape[0]
        assert (n, n % 64, n % 256) == PROBLEM_REMAINDERS[name], name


@pytest.mark.parametrize("entry", SOLVES)
@pytest.mark.parametrize("pname", PROBLEMS)
def test_dev_solves_on_strided_offset_arrays(probs, pname, entry):
    P = probs(pname)
    P.prepare(entry)
    keys = P.keys(entry)
    what = "backward" if entry == "backward_solve_dev" else "solve"
    pipelined = entry in ("refactorize_solve_dev", "refactorize_update_solve_dev")
    for r in NRHS:
        W = P.B[:, :r]
        ref = {}
        for k in keys:
            msg = f"{pname} {entry} nrhs={r} contiguous reference, values {k}"
            ref[k] = P.run(entry, k, W, LAYOUTS["contig"], msg)
            err = relerr(ref[k], P.ref(what, k)[:, :r])
            assert err < 1e-10, f"{msg}: {err:.3e} from the dense reference"
            if pipelined:
                # WHICH BRANCH RAN. Device::refactorize_solve takes the plain sequence (refactorize, then solve) only for nrhs <= 0,
                # on a caller's stream, or while the handle's inverse cap is undecided; the handle's statistics do not tell the two
                # branches apart. Here nrhs > 0, no stream was ever handed to the handle, and the cap was decided by the successful
                # factorisation in Problem.__init__ (decide_inverse_cap runs behind every factorisation and sticks after the first
                # one without a failed pivot): every call of this test takes the pipelined branch. The second handle makes the
                # separate calls, and the header promises their bits.
                assert same_bits(ref[k], P.separate(k, W)), f"{msg}: differs from gmrfx_refactorize_dev + gmrfx_solve_dev on a second handle"
        for i, (lname, lay) in enumerate(LAYOUTS.items()):
            k = keys[i % len(keys)]                                 # (refactorising entries: never the values of the call before)
            msg = f"{pname} {entry} nrhs={r} layout={lname}"
            X = P.run(entry, k, W, lay, msg)
            assert same_bits(X, ref[k]), f"{msg}: differs from the contiguous call by {relerr(X, ref[k]):.3e}"
        if r in ALIAS_NRHS:
            # d_X == d_B with equal leading dimensions: every pass reads its own columns before it writes them
            for i, (pad, off) in enumerate(((0, 0), (3, 1))):
                k = keys[i % len(keys)]
                msg = f"{pname} {entry} nrhs={r} in place, ld=n+{pad} offset={off}"
                X = P.run(entry, k, W, (pad, pad, off, off), msg, alias=True)
                assert same_bits(X, ref[k]), f"{msg}: differs from the out-of-place call by {relerr(X, ref[k]):.3e}"


@pytest.mark.parametrize("entry", SOLVES)
@pytest.mark.parametrize("pname", PROBLEMS)
def test_dev_solves_argument_contract(probs, pname, entry):
    """ld < n and null arrays are refused with GMRFX_ERR_INVALID_ARG (ValueError here) before anything is touched, nrhs = 0 is a
    successful no-op on B and X, and the handle goes on giving the contiguous bits after each of them."""
    import torch
    P = probs(pname)
    P.prepare(entry)
    keys = P.keys(entry)
    n, r = P.n, 3
    W = P.B[:, :r]
    ref = {k: P.run(entry, k, W, LAYOUTS["contig"], f"{pname} {entry} reference, values {k}") for k in keys}
    hb, hx = input_buffer(W, n + 1, 0), output_buffer(r, n + 1, 0)
    bad = {"ldb < n": dict(ldb=n - 1), "ldx < n": dict(ldx=n - 1), "null B": dict(pB=0), "null X": dict(pX=0), "nrhs = 0": dict(r=0),
           "nrhs = 0, null arrays": dict(r=0, pB=0, pX=0)}
    for i, (bname, change) in enumerate(bad.items()):
        msg = f"{pname} {entry} {bname}"
        d_B, d_X = torch.from_numpy(hb.copy()).cuda(), torch.from_numpy(hx.copy()).cuda()
        torch.cuda.synchronize()
        args = dict(pB=d_B.data_ptr(), ldb=n + 1, r=r, pX=d_X.data_ptr(), ldx=n + 1)
        args.update(change)
        k = keys[i % len(keys)]
        if args["r"] == 0:
            P.call(entry, k, **args)
        else:
            with pytest.raises(ValueError):
                P.call(entry, k, **args)
        torch.cuda.synchronize()
        assert np.all(d_X.cpu().numpy() == SENTINEL), f"{msg}: X was written"
        assert same_bits(d_B.cpu().numpy(), hb), f"{msg}: B was written"
        k = keys[(i + 1) % len(keys)]
        X = P.run(entry, k, W, LAYOUTS["odd_base"], f"{msg}, then a good call")
        assert same_bits(X, ref[k]), f"{msg}: the next good call differs from the contiguous one"


# ---- quadratic forms ---------------------------------------------------------------------------------------------------------------

def _quad_call(P, entry, key, W, xlay, mu_off, msg, args=None):
    """(x_v - mu)' Q (x_v - mu) for the columns of W (n, nvec) laid out as xlay = (ldx - n, offset); mu absent (None) or at an
    offset in doubles. Returns every scalar of the call: the quadratic forms, and for refactorize_logpdf_dev log det Q behind them.
    X, mu and the values must come back bit-identical."""
    import torch
    n, nvec = W.shape
    ldx, ox = n + xlay[0], xlay[1]
    hx = input_buffer(W, ldx, ox)
    d_X = torch.from_numpy(hx.copy()).cuda()
    hm = None if mu_off is None else input_buffer(P.mu[:, None], n, mu_off)
    d_mu = None if hm is None else torch.from_numpy(hm.copy()).cuda()
    torch.cuda.synchronize()
    assert d_X.data_ptr() % 16 == 0 and (d_mu is None or d_mu.data_ptr() % 16 == 0)
    a = dict(pX=d_X.data_ptr() + 8 * ox, ldx=ldx, nvec=nvec, pmu=0 if d_mu is None else d_mu.data_ptr() + 8 * mu_off)
    a.update(args or {})
    v = P.d_vals[key].data_ptr()
    if entry == "quadform_dev":
        out = P.be.quadform_dev(v, a["pX"], a["ldx"], a["nvec"], a["pmu"])
    else:
        quad, logdet = P.be.refactorize_logpdf_dev(v, a["pX"], a["ldx"], a["nvec"], a["pmu"])
        assert P.be.last_info == 0
        out = np.append(quad, logdet)
    torch.cuda.synchronize()
    assert same_bits(d_X.cpu().numpy(), hx), f"{msg}: X changed"
    assert d_mu is None or same_bits(d_mu.cpu().numpy(), hm), f"{msg}: mu changed"
    assert same_bits(P.d_vals[key].cpu().numpy(), P.h_vals[key]), f"{msg}: the device array of values changed"
    return out


@pytest.mark.parametrize("entry", QUADS)
@pytest.mark.parametrize("pname", PROBLEMS)
def test_dev_quadratic_forms_on_strided_offset_arrays(probs, pname, entry):
    P = probs(pname)
    keys = P.keys(entry)
    n = P.n
    refs = {}
    for nvec in NVEC:
        W = P.B[:, :nvec]
        ref = refs[nvec] = {}
        for mm, k in itertools.product((None, 0), keys):           # (values alternate from call to call)
            msg = f"{pname} {entry} nvec={nvec} contiguous reference, values {k}, mu {'absent' if mm is None else 'aligned'}"
            ref[k, mm] = got = _quad_call(P, entry, k, W, X_LAYOUTS["contig"], mm, msg)
            D = P.dense(k)
            R = W if mm is None else W - P.mu[:, None]
            for v in range(nvec):
                want = D[0, 0] * R[0, v] * R[0, v] if n == 1 else R[:, v] @ (D @ R[:, v])
                assert abs(got[v] - want) <= 1e-11 * max(1.0, abs(want)), f"{msg}: vector {v}: {got[v]!r} against {want!r}"
            if entry == "refactorize_logpdf_dev":
                want = np.log(D[0, 0]) if n == 1 else np.linalg.slogdet(D)[1]
                assert abs(got[nvec] - want) <= 1e-10 * max(1.0, abs(want)), f"{msg}: log det {got[nvec]!r} against {want!r}"
        for i, ((lname, xlay), mm) in enumerate(itertools.product(X_LAYOUTS.items(), (None, 0, 1))):
            k = keys[i % len(keys)]
            msg = f"{pname} {entry} nvec={nvec} layout={lname} mu={'absent' if mm is None else f'offset {mm}'}"
            got = _quad_call(P, entry, k, W, xlay, mm, msg)
            assert same_bits(got, ref[k, None if mm is None else 0]), f"{msg}: {got!r} differs from the contiguous call"
    # the argument contract
    W, ref = P.B[:, :3], refs[3]
    for i, (bname, change) in enumerate({"ldx < n": dict(ldx=n - 1), "null X": dict(pX=0)}.items()):
        msg = f"{pname} {entry} {bname}"
        with pytest.raises(ValueError):
            _quad_call(P, entry, keys[i % 2], W, X_LAYOUTS["contig"], None, msg, args=change)
        k = keys[(i + 1) % 2]
        got = _quad_call(P, entry, k, W, X_LAYOUTS["odd_base"], 1, f"{msg}, then a good call")
        assert same_bits(got, ref[k, 0]), f"{msg}: the next good call differs from the contiguous one"
    got = _quad_call(P, entry, keys[0], W, X_LAYOUTS["contig"], None, f"{pname} {entry} nvec = 0", args=dict(nvec=0))
    assert len(got) == (0 if entry == "quadform_dev" else 1)


# ---- the host forms with ld > n: the strided-copy branches of Device::solve and of gmrfx_quadform's staging --------------------------

HOST_NRHS = (1, 9, 65)


def _host_solve(P, name, W, lay, msg):
    n, r = W.shape
    ldb, ldx, ob, ox = n + lay[0], n + lay[1], lay[2], lay[3]
    hb, hx = input_buffer(W, ldb, ob), output_buffer(r, ldx, ox)
    hb0 = hb.copy()
    code = getattr(lib(), name)(P.be._h, hb.ctypes.data + 8 * ob, ldb, r, hx.ctypes.data + 8 * ox, ldx)
    assert code == 0, f"{msg}: error {code}"
    X, rest = split(hx, n, r, ldx, ox)
    assert np.all(rest == SENTINEL), f"{msg}: wrote outside the n x nrhs window of X"
    assert same_bits(hb, hb0), f"{msg}: the input buffer changed"
    return X


@pytest.mark.parametrize("name", ("gmrfx_solve", "gmrfx_backward_solve"))
def test_host_solves_with_padded_leading_dimensions(probs, name):
    P = probs("matern513")
    P.prepare("solve_dev")
    what = "backward" if name == "gmrfx_backward_solve" else "solve"
    for r in HOST_NRHS:
        W = P.B[:, :r]
        msg = f"matern513 {name} nrhs={r}"
        ref = _host_solve(P, name, W, LAYOUTS["contig"], f"{msg} contiguous reference")
        err = relerr(ref, P.ref(what, "1")[:, :r])
        assert err < 1e-10, f"{msg}: {err:.3e} from the dense reference"
        dev = P.run(name[len("gmrfx_"):] + "_dev", "1", W, LAYOUTS["contig"], f"{msg} device form")
        assert same_bits(ref, dev), f"{msg}: the host and the device form differ"
        for lname, lay in LAYOUTS.items():
            X = _host_solve(P, name, W, lay, f"{msg} layout={lname}")
            assert same_bits(X, ref), f"{msg} layout={lname}: differs from the contiguous call by {relerr(X, ref):.3e}"


def test_host_quadform_with_padded_leading_dimension(probs):
    P = probs("matern513")
    n, nz = P.n, P.qvals["a"]
    D = P.dense("a")

    def call(W, xlay, mu_off, msg):
        nvec = W.shape[1]
        ldx, ox = n + xlay[0], xlay[1]
        hx = input_buffer(W, ldx, ox)
        hm = None if mu_off is None else input_buffer(P.mu[:, None], n, mu_off)
        hx0, hm0, nz0, out = hx.copy(), None if hm is None else hm.copy(), nz.copy(), np.empty(nvec)
        code = lib().gmrfx_quadform(P.be._h, nz.ctypes.data, hx.ctypes.data + 8 * ox, ldx, nvec,
                                    None if hm is None else hm.ctypes.data + 8 * mu_off, out.ctypes.data)
        assert code == 0, f"{msg}: error {code}"
        assert same_bits(hx, hx0) and (hm is None or same_bits(hm, hm0)) and same_bits(nz, nz0), f"{msg}: an input changed"
        return out

    for nvec in HOST_NRHS:
        W = P.B[:, :nvec]
        for mm in (None, 1):
            msg = f"matern513 gmrfx_quadform nvec={nvec} mu={'absent' if mm is None else 'offset 1'}"
            ref = call(W, X_LAYOUTS["contig"], None if mm is None else 0, f"{msg} contiguous reference")
            R = W if mm is None else W - P.mu[:, None]
            want = np.einsum("iv,iv->v", R, D @ R)
            assert np.all(np.abs(ref - want) <= 1e-11 * np.maximum(1.0, np.abs(want))), f"{msg}: {ref!r} against {want!r}"
            for lname, xlay in X_LAYOUTS.items():
                got = call(W, xlay, mm, f"{msg} layout={lname}")
                assert same_bits(got, ref), f"{msg} layout={lname}: {got!r} differs from the contiguous call"
