"""The RBMC variance kernels (csrc/rbmc.hip) on the edges that tests/test_gpu_rbmc.py's one geometry never reaches, on the patterns
of tests/rbmc_patterns.py (tests/test_rbmc_host.py pins their plans): every size-class boundary of k_rbmc_block (32/33, 64/65,
128/129, 512 rows, a 1-row block), subsets of more than 64 rows (2, 3 and 8 passes of unit vectors), s0 > 0 at the boundaries, more
blocks of a class than one launch takes (b0 = 128 of the <= 512 class, b0 = 1024 of the <= 128 class), a hub held by 200 subsets,
n below one tile (1, 2, 3, 5, 63, 64, 65), the documented NaN path, the block form on a batched handle, a handle whose LOWER
triangle defines Q, and plan switching on one handle.

Comparison rule: the restatement (tests/rbmc_ref.py) is fed the samples X = backend_backward_solve(Z) of the same handle, and the
bound is PER ENTRY, |v_i - ref_i| <= 1e-8 |ref_i| (1e-8: the project's tolerance for marginal variances) -- the variances of
`cliques` span three orders of magnitude (about 1 / s), which a max-norm bound would not see. Every case prints its largest
per-entry ratio."""
import numpy as np
import pytest

import gmrfx
import rbmc_patterns as rp
import rbmc_ref

pytestmark = pytest.mark.gpu

TOL = 1e-8
KMAX = 65


class Model:
    """one pattern: its handle, the restatement's dense image, the samples and the per-enclosure block inverses, each built once"""

    def __init__(self, name):
        self.Q = rp.EDGE[name].build()
        self.n = self.Q.shape[0]
        self.be = gmrfx.MI355XBackend(self.Q, device=0)
        self.sq = rbmc_ref.SymQ(self.Q)
        self.Z = np.asfortranarray(np.random.default_rng(self.n).standard_normal((self.n, KMAX)))
        self._ops, self._X = {}, {}

    def ops(self, enc):
        if enc >= 0 and enc not in self._ops:
            self._ops[enc] = rbmc_ref.block_ops(self.sq, enc)
        return self._ops.get(enc)

    def X(self, k):
        if k not in self._X:
            self._X[k] = self.be.backend_backward_solve(self.Z[:, :k]).reshape(self.n, k)
        return self._X[k]


_MODELS = {}


@pytest.fixture(scope="module")
def models():
    def get(name):
        if name not in _MODELS:
            _MODELS[name] = Model(name)
        return _MODELS[name]
    yield get
    for m in _MODELS.values():
        m.be.close()
    _MODELS.clear()


def _entry_err(v, ref):
    assert (ref > 0).all()
    return (np.abs(v - ref) / np.abs(ref)).max()


CASES = [(e.name, enc, k) for e in rp.EDGES for enc in [-1] + sorted(e.plans) for k in e.ks]


@pytest.mark.parametrize("name,enclosure_size,k", CASES)
def test_edges_against_the_restatement(models, name, enclosure_size, k):
    """k = 65: two sample blocks (first != last, one Chan merge, w = 1 in the last); k = 3: one block (first = last)"""
    m = models(name)
    v = m.be.rbmc_var(m.Z[:, :k], enclosure_size)
    ref = rbmc_ref.rbmc_var(m.sq, m.X(k), enclosure_size, m.ops(enclosure_size))
    assert np.isfinite(v).all()
    err = _entry_err(v, ref)
    print(f"rbmc edges {name} enclosure={enclosure_size} k={k}: max_i |v_i - ref_i| / |ref_i| = {err:.3e} "
          f"(ms_rbmc {m.be.stats()['ms_rbmc']:.1f})")
    assert err <= TOL


@pytest.mark.parametrize("enclosure_size", [-1, 1])
def test_lower_triangle_defines_q(models, enclosure_size):
    """banded(400, 32) stored as both triangles, uplo = "L": 1e30 in the upper one changes no bit (the mirrored `pos` table of
    rbmc_build_sym on the device)"""
    m = models("banded400_32")
    Q, n = m.Q, m.n
    cols = np.repeat(np.arange(n), np.diff(Q.indptr))
    junk = Q.copy()
    junk.data = np.where(Q.indices < cols, 1e30, Q.data)
    assert (junk.data == 1e30).sum() == (Q.nnz - n) // 2
    Z = m.Z
    clean = gmrfx.MI355XBackend(Q, device=0, uplo="L")
    dirty = gmrfx.MI355XBackend(junk, device=0, uplo="L")
    v, w = clean.rbmc_var(Z, enclosure_size), dirty.rbmc_var(Z, enclosure_size)
    assert np.array_equal(v, w)
    assert np.array_equal(dirty.rbmc_var(Z, enclosure_size, nzval=junk.data), v)
    X = dirty.backend_backward_solve(Z)
    err = _entry_err(w, rbmc_ref.rbmc_var(rbmc_ref.SymQ(junk, "L"), X, enclosure_size))
    print(f"rbmc edges uplo=L banded400_32 enclosure={enclosure_size}: {err:.3e}")
    assert err <= TOL
    clean.close(); dirty.close()


def _diag_pos(Q, i):
    return Q.indptr[i] + int(np.searchsorted(Q.indices[Q.indptr[i]:Q.indptr[i + 1]], i))


@pytest.mark.parametrize("s", [33, 128, 129, 512])
@pytest.mark.parametrize("which", ["first", "last"])
def test_non_positive_pivot_makes_the_block_nan(models, s, which):
    """include/gmrfx.h: a non-positive pivot in a block turns that block's outputs into NaN. One diagonal entry of the s-clique is
    -1e3 in the values handed to rbmc_var (the factor of the true values stays): all s rows are NaN, every other row keeps its bits
    (no other block reads the entry), and the handle still gives the clean result afterwards. The clique's first node is its
    block's LAST pivot, so only the kernel's flag can turn the other rows into NaN; its last node is the first pivot."""
    m = models("cliques")
    Z = m.Z
    if not hasattr(m, "good"):
        m.good = m.be.rbmc_var(Z, 0)
    good = m.good
    rows = rp.clique_rows(s)
    node = int(rows[0] if which == "first" else rows[-1])
    bad = m.Q.data.copy()
    p = _diag_pos(m.Q, node)
    assert m.Q.indices[p] == node and bad[p] == s + 1.0            # ones(s, s) + s I
    bad[p] = -1e3
    v = m.be.rbmc_var(Z, 0, nzval=bad)
    assert np.isnan(v[rows]).all()
    others = np.setdiff1d(np.arange(m.n), rows)
    assert np.array_equal(v[others], good[others])
    assert np.array_equal(m.be.rbmc_var(Z, 0), good)


@pytest.mark.parametrize("enclosure_size", [0, 1])
def test_batched_handle_block_form(enclosure_size):
    Q = rp.banded(200, 16)
    n, B, k = Q.shape[0], 3, KMAX
    scales = (1.0, 2.0, 0.5)
    bb = gmrfx.MI355XBatchBackend(Q, B, device=0)
    NZ = np.stack([Q.data * s for s in scales], axis=1)
    assert not bb.refactorize_values(NZ).any()
    Z = np.random.default_rng(5).standard_normal((n * B, k))
    v = bb.rbmc_var(Z, enclosure_size)
    assert v.shape == (n, B)
    X = bb.backward_solve(Z.reshape(B, n, k).transpose(1, 2, 0))          # (n, k, B)
    for b, s in enumerate(scales):
        ref = rbmc_ref.block_var(rbmc_ref.SymQ(Q * s), np.ascontiguousarray(X[:, :, b]), enclosure_size)
        err = _entry_err(v[:, b], ref)
        print(f"rbmc edges batch member {b} banded200_16 enclosure={enclosure_size}: {err:.3e}")
        assert err <= TOL, b
    assert np.array_equal(bb.rbmc_var(Z, enclosure_size, nzval=NZ), v)
    bb.close()


def test_plan_switching_on_one_handle(models):
    """enclosure 1, 0, 1, -1, 1 on one handle: every repeat gives the bits of the first call of that enclosure (rbmc_upload_plan
    re-uploads tables and scratch of other sizes: banded(400, 32) has blocks of the <= 512 class with enclosure 1 and none with 0)"""
    m = models("banded400_32")
    be = gmrfx.MI355XBackend(m.Q, device=0)
    Z = m.Z
    seen = {}
    for enc in (1, 0, 1, -1, 1):
        v = be.rbmc_var(Z, enc)
        assert np.array_equal(seen.setdefault(enc, v), v), enc
    X = be.backend_backward_solve(Z)
    for enc, v in seen.items():
        assert _entry_err(v, rbmc_ref.rbmc_var(m.sq, X, enc, m.ops(enc))) <= TOL, enc
    be.close()
