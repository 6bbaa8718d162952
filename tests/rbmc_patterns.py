"""Pattern builders for the RBMC edge tests (tests/test_rbmc_host.py pins the plans, tests/test_gpu_rbmc_edges.py and
tests/test_gpu_scaling.py run them on the device). Every matrix is strictly diagonally dominant with a positive diagonal, hence
positive definite and well conditioned, stores both triangles with sorted rows, and has n <= 1500, so the dense restatement of
tests/rbmc_ref.py applies unchanged. The patterns put the blocks of BlockRBMCStrategy on the edges of csrc/rbmc.hip: the size
classes of k_rbmc_block (<= 32 / 64 / 128 / 512 rows), subsets of more than 64 rows (a second pass of unit vectors), more
blocks of a class than one launch takes (rbmc_class_chunk: 128 of the <= 512 class, 1024 of the <= 128 class), a node held by
every subset, and n below one tile."""
import numpy as np
import scipy.sparse as sp

CLIQUE_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 512]
TRIDIAG_SIZES = [1, 2, 3, 5, 63, 64, 65]
CLASS_CHUNK = {2: 1024, 3: 128}        # blocks per launch of the two classes with global scratch (csrc/kernels.h: rbmc_class_chunk)


def _csc(Q):
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    return Q


def cliques():
    """block-diagonal, one dense block ones(s, s) + s I per s of CLIQUE_SIZES (n = 1187): with enclosure_size 0 or 1 one block per
    clique, ns = nb = s"""
    return _csc(sp.block_diag([np.ones((s, s)) + s * np.eye(s) for s in CLIQUE_SIZES]))


def clique_rows(s):
    """the rows of the s-clique"""
    at = int(np.sum(CLIQUE_SIZES[:CLIQUE_SIZES.index(s)]))
    return np.arange(at, at + s)


def banded(n, p):
    """all diagonals -p .. p: -1 / (1 + |offset|) off the diagonal, 2 p + 1 on it"""
    offs = [o for o in range(-p, p + 1) if abs(o) < n]
    return _csc(sp.diags([np.full(n - abs(o), 2.0 * p + 1.0 if o == 0 else -1.0 / (1 + abs(o))) for o in offs], offs, format="csc"))


def tridiag(n):
    return banded(n, 1)


def star(leaves, hub_last):
    """one hub joined to `leaves` leaves: 2 (leaves + 1) on the diagonal, -1 on the edges; the hub is the last node or the first"""
    n = leaves + 1
    hub = n - 1 if hub_last else 0
    leaf = np.array([i for i in range(n) if i != hub])
    rows = np.r_[np.arange(n), leaf, np.full(leaves, hub)]
    cols = np.r_[np.arange(n), np.full(leaves, hub), leaf]
    vals = np.r_[np.full(n, 2.0 * n), np.full(2 * leaves, -1.0)]
    return _csc(sp.coo_matrix((vals, (rows, cols)), shape=(n, n)))


def star_forest(m, leaves):
    """m disjoint star(leaves, hub_last=True) components"""
    return _csc(sp.block_diag([star(leaves, True)] * m))


def rbmc_class(rows):
    return 0 if rows <= 32 else (1 if rows <= 64 else (2 if rows <= 128 else 3))


def plan_sizes(plan):
    """[(ns, nb)] of a plan (MI355XBackend.rbmc_plan) or of rbmc_ref.build_blocks' list"""
    if isinstance(plan, dict):
        return [(int(s), int(b)) for s, b in zip(plan["n_interior"], np.diff(plan["block_ptr"]))]
    return [(len(S), len(S) + len(E)) for S, E in plan]


def class_counts(sizes):
    out = [0, 0, 0, 0]
    for _, nb in sizes:
        out[rbmc_class(nb)] += 1
    return out


class Edge:
    """one pattern with, per enclosure size the device tests run, what its plan must contain: `sizes` {(ns, nb): count} (count
    None: at least one), `exact` (the plan holds nothing else), `classes` {size class: number of blocks}"""

    def __init__(self, name, build, plans, ks=(65,)):
        self.name, self.build, self.plans, self.ks = name, build, plans, tuple(ks)


def _p(sizes, classes=None, exact=False):
    return dict(sizes=sizes, classes=classes or {}, exact=exact)


_CL = _p({(s, s): 1 for s in CLIQUE_SIZES}, {0: 4, 1: 3, 2: 3, 3: 2}, exact=True)

EDGES = [
    Edge("cliques", cliques, {0: _CL, 1: _CL}, ks=(3, 65)),
    Edge("banded200_16", lambda: banded(200, 16), {1: _p({(33, 65): 8, (17, 33): 1}, {1: 4, 2: 8, 3: 0})}),
    Edge("banded400_32", lambda: banded(400, 32), {1: _p({(65, 129): 9, (33, 65): 1}, {2: 4, 3: 9})}),
    Edge("banded300_31", lambda: banded(300, 31), {0: _p({(32, 32): 1, (63, 63): 8}, {0: 1, 1: 9, 3: 0})}),
    Edge("banded300_63", lambda: banded(300, 63), {0: _p({(64, 64): 1, (127, 127): 3}, {1: 1, 2: 4, 3: 0})}),
    Edge("banded1200_85", lambda: banded(1200, 85), {2: _p({(171, 511): 8, (86, 256): None}, {3: 14})}, ks=(3, 65)),
    Edge("star200_hub_last", lambda: star(200, True), {0: _p({(2, 2): 200}, {0: 200}, exact=True),
                                                       1: _p({(2, 201): 200}, {3: 200}, exact=True)}),
    Edge("star200_hub_first", lambda: star(200, False), {0: _p({(201, 201): 1}, {3: 1}, exact=True)}),
    Edge("star_forest11x100", lambda: star_forest(11, 100), {1: _p({(2, 101): 1100}, {2: 1100}, exact=True)}),
    # a chain: node 0 opens {0, 1}, every later subset is {i - 1, i, i + 1} or, at the end, {n - 2, n - 1}
    Edge("tridiag1", lambda: tridiag(1), {0: _p({(1, 1): 1}, exact=True), 1: _p({(1, 1): 1}, exact=True)}, ks=(3, 65)),
    Edge("tridiag2", lambda: tridiag(2), {0: _p({(2, 2): 1}, exact=True), 1: _p({(2, 2): 1}, exact=True)}, ks=(3, 65)),
    Edge("tridiag3", lambda: tridiag(3), {0: _p({(2, 2): 2}, exact=True), 1: _p({(2, 3): 2}, exact=True)}, ks=(3, 65)),
    Edge("tridiag5", lambda: tridiag(5), {0: _p({(2, 2): 2, (3, 3): 1}, exact=True), 1: _p({(2, 3): 2, (3, 5): 1}, exact=True)}, ks=(3, 65)),
    Edge("tridiag63", lambda: tridiag(63), {0: _p({(2, 2): 2, (3, 3): 30}, exact=True), 1: _p({(3, 5): None})}, ks=(3, 65)),
    Edge("tridiag64", lambda: tridiag(64), {0: _p({(2, 2): 1, (3, 3): 31}, exact=True), 1: _p({(3, 5): None})}, ks=(3, 65)),
    Edge("tridiag65", lambda: tridiag(65), {0: _p({(2, 2): 2, (3, 3): 31}, exact=True), 1: _p({(3, 5): None})}, ks=(3, 65)),
]
EDGE = {e.name: e for e in EDGES}


def check_sizes(sizes, want):
    """the (ns, nb) list of a plan against one entry of Edge.plans"""
    have = {}
    for s in sizes:
        have[s] = have.get(s, 0) + 1
    for pair, cnt in want["sizes"].items():
        assert pair in have, (pair, sorted(have))
        if cnt is not None:
            assert have[pair] == cnt, (pair, have[pair], cnt)
    if want["exact"]:
        assert set(have) == set(want["sizes"]), sorted(have)
    cc = class_counts(sizes)
    for cls, cnt in want["classes"].items():
        assert cc[cls] == cnt, (cls, cc)
