"""numpy restatement of the reference's Rao-Blackwellised Monte Carlo variance estimators (src/solvers/rbmc.jl), the checker of
tests/test_rbmc_host.py and tests/test_gpu_rbmc.py: `_build_disjoint_subsets` (:106-117; despite the name the subsets overlap),
`_build_enclosure_idcs` (:93-104), `var(gmrf, ::RBMCStrategy)` (:71-87) and `var(gmrf, ::BlockRBMCStrategy)` (:124-158) with a dense
inverse per block, last subset wins, and the corrected sample variance `var(...; dims = 2)`. Q is Symmetric(Q, uplo): neighbours and
values come from the stored triangle that defines Q, mirrored -- explicit zeros are neighbours (what `findnz` returns)."""
import numpy as np
import scipy.sparse as sp


class SymQ:
    """Symmetric(Q, uplo) of a CSC matrix that may store one triangle or both: dense values + stored-neighbour lists."""

    def __init__(self, Q, uplo="U", nzval=None):
        Q = sp.csc_matrix(Q)
        n = Q.shape[0]
        cols = np.repeat(np.arange(n), np.diff(Q.indptr))
        rows = Q.indices
        vals = Q.data if nzval is None else np.asarray(nzval, dtype=np.float64)
        use = rows <= cols if uplo.upper().startswith("U") else rows >= cols
        self.n = n
        self.dense = np.zeros((n, n))
        self.dense[rows[use], cols[use]] = vals[use]
        self.dense[cols[use], rows[use]] = vals[use]
        nb = [set() for _ in range(n)]
        for i, j in zip(rows[use], cols[use]):
            nb[i].add(int(j))
            nb[j].add(int(i))
        self.nbrs = [sorted(s) for s in nb]


def build_blocks(sq, enclosure_size):
    """[(S, E)] in the order of the walk: S = stored neighbours of the first node no earlier subset has taken (ascending), E = the
    enclosure rings."""
    visited = np.zeros(sq.n, bool)
    out = []
    for i in range(sq.n):
        if visited[i]:
            continue
        S = list(sq.nbrs[i])
        visited[S] = True
        explored, new, E = set(S), list(S), []
        for _ in range(enclosure_size):
            nxt = set()
            for v in new:
                nxt.update(sq.nbrs[v])
            nxt -= explored
            E += sorted(nxt)
            explored |= nxt
            new = list(nxt)
        out.append((S, E))
    return out


def owner_masks(blocks, n):
    """per block: 1 for the rows of S this block is the LAST to contain"""
    last = np.full(n, -1)
    for b, (S, _) in enumerate(blocks):
        last[S] = b
    return [np.array([1 if last[v] == b else 0 for v in S]) for b, (S, _) in enumerate(blocks)], last


def plain_var(sq, X):
    D = np.diag(sq.dense).copy()
    T = (sq.dense @ X - D[:, None] * X) / D[:, None]
    return 1.0 / D + T.var(axis=1, ddof=1)


def block_ops(sq, enclosure_size):
    """per block (S, B, Q_BB, inv(Q_BB)): independent of the samples, computed once per (model, enclosure_size) and left unchanged"""
    out = []
    for S, E in build_blocks(sq, enclosure_size):
        B = np.array(S + E)
        QBB = sq.dense[np.ix_(B, B)]
        out.append((S, B, QBB, np.linalg.inv(QBB)))
    return out


def block_var(sq, X, enclosure_size, ops=None):
    v = np.zeros(sq.n)
    for S, B, QBB, inv in (ops if ops is not None else block_ops(sq, enclosure_size)):
        kap = inv @ (sq.dense[B, :] @ X - QBB @ X[B, :])
        v[S] = np.diag(inv)[:len(S)] + kap.var(axis=1, ddof=1)[:len(S)]
    return v


def rbmc_var(sq, X, enclosure_size, ops=None):
    return plain_var(sq, X) if enclosure_size < 0 else block_var(sq, X, enclosure_size, ops)


def check_plan(plan, sq, enclosure_size, index_base=0):
    """the library's plan (MI355XBackend.rbmc_plan) against the restatement: blocks as sets with S first, n_interior, owner masks,
    and the owner masks partition 0..n-1 exactly once"""
    ref = build_blocks(sq, enclosure_size)
    own, _ = owner_masks(ref, sq.n)
    bp, rows, ni, ow = plan["block_ptr"], plan["rows"] - index_base, plan["n_interior"], plan["owner"]
    assert len(bp) == len(ref) + 1 and bp[0] == 0 and len(rows) == bp[-1] == len(ow)
    assert plan["max_block"] == max(len(S) + len(E) for S, E in ref)
    written = np.zeros(sq.n, np.int64)
    for b, (S, E) in enumerate(ref):
        r = rows[bp[b]:bp[b + 1]]
        assert ni[b] == len(S), b
        assert len(r) == len(S) + len(E) and len(set(r.tolist())) == len(r), b
        assert set(r[:ni[b]].tolist()) == set(S), b
        assert set(r[ni[b]:].tolist()) == set(E), b
        o = ow[bp[b]:bp[b + 1]]
        want = dict(zip(S, own[b]))
        assert [int(x) for x in o[:ni[b]]] == [int(want[int(v)]) for v in r[:ni[b]]], b
        assert not o[ni[b]:].any(), b
        np.add.at(written, r[:ni[b]][o[:ni[b]] == 1], 1)
    assert (written == 1).all()
    return ref
