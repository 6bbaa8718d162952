"""The smallest input on which a level of the factorisation runs TWO panel chains (csrc/device.cpp, factor_panel_chains: at
least two big fronts on the level and at least four 64-column blocks in the widest): a block-diagonal precision of three dense
blocks with 260, 258 and 200 columns. An odd count, so the chains hold 2 and 1 fronts; the last 64-column block of either chain
has a single active front (the panel kernels then get its geometry in their arguments), and block 3 -> 4 crosses the 256-column
outer block of the two-level blocking (the K = 256 update). Everything against the CPU oracle on the same permutation."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmrfx
import orc

pytestmark = pytest.mark.gpu

WIDTHS = (260, 258, 200)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def three():
    rng = np.random.default_rng(260)
    blocks = [np.cov(rng.standard_normal((c, 3 * c))) + np.eye(c) for c in WIDTHS]
    Q = sp.csc_matrix(sp.block_diag(blocks))
    be = gmrfx.MI355XBackend(Q)
    F = orc.OracleFactor(Q, be.ordering_permutation())
    yield Q, be, F
    be.close()


def test_one_level_holds_the_three_blocks_as_big_fronts(three):
    _, be, _ = three
    sy = be.symbolic()
    cols = np.diff(sy.super_first)
    assert sorted(cols.tolist(), reverse=True) == list(WIDTHS)        # one front per block, nothing else
    assert len(set(sy.level.tolist())) == 1                           # ... all on one level
    assert np.array_equal(np.diff(sy.row_ptr), cols)                  # no trailing rows: the level is its panel chains alone


def test_factor_matches_oracle_entry_by_entry(three):
    _, be, F = three
    Lg, Lo = be.factor_csc(), F.L()
    assert abs(Lg - Lo).max() <= 1e-10 * abs(Lo).max()
    assert be.last_info == 0


@pytest.mark.parametrize("nrhs", [1, 17, 64, 70])
def test_solves_match_oracle_and_repeat_bit_for_bit(three, nrhs):
    Q, be, F = three
    B = np.random.default_rng(nrhs).standard_normal((Q.shape[0], nrhs))
    X = be.backend_solve(B)
    assert relerr(X, F.solve(B)) < 1e-10
    assert np.array_equal(X, be.backend_solve(B))
    Z = be.backend_backward_solve(B)
    assert relerr(Z, F.backward_solve(B)) < 1e-10
    assert np.array_equal(Z, be.backend_backward_solve(B))


@pytest.mark.parametrize("nrhs", [1, 70])
def test_pipelined_step_gives_the_bits_of_the_two_calls(three, nrhs):
    Q, be, _ = three
    nz = 1.5 * Q.data
    B = np.random.default_rng(100 + nrhs).standard_normal((Q.shape[0], nrhs))
    be.refactorize_values(nz)
    X2 = be.backend_solve(B)
    X1 = be.refactorize_solve(nz, B)
    assert np.array_equal(X1, X2)
    be.refactorize_values(Q.data)          # (the module's other tests compare with the oracle of Q)
