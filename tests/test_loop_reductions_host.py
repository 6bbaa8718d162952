"""The checks of tests/test_gpu_loop_reductions.py, tested on the CPU (tests/loop_reduction_ref.py): the geometry is that of the source;
the problems have what the checks need (every term at least TERM_FLOOR of its sum, |step|_inf where peaked() wants it, a rejected full
step); a float64 numpy evaluation passes every check with the factor 16 of the decrement's bound taken down to 1; four deliberately
wrong reductions fail at least one check at every size at which they differ from the right one."""
import os
import re

import numpy as np
import pytest

import loop_reduction_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianmarkovrandomfields.jl_amd", "csrc")
ALL = lr.SIZES + (lr.BIG,)


def test_geometry_is_restated_from_the_source():
    hdr = open(os.path.join(CSRC, "kernels.h")).read()
    assert int(re.search(r"kFisherStatChunk = (\d+)", hdr).group(1)) == lr.CHUNK
    hip = open(os.path.join(CSRC, "fisher.hip")).read()
    launch = hip.split("void launch_fisher_stats")[1]
    assert re.search(r"k_fisher_stats, dim3\(\(unsigned\)nblocks, \(unsigned\)m\.nbatch\), dim3\((\d+)\)", launch).group(1) == str(lr.THREADS)
    assert re.search(r"k_fisher_stats_final, dim3\(\(unsigned\)m\.nbatch\), dim3\((\d+)\)", launch).group(1) == str(lr.THREADS)
    assert f"t += {lr.THREADS}" in hip and f"bk += {lr.THREADS}" in hip


def test_sizes_sit_on_every_edge():
    T, C = lr.THREADS, lr.CHUNK
    assert {T - 1, T, T + 1, C - 1, C, C + 1, 2 * C + 1} == set(lr.SIZES) and lr.BIG == T * C + 1
    assert lr.depth(255) == 1 + 8 + 1 + 8 and lr.depth(257) == 2 + 8 + 1 + 8 and lr.depth(8193) == 16 + 8 + 1 + 8 and lr.depth(lr.BIG) == 16 + 8 + 2 + 8
    # the bracket of the mean-change checks stands a factor 50 above the error it allows for
    assert 50 * (lr.depth(lr.BIG) * lr.EPS / 2 + 3 * lr.EPS) < lr.BRACKET


@pytest.mark.parametrize("n", ALL)
def test_problems_have_what_the_checks_need(n):
    Q, y = lr.problem(n)
    z = np.zeros(n)
    for x0 in (z, lr.start(n)):
        score, step, accept, full = lr.first_iterate(Q, y, x0)
        assert min(lr.smallest_terms(score, step, x0 - step, x0)) >= lr.TERM_FLOOR
    assert np.linalg.norm(lr.start(n)) >= 1
    for p in lr.peak_positions(n):
        score, step, accept, full = lr.first_iterate(Q, lr.peaked(n, p), z)
        a = np.abs(step)
        assert int(a.argmax()) == p and np.sort(a)[-2] < 0.5 * a[p]          # |step|_inf sits at p, alone
        assert full > accept + 1e6 * abs(accept)                             # the full step is rejected: the loop backtracks at alpha = 1
    assert {0, n - 1} <= set(lr.peak_positions(n))


@pytest.mark.parametrize("n", ALL)
def test_float64_numpy_passes_every_check_without_the_factor(n):
    assert lr.failures(lr.reduce_f64(), n, factor=1) == []


@pytest.mark.parametrize("mutant", lr.MUTANTS)
@pytest.mark.parametrize("n", ALL)
def test_wrong_reductions_are_caught(n, mutant):
    failed = lr.failures(lr.reduce_f64(mutant), n)
    assert bool(failed) == lr.differs(n, mutant), failed
    if failed:       # every sum notices, not only the maximum at one position
        assert {"dec", "mean_change", "mean_change_rel"} <= set(failed), failed


def test_mutants_differ_where_they_should():
    T, C = lr.THREADS, lr.CHUNK
    for n in ALL:
        assert lr.differs(n, "drop_last_entry") and lr.differs(n, "drop_last_chunk")
        assert lr.differs(n, "first_256_of_each_chunk") == (n > T)
        assert lr.differs(n, "no_partial_tail") == (n % T != 0)
    assert len(lr.kept(C + 1, "drop_last_chunk")) == C and len(lr.kept(C, "drop_last_chunk")) == 0
    assert len(lr.kept(2 * C + 1, "first_256_of_each_chunk")) == 2 * T + 1
