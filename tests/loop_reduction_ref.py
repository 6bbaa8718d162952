"""The four reductions of the Newton loop (csrc/fisher.hip: k_fisher_stats, k_fisher_stats_final) against long double, at the sizes where
their launch changes shape, no device.

k_fisher_stats forms {sum a b, sum (c - d)^2, sum d^2, max |b|} over chunks of CHUNK entries: thread t of THREADS adds entries
t, t + THREADS, ... of its chunk, a tree joins the threads; k_fisher_stats_final joins the chunks, thread t adding chunks
t, t + THREADS, ..., then a tree. CHUNK and THREADS restate csrc/kernels.h (kFisherStatChunk) and the launch of csrc/fisher.hip;
tests/test_loop_reductions_host.py checks them against the source.

The loop shows the four values only through what it does with them, so every check reads them off one iterate whose operands are
known bit for bit (tests/test_gpu_loop_reductions.py):
* sum a b is the Newton decrement score' step of the trace. From x0 = 0 without a line search x_1 = 0 - 1 step, so step = -x_1
  exactly, and score is the evaluation at x0. Bound: dec_bound().
* sum (c - d)^2 and sum d^2 decide `converged` through mean_change = |x_1 - x0| and mean_change_rel = mean_change / max(|x0|, 1e-10).
  From x0 = 0 the relative one is 1e10 times the absolute one, so converged = (mean_change < mean_change_tol); from an x0 of norm >= 1
  it is the smaller one, so converged = (mean_change_rel < mean_change_tol). deciding() gives that value in long double; the loop is
  run with the tolerance a factor 1 -+ BRACKET from it. BRACKET = 1e-12 is derived: a sum of non-negative terms has a relative
  error of at most depth(n) eps < 1e-14, the square root halves it, the quotient adds an eps or two.
* max |b| is exact. It decides the tiny-step exit, alpha |step|_inf < newton_dec_tol / 1000, after the first backtrack (alpha = 0.1):
  with newton_dec_tol = max_tol(|step|_inf, +1) the loop leaves with 1 merit evaluation and alpha = 0.1, with max_tol(|step|_inf, -1)
  it goes on. peaked() puts |step|_inf at a chosen index.

first_iterate() is the float64 CPU form of the iterate (a banded solve), reduce_ld() the reference, reduce_f64() plain numpy in float64
and, with a mutant's name, four reductions that are wrong in the ways a launch goes wrong; failures() runs every check on a reduction.
"""
import numpy as np
import scipy.linalg as sla

import fisher_ref as ref

CHUNK, THREADS = 4096, 256
SIZES = (255, 256, 257, 4095, 4096, 4097, 8193)
BIG = THREADS * CHUNK + 1                # one chunk more than k_fisher_stats_final has threads: its strided loop runs twice for thread 0
BRACKET, MAX_BRACKET = 1e-12, 1e-9
TERM_FLOOR = 1e-9                        # every term is at least this part of its sum: a dropped entry moves it 1000 brackets
PEAK, COUNT = 5000.0, 200.0
LD, EPS = ref.LD, ref.EPS
MUTANTS = ("drop_last_entry", "drop_last_chunk", "first_256_of_each_chunk", "no_partial_tail")


def depth(n):
    """additions on the longest path: a thread's chain, its tree, the final kernel's strided loop, its tree"""
    chunks = -(-n // CHUNK)
    return -(-min(n, CHUNK) // THREADS) + 8 + -(-chunks // THREADS) + 8


def problem(n):
    """(Q, y): the tridiagonal of fisher_ref.banded and Poisson counts of mean COUNT"""
    return ref.banded(n, 1), np.random.default_rng(n).poisson(COUNT, n).astype(float)


def start(n):
    """an x0 of norm >= 1 with every entry of the size of the others"""
    return np.random.default_rng(n + 1).uniform(0.5, 1.5, n)


def peak_positions(n):
    return sorted({p for p in (0, THREADS - 1, THREADS, CHUNK - 1, CHUNK, n - 1) if p < n})


def peaked(n, p):
    """counts of COUNT with PEAK at node p"""
    y = np.full(n, COUNT)
    y[p] = PEAK
    return y


def first_iterate(Q, y, x0):
    """(score, step, obj_accept, merit of the full step) of the loop's first iterate for Poisson counts on every node, in float64"""
    n = Q.shape[0]
    m = np.exp(x0)
    score = Q @ x0 - (y - m)
    ab = np.zeros((3, n))
    ab[1] = Q.diagonal() + m
    if n > 1:
        ab[0, 1:] = Q.diagonal(1)
        ab[2, :-1] = Q.diagonal(-1)
    step = sla.solve_banded((1, 1), ab, score)

    def parts(x):
        with np.errstate(over="ignore"):          # (the full step towards a count of PEAK overflows exp: its merit is +inf, rejected)
            return x @ (Q @ x) / 2, float((y * x - np.exp(x)).sum())
    en, ll = parts(x0)
    ef, lf = parts(x0 - step)
    return score, step, (en - ll) + 64 * EPS * max(abs(en) + abs(ll), 1), ef - lf


def kept(n, mutant):
    """the entries a reduction adds up: all of them, or what a mutant keeps"""
    i = np.arange(n)
    if mutant is None:
        return i
    if mutant == "drop_last_entry":
        return i[:-1]
    if mutant == "drop_last_chunk":
        return i[i // CHUNK < (n - 1) // CHUNK]
    if mutant == "first_256_of_each_chunk":
        return i[i % CHUNK < THREADS]
    if mutant == "no_partial_tail":          # only whole rounds of THREADS entries
        return i[:n - n % THREADS]
    raise ValueError(mutant)


def differs(n, mutant):
    return len(kept(n, mutant)) != n


def _four(a, b, c, d, dtype, keep):
    z = dtype(0)
    sel = (lambda v: np.asarray(v, dtype)[keep])
    return (sel(a) @ sel(b) if a is not None and b is not None else z,
            ((sel(c) - sel(d)) ** 2).sum(dtype=dtype) if c is not None and d is not None else z,
            (sel(d) ** 2).sum(dtype=dtype) if d is not None else z,
            np.abs(sel(b)).max(initial=0.0) if b is not None else z)


def reduce_ld(a, b, c, d):
    n = len(a if a is not None else b if b is not None else d)
    return _four(a, b, c, d, LD, kept(n, None))


def reduce_f64(mutant=None):
    """a reduction (a, b, c, d) -> four float64 values: numpy's, or a mutant's"""
    def run(a, b, c, d):
        n = len(a if a is not None else b if b is not None else d)
        return tuple(float(v) for v in _four(a, b, c, d, np.float64, kept(n, mutant)))
    return run


def dec_bound(score, step, factor=16):
    n = len(score)
    return factor * depth(n) * EPS * float(np.abs(np.asarray(score, LD) * np.asarray(step, LD)).sum(dtype=LD))


def dec_ok(got, score, step, factor=16):
    return abs(LD(got) - reduce_ld(score, step, None, None)[0]) <= dec_bound(score, step, factor)


def deciding(x1, x0):
    """the long-double value `converged` compares with mean_change_tol (see the header)"""
    _, ssd, sd2, _ = reduce_ld(None, None, x1, x0)
    mc, nx = np.sqrt(ssd), np.sqrt(sd2)
    if nx == 0:
        return mc
    assert nx >= 1
    return mc / nx


def bracket(value, side):
    """mean_change_tol a factor 1 + side BRACKET from the deciding value: side = -1 must not converge, +1 must"""
    return float(value * (1 + side * LD(BRACKET)))


def max_tol(step_inf, side):
    """newton_dec_tol with the tiny-step threshold a factor 1 + side MAX_BRACKET from 0.1 |step|_inf"""
    return 1000 * 0.1 * step_inf * (1 + side * MAX_BRACKET)


def smallest_terms(score, step, x1, x0):
    """every sum's smallest term over the sum"""
    out = [float(np.abs(score * step).min() / np.abs(score * step).sum()), float(((x1 - x0) ** 2).min() / ((x1 - x0) ** 2).sum())]
    if np.any(x0):
        out.append(float((x0 ** 2).min() / (x0 ** 2).sum()))
    return out


# ---- the loop's decisions on top of a reduction (csrc/device_fisher.cpp: the lines after `stats`) ---------------------------------------------
def converged(reduce, x1, x0, mean_tol):
    _, ssd, sd2, _ = reduce(None, None, x1, x0)
    mc = np.sqrt(ssd)
    return bool(mc < mean_tol or mc / max(np.sqrt(sd2), 1.0e-10) < mean_tol)


def tiny_exit(reduce, step, dec_tol):
    """the loop leaves after its first backtrack"""
    return bool(0.1 * reduce(None, step, None, None)[3] < dec_tol / 1000)


def failures(reduce, n, factor=16):
    """the names of the checks a reduction fails on the problem of size n, with the operands of the CPU's first iterate"""
    Q, y = problem(n)
    out = []
    z = np.zeros(n)
    score, step, _, _ = first_iterate(Q, y, z)
    if not dec_ok(reduce(score, step, None, None)[0], score, step, factor):
        out.append("dec")
    for name, x0 in (("mean_change", z), ("mean_change_rel", start(n))):
        x1 = x0 - first_iterate(Q, y, x0)[1]
        v = deciding(x1, x0)
        if converged(reduce, x1, x0, bracket(v, -1)) or not converged(reduce, x1, x0, bracket(v, +1)):
            out.append(name)
    for p in peak_positions(n):
        step = first_iterate(Q, peaked(n, p), z)[1]
        sinf = float(np.abs(step).max())          # (exact in any arithmetic)
        if not tiny_exit(reduce, step, max_tol(sinf, +1)) or tiny_exit(reduce, step, max_tol(sinf, -1)):
            out.append(f"max@{p}")
    return out
