"""Shapes and data of the scaled-score tests (tests/test_scaled_scores_cpu.py, tests/test_gpu_scaled_scores.py).  Nothing here
imports the package under test.

The shapes are the smallest at which the kernels can still go wrong:
  n_cols     1, 63, 64, 65, 130   one lane, one short of a wavefront, a whole one, one more, more than two; ld is n_cols rounded up
                                  to 64 and the padding columns hold NaN
  t_rows     1, 2, 3, 15, 16, 17, 33, 100   both sides of every rows-in-flight block (1, 4, 8, 16) and a last block that is partial;
                                  the lengths are ragged -- 0, 1 and t_rows among them -- and the rows past a length hold NaN
  lag        1 (the previous row's register), 7 (the second stream), 20 (larger than the largest block of loads); a lag that is
             at least some lengths (status 1)
  tail_rows  1, 28, and above the length
  leading zeros: none, some, -0.0 among them, all zero (status 1), one non-zero last row (status 1)
  specials   a constant series (status 3), a NaN inside (status 2), NaN only past the length (status 0), +inf, a NaN in w_src outside
             the tail (no effect) and inside it (status 2)
  ranges     the whole, [3, 68) (an unaligned begin and 65 terms), [64, 130), one column, a range whose every column is left out, an
             empty one, a reversed one, one beyond n_cols
  loss rows  1, 9, 16, both transforms
"""
from __future__ import annotations

import numpy as np

# (n_cols, t_rows, lag, tail_rows, trim, with_w_src)
SCALE_CASES = (
    (1, 1, 1, 1, True, False),
    (1, 100, 1, 28, True, False),
    (63, 2, 1, 1, True, False),
    (64, 3, 1, 28, True, True),
    (65, 15, 1, 28, True, False),
    (130, 16, 7, 28, True, True),
    (65, 17, 1, 1, True, True),
    (130, 33, 7, 40, True, False),
    (130, 100, 1, 28, True, True),
    (64, 100, 20, 28, True, False),
    (63, 33, 1, 28, False, False),
    (130, 100, 7, 200, False, True),
)
EDGE_LENGTHS = (15, 16, 17, 33, 14, 18, 32, 34, 1, 0, 40, 4, 5, 8, 9, 3)      # both sides of every block edge, in one wavefront

# (n_cols, n_loss, transform)
WEIGHTED_CASES = (
    (1, 1, 1),
    (63, 16, 0),
    (64, 1, 0),
    (65, 9, 1),
    (130, 1, 1),
    (130, 9, 0),
    (130, 16, 1),
)


def scale_id(c):
    return "n%d-T%d-lag%d-tail%d-%s-%s" % (c[0], c[1], c[2], c[3], "trim" if c[4] else "keep", "w" if c[5] else "y")


def weighted_id(c):
    return "n%d-r%d-%s" % (c[0], c[1], "root" if c[2] else "ratio")


def ld_of(n):
    return (n + 63) // 64 * 64


def make_scale_case(n, T, seed, with_w, lengths=None):
    """-> (block fp64 [T, ld], lengths int32 [ld], w_block fp64 [T, ld] or None).  Columns alternate between integer counts with
    leading zeros (intermittent demand) and reals over six decades.  With enough columns and rows: column 1 is empty, column 2 has one
    row, column 3 is constant after two leading zeros, column 4 holds a NaN inside, column 5 +inf, column 6 is all zero, column 7 has
    a single non-zero last row, column 8 has -0.0 among its leading zeros, column 9 has a NaN in w_src before the tail rows (when
    there are rows before them), column 10 one inside them.  The rows past a length and the padding columns hold NaN."""
    rng = np.random.default_rng(5000 + seed)
    ld = ld_of(n)
    block = np.full((T, ld), np.nan)
    lens = np.zeros(ld, dtype=np.int32)
    for c in range(n):
        if lengths is not None:
            m = min(int(lengths[c % len(lengths)]), T)
        else:
            m = T if c % 3 == 0 else int(rng.integers(0, T + 1))
        lens[c] = m
        if c % 2 == 0:
            col = rng.poisson(1.5, size=T).astype(np.float64) * (rng.random(T) < 0.6)
            col[:int(rng.integers(0, max(T // 3, 1) + 1))] = 0.0
        else:
            col = rng.normal(0.0, 1.0, size=T) * 10.0 ** float(rng.integers(-3, 4))
            if c % 4 == 1:
                col[:int(rng.integers(0, max(T // 4, 1) + 1))] = 0.0
        block[:m, c] = col[:m]
    if lengths is None:
        if n > 1:
            lens[1] = 0
            block[:, 1] = np.nan
        if n > 2:
            lens[2] = 1
            block[:, 2] = np.nan
            block[0, 2] = 3.0
        for c in range(3, min(n, 11)):
            lens[c] = T
        if n > 3:
            block[:, 3] = 2.5
            block[:min(2, T - 1), 3] = 0.0
        if n > 4:
            block[:, 4] = rng.normal(0.0, 1.0, size=T)
            block[T // 2, 4] = np.nan
        if n > 5:
            block[:, 5] = rng.normal(0.0, 1.0, size=T)
            block[T // 2, 5] = np.inf
        if n > 6:
            block[:, 6] = 0.0
            block[T // 2, 6] = -0.0
        if n > 7:
            block[:, 7] = 0.0
            block[T - 1, 7] = 4.0
        if n > 8:
            block[:, 8] = rng.poisson(2.0, size=T).astype(np.float64) + 1.0
            block[:min(3, T - 1), 8] = 0.0
            block[min(1, max(T - 2, 0)), 8] = -0.0 if T > 1 else block[0, 8]
        if n > 10:
            block[:, 9] = rng.random(T) + 0.5
            block[:, 10] = rng.random(T) + 0.5
    w = None
    if with_w:
        w = np.full((T, ld), np.nan)
        price = rng.random(ld) * 9.0 + 1.0
        for c in range(n):
            w[:lens[c], c] = np.abs(block[:lens[c], c]) * price[c]
        if lengths is None and n > 10:
            w[:, 9] = rng.random(T)
            w[:, 10] = rng.random(T)
            w[0, 9] = np.nan                       # outside the tail whenever tail_rows < T: no effect; inside it otherwise
            w[T - 1, 10] = np.nan                  # the last row: inside every tail
    return block, lens, w


def make_edge_case(seed):
    """130 columns x 40 rows whose lengths walk EDGE_LENGTHS: columns of one wavefront end on both sides of every block edge."""
    return make_scale_case(130, 40, seed, True, lengths=EDGE_LENGTHS)


def ranges_of(n):
    """The column ranges of a weighted case with n columns (the invalid ones included)."""
    if n >= 130:
        return [(0, n), (3, 68), (64, 130), (77, 78), (100, 104), (5, 5), (9, 4), (120, n + 1)]
    if n >= 63:
        return [(0, n), (3, n - 1), (n - 1, n), (7, 7), (0, n + 1)]
    return [(0, n), (0, 0)]


def make_weighted_case(n, n_loss, seed):
    """-> (loss fp64 [n_loss, ld], scale fp64 [ld], weight fp64 [ld], col_status int32 [ld]).  Positive losses, scales and weights over
    several decades, with a zero, a negative, a NaN and an infinite scale, a NaN, a negative and a zero weight, a NaN, a negative and
    an infinite loss in single cells, a few columns with a status, and (n >= 130) columns 100 .. 103 all left out for one reason each.
    The padding columns hold NaN."""
    rng = np.random.default_rng(7000 + seed)
    ld = ld_of(n)
    loss = np.full((n_loss, ld), np.nan)
    scale = np.full(ld, np.nan)
    weight = np.full(ld, np.nan)
    status = np.zeros(ld, dtype=np.int32)
    loss[:, :n] = rng.random((n_loss, n)) * 10.0 ** rng.integers(-2, 3, size=(n_loss, n)).astype(np.float64)
    scale[:n] = (rng.random(n) + 0.1) * 10.0 ** rng.integers(-2, 3, size=n).astype(np.float64)
    weight[:n] = np.round(rng.random(n) * 1000.0, 2)
    if n >= 63:
        scale[11], scale[12], scale[13], scale[14] = 0.0, -1.0, np.nan, np.inf
        weight[15], weight[16], weight[17], weight[18] = np.nan, -2.0, 0.0, -0.0
        loss[0, 19], loss[n_loss - 1, 20], loss[0, 21], loss[n_loss // 2, 22] = np.nan, -1.0, np.inf, 0.0
        status[23], status[24], status[25] = 1, 2, 3
    if n >= 130:
        status[100], scale[101], weight[102] = 3, 0.0, np.nan
        loss[:, 103] = np.nan
    return loss, scale, weight, status


def make_hierarchy(n, seed):
    """Three groupings over n leaves, numbered grouping by grouping: the total (column 0), groups of about 13 leaves, the leaves."""
    groups = np.arange(n) // 13
    g = int(groups.max()) + 1
    return np.array([np.zeros(n, dtype=np.int64), 1 + groups, 1 + g + np.arange(n)], dtype=np.int32)


def make_training(n, T, seed, ragged=True):
    """n intermittent count series that end on the same date: lists of arrays (the shorter ones start later), and prices."""
    rng = np.random.default_rng(9000 + seed)
    series, prices = [], []
    for s in range(n):
        m = T if (s % 4 == 0 or not ragged) else int(rng.integers(max(T // 2, 1), T + 1))
        col = rng.poisson(1.2, size=m).astype(np.float64) * (rng.random(m) < 0.7)
        col[:int(rng.integers(0, m // 3 + 1))] = 0.0
        series.append(col)
        prices.append(np.round(rng.random(m) * 5.0 + 0.5, 2))
    return series, prices
