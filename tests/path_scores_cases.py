"""Shapes and data of the path-score tests (tests/test_path_scores_cpu.py, tests/test_gpu_path_scores.py).  Nothing here imports
the package under test.

The shapes are the smallest at which the kernels can still go wrong:
  n_cols    1, 63, 64, 65, 130   one lane, one short of a wavefront, a whole one, one more, more than two: the tile of columns of a
                                 workgroup, and an ld (n_cols rounded up to 64) larger than n_cols
  horizon   1, 3, 28             one step, a few, M5's horizon: the means carried across the step loop
  n_paths   1, 2, 63, 64, 65, 100, 1000, 2048   the classes of the wave sum (fewer terms than lanes, exactly 64, one more), the sort's
                                 padding to a power of two, and the limit; 256/257, 512/513, 1024/1025: the score kernel stages 16
                                 columns of up to 256 keys per workgroup, 15 of up to 512, 7 of up to 1,024 and 3 of up to 2,048
  levels    none, the nine of paths_cases.LEVELS, sixteen
  ranges    of the energy score: the whole, [3, 68) (an unaligned begin and 65 terms: one more than the lanes), [64, 130), one column
"""
from __future__ import annotations

import numpy as np

LEVELS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 1.0)            # = paths_cases.LEVELS (tests/test_path_scores_cpu.py checks it)
LEVELS_16 = tuple(k / 15.0 for k in range(16))

# (n_cols, horizon, n_paths, levels): every value of the lists above at least once
CASES = (
    (1, 1, 1, "nine"),
    (1, 3, 2, "none"),
    (63, 3, 63, "nine"),
    (64, 1, 64, "sixteen"),
    (65, 3, 65, "nine"),
    (130, 3, 100, "none"),
    (130, 28, 1000, "nine"),
    (65, 28, 2048, "nine"),
    (63, 3, 256, "nine"),
    (63, 3, 257, "nine"),
    (1, 3, 512, "sixteen"),
    (1, 3, 513, "nine"),
    (64, 3, 1024, "nine"),
    (64, 3, 1025, "none"),
)
LEVEL_SETS = {"none": (), "nine": LEVELS, "sixteen": LEVELS_16}

# (n_cols, horizon, n_paths, col_begin, col_end): the energy score
ENERGY_CASES = (
    (1, 1, 1, 0, 1),
    (130, 3, 2, 0, 130),
    (130, 3, 65, 3, 68),
    (130, 28, 100, 64, 130),
    (130, 3, 64, 77, 78),
    (65, 3, 1000, 0, 65),
    (63, 1, 2048, 0, 63),
)


def case_id(c):
    return "n%d-h%d-P%d-%s" % c


def energy_id(c):
    return "n%d-h%d-P%d-c%d-%d" % c


def make_block(n, h, P, seed, special=True):
    """-> (block fp64 [P * h, n] time-major, actual fp64 [n, h]).  Per column a level and a spread over six decades; values repeat
    (rounded draws), both zeros occur, some actuals tie with a path, one lies below every path and one above.  With `special` (and
    enough columns): column 2 has no actual at all, single steps elsewhere have none, column 5 holds one NaN path value, column 7
    holds +inf in one cell and -inf in another step."""
    rng = np.random.default_rng(3000 + seed)
    scale = 10.0 ** rng.integers(-3, 4, size=n).astype(np.float64)
    level = rng.normal(0.0, 50.0, size=n) * scale
    cube = level[None, None, :] + rng.normal(0.0, 1.0, size=(P, h, n)) * scale[None, None, :]
    cube = np.where(rng.random((P, h, n)) < 0.3, np.round(cube), cube)
    cube[rng.random((P, h, n)) < 0.05] = 0.0
    cube[rng.random((P, h, n)) < 0.03] = -0.0
    actual = level[:, None] + rng.normal(0.0, 1.0, size=(n, h)) * scale[:, None]
    for c in range(n):
        k = int(rng.integers(0, h))
        kind = c % 5
        if kind == 0:
            actual[c, k] = cube[int(rng.integers(0, P)), k, c]           # a tie between a path and the actual
        elif kind == 1:
            actual[c, k] = cube[:, k, c].min() - 3.0 * scale[c]          # below every path
        elif kind == 2:
            actual[c, k] = cube[:, k, c].max() + 3.0 * scale[c]          # above every path
        elif kind == 3:
            actual[c, k] = 0.0 if c % 2 else -0.0
    if special:
        if n > 2:
            actual[2, :] = np.nan                                        # no actual at all: status 1
        for c in range(3, n, 11):
            actual[c, int(rng.integers(0, h))] = np.nan                  # single steps without an actual
        if n > 5:
            cube[P // 2, h - 1, 5] = np.nan                              # a NaN path: status 2
            actual[5, 0] = np.nan
        if n > 7:
            cube[0, 0, 7] = np.inf
            cube[P - 1, h - 1, 7] = -np.inf
    return cube.reshape(P * h, n), actual


def time_major(a, ld=None, fill=np.nan):
    """[n, h] series-major -> [h, ld] time-major, the padding columns filled (nothing may read them into a result)."""
    n, h = a.shape
    ld = (n + 63) // 64 * 64 if ld is None else ld
    out = np.full((h, ld), fill)
    out[:, :n] = a.T
    return out


def pad_columns(block, ld=None, fill=np.nan):
    n = block.shape[1]
    ld = (n + 63) // 64 * 64 if ld is None else ld
    out = np.full((block.shape[0], ld), fill)
    out[:, :n] = block
    return out
