"""Shapes and data of the sample-path tests (tests/test_paths_cpu.py, tests/test_gpu_paths.py).  Nothing here imports the package
under test.

The shapes are the smallest at which the kernels can still go wrong:
  n_series  1, 63, 64, 65, 130   one lane, one short of a wavefront, a whole one, one more, more than two: lane and tile edges, and an
                                 ld (n_series rounded up to 64) larger than n_series
  horizon   1, 3, 4, 5, 8, 9, 28 a Philox block gives four steps: below, at and above one and two blocks, and M5's horizon
  n_paths   1, 2, 63, 64, 65, 100, 1000, 2048   the sort's padding to a power of two, and the limit; 257, 513, 1025 besides: the
                                 quantile kernel stages 16 columns of up to 256 keys per workgroup, 15 of up to 512, 7 of up to 1,024
                                 and 3 of up to 2,048 (QUANTILE_TILE_BOUNDARIES: the last count of one tile width, the first of the next)
  pool rows 1, 2, 3 and ragged per series; the generating kernel stages nothing -- a lane reads its pool rows from memory -- and the
                                 status kernel walks a pool in 4 row slices: 4 and 5 lie on either side of that boundary (POOL_LENGTHS)
"""
from __future__ import annotations

import numpy as np

N_SERIES = (1, 63, 64, 65, 130)
HORIZONS = (1, 3, 4, 5, 8, 9, 28)
N_PATHS = (1, 2, 63, 64, 65, 100, 1000, 2048)
QUANTILE_TILE_BOUNDARIES = ((256, 257), (512, 513), (1024, 1025))
POOL_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 50)
STATUS_SLICE_BOUNDARY = (4, 5)

LEVELS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 1.0)            # the nine of M5's uncertainty track, with both ends
LEVELS_16 = tuple(k / 15.0 for k in range(16))                          # the limit

# (n_series, horizon, n_paths, mode, joint): every value of the three lists above at least once, every (mode, joint) pair on a small and
# on a large shape
CASES = (
    (1, 1, 1, "cumulative", False),
    (1, 1, 1, "independent", True),
    (63, 3, 2, "cumulative", True),
    (63, 3, 2, "independent", False),
    (64, 4, 63, "cumulative", False),
    (64, 4, 63, "independent", True),
    (65, 5, 64, "cumulative", True),
    (65, 5, 64, "independent", False),
    (130, 8, 65, "cumulative", False),
    (130, 8, 65, "cumulative", True),
    (64, 9, 100, "independent", False),
    (64, 9, 100, "independent", True),
    (130, 28, 1000, "cumulative", True),
    (130, 28, 1000, "independent", False),
    (65, 28, 2048, "cumulative", False),
    (65, 9, 2048, "independent", True),
    (63, 9, 256, "cumulative", False),
    (63, 9, 257, "cumulative", False),
    (1, 4, 512, "cumulative", True),
    (1, 4, 513, "cumulative", True),
    (64, 3, 1024, "independent", False),
    (64, 3, 1025, "independent", False),
)


def case_id(c):
    return "n%d-h%d-P%d-%s-%s" % (c[0], c[1], c[2], c[3][:3], "joint" if c[4] else "own")


def make_points(n, h, seed):
    rng = np.random.default_rng(1000 + seed)
    pts = rng.normal(50.0, 20.0, size=(n, h))
    pts[0, 0] = -0.0                                                     # a zero of either sign among the points
    if n > 1:
        pts[1, h - 1] = 0.0
    return pts


def make_pools(n, seed, joint, rows=None):
    """-> (pools: a list of n vectors, pool_rows).  Independent: ragged lengths cycling through POOL_LENGTHS, pool_rows three above the
    longest (a block with rows beyond every length).  Joint: every pool has `rows` (default 9) rows.  The values repeat, change sign
    and span magnitudes, so that ties, both zeros and the order of the additions all show in the bits."""
    rng = np.random.default_rng(2000 + seed)
    if joint:
        rows = 9 if rows is None else rows
        lengths = [rows] * n
    else:
        lengths = [POOL_LENGTHS[(s + seed) % len(POOL_LENGTHS)] for s in range(n)]
    pools = []
    for s in range(n):
        e = rng.normal(0.0, 1.0, size=lengths[s]) * 10.0 ** rng.integers(-3, 4)
        e[rng.random(lengths[s]) < 0.2] = 0.0
        e[rng.random(lengths[s]) < 0.1] = -0.0
        e = np.where(rng.random(lengths[s]) < 0.3, np.round(e), e)
        pools.append(e)
    return pools, (lengths[0] if joint else max(lengths) + 3)


def pool_block(pools, pool_rows, fill=777.0):
    """[n, pool_rows] series-major; the rows beyond a pool's length hold `fill` (they must never be drawn)."""
    out = np.full((len(pools), pool_rows), fill)
    for s, e in enumerate(pools):
        out[s, :len(e)] = e
    return out


def three_level_plan():
    """12 leaves, three levels: the total, 3 groups of 4, the 12 leaves themselves -> column_of int32 [3, 12], 16 output columns."""
    leaves = np.arange(12)
    return np.stack([np.zeros(12, dtype=np.int32), (1 + leaves // 4).astype(np.int32), (4 + leaves).astype(np.int32)])
