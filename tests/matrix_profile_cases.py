"""Seeded input families and the case list shared by tests/test_matrix_profile_cpu.py and tests/test_gpu_matrix_profile.py.  The
same call gives the same series."""
import math

import numpy as np


def family(name, n, period=7, seed=0):
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(7000 + seed)
    if name == "seasonal":             # noisy, non-integer values: the order of additions shows in the bits
        return 10.0 + 0.02 * t + 3.7 * np.sin(2.0 * math.pi * t / float(period)) + rng.normal(0.0, 0.6, n)
    if name == "counts":               # integers over a small alphabet: many equal distances, and sums that share a square root
        return rng.integers(0, 4, n).astype(np.float64)
    if name == "intermittent":         # M5-like demand, mostly zero: constant subsequences (std = EPSILON) among the others
        return (rng.poisson(1.2, n) * (rng.random(n) < 0.3)).astype(np.float64)
    if name == "constant":
        return np.full(n, 5.0)
    if name == "periodic":             # exactly periodic: every distance at a multiple of the period is 0.0
        return np.resize(rng.integers(0, 9, period).astype(np.float64), n)
    if name == "nan":
        v = family("seasonal", n, period, seed)
        v[n // 3] = math.nan
        return v
    if name == "inf":
        v = family("seasonal", n, period, seed)
        v[n // 2] = math.inf
        return v
    raise KeyError(name)


# (id, family, n, period, seed, subsequence_length, n_best, form): form "plain" is checked against the literal restatement, "numpy"
# against the vectorised one (the CPU test proves the two equal on every "plain" case of at most 200 rows).
CASES = [
    # the smallest series: m = 4, excl = 1, P = 29
    ("n32", "seasonal", 32, 7, 1, None, None, "plain"),
    # integer counts at the defaults: the cases on which comparing before the square root changes an index
    ("counts_a", "counts", 61, 7, 1, None, None, "plain"),
    ("counts_b", "counts", 66, 7, 1, None, None, "plain"),
    ("counts_c", "counts", 47, 7, 5, None, None, "plain"),
    ("counts_d", "counts", 52, 7, 12, None, None, "plain"),
    ("counts_e", "counts", 70, 7, 2, None, None, "plain"),
    # the families
    ("seasonal", "seasonal", 150, 12, 4, None, None, "plain"),
    ("intermittent", "intermittent", 120, 7, 5, None, None, "plain"),
    ("constant", "constant", 90, 7, 0, None, None, "plain"),
    ("periodic7", "periodic", 100, 7, 1, None, None, "plain"),
    ("periodic12", "periodic", 140, 12, 2, 6, None, "plain"),
    ("nan", "nan", 110, 9, 3, None, None, "plain"),
    ("inf", "inf", 110, 9, 4, None, None, "plain"),
    # P one below, at and one above the edges of the 64 x 64 tiles (m = 4: P = n - 3)
    ("p63", "seasonal", 66, 9, 10, 4, None, "plain"),
    ("p64", "counts", 67, 9, 11, 4, None, "plain"),
    ("p65", "seasonal", 68, 9, 12, 4, None, "plain"),
    ("p127", "seasonal", 130, 9, 13, 4, None, "plain"),
    ("p128", "seasonal", 131, 9, 14, 4, None, "plain"),
    ("p129", "counts", 132, 9, 15, 4, None, "plain"),
    ("p129_m8", "intermittent", 136, 9, 16, 8, 70, "plain"),          # an exclusion past the first column tile
    # m one below, at and one above the chunk of 16 steps of k, and two chunks and one
    ("m15", "seasonal", 100, 11, 20, 15, None, "plain"),
    ("m16", "seasonal", 100, 11, 21, 16, None, "plain"),
    ("m17", "seasonal", 100, 11, 22, 17, None, "plain"),
    ("m33", "counts", 160, 11, 23, 33, None, "plain"),
    # exclusions: no pair at all; fewer than 11 finite profile values (the +inf threshold)
    ("no_pair", "seasonal", 40, 7, 30, None, 1000, "plain"),
    ("few_finite", "seasonal", 40, 7, 31, 4, 32, "plain"),
    # m = n / 4
    ("quarter", "seasonal", 2300, 24, 40, 10 ** 6, None, "numpy"),
    # one series on each side of the LDS / workspace boundary (forced m = 4: 2,203 rows fit, 2,204 do not)
    ("lds_last", "seasonal", 2203, 7, 41, 4, None, "numpy"),
    ("ws_first", "seasonal", 2204, 7, 42, 4, None, "numpy"),
    # the largest subsequence length, with an exclusion that leaves 36 pairs
    ("m2048", "seasonal", 8192, 365, 43, 2048, 8192 - 2048 + 1 - 8, "plain"),
]

SQUARED_DIFFERS = ("counts_a", "counts_b", "counts_c", "counts_d", "counts_e")          # comparing before the root changes an mpi
TIED = ("counts_a", "counts_b", "counts_c", "counts_d")                             # several lags share the best count


def series(case):
    _, fam, n, period, seed = case[:5]
    return family(fam, n, period, seed)


def by_id(name):
    return next(c for c in CASES if c[0] == name)
