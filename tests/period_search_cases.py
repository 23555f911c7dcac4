"""Input families and batches shared by tests/test_period_search_cpu.py and tests/test_gpu_period_search.py.  Everything is seeded:
the same call gives the same series."""
import math

import numpy as np


def family(name, n, period=12, seed=0):
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(1000 + seed)
    if name == "zeros":
        return np.zeros(n)
    if name == "constant":
        return np.full(n, 5.0)
    if name == "sine":                 # rank two
        return np.sin(2.0 * math.pi * t / float(period))
    if name == "seasonal":             # noisy, non-integer values: the order of additions shows in the bits
        return 10.0 + 0.031 * t + 3.7 * np.sin(2.0 * math.pi * t / float(period)) + 1.3 * np.cos(2.0 * math.pi * t / (2.5 * period)) + rng.normal(0.0, 0.8, n)
    if name == "noise":
        return rng.normal(0.0, 1.0, n)
    if name == "demand":               # intermittent counts, M5-like
        return rng.poisson(0.6 + 0.5 * (1.0 + np.sin(2.0 * math.pi * t / 7.0)), n).astype(np.float64)
    if name == "nan":
        v = family("seasonal", n, period, seed)
        v[n // 3] = math.nan
        return v
    if name == "inf":
        v = family("seasonal", n, period, seed)
        v[n // 2] = math.inf
        return v
    raise KeyError(name)


def ssa_ragged_batch():
    """About 130 series (series, note): short ones that fail, every input family, default windows on both sides of the one-wavefront
    limit (l = 64 at n = 192 .. 194) and of the LDS-matrix limit (l = 86 at n = 258 .. 260, l = 87 at n = 261), odd lengths."""
    out = []
    for i in range(100):
        n = 16 + 2 * i + (i % 3)                     # 16 .. 216, default windows 5 .. 72
        out.append(family(("seasonal", "demand", "noise", "sine")[i % 4], n, 7 + i % 6, seed=i))
    for n in (5, 15, 0, 9):
        out.append(family("noise", n, seed=n))
    for name in ("zeros", "constant", "nan", "inf"):
        out.append(family(name, 40, seed=3))
        out.append(family(name, 200, seed=4))
    for n in (192, 195, 196, 258, 261, 264, 300):
        out.append(family("seasonal", n, 12, seed=n))
    for n in (330, 390, 420):                        # windows 110 .. 140: the matrix in the workspace, shared by persistent workgroups
        out.append(family("demand", n, 7, seed=n))
    return out


def stl_ragged_batch():
    """About 130 series with different candidate lists per series (max_period defaults to n / 3), failures included."""
    out = []
    for i in range(110):
        n = 16 + i + (i % 5)
        out.append(family(("seasonal", "demand", "noise", "sine")[i % 4], n, 5 + i % 9, seed=200 + i))
    for n in (3, 15, 0):
        out.append(family("noise", n, seed=n))
    for name in ("zeros", "constant"):
        out.append(family(name, 50, seed=1))
    for n in (200, 288, 289, 721, 722, 801):                       # the rows leave LDS above 721 observations
        out.append(family("seasonal", n, 24, seed=n))
    return out
