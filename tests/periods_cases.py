"""Input families and cases of the period-detection tests, with their restatement results computed once per process."""
import functools
import json
import os

import numpy as np

import periods_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "periods_kats.json")


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def family(name, n=None, seed=0):
    """seasonal_4 / seasonal_7 (the SQL files' series, cut or repeated to n), sine12 (noisy sine of period 12), poisson7 (Poisson
    counts with a weekly rate), noise (white noise), ramp4 ([10, 20, 30, 40]), constant."""
    g = golden()["series"]
    rng = np.random.default_rng(1000 + seed)
    if name in ("seasonal_4", "seasonal_7"):
        base = np.array(g[name], dtype=np.float64)
        n = len(base) if n is None else n
        return np.resize(base, n).copy()
    if name == "sine12":
        t = np.arange(n)
        return 10.0 * np.sin(2 * np.pi * t / 12.0) + rng.normal(0.0, 1.0, n) + 50.0
    if name == "poisson7":
        rate = np.array([3.0, 4.0, 6.0, 9.0, 12.0, 15.0, 5.0])
        return rng.poisson(rate[np.arange(n) % 7]).astype(np.float64)
    if name == "noise":
        return rng.normal(0.0, 1.0, n)
    if name == "ramp4":
        return np.array(g["ramp4"], dtype=np.float64)
    if name == "constant":
        return np.full(n, 5.0)
    raise KeyError(name)


_KEYS = {}


def _key(values, kw):
    k = (np.asarray(values, dtype=np.float64).tobytes(), tuple(sorted(kw.items())))
    _KEYS[k] = np.asarray(values, dtype=np.float64)
    return k


@functools.lru_cache(maxsize=None)
def _contract(method, key):
    return ref.contract(method, _KEYS[key], **dict(key[1]))


def contract(method, values, **kw):
    """ref.contract, computed once per (method, series, parameters)."""
    kw = {k: v for k, v in kw.items() if v is not None}
    return _contract(method, _key(values, kw))


# (family, n) of the single-series cases: every length of the list, the error lengths included
LENGTHS = [("noise", 3), ("ramp4", 4), ("noise", 7), ("noise", 8), ("noise", 15), ("noise", 16), ("noise", 17), ("seasonal_7", 28),
           ("seasonal_4", 32), ("sine12", 63), ("noise", 64), ("sine12", 65), ("sine12", 96), ("poisson7", 120)]


def ragged_batch(count=130):
    """`count` series of four families with lengths 3 .. 120, too-short ones included."""
    fams = ("sine12", "poisson7", "noise", "seasonal_7")
    lens = [3, 7, 15, 16, 17, 28, 33, 48, 64, 65, 96, 120]
    return [family(fams[i % 4], lens[i % len(lens)] if i % 4 != 3 else max(lens[i % len(lens)], 8), seed=i) for i in range(count)]
