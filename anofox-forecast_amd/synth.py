"""Deterministic synthetic M5-shape batches.

Counter-based: series block b (1024 series) is drawn from Philox keyed by (seed, b), so any
shard regenerates exactly its slice.  Intermittent retail demand: log-normal level, weekly
profile, slow trend, Poisson counts, leading zeros.  `positive=True` adds 1 so that the
multiplicative ETS specs are admissible ("full grid" variant).
"""
from __future__ import annotations

import numpy as np

BLOCK = 1024
SEED_M5 = 20260101
SEED_STRESS = 20260102


def gen_block(seed: int, block: int, T: int, m: int = 7, positive: bool = False) -> np.ndarray:
    """Return [BLOCK, T] float64 series of block `block`."""
    rng = np.random.Generator(np.random.Philox(key=[seed, block]))
    level = np.exp(rng.normal(0.0, 1.2, size=BLOCK))
    phase = rng.uniform(0.0, 2.0 * np.pi, size=BLOCK)
    tau = rng.uniform(-1.0, 1.0, size=BLOCK)
    lead = rng.integers(0, T // 3 + 1, size=BLOCK)
    t = np.arange(T, dtype=np.float64)
    prof = 1.0 + 0.3 * np.sin(2.0 * np.pi * (np.arange(T) % m)[None, :] / m + phase[:, None])
    trend = 1.0 + 0.0002 * t[None, :] * tau[:, None]
    lam = np.maximum(level[:, None] * prof * trend, 0.0)
    y = rng.poisson(lam).astype(np.float64)
    y[t[None, :] < lead[:, None]] = 0.0
    if positive:
        y += 1.0
    return y


def gen_series(seed: int, start: int, count: int, T: int, m: int = 7, positive: bool = False) -> np.ndarray:
    """Series [start, start+count) as a [count, T] float64 array (series-major)."""
    out = np.empty((count, T), dtype=np.float64)
    s = start
    while s < start + count:
        b, off = divmod(s, BLOCK)
        take = min(BLOCK - off, start + count - s)
        out[s - start:s - start + take] = gen_block(seed, b, T, m, positive)[off:off + take]
        s += take
    return out


SEED_EXOG = 20260103


def gen_regressors(seed: int, start: int, count: int, T: int, h: int, k: int = 3) -> np.ndarray:
    """M5-like exogenous regressors of series [start, start+count): a [count, k, T + h] float64 array whose first T columns are the
    history and whose last h the future.  Regressor j is of kind j % 4: 0 a sell-price random walk around 5, 1 a promotion flag (rate
    0.2), 2 a noisy yearly temperature sine, 3 a weekday dummy (one weekday).  Counter-based like gen_block: block b of 1024
    series is drawn from Philox keyed by (seed, b), so any shard regenerates exactly its slice."""
    out = np.empty((count, k, T + h), dtype=np.float64)
    t = np.arange(T + h)
    s = start
    while s < start + count:
        b, off = divmod(s, BLOCK)
        take = min(BLOCK - off, start + count - s)
        rng = np.random.Generator(np.random.Philox(key=[seed, b]))
        blk = np.empty((BLOCK, k, T + h))
        for j in range(k):
            kind = j % 4
            if kind == 0:
                blk[:, j] = 5.0 + rng.normal(0.0, 0.5, size=(BLOCK, 1)) + np.cumsum(rng.normal(0.0, 0.05, size=(BLOCK, T + h)), axis=1)
            elif kind == 1:
                blk[:, j] = (rng.random(size=(BLOCK, T + h)) < 0.2).astype(np.float64)
            elif kind == 2:
                blk[:, j] = 15.0 + 10.0 * np.sin(2.0 * np.pi * t[None, :] / 365.0 + rng.uniform(0.0, 6.0, size=(BLOCK, 1))) + rng.normal(0.0, 2.0, size=(BLOCK, T + h))
            else:
                blk[:, j] = (t[None, :] % 7 == rng.integers(0, 7, size=(BLOCK, 1))).astype(np.float64)
        out[s - start:s - start + take] = blk[off:off + take]
        s += take
    return out


def gen_exog_target(seed: int, start: int, count: int, X: np.ndarray, real_valued: bool = False) -> np.ndarray:
    """A demand series driven by the regressors X [count, k, T] of gen_regressors: level 20, a slow trend, price elasticity -2 on
    regressor 0, +4 on regressor 1 (when present), noise sd 2; counts (rounded, clipped at 0) unless `real_valued`."""
    count_, k, T = X.shape
    rng = np.random.Generator(np.random.Philox(key=[seed + 1, start]))
    t = np.arange(T, dtype=np.float64)
    y = 20.0 + 0.02 * t[None, :] - 2.0 * (X[:, 0] - 5.0) + (4.0 * X[:, 1] if k > 1 else 0.0) + rng.normal(0.0, 2.0, size=(count_, T))
    return y if real_valued else np.round(np.maximum(0.0, y))
