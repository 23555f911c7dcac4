"""Restatement of the bootstrap sample paths and their quantiles, independent of the library: THE definition of what the
sample-path entries compute, bit for bit.

Method: residual bootstrap with cumulative resampling (the errors drawn for the steps of a path add up, so a band grows with the
horizon), per series or jointly across series (Panagiotelis et al. 2023: one residual ROW -- one date -- per path and step for all
series, which keeps their dependence in the sums).

Random numbers: Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011), counter-based.  The draw of (series s, path p, step k) is output
word k & 3 of the block with counter (p, joint ? 0 : s, k >> 2, joint ? 1 : 0) and key (seed & 0xffffffff, seed >> 32).  The pool
row is j = (u * n) >> 32 on integers, n the pool length of the series (joint: pool_rows); no rejection step.

`philox4x32_10` is the scalar statement, in Python integers; `philox_words` is the same on numpy arrays (uint64 lanes holding 32-bit
words) and is checked against the scalar one by tests/test_paths_cpu.py.  All floating-point work is numpy fp64 elementwise
arithmetic: single IEEE operations, nothing fused.

Nothing here imports the package under test.
"""
from __future__ import annotations

import math
import struct

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

OK, EMPTY, NAN, RAGGED = 0, 1, 2, 3
MAX_PATHS, MAX_LEVELS, MAX_POOL_ROWS, MAX_ROWS = 2048, 16, 1 << 20, 1 << 30
MODES = ("cumulative", "independent")


# ---- Philox4x32-10 ----
def philox4x32_10(counter, key):
    """(c0, c1, c2, c3), (k0, k1) -> four 32-bit output words.  Ten rounds; the key is bumped between rounds."""
    c0, c1, c2, c3 = [int(c) & MASK32 for c in counter]
    k0, k1 = [int(k) & MASK32 for k in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & MASK32, p1 >> 32, p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox_words(c0, c1, c2, c3, seed):
    """The same on broadcastable integer arrays: -> uint64 array [4, ...] of the four output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in (c0, c1, c2, c3)])
    k0, k1 = int(seed) & MASK32, (int(seed) >> 32) & MASK32
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                # 32 x 32 bits: no overflow in 64
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & m32, p1 >> s32, p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3])


def counter(s, p, k, joint):
    return (p, 0 if joint else s, k >> 2, 1 if joint else 0)


def key_of(seed):
    return (int(seed) & MASK32, (int(seed) >> 32) & MASK32)


def draw(seed, s, p, k, joint):
    """The 32-bit draw of (series, path, step)."""
    return philox4x32_10(counter(s, p, k, joint), key_of(seed))[k & 3]


def index(u, n):
    """The pool row of a draw: (u * n) >> 32."""
    return (int(u) * int(n)) >> 32


def draws(seed, n_series, n_paths, horizon, joint):
    """uint64 [n_paths, horizon, n_series]: every draw of a call."""
    p = np.arange(n_paths, dtype=np.uint64).reshape(-1, 1, 1)
    b = np.arange((horizon + 3) // 4, dtype=np.uint64).reshape(1, -1, 1)
    s = np.zeros((1, 1, n_series), dtype=np.uint64) if joint else np.arange(n_series, dtype=np.uint64).reshape(1, 1, -1)
    w = philox_words(p, s, b, np.uint64(1 if joint else 0), seed)        # [4, P, blocks, n]
    w = np.moveaxis(w, 0, 2).reshape(n_paths, -1, n_series)             # step k = 4 * block + word
    return w[:, :horizon, :]


# ---- paths ----
def series_status(point_row, pool, length, pool_rows, joint):
    """The status of one series; precedence RAGGED, EMPTY, NAN.  `length` is the raw length; the draws use it cut to [0, pool_rows]."""
    n = min(max(int(length), 0), int(pool_rows))
    if joint and int(length) != int(pool_rows):
        return RAGGED
    if n == 0:
        return EMPTY
    if any(math.isnan(float(v)) for v in list(pool[:n]) + list(point_row)):
        return NAN
    return OK


def one_path(point_row, pool, n, seed, s, p, mode, joint):
    """One path, statement for statement (scalar; the block form below is checked against it)."""
    acc, out = 0.0, []
    for k in range(len(point_row)):
        e = float(pool[index(draw(seed, s, p, k, joint), n)])
        if mode == "cumulative":
            acc = acc + e
            out.append(float(point_row[k]) + acc)
        else:
            out.append(float(point_row[k]) + e)
    return out


def paths(points, pools, n_paths, mode="cumulative", joint=False, seed=0, lengths=None, pool_rows=None):
    """points [n, h]; pools: a list of n vectors (or an [n, pool_rows] array); lengths: raw pool lengths (None: len of each pool);
    pool_rows: the call's pool_rows (None: the longest pool).  -> (block fp64 [n_paths * h, n], row p * h + k; status int32 [n])."""
    assert mode in MODES
    points = np.asarray(points, dtype=np.float64)
    n, h = points.shape
    pools = [np.asarray(e, dtype=np.float64).reshape(-1) for e in pools]
    lengths = [len(e) for e in pools] if lengths is None else [int(v) for v in lengths]
    pool_rows = max(lengths + [0]) if pool_rows is None else int(pool_rows)
    status = np.array([series_status(points[s], pools[s], lengths[s], pool_rows, joint) for s in range(n)], dtype=np.int32)
    u = draws(seed, n, n_paths, h, joint)                               # [P, h, n]
    block = np.full((n_paths, h, n), np.nan)
    for s in range(n):
        if status[s] != OK:
            continue
        m = min(max(lengths[s], 0), pool_rows)
        j = ((u[:, :, s] * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
        e = pools[s][j]                                                 # [P, h]
        with np.errstate(invalid="ignore", over="ignore"):              # (+-inf are ordinary values: inf - inf is a NaN path value)
            if mode == "cumulative":
                acc = np.zeros(n_paths)
                for k in range(h):
                    acc = acc + e[:, k]
                    block[:, k, s] = points[s, k] + acc
            else:
                block[:, :, s] = points[s][None, :] + e
    return block.reshape(n_paths * h, n), status


# ---- quantiles ----
def order_key(x):
    """The total-order key of an fp64 value: unsigned order = value order, -0.0 below +0.0, a NaN beyond the infinity of its sign."""
    bits = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return (~bits) & 0xFFFFFFFFFFFFFFFF if bits >> 63 else bits | (1 << 63)


def keys_of(a):
    bits = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))


def values_of(keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    return np.where(keys >> np.uint64(63) != 0, keys ^ np.uint64(1 << 63), ~keys).view(np.float64)


def sort_total(values):
    """A list sorted by the total-order key."""
    return sorted([float(v) for v in values], key=order_key)


def compute_quantile(s, q):
    """Level q of a sorted list: s[lo] * (1 - frac) + s[up] * frac at index q * (P - 1); q <= 0 the first value, q >= 1 the last."""
    if not s:
        return math.nan
    if q <= 0.0:
        return s[0]
    if q >= 1.0:
        return s[-1]
    n = len(s)
    idx = q * float(n - 1)
    lo = int(math.floor(idx))
    up = min(lo + 1, n - 1)
    frac = idx - float(lo)
    return s[lo] * (1.0 - frac) + s[up] * frac


def quantiles(block, horizon, n_paths, levels, n_cols=None):
    """block [n_paths * horizon, >= n_cols] -> (fp64 [n_levels, n_cols, horizon], status int32 [n_cols]): a column with a NaN among
    its paths has status NAN and NaN in every quantile."""
    block = np.asarray(block, dtype=np.float64)
    n_cols = block.shape[1] if n_cols is None else int(n_cols)
    cube = block[:n_paths * horizon, :n_cols].reshape(n_paths, horizon, n_cols)
    srt = values_of(np.sort(keys_of(cube), axis=0))                    # [P, h, n]
    out = np.empty((len(levels), n_cols, horizon))
    for l, q in enumerate(levels):
        q = float(q)
        if q <= 0.0:
            v = srt[0]
        elif q >= 1.0:
            v = srt[n_paths - 1]
        else:
            idx = q * float(n_paths - 1)
            lo = int(math.floor(idx))
            up = min(lo + 1, n_paths - 1)
            frac = idx - float(lo)
            with np.errstate(invalid="ignore", over="ignore"):
                v = srt[lo] * (1.0 - frac) + srt[up] * frac
        out[l] = v.T
    status = np.where(np.isnan(cube).any(axis=(0, 1)), NAN, OK).astype(np.int32)
    out[:, status == NAN, :] = np.nan
    return out, status


def same_bits(a, b):
    """Elementwise: equal bit patterns, or both NaN (the payload of a NaN is exempt; the sign of a zero is not)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
