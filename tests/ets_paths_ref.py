"""Restatement of the sample paths simulated from fitted ETS models (anofox_hip_ets_paths_device and what is built on it): THE
definition of what those entries compute, bit for bit.

Method: the state equations of the fitted spec run forward from the final states, the drawn innovation in place of the observed one
(Hyndman, Koehler, Ord & Snyder 2008, section 6.1).  The step is the state-space form that ets_ref.replay_many writes out:
with q = l, l + phi b, l b^phi, p the trend's part of it and s the seasonal state of the step's phase (n + k) % m,
    mu = q, q + s, q s
    additive error        y = mu + e:        l' = q + alpha e  [e / s],  b' = p + beta e [e / s]  or  p + beta e / l [e / (s l)],
                                             s' = s + gamma e  or  s + gamma e / q
    multiplicative error  y = mu (1 + e):    l' = q (1 + alpha e),  b' = p + beta q e  or  p (1 + beta e),  s' = s (1 + gamma e)
in numpy fp64 elementwise arithmetic: single IEEE operations, left to right, nothing fused.  b^phi of a damped multiplicative trend
is the checker's det_pow_pos; where b is not a finite positive number at that point the path is broken: that step and every later
one are NaN.  Nothing else is clamped.

Draws: Philox4x32-10 of paths_ref.  Bootstrap: the index rule and the counters of paths_ref unchanged.  Gaussian: counter
(p, s, k >> 2, 2); words (w0, w1) serve steps 4j and 4j + 1, (w2, w3) steps 4j + 2 and 4j + 3; u1 = (wa + 0.5) 2^-32, u2 = (wb + 0.5)
2^-32 (exact), r = sqrt(-2 det_log(u1)), (sin, cos) = det_sincos(6.283185307179586 u2); the even step takes r cos, the odd one r sin;
e = sigma z with sigma = sqrt(sse / n).

Vectorised over series (and paths), as ets_ref.replay_many is.  Of oracle/ it calls det_eval for log, sincos and pow_pos and nothing
else; nothing here imports the package under test.
"""
from __future__ import annotations

import numpy as np

import inspect_ref as R
import paths_ref as P

OK, EMPTY, NAN, RAGGED, NO_MODEL = 0, 1, 2, 3, 4
GAUSSIAN, BOOTSTRAP = 0, 1
MAX_PERIOD, MAX_RING = 2048, 128
TWO_PI = 6.283185307179586
DBL_MAX = np.finfo(np.float64).max


def _det(fn, x, y=None):
    from oracle import oracle as O
    return O.det_eval(fn, x, y)


def spec_ok(sid):
    """One of the 25 specs of the project: no multiplicative error with an additive season."""
    sid = int(sid)
    return 0 <= sid < 30 and not (sid // 15 == 1 and sid % 3 == 1)


def ring_size(m, horizon):
    return min(int(m), int(horizon))


# ---- draws ----
def normal_words(seed, n_series, n_paths, horizon):
    """uint64 [4, n_paths, blocks, n_series]: the Philox blocks of the Gaussian draws, counter (p, s, block, 2)."""
    p = np.arange(n_paths, dtype=np.uint64).reshape(-1, 1, 1)
    b = np.arange((horizon + 3) // 4, dtype=np.uint64).reshape(1, -1, 1)
    s = np.arange(n_series, dtype=np.uint64).reshape(1, 1, -1)
    return P.philox_words(p, s, b, np.uint64(2), seed)


def normal_pair(wa, wb):
    """Two words -> (the even step's z, the odd step's z)."""
    u1 = (np.asarray(wa).astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (np.asarray(wb).astype(np.float64) + 0.5) * 2.0 ** -32
    r = np.sqrt(-2.0 * _det("log", u1))
    sn, cs = _det("sincos", TWO_PI * u2)
    return r * cs, r * sn


def normal_draws(seed, n_series, n_paths, horizon):
    """fp64 [n_paths, horizon, n_series]: z of every (path, step, series)."""
    w = normal_words(seed, n_series, n_paths, horizon)
    blocks = w.shape[2]
    z = np.empty((n_paths, blocks, 4, n_series))
    z[:, :, 0], z[:, :, 1] = normal_pair(w[0], w[1])
    z[:, :, 2], z[:, :, 3] = normal_pair(w[2], w[3])
    return z.reshape(n_paths, blocks * 4, n_series)[:, :horizon, :]


# ---- statuses ----
def _cut(length, pool_rows):
    return min(max(int(length), 0), int(pool_rows))


def series_status(sid, info, states, m, length, horizon, innovations, pool=None, pool_length=None, pool_rows=0, joint=False):
    """The status of one series (info [8], states [2 + max(m, 1)], pool: its column).  Precedence NO_MODEL, RAGGED, EMPTY, NAN."""
    if not spec_ok(sid) or int(length) < 1:
        return NO_MODEL
    boot = innovations == BOOTSTRAP
    n = 0
    if boot:
        raw = pool_rows if pool_length is None else int(pool_length)
        if joint and pool_length is not None and raw != pool_rows:
            return RAGGED
        n = _cut(raw, pool_rows)
        if n == 0:
            return EMPTY
    t, s = (int(sid) % 15) // 3, int(sid) % 3
    read = [info[0], states[0]]
    if t != 0:
        read += [info[1], states[1]]
    if s != 0:
        read += [info[2]] + [states[2 + (int(length) + k) % m] for k in range(ring_size(m, horizon))]
    if t in (2, 4):
        read.append(info[3])
    if boot:
        read += list(pool[:n])
    else:
        with np.errstate(all="ignore"):
            read.append(np.sqrt(np.float64(info[7]) / np.float64(int(length))))
    return NAN if any(np.isnan(np.float64(v)) for v in read) else OK


# ---- the recursion ----
def simulate(notation, m, alpha, beta, gamma, phi, level, growth, seasonal, lengths, e):
    """Series of ONE spec together: parameters and final states fp64 [g] (seasonal [g, m], phase-indexed), innovations e [P, h, g] ->
    paths [P, h, g].  A parameter the spec has not is not read."""
    er, t, s = R.parts(notation)
    assert not (er == "M" and s == "A"), "not a spec of this project"
    e = np.asarray(e, dtype=np.float64)
    n_paths, h, g = e.shape
    one = np.float64(1)
    a = np.asarray(alpha, dtype=np.float64)[None, :]
    b_ = np.asarray(beta, dtype=np.float64)[None, :]
    gm = np.asarray(gamma, dtype=np.float64)[None, :]
    ph = np.asarray(phi, dtype=np.float64)[None, :] if t in ("Ad", "Md") else np.ones((1, g))
    l = np.repeat(np.asarray(level, dtype=np.float64)[None, :], n_paths, axis=0)
    b = np.repeat(np.asarray(growth, dtype=np.float64)[None, :], n_paths, axis=0) if t != "N" else None
    ring = np.repeat(np.asarray(seasonal, dtype=np.float64)[None, :, :], n_paths, axis=0) if s != "N" else None
    lens = np.asarray(lengths, dtype=np.int64)
    cols = np.arange(g)
    broken = np.zeros((n_paths, g), dtype=bool)
    out = np.full((n_paths, h, g), np.nan)
    with np.errstate(all="ignore"):
        for k in range(h):
            j = (lens + k) % m
            if t == "N":
                p, q = None, l
            elif t in ("A", "Ad"):
                p = ph * b
                q = l + p
            elif t == "M":
                p = b
                q = l * p
            else:
                broken = broken | ~((b > 0.0) & (b <= DBL_MAX))
                p = _det("pow_pos", np.where(broken, one, b), np.broadcast_to(ph, b.shape))
                q = l * p
            sj = ring[:, cols, j] if s != "N" else None
            mu = q if s == "N" else (q + sj if s == "A" else q * sj)
            if er == "A":
                err = e[:, k, :]
                y = mu + err
                l_new = q + a * (err if s != "M" else err / sj)
                if t in ("A", "Ad"):
                    b_new = p + b_ * (err if s != "M" else err / sj)
                elif t in ("M", "Md"):
                    b_new = p + b_ * (err / l if s != "M" else err / (sj * l))
                if s == "A":
                    s_new = sj + gm * err
                elif s == "M":
                    s_new = sj + gm * err / q
            else:
                eps = e[:, k, :]
                y = mu * (one + eps)
                l_new = q * (one + a * eps)
                if t in ("A", "Ad"):
                    b_new = p + b_ * q * eps
                elif t in ("M", "Md"):
                    b_new = p * (one + b_ * eps)
                if s == "M":
                    s_new = sj * (one + gm * eps)
            out[:, k, :] = np.where(broken, np.nan, y)
            l = np.where(broken, l, l_new)
            if t != "N":
                b = np.where(broken, b, b_new)
            if s != "N":
                ring[:, cols, j] = np.where(broken, sj, s_new)
    return out


def innovations_of(spec, info, lengths, n_paths, horizon, innovations, status, pool=None, pool_lengths=None, pool_rows=0, joint=False, seed=0):
    """fp64 [n_paths, horizon, n]: the innovation of every (path, step, series) whose status is 0 (0.0 elsewhere)."""
    n = len(spec)
    e = np.zeros((n_paths, horizon, n))
    live = np.flatnonzero(np.asarray(status) == OK)
    if innovations == GAUSSIAN:
        z = normal_draws(seed, n, n_paths, horizon)
        with np.errstate(all="ignore"):
            sigma = np.sqrt(np.asarray(info[7], dtype=np.float64) / np.asarray(lengths, dtype=np.float64))
        e[:, :, live] = sigma[None, None, live] * z[:, :, live]
    else:
        u = P.draws(seed, n, n_paths, horizon, joint)
        for s in live:
            cut = _cut(pool_rows if pool_lengths is None else pool_lengths[s], pool_rows)
            j = ((u[:, :, s] * np.uint64(cut)) >> np.uint64(32)).astype(np.int64)
            e[:, :, s] = np.asarray(pool, dtype=np.float64)[j, s]
    return e


def paths(spec, info, states, m, lengths, n_paths, horizon, innovations=GAUSSIAN, pool=None, pool_lengths=None, joint=False, seed=0):
    """spec int [n] (inspect_ref.spec_id); info fp64 [8, >= n] (rows alpha, beta, gamma, phi, -, -, -, sse); states fp64
    [2 + max(m, 1), >= n] (level, growth, seasonal state of phase j in row 2 + j); lengths int [n]; pool fp64 [pool_rows, >= n]
    time-major (bootstrap), pool_lengths the raw lengths (None: all pool_rows).
    -> (block fp64 [n_paths * horizon, n], row p * horizon + k; status int32 [n]; n_broken int32 [n]: the paths that hold a NaN)."""
    spec = np.asarray(spec, dtype=np.int64)
    n = len(spec)
    info = np.asarray(info, dtype=np.float64)[:, :n]
    states = np.asarray(states, dtype=np.float64)[:, :n]
    lengths = np.asarray(lengths, dtype=np.int64)[:n]
    m, h = int(m), int(horizon)
    assert 1 <= m <= MAX_PERIOD and ring_size(m, h) <= MAX_RING and states.shape[0] >= 2 + m
    assert not (joint and innovations == GAUSSIAN)
    pool_rows = 0
    if innovations == BOOTSTRAP:
        pool = np.asarray(pool, dtype=np.float64)
        pool_rows = int(pool.shape[0])
    status = np.array([series_status(spec[s], info[:, s], states[:, s], m, lengths[s], h, innovations,
                                     None if pool is None or innovations == GAUSSIAN else pool[:, s],
                                     None if pool_lengths is None else pool_lengths[s], pool_rows, joint) for s in range(n)], dtype=np.int32)
    e = innovations_of(spec, info, lengths, n_paths, h, innovations, status, pool, pool_lengths, pool_rows, joint, seed)
    block = np.full((n_paths, h, n), np.nan)
    for sid in sorted(set(int(v) for v in spec[status == OK])):
        g = np.flatnonzero((spec == sid) & (status == OK))
        block[:, :, g] = simulate(R.notation_of(sid), m, info[0, g], info[1, g], info[2, g], info[3, g], states[0, g], states[1, g],
                                  states[2:2 + m, g].T, lengths[g], e[:, :, g])
    n_broken = np.isnan(block).any(axis=1).sum(axis=0).astype(np.int32)
    return block.reshape(n_paths * h, n), status, n_broken


def innovations(y, fitted, lengths, spec):
    """y, fitted fp64 [T, >= n] time-major -> (pool fp64 [T, n] with NaN where nothing is written, pool_lengths int32 [n]): y - fitted for
    an additive error, (y - fitted) / fitted for a multiplicative one; length 0 for a spec that is none of the project's."""
    spec = np.asarray(spec, dtype=np.int64)
    n = len(spec)
    y, fitted = np.asarray(y, dtype=np.float64), np.asarray(fitted, dtype=np.float64)
    T = y.shape[0]
    pool = np.full((T, n), np.nan)
    lens = np.zeros(n, dtype=np.int32)
    with np.errstate(all="ignore"):
        for s in range(n):
            if not spec_ok(spec[s]):
                continue
            k = _cut(lengths[s], T)
            lens[s] = k
            v = y[:k, s] - fitted[:k, s]
            pool[:k, s] = v / fitted[:k, s] if spec[s] // 15 == 1 else v
    return pool, lens
