"""Restatement of the scaled, weighted scores of a hierarchy, independent of the library: THE definition of what the scaled-score
entries compute (include/anofox_fcst_hip.h block 11), bit for bit.

The method is that of the M5 competition (Makridakis et al., competitors' guide): a loss per column divided by the column's in-sample
scale -- the mean squared (RMSSE) or mean absolute (MASE, scaled pinball loss) lag difference of the training series from its first
non-zero row on --, and the mean of the scaled losses over the columns of a level, weighted by the mass of the columns' last rows.
The names and the contract are this package's own.

All arithmetic is Python floats (fp64), one rounding per operation, nothing fused, in explicit loops.  Sums over rows, over ranges
and over loss rows are serial from 0.0; sums over the columns of a range are the wave sum W: a_l is the serial sum from 0.0 of the
terms t_i with i = l (mod 64), ascending in i, and W = ((a_0 + a_1) + a_2) + ... + a_63.

Nothing here imports the package under test.
"""
from __future__ import annotations

import math

import numpy as np

OK, SHORT, NAN, CONSTANT = 0, 1, 2, 3
RATIO, ROOT = 0, 1
MAX_LOSS, MAX_ROWS = 16, 1 << 30
WAVE = 64


def wave_sum(terms):
    """W(t_0 ... t_{n-1}) in Python floats."""
    a = [0.0] * WAVE
    for i, t in enumerate(terms):
        a[i % WAVE] = a[i % WAVE] + float(t)
    w = a[0]
    for l in range(1, WAVE):
        w = w + a[l]
    return w


# ---- the scale of one column ----
def first_nonzero(y, n):
    """The first row t < n with y[t] != 0.0 (both zeros are zero; a NaN is not zero); n when there is none."""
    for t in range(n):
        if float(y[t]) != 0.0:
            return t
    return n


def scale_sums(y, n, lag, trim):
    """-> (t0, n_terms, sq, ab): the serial sums of d * d and |d|, d = y[t] - y[t - lag], over t = t0 + lag .. n - 1 in row order."""
    t0 = first_nonzero(y, n) if trim else 0
    sq, ab = 0.0, 0.0
    for t in range(t0 + lag, n):
        d = float(y[t]) - float(y[t - lag])
        sq = sq + d * d
        ab = ab + abs(d)
    return t0, n - t0 - lag, sq, ab


def tail_sum(w, n, tail_rows):
    """The serial sum from 0.0 of w over the rows max(0, n - tail_rows) .. n - 1."""
    s = 0.0
    for t in range(max(0, n - tail_rows), n):
        s = s + float(w[t])
    return s


def scale_column(y, n, lag=1, trim=True, tail_rows=28, w=None):
    """One column: y (at least n values; rows >= n are not read), w the weight source (None: y).
    -> {"msd", "mad", "n_terms", "tail", "first", "status"}."""
    w = y if w is None else w
    t0, n_terms, sq, ab = scale_sums(y, n, lag, trim)
    tail = tail_sum(w, n, tail_rows)
    nan = math.nan
    bad = any(math.isnan(float(y[t])) for t in range(n)) or any(math.isnan(float(w[t])) for t in range(max(0, n - tail_rows), n))
    if bad:
        return {"msd": nan, "mad": nan, "n_terms": nan, "tail": nan, "first": t0, "status": NAN}
    if n_terms <= 0:
        return {"msd": nan, "mad": nan, "n_terms": float(n_terms), "tail": tail, "first": t0, "status": SHORT}
    msd, mad = sq / float(n_terms), ab / float(n_terms)
    if msd == 0.0:
        return {"msd": 0.0, "mad": 0.0, "n_terms": float(n_terms), "tail": tail, "first": t0, "status": CONSTANT}
    return {"msd": msd, "mad": mad, "n_terms": float(n_terms), "tail": tail, "first": t0, "status": OK}


def scale_block(block, lengths, lag=1, trim=True, tail_rows=28, w_block=None, n_cols=None):
    """block [t_rows, >= n_cols] time-major, left-aligned; lengths [>= n_cols] (cut to [0, t_rows]).
    -> {"scale": fp64 [4, n_cols] in the rows msd, mad, n_terms, tail; "first", "status": int32 [n_cols]}."""
    block = np.asarray(block, dtype=np.float64)
    t_rows = block.shape[0]
    n_cols = block.shape[1] if n_cols is None else int(n_cols)
    scale = np.full((4, n_cols), np.nan)
    first = np.zeros(n_cols, dtype=np.int32)
    status = np.zeros(n_cols, dtype=np.int32)
    for c in range(n_cols):
        n = min(max(int(lengths[c]), 0), t_rows)
        r = scale_column(block[:, c].tolist(), n, lag, trim, tail_rows, None if w_block is None else np.asarray(w_block)[:, c].tolist())
        scale[:, c] = (r["msd"], r["mad"], r["n_terms"], r["tail"])
        first[c], status[c] = r["first"], r["status"]
    return {"scale": scale, "first": first, "status": status}


# ---- the scaled loss of one cell ----
def scaled_loss(loss, scale, weight, status, transform):
    """-> (s, left_out).  Left out: a status that is not 0, a scale that is not finite or is <= 0.0, a weight that is NaN or negative,
    a scaled loss that is not finite."""
    loss, scale, weight = float(loss), float(scale), float(weight)
    q = loss / scale if scale != 0.0 else math.nan                         # (a zero scale is left out whatever the quotient)
    if transform == ROOT:
        s = math.sqrt(q) if q >= 0.0 else math.nan                         # (sqrt of -0.0 is -0.0, of a negative NaN)
    else:
        s = q
    out = int(status) != 0 or not (scale > 0.0 and scale < math.inf) or not (weight >= 0.0) or not (abs(s) < math.inf)
    return (math.nan if out else s), out


def weighted_scores(loss, scale, weight, ranges, transform, col_status=None, n_cols=None):
    """loss [n_loss][>= n_cols]; scale, weight [>= n_cols]; ranges [(begin, end)].
    -> {"scaled": fp64 [n_loss, n_cols] (NaN where left out; also NaN where no valid range covers the cell -- the entry does not
    touch those, the caller fills them), "covered": bool [n_cols], "score", "weight_sum": fp64 [n_ranges, n_loss], "left": int32
    [n_ranges, n_loss] (-1: a range that is empty, reversed or beyond n_cols), "total": fp64 [n_loss], "total_mean": float}."""
    loss = np.asarray(loss, dtype=np.float64)
    if loss.ndim == 1:
        loss = loss.reshape(1, -1)
    n_loss = loss.shape[0]
    n_cols = loss.shape[1] if n_cols is None else int(n_cols)
    R = len(ranges)
    nan = math.nan
    scaled = np.full((n_loss, n_cols), nan)
    covered = np.zeros(n_cols, dtype=bool)
    score = np.full((R, n_loss), nan)
    wsum = np.full((R, n_loss), nan)
    left = np.full((R, n_loss), -1, dtype=np.int32)
    for g, (b, e) in enumerate(ranges):
        b, e = int(b), int(e)
        if b < 0 or e <= b or e > n_cols:
            continue
        covered[b:e] = True
        for r in range(n_loss):
            num, den, out_count = [], [], 0
            for c in range(b, e):
                s, out = scaled_loss(loss[r, c], scale[c], weight[c], 0 if col_status is None else col_status[c], transform)
                scaled[r, c] = s
                w = float(weight[c])
                num.append(0.0 if out else w * s)
                den.append(0.0 if out else w)
                out_count += 1 if out else 0
            N, D = wave_sum(num), wave_sum(den)
            score[g, r] = N / D if D > 0.0 else nan
            wsum[g, r] = D
            left[g, r] = out_count
    total = np.full(n_loss, nan)
    all_rows = 0.0
    for r in range(n_loss):
        s, count = 0.0, 0
        for g in range(R):
            v = float(score[g, r])
            if v == v:
                s, count = s + v, count + 1
        total[r] = s / float(count) if count else nan
        all_rows = all_rows + float(total[r])
    return {"scaled": scaled, "covered": covered, "score": score, "weight_sum": wsum, "left": left, "total": total,
            "total_mean": all_rows / float(n_loss)}


# ---- the mse of the metrics entry with drop_nan, for the WRMSSE chain ----
def mse_drop_nan(forecast, actual):
    """The serial sum from 0.0 of (a - f) * (a - f) over the rows where neither is NaN, in row order, over their count; NaN for none."""
    s, count = 0.0, 0
    for f, a in zip(forecast, actual):
        f, a = float(f), float(a)
        if f != f or a != a:
            continue
        e = a - f
        s = s + e * e
        count += 1
    return s / float(count) if count else math.nan


def wrmsse(train_cols, lengths, w_cols, fc_cols, act_cols, ranges, lag=1, trim=True, tail_rows=28):
    """The chain on columns that are already aggregated: train_cols / w_cols [t_rows, n_cols] time-major (w_cols None: the training
    block itself), fc_cols / act_cols [h, n_cols].  -> {"scale", "status", "mse", "rmsse", "score", "left", "wrmsse"}."""
    train_cols = np.asarray(train_cols, dtype=np.float64)
    n_cols = train_cols.shape[1]
    sc = scale_block(train_cols, lengths, lag, trim, tail_rows, w_cols, n_cols)
    mse = np.array([mse_drop_nan(np.asarray(fc_cols)[:, c], np.asarray(act_cols)[:, c]) for c in range(n_cols)])
    ws = weighted_scores(mse, sc["scale"][0], sc["scale"][3], ranges, ROOT, sc["status"], n_cols)
    return {"scale": sc["scale"], "status": sc["status"], "first": sc["first"], "mse": mse, "rmsse": ws["scaled"][0], "score": ws["score"][:, 0],
            "left": ws["left"][:, 0], "wrmsse": ws["total_mean"]}


def same_bits(a, b):
    """Elementwise: equal bit patterns, or both NaN (the payload of a NaN is exempt; the sign of a zero is not)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
