"""Pure-Python restatement of the selection entries (include/anofox_fcst_hip.h block 8, DESIGN.md section 3 "Selection"): the winner
of every series, the stable partition by winner, and the combination of the methods' forecasts.  Python floats are IEEE doubles and
every sum below runs serially in method order, so the results are the contract's bits.  It shares nothing with the product or with
oracle/."""
import math
import struct

NAN = float("nan")
MODES = ("pick", "mean", "median", "inverse_score")
MAX_METHODS = 16


def admissible(score, status):
    return status == 0 and score == score


def choose(scores, status, fallback):
    """scores[m][s], status[m][s] -> (winner [N], best_score [N], from_fallback [N], offsets [M + 1], members).  The winner is the
    admissible method with the smallest score, the lowest m among equals (-0.0 == +0.0); `fallback` when none is admissible."""
    M = len(scores)
    N = len(scores[0]) if M else 0
    winner, best, ff = [], [], []
    for s in range(N):
        w, b = -1, NAN
        for m in range(M):
            x = scores[m][s]
            if not admissible(x, status[m][s]):
                continue
            if w < 0 or x < b:
                w, b = m, x
        if w < 0:
            winner.append(fallback)
            best.append(NAN)
            ff.append(1 if fallback >= 0 else 0)
        else:
            winner.append(w)
            best.append(b)
            ff.append(0)
    offsets, members = [0], []
    for m in range(M):
        for s in range(N):
            if winner[s] == m:
                members.append(s)
        offsets.append(len(members))
    return winner, best, ff, offsets, members


def order_key(x):
    """The total order of the bit patterns: -0.0 below +0.0 (the key of wave_sort.hpp)."""
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    return (~u & 0xFFFFFFFFFFFFFFFF) if u >> 63 else (u | 0x8000000000000000)


def _div(x, y):
    """IEEE division (Python raises on a zero divisor)."""
    if y == 0.0:
        if x != x or x == 0.0:
            return NAN
        return math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y


def combine_cell(values, status, mode, winner=None, scores=None):
    """One cell: values[m] and status[m] of the M members, winner (pick) and scores[m] (inverse_score) of the row's group."""
    M = len(values)
    if mode == "pick":
        return values[winner] if 0 <= winner < M else NAN
    live = [m for m in range(M) if status[m] == 0 and values[m] == values[m]]
    if mode == "median":
        v = sorted((values[m] for m in live), key=order_key)
        if not v:
            return NAN
        c = len(v)
        return v[c // 2] if c % 2 else (v[c // 2 - 1] + v[c // 2]) * 0.5
    if mode == "mean":
        if not live:
            return NAN
        s = 0.0
        for m in live:
            s = s + values[m]
        return s / float(len(live))
    assert mode == "inverse_score"
    part = [m for m in live if scores[m] == scores[m]]
    if not part:
        return NAN
    zero = [m for m in part if scores[m] == 0.0]
    if zero:
        s = 0.0
        for m in zero:
            s = s + values[m]
        return s / float(len(zero))
    wy, ws = 0.0, 0.0
    for m in part:
        w = _div(1.0, scores[m])
        t = w * values[m]
        wy = wy + t
        ws = ws + w
    return _div(wy, ws)


def combine(blocks, status, mode, winner=None, scores=None, group_div=1):
    """blocks[m][r][i], status[m][r], winner[g], scores[m][g], row r in group r // group_div -> (out[r][i], row_status[r])."""
    M = len(blocks)
    R = len(blocks[0])
    out, row_status = [], []
    for r in range(R):
        g = r // group_div
        row = []
        for i in range(len(blocks[0][r])):
            row.append(combine_cell([blocks[m][r][i] for m in range(M)], [status[m][r] for m in range(M)], mode,
                                    winner[g] if winner is not None else None, [scores[m][g] for m in range(M)] if scores is not None else None))
        out.append(row)
        row_status.append(0 if any(v == v for v in row) else 1)
    return out, row_status


def gather(y, lengths, members, off, n_m, ld_m):
    """y[t][s] -> (y_m[t][j], len_m[j]): column j < n_m is series members[off + j], the rest 0.0 with length 0."""
    T = len(y)
    ym = [[0.0] * ld_m for _ in range(T)]
    lm = [0] * ld_m
    for j in range(n_m):
        s = members[off + j]
        lm[j] = min(max(lengths[s], 0), T)
        for t in range(T):
            ym[t][j] = y[t][s]
    return ym, lm


def same_bits(a, b):
    """Equality of two doubles as the contract means it: equal bits, any NaN equal to any NaN."""
    if a != a or b != b:
        return a != a and b != b
    return struct.pack("<d", a) == struct.pack("<d", b)
