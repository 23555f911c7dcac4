"""The reference's matrix_profile_period, restated twice from its description (sharing nothing with oracle/):

  matrix_profile_plain   Python floats, the source's loops as they stand: for i, for j >= i + excl, for k; both strict < updates.
                         (The subsequence statistics are computed when a pair first needs them; the values are the same.)
  matrix_profile         numpy, vectorised over pairs and serial over k, reduced with a lexicographic (distance, index) minimum.

Every operation is a single IEEE operation (d * d for powi(2), math.sqrt / np.sqrt, /), so the two agree with == and the kernels
are held to the same.  The source picks among lags of equal best count by the iteration order of a hash map: both forms return the
whole SET of tied lags, and `period` is its minimum, the rule of this package.

squared_compare=True (plain form only) compares the sums before the square root.  It is NOT the source; it exists to select test
cases on which that shortcut changes an index."""
import math

import numpy as np

EPS = 2.220446049250313e-16
MIN_ROWS, MAX_M, MAX_ROWS, TILE, KCHUNK, HOME_DOUBLES = 32, 2048, 65536, 64, 16, 5504
FIGURES = ("period", "confidence", "n_motifs", "subsequence_length", "best_count", "n_tied")


class InsufficientData(Exception):
    def __init__(self, needed, got):
        super().__init__(f"Insufficient data: need at least {needed} observations, got {got}")


def subsequence(n, subsequence_length=None):
    return min(max(subsequence_length if subsequence_length else n // 10, 4), n // 4)


def exclusion(m, n_best=None):
    return max(n_best if n_best else m // 4, 1)


def profile_len(n, subsequence_length=None):
    return 0 if n < MIN_ROWS else n - subsequence(n, subsequence_length) + 1


def in_lds(n, subsequence_length=None):
    p = profile_len(n, subsequence_length)
    return n + p + (p + 1) // 2 <= HOME_DOUBLES


def _finish(mp, mpi, n, m, excl):
    finite = sorted(x for x in mp if math.isfinite(x))
    threshold = finite[len(finite) // 4] * 2.0 if len(finite) > 10 else math.inf
    counts, n_motifs = {}, 0
    for i, d in enumerate(mp):
        if d < threshold and math.isfinite(d):
            lag = abs(mpi[i] - i)
            if excl < lag < n // 2:
                counts[lag] = counts.get(lag, 0) + 1
                n_motifs += 1
    best = max(counts.values()) if counts else 0
    tied = sorted(lag for lag, c in counts.items() if c == best)
    return {"period": float(tied[0]) if tied else math.nan, "confidence": best / n_motifs if n_motifs else 0.0, "n_motifs": n_motifs,
            "subsequence_length": m, "best_count": best, "n_tied": len(tied), "tied_lags": set(tied), "mp": list(mp), "mpi": list(mpi),
            "exclusion": excl, "method": "matrix_profile"}


class _Stats:
    """mean and std of subsequence i, as the source computes them, on first use."""

    def __init__(self, v, m):
        self.v, self.m, self.seen = v, m, {}

    def __call__(self, i):
        if i not in self.seen:
            s = 0.0
            for k in range(self.m):
                s += self.v[i + k]
            mean = s / self.m
            q = 0.0
            for k in range(self.m):
                d = self.v[i + k] - mean
                q += d * d
            var = q / self.m
            sd = math.sqrt(var) if var == var else math.nan
            self.seen[i] = (mean, sd if sd >= EPS else EPS)          # f64::max returns the operand that is not NaN
        return self.seen[i]


def _dist2(v, m, stats, i, j):
    mi, si = stats(i)
    mj, sj = stats(j)
    acc = 0.0
    for k in range(m):
        zi = (v[i + k] - mi) / si
        zj = (v[j + k] - mj) / sj
        d = zi - zj
        acc += d * d
    return acc


def _setup(values, subsequence_length, n_best):
    v = [float(x) for x in values]
    n = len(v)
    if n < MIN_ROWS:
        raise InsufficientData(MIN_ROWS, n)
    m = subsequence(n, subsequence_length)
    return v, n, m, exclusion(m, n_best), n - m + 1


def matrix_profile_plain(values, subsequence_length=None, n_best=None, squared_compare=False):
    v, n, m, excl, P = _setup(values, subsequence_length, n_best)
    stats = _Stats(v, m)
    mp, mpi = [math.inf] * P, [0] * P
    for i in range(P):
        for j in range(i + excl, P):
            d = _dist2(v, m, stats, i, j)
            if not squared_compare:
                d = math.sqrt(d) if d == d else math.nan
            if d < mp[i]:
                mp[i], mpi[i] = d, j
            if d < mp[j]:
                mp[j], mpi[j] = d, i
    if squared_compare:
        mp = [math.sqrt(x) for x in mp]
    return _finish(mp, mpi, n, m, excl)


def first_minimum_profile(values, subsequence_length=None, n_best=None):
    """mp[x] as the minimum over x's admissible partners taken in ascending order with a strict <: what the source's visiting order
    amounts to."""
    v, n, m, excl, P = _setup(values, subsequence_length, n_best)
    stats = _Stats(v, m)
    mp, mpi = [math.inf] * P, [0] * P
    for x in range(P):
        for y in range(P):
            if abs(x - y) >= excl:
                d = _dist2(v, m, stats, min(x, y), max(x, y))
                d = math.sqrt(d) if d == d else math.nan
                if d < mp[x]:
                    mp[x], mpi[x] = d, y
    return mp, mpi


def matrix_profile(values, subsequence_length=None, n_best=None, rows=64):
    v, n, m, excl, P = _setup(values, subsequence_length, n_best)
    a = np.array(v)
    with np.errstate(all="ignore"):
        s = np.zeros(P)
        for k in range(m):
            s = s + a[k:k + P]
        mean = s / float(m)
        q = np.zeros(P)
        for k in range(m):
            d = a[k:k + P] - mean
            q = q + d * d
        sd = np.sqrt(q / float(m))
        sd = np.where(sd >= EPS, sd, EPS)
        mp = np.full(P, np.inf)
        idx = np.full(P, np.iinfo(np.int64).max)

        def update(where, d, partner):
            better = (d < mp[where]) | ((d == mp[where]) & (partner < idx[where]))
            mp[where] = np.where(better, d, mp[where])
            idx[where] = np.where(better, partner, idx[where])

        for i0 in range(0, P, rows):
            i1 = min(i0 + rows, P)
            j0 = i0 + excl
            if j0 >= P:
                break
            acc = np.zeros((i1 - i0, P - j0))
            tmp = np.empty_like(acc)
            for k in range(m):
                zi = (a[i0 + k:i1 + k] - mean[i0:i1]) / sd[i0:i1]
                zj = (a[j0 + k:P + k] - mean[j0:P]) / sd[j0:P]
                np.subtract(zi[:, None], zj[None, :], out=tmp)
                np.multiply(tmp, tmp, out=tmp)
                acc += tmp
            dist = np.sqrt(acc)
            ii, jj = np.arange(i0, i1)[:, None], np.arange(j0, P)[None, :]
            dist = np.where((jj - ii >= excl) & (dist < np.inf), dist, np.inf)          # a NaN and a pair inside the zone never update
            jbest = np.argmin(dist, axis=1)                                           # the first of the smallest: the smallest j
            dbest = dist[np.arange(i1 - i0), jbest]
            update(np.arange(i0, i1), dbest, np.where(dbest < np.inf, jbest + j0, idx[i0:i1]))
            ibest = np.argmin(dist, axis=0)
            dbest = dist[ibest, np.arange(P - j0)]
            update(np.arange(j0, P), dbest, np.where(dbest < np.inf, ibest + i0, idx[j0:P]))
        mpi = np.where(mp < np.inf, idx, 0)
    return _finish([float(x) for x in mp], [int(x) for x in mpi], n, m, excl)
