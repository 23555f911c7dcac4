"""Seeded inputs of the selection tests (tests/test_select_cpu.py, tests/test_gpu_select.py), with the properties the tests assert of
them before they compare anything: a generator that degenerates cannot pass."""
import numpy as np

import select_ref as R

NAN = float("nan")
INF = float("inf")


def loser_of(M):
    """The method that wins nothing in a score table (none when there is only one method)."""
    return M - 1 if M >= 2 else -1


def score_table(N, M, seed):
    """scores fp64 [M, ld] (ld = N rounded up to 64, the padding columns hold a sentinel) and status int32 [M, N].  Every method but
    loser_of(M) is the designated winner of every (M - 1)-th series; on top of that come exact ties (a two-way tie on 10 % of the
    series, a three-way tie and a -0.0 / +0.0 tie among them), NaN scores, +inf scores, status-1 entries whose score would have won,
    and series without an admissible method."""
    rng = np.random.default_rng(seed)
    ld = (N + 63) // 64 * 64
    scores = np.full((M, ld), -777.0)
    scores[:, :N] = rng.uniform(1.0, 2.0, size=(M, N))
    status = np.zeros((M, N), dtype=np.int32)
    lose = loser_of(M)
    K = M - 1 if lose >= 0 else M                          # the methods that may win
    if lose >= 0:
        scores[lose, :N] += 10.0
    for s in range(N):
        d = s % K
        scores[d, s] = 0.5
        if s // K == 1:
            continue                                       # one plain round: every method that may win does win something
        if M >= 3:
            if s % 10 == 0:
                scores[(d + 1) % K, s] = 0.5               # a two-way tie: the lower index wins
            if s % 20 == 5:
                scores[0, s] = scores[1, s] = scores[2, s] = 0.25      # three-way
            if s % 30 == 7:
                scores[0, s], scores[1, s] = 0.0, -0.0     # -0.0 is no smaller than +0.0: method 0 wins
        if s % 7 == 3:
            scores[d, s] = NAN
        if s % 9 == 4:
            scores[d, s], status[d, s] = 1e-4, 1           # would win if the status were ignored
        if s % 11 == 6:
            scores[(d + 1) % M, s] = INF
        if s % 13 == 8:
            scores[:, s] = INF                             # all equal: method 0 (or the first admissible)
            if M >= 2:
                status[0, s] = 2
        if s % 17 == 9:
            scores[:, s] = NAN                             # nothing admissible ...
        if s % 34 == 12:
            status[:, s] = 1                               # ... by status
    if lose >= 0:                                          # where only the loser was left, it is not admissible either
        winner = R.choose(scores[:, :N].tolist(), status.tolist(), -1)[0]
        for s in range(N):
            if winner[s] == lose:
                status[lose, s] = 1
    return scores, status


def table_properties(scores, status, N, M, fallback):
    """What test_gpu_select asserts of a table before it compares: counts from the restatement."""
    winner, best, ff, offsets, members = R.choose(scores[:, :N].tolist(), status.tolist(), fallback)
    ties = three = zero_tie = 0
    for s in range(N):
        adm = [scores[m, s] for m in range(M) if R.admissible(scores[m, s], status[m, s])]
        if not adm:
            continue
        lo = min(adm)
        k = sum(1 for v in adm if v == lo)
        ties += k >= 2
        three += k >= 3
        zero_tie += k >= 2 and lo == 0.0 and len({np.signbit(v) for v in adm if v == 0.0}) == 2
    wins = [offsets[m + 1] - offsets[m] for m in range(M)]
    return {"winner": winner, "best": best, "from_fallback": ff, "offsets": offsets, "members": members, "wins": wins, "ties": ties,
            "three_way": three, "zero_tie": zero_tie, "n_nan": int(np.isnan(scores[:, :N]).sum()), "n_inf": int(np.isinf(scores[:, :N]).sum()),
            "n_status": int((status != 0).sum()), "n_none": sum(1 for s in range(N) if best[s] != best[s])}


def combine_case(R_rows, h, M, group_div, seed):
    """M blocks [R, h], status [M, R], scores [M, G] and winner [G].  Row classes by r % 8: 0 no live member, 1 exactly one, 2 exactly
    two (the even-count median), 3 all M live without a NaN; the other rows have random statuses and NaN cells inside live members.
    Groups g % 5 == 1 hold a zero score (g % 10 == 1: two of them, +0.0 and -0.0); some scores are NaN or +inf."""
    rng = np.random.default_rng(seed)
    G = (R_rows + group_div - 1) // group_div
    blocks = np.round(rng.normal(10.0, 5.0, size=(M, R_rows, h)), 3)
    status = np.zeros((M, R_rows), dtype=np.int32)
    for r in range(R_rows):
        c = r % 8
        if c == 0:
            status[:, r] = 1 + (r % 3)
        elif c == 1:
            status[:, r] = 1
            status[r % M, r] = 0
        elif c == 2 and M >= 2:
            status[:, r] = 1
            status[r % M, r] = status[(r + 5) % M, r] = 0
        elif c == 3:
            pass
        else:
            status[:, r] = (rng.random(M) < 0.3).astype(np.int32) * 3
            blocks[:, r, :][rng.random((M, h)) < 0.15] = NAN
    blocks[blocks == 0.0] = 1.0
    if R_rows > 4:
        blocks[0, 4, 0], blocks[M - 1, 4, 0] = 0.0, -0.0   # the total order of the median: -0.0 below +0.0
    scores = rng.uniform(0.5, 3.0, size=(M, G))
    scores[rng.random((M, G)) < 0.1] = NAN
    scores[rng.random((M, G)) < 0.05] = INF
    for g in range(G):
        if g % 5 == 1:
            scores[min(2, M - 1), g] = 0.0
        if g % 10 == 1 and M > 5:
            scores[5, g] = -0.0
    winner = rng.integers(-1, M, size=G).astype(np.int32)
    return blocks, status, scores, winner
