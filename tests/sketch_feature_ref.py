"""Restatement of gm_sketch_pair_features (THE definition is in include/gmeta_hip.h): the structure columns of a BUDDY predictor from the integers of
gm_sketch_pair_counts, pair by pair and cell by cell in plain Python floats (IEEE double, every operation rounded once) -- written as loops over one pair, so
that it shares no code and no summation order with the vectorised numpy chain of gmeta_amd.heuristics (hll_cardinality, sketch_intersections,
sketch_distance_profile, sketch_profile_features), which test_sketch_feature_restatement.py holds it against.

The bar of the GPU tests, and where it comes from.  Let M = max(n_nodes, the largest card value (ball or union estimate) of the pair).
  - every C[a][b] is at most its union's card (match <= K), every ball size is a card: all terms are of magnitude <= M;
  - a cell of T is reached through fewer than 2^7 roundings (at H = 4: 3 subtractions per inner cell, 6 per edge cell, 35 additions and the inner ones' for
    the corner, one more for P + P^T) on sums of fewer than 2^6 terms of magnitude <= M: its absolute error is below 2^7 * 2^6 * 2^-53 M = 2^-40 M, whatever
    the order the sums are taken in;
  - max(., 0) and log1p on [0, inf) are 1-Lipschitz, so the column inherits that absolute error; the device's log and log1p are within a few fp64 ulp (a
    relative 2^-50, far below the next term); a linear-count card moves by m * (a few ulp of log) <= 2^-40 M as well;
  - the cast to float32 adds a relative 2^-24.
  BAR:  |dev - ref| <= 2^-23 |ref| + 2^-39 M  per cell, none left out  (within_bar).
The two sides must take the same branch of card.  That is a condition on the INPUTS, not on the device: branch_margin gives the smallest |est - 2.5 m| / m over
every entry of the inputs, and the tests assert on the reference alone that it is at least 1e-9 (an fp64 rounding of est is below 2^-50 of it)."""
import math

import numpy as np

ALPHA = {16: 0.673, 32: 0.697, 64: 0.709}
BRANCH_MARGIN = 1e-9


def alpha_of(p):
    m = float(1 << p)
    return ALPHA.get(1 << p, 0.7213 / (1.0 + 1.079 / m))


def raw_estimate(zsum, p):
    """est of card: ((alpha * m) * m) / (zsum / 2^32), 0.0 where zsum == 0"""
    m = float(1 << p)
    s = float(int(zsum)) / 4294967296.0
    return alpha_of(p) * m * m / s if s > 0.0 else 0.0


def card(zeros, zsum, p):
    """-> (value, branch): branch 'zero' (zsum == 0), 'linear' (m log(m / zeros)) or 'raw'"""
    m = float(1 << p)
    if int(zsum) == 0:
        return 0.0, 'zero'
    est = raw_estimate(zsum, p)
    if est <= 2.5 * m and int(zeros) > 0:
        return m * math.log(m / float(int(zeros))), 'linear'
    return est, 'raw'


def table(counts, balls, n_nodes, p, k):
    """One pair: counts int64 [L, L, 3], balls int64 [2, L, 2] -> (P as a list of L + 1 lists of L + 1 floats, the pair's largest card value, the set of card
    branches taken)"""
    L = len(counts)
    big, branches = 0.0, set()

    def est(zeros, zsum):
        nonlocal big
        v, br = card(zeros, zsum, p)
        big = max(big, v)
        branches.add(br)
        return v

    C = [[float(int(counts[a][b][0])) / float(int(k)) * est(counts[a][b][1], counts[a][b][2]) for b in range(L)] for a in range(L)]
    size = [[est(balls[side][a][0], balls[side][a][1]) for a in range(L)] for side in range(2)]
    P = [[0.0] * (L + 1) for _ in range(L + 1)]
    for a in range(L):
        for b in range(L):
            up = C[a - 1][b] if a else 0.0
            left = C[a][b - 1] if b else 0.0
            diag = C[a - 1][b - 1] if a and b else 0.0
            P[a][b] = (C[a][b] - up) - (left - diag)
    for i in range(L):
        row = col = 0.0
        for j in range(L):
            row = row + P[i][j]
            col = col + P[j][i]
        P[i][L] = (size[0][i] - (size[0][i - 1] if i else 0.0)) - row
        P[L][i] = (size[1][i] - (size[1][i - 1] if i else 0.0)) - col
    total = 0.0
    for a in range(L + 1):
        for b in range(L + 1):
            if (a, b) != (L, L):
                total = total + P[a][b]
    P[L][L] = float(int(n_nodes)) - total
    return P, big, branches


def features(counts, balls, pairs, n_nodes, p, k, symmetric=True):
    """The columns of every pair: counts int64 [n, L, L, 3], balls int64 [n, 2, L, 2] (the canonical pair's, as pair_counts gives them), pairs [n, 2] in the
    CALLER'S orientation -> (float64 [n, (L + 1)^2] BEFORE the cast to float32, M float64 [n] = max(n_nodes, the pair's largest card value), the set of card
    branches met)"""
    counts, balls = np.asarray(counts, np.int64), np.asarray(balls, np.int64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n, L = len(counts), counts.shape[1]
    W = L + 1
    out = np.zeros((n, W * W), np.float64)
    M = np.zeros(n, np.float64)
    met = set()
    for e in range(n):
        P, big, br = table(counts[e].tolist(), balls[e].tolist(), n_nodes, p, k)
        met |= br
        M[e] = max(float(n_nodes), big)
        forward = int(pairs[e, 0]) <= int(pairs[e, 1])
        for a in range(W):
            for b in range(W):
                t = P[a][b] + P[b][a] if symmetric else (P[a][b] if forward else P[b][a])
                out[e, a * W + b] = math.log1p(t if t > 0.0 else 0.0)
    return out, M, met


def features_many(counts, balls, pairs, n_nodes, p, k, symmetric=True):
    """`features` for many pairs at once: the SAME chain, cell by cell and term by term in the same order, each Python float replaced by a float64 array over
    the pairs (element-wise IEEE operations: the same roundings; only numpy's log / log1p may differ from math's in the last place).  For the GPU tests, which
    take every ordered pair of a graph.  -> (float64 [n, (L + 1)^2], M [n], the unclipped tables P float64 [n, L + 1, L + 1], zeros-is-0 / linear / raw masks'
    any() as a dict)"""
    counts, balls = np.asarray(counts, np.int64), np.asarray(balls, np.int64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n, L = len(counts), counts.shape[1]
    W = L + 1
    m = float(1 << p)
    alpha = alpha_of(p)
    big = np.zeros(n, np.float64)
    met = {'zero': False, 'linear': False, 'raw': False, 'raw_no_zero_register': False}

    def est(zeros, zsum):
        nonlocal big
        z = zeros.astype(np.float64)
        s = zsum.astype(np.float64) / 4294967296.0
        live = zsum != 0
        raw = alpha * m * m / np.where(live, s, 1.0)
        lin = live & (raw <= 2.5 * m) & (zeros > 0)
        v = np.where(live, np.where(lin, m * np.log(m / np.where(zeros > 0, z, 1.0)), raw), 0.0)
        big = np.maximum(big, v)
        met['zero'] |= bool((~live).any()); met['linear'] |= bool(lin.any()); met['raw'] |= bool((live & ~lin).any())
        met['raw_no_zero_register'] |= bool((live & (zeros == 0)).any())
        return v

    C = [[counts[:, a, b, 0].astype(np.float64) / float(int(k)) * est(counts[:, a, b, 1], counts[:, a, b, 2]) for b in range(L)] for a in range(L)]
    size = [[est(balls[:, side, a, 0], balls[:, side, a, 1]) for a in range(L)] for side in range(2)]
    zero = np.zeros(n, np.float64)
    P = [[zero] * W for _ in range(W)]
    for a in range(L):
        for b in range(L):
            up = C[a - 1][b] if a else zero
            left = C[a][b - 1] if b else zero
            diag = C[a - 1][b - 1] if a and b else zero
            P[a][b] = (C[a][b] - up) - (left - diag)
    for i in range(L):
        row, col = zero, zero
        for j in range(L):
            row = row + P[i][j]
            col = col + P[j][i]
        P[i][L] = (size[0][i] - (size[0][i - 1] if i else zero)) - row
        P[L][i] = (size[1][i] - (size[1][i - 1] if i else zero)) - col
    total = zero
    for a in range(W):
        for b in range(W):
            if (a, b) != (L, L):
                total = total + P[a][b]
    P[L][L] = float(int(n_nodes)) - total
    forward = pairs[:, 0] <= pairs[:, 1]
    out = np.zeros((n, W * W), np.float64)
    for a in range(W):
        for b in range(W):
            t = P[a][b] + P[b][a] if symmetric else np.where(forward, P[a][b], P[b][a])
            out[:, a * W + b] = np.log1p(np.where(t > 0.0, t, 0.0))
    return out, np.maximum(float(n_nodes), big), np.stack([np.stack(r, 1) for r in P], 1), met


def tables(counts, balls, n_nodes, p, k):
    """float64 [n, L + 1, L + 1]: P of every pair (not clipped, not oriented)"""
    return np.array([table(c, b, n_nodes, p, k)[0] for c, b in zip(np.asarray(counts).tolist(), np.asarray(balls).tolist())], np.float64).reshape(
        len(counts), np.shape(counts)[1] + 1, np.shape(counts)[1] + 1)


def branch_margin(counts, balls, p):
    """The smallest |est - 2.5 m| / m over every entry with zsum != 0 (inf if there is none): how far the inputs stay from the switch of card"""
    m = float(1 << p)
    c, b = np.asarray(counts, np.int64), np.asarray(balls, np.int64)
    zs = np.concatenate([c[..., 2].reshape(-1), b[..., 1].reshape(-1)])
    zs = zs[zs != 0]
    if not len(zs):
        return float('inf')
    est = alpha_of(p) * m * m / (zs.astype(np.float64) / 4294967296.0)          # raw_estimate, element-wise
    return float((np.abs(est - 2.5 * m) / m).min())


def bar(want, M):
    """float64, the shape of `want`: 2^-23 |want| + 2^-39 M, M per row"""
    return 2.0 ** -23 * np.abs(want) + 2.0 ** -39 * np.asarray(M, np.float64)[:, None]


def within_bar(got, want, M):
    """-> (every cell within the bar, the worst |got - want| / bar)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ratio = np.abs(got - want) / bar(want, M)
    return bool((ratio <= 1.0).all()) and got.shape == want.shape, float(ratio.max()) if ratio.size else 0.0
