"""Restatement of the pair-score definition of include/gmeta_hip.h (gm_store_pair_scores), literally: Python sets for the neighbourhoods, one pair at a
time, fp64 sums.  Pure numpy / math.  The GPU tests hold the device result against it: cn and pref_attachment equal, the other three within the
tolerances the issue derives (tests/test_hip_pair_scores.py)."""
import math

import numpy as np

COLS = ('cn', 'jaccard', 'adamic_adar', 'resource_allocation', 'pref_attachment')
MASK_TARGET = 1


def neighbourhoods(N, src, dst):
    """Gamma(x) = { z != x : an edge x -> z or z -> x }, as a list of sets: distinct nodes, no self loops, weights ignored."""
    nb = [set() for _ in range(N)]
    for u, v in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if u != v:
            nb[u].add(v); nb[v].add(u)
    return nb


def degrees(N, src, dst):
    return np.array([len(s) for s in neighbourhoods(N, src, dst)], np.int32)


def w_aa(deg):
    """1 / ln(deg) for deg >= 2, else 0: computed in double, rounded once to fp32 (returned as the double that fp32 value is)."""
    return float(np.float32(1.0 / math.log(deg))) if deg >= 2 else 0.0


def w_ra(deg):
    return float(np.float32(1.0 / deg)) if deg >= 1 else 0.0


def pair_scores(N, src, dst, pairs, flags=0, nb=None):
    """-> float64 [n, 5] (the exact columns cn and pref_attachment hold integers; the caller rounds to fp32 where it compares for equality)."""
    nb = neighbourhoods(N, src, dst) if nb is None else nb
    out = np.zeros((len(pairs), 5), np.float64)
    for k, (a, b) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2).tolist()):
        if not (0 <= a < N and 0 <= b < N):
            continue                                                        # a node outside the graph: five zeros
        a, b = min(a, b), max(a, b)
        da, db = len(nb[a]), len(nb[b])
        I = nb[a] & nb[b]
        if a != b:
            assert a not in I and b not in I
            if (flags & MASK_TARGET) and b in nb[a]:
                da, db = da - 1, db - 1
            U = da + db - len(I)
        else:
            assert I == nb[a]
            U = len(nb[a])
        out[k, 0] = len(I)
        out[k, 1] = len(I) / U if U else 0.0
        out[k, 2] = math.fsum(w_aa(len(nb[z])) for z in I)
        out[k, 3] = math.fsum(w_ra(len(nb[z])) for z in I)
        out[k, 4] = float(np.float32(da * db))                              # (float)((int64) da * db): the integer rounded once to fp32
    return out


def auc_by_pair_count(scores, labels):
    """ROC AUC by its definition, O(n^2): over all (positive, negative) pairs, 1 where the positive scores higher, 1/2 on a tie."""
    s = np.asarray(scores, np.float64); y = np.asarray(labels).astype(np.int64)
    pos, neg = s[y == 1], s[y == 0]
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg)))


# ---------------------------------------------------------------------------------------------------- shared cases
PLANTED_ROWS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129, 3000)


def planted_case():
    """A directed graph whose nodes 0 .. 12 have Gamma rows of exactly PLANTED_ROWS[k] entries (the lengths around every lane width, and one hub row), drawn
    from a shared pool so that the rows overlap; edges in a random direction, some doubled, and a few among the planted nodes themselves.
    -> (N, src, dst, planted node ids)."""
    rng = np.random.default_rng(5)
    P = len(PLANTED_ROWS)
    N = P + 3200
    pool = np.arange(P, N)
    src, dst = [], []
    # edges among the planted nodes first (they count towards the row lengths): 3-4, 5-6, 9-12, 11-12, 10-11
    among = [(3, 4), (5, 6), (9, 12), (11, 12), (10, 11)]
    have = {k: set() for k in range(P)}
    for a, b in among:
        have[a].add(b); have[b].add(a)
        src.append(a); dst.append(b)
    for k, want in enumerate(PLANTED_ROWS):
        need = want - len(have[k])
        assert need >= 0
        # overlapping picks: a window of the pool that starts at 0 for every row, so shorter rows are subsets of longer ones up to a random thinning
        span = min(len(pool), max(need, 2 * need))
        pick = np.sort(rng.choice(pool[:span], need, replace=False)) if need else np.zeros(0, np.int64)
        for z in pick.tolist():
            if rng.random() < 0.5:
                src.append(k); dst.append(z)
            else:
                src.append(z); dst.append(k)
            if rng.random() < 0.1:                                          # a parallel copy, or the reverse edge: still one neighbour
                u, v = (src[-1], dst[-1]) if rng.random() < 0.5 else (dst[-1], src[-1])
                src.append(u); dst.append(v)
    src.extend([0, 2, 12]); dst.extend([0, 2, 12])                          # self loops: never a neighbour (node 0 stays isolated)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    deg = degrees(N, src, dst)
    assert tuple(deg[:P].tolist()) == PLANTED_ROWS, deg[:P]
    return N, src, dst, list(range(P))
