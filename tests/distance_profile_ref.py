"""Restatement of the joint hop-distance profile of include/gmeta_hip.h (gm_store_pair_distance_profile), literally: the two columns of a pair are the plain
breadth-first searches of distance_ref.column (a masked column actually removes its edge), capped, and the table is a count over the nodes.  Everything is an
integer, so the GPU tests ask for equality."""
import numpy as np

import distance_ref
import pair_score_ref

MASK_TARGET = 1
MAX_DIST = 7


def cap(d, max_dist):
    """cap(d) = d where d <= max_dist, else max_dist + 1: the farther nodes and the unreached ones (byte 255) alike."""
    d = np.asarray(d, np.int64)
    return np.where(d <= max_dist, d, max_dist + 1)


def profile(N, src, dst, pairs, flags=0, max_dist=3, nb=None, cols=None):
    """-> int32 [n, D + 2, D + 2]: P[a][b] = |{z : cap(d_(u,xu)[z]) == a and cap(d_(v,xv)[z]) == b}| of the canonical pair (u, v) = (min, max); xu = v, xv = u
    with the mask flag for an adjacent pair, else -1.  A node outside the graph: zeros.  A column is searched once, at 254: cap_D of the full distance is cap_D of
    the search that stops at D; `cols` (optional, a dict) keeps the searched columns of one graph across calls."""
    assert 1 <= max_dist <= MAX_DIST
    nb = pair_score_ref.neighbourhoods(N, src, dst) if nb is None else nb
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    S = max_dist + 2
    out = np.zeros((len(pairs), S, S), np.int32)
    cols = {} if cols is None else cols
    tables = {}

    def column(s, x):
        if (s, x) not in cols:
            cols[(s, x)] = distance_ref.column(N, nb, s, x, 254)
        return cap(cols[(s, x)], max_dist)
    for k, (p, q) in enumerate(pairs.tolist()):
        if not (0 <= p < N and 0 <= q < N):
            continue
        u, v = min(p, q), max(p, q)
        cut = bool(flags & MASK_TARGET) and u != v and v in nb[u]
        if (u, v) not in tables:
            a, b = column(u, v if cut else -1), column(v, u if cut else -1)
            tables[(u, v)] = np.bincount(a * S + b, minlength=S * S).reshape(S, S).astype(np.int32)
        out[k] = tables[(u, v)]
    return out


def oriented(tables, pairs):
    """The tables of profile() in the orientation of their pairs: entry [a][b] counts the nodes a hops from pairs[k][0] and b hops from pairs[k][1]."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = np.array(tables, np.int32)
    swap = pairs[:, 0] > pairs[:, 1]
    out[swap] = out[swap].transpose(0, 2, 1)
    return out


def wide_case():
    """A seeded sparse graph of N = 64 * 70 + 17 nodes, mean degree about 3: 71 node-words, more than a wave has lanes, the last one 17 bits wide.
    -> (N, src, dst)"""
    N = 64 * 70 + 17
    rng = np.random.default_rng(77)
    m = 3 * N // 2
    return N, rng.integers(0, N, m).astype(np.int64), rng.integers(0, N, m).astype(np.int64)
