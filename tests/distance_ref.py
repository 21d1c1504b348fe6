"""Restatement of the shortest-path-distance definition of include/gmeta_hip.h (gm_store_node_distances, gm_store_pair_distance), literally: the
neighbourhoods are the Python sets of pair_score_ref, a masked column actually removes its edge from the two sets, and the search is a plain breadth-first
search with a queue -- one source at a time, no bit tricks.  Everything is an integer, so the GPU tests ask for equality."""
from collections import deque

import numpy as np

import pair_score_ref

MASK_TARGET = 1
UNREACHED = 255


def column(N, nb, s, x, max_dist):
    """uint8 [N]: d_(s, x) -- the distances from s in the graph without the edge {s, x} (x = -1, x == s or x not in G(s): the whole graph); UNREACHED where
    no path of at most max_dist edges leads."""
    assert 1 <= max_dist <= 254
    if 0 <= x < N and x != s and x in nb[s]:
        nb = list(nb)
        nb[s] = nb[s] - {x}
        nb[x] = nb[x] - {s}
    d = np.full(N, UNREACHED, np.uint8)
    d[s] = 0
    queue = deque([s])
    while queue:
        z = queue.popleft()
        if d[z] == max_dist:
            continue                                                          # its neighbours would lie beyond max_dist
        for v in nb[z]:
            if d[v] == UNREACHED:
                d[v] = d[z] + 1
                queue.append(v)
    return d


def node_distances(N, src, dst, sources, max_dist=8, nb=None):
    """-> uint8 [m, N]: row r = d_(sources[r], -1); a source outside [0, N) gives a row of UNREACHED."""
    nb = pair_score_ref.neighbourhoods(N, src, dst) if nb is None else nb
    sources = np.asarray(sources, np.int64).reshape(-1)
    out = np.full((len(sources), N), UNREACHED, np.uint8)
    done = {}
    for r, s in enumerate(sources.tolist()):
        if not 0 <= s < N:
            continue
        if s not in done:
            done[s] = column(N, nb, s, -1, max_dist)
        out[r] = done[s]
    return out


def pair_distance(N, src, dst, pairs, flags=0, max_dist=8, nb=None):
    """-> uint8 [n]: d_(u,x)[v] of the canonical pair (u, v) = (min, max); x = v with the mask flag, else -1.  A node outside the graph: UNREACHED."""
    nb = pair_score_ref.neighbourhoods(N, src, dst) if nb is None else nb
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = np.full(len(pairs), UNREACHED, np.uint8)
    done = {}
    for k, (p, q) in enumerate(pairs.tolist()):
        if not (0 <= p < N and 0 <= q < N):
            continue
        u, v = min(p, q), max(p, q)
        x = v if flags & MASK_TARGET and u != v and v in nb[u] else -1        # otherwise the column's graph is the whole graph: the same vector
        if (u, x) not in done:
            done[(u, x)] = column(N, nb, u, x, max_dist)
        out[k] = done[(u, x)][v]
    return out


def chain_case():
    """331 nodes, undirected edges given once in a random direction, N no multiple of 64:
        0 .. 259      a path of 260 nodes: distances reach 259, every path edge is a bridge
        260 .. 326    a cycle of 67 nodes hung on path node 100 by the one edge {100, 260}: a masked cycle edge has distance 66
        327           a pendant of path node 0
        328           a pendant of cycle node 290
        329, 330      isolated
    -> (N, src, dst, L) with L the cycle's length."""
    N, L = 331, 67
    e = [(k, k + 1) for k in range(259)]
    e += [(260 + k, 260 + (k + 1) % L) for k in range(L)]
    e += [(100, 260), (0, 327), (290, 328)]
    rng = np.random.default_rng(5)
    e = [(a, b) if rng.integers(2) else (b, a) for a, b in e]
    return N, np.array([a for a, _ in e], np.int64), np.array([b for _, b in e], np.int64), L
