"""Restatement of the rooted-PageRank definition of include/gmeta_hip.h (gm_store_rooted_pagerank, gm_store_pair_pagerank), literally and in float64: the
neighbourhoods are the Python sets of pair_score_ref, a masked column actually removes its edge from the two sets, a and b are the fp32-rounded values the
definition names, and one iteration is one np.bincount over the (row, neighbour) entries.  The GPU tests hold the fp32 device result against it within a
bound derived from the number of roundings."""
import numpy as np

import pair_score_ref

MASK_TARGET = 1


def constants(alpha):
    """(a, b) of the definition: a = (float)alpha, b = 1.0f - a in fp32, as float64 numbers."""
    a = np.float32(alpha)
    return float(a), float(np.float32(1.0) - a)


def column(N, nb, s, x, alpha, iters):
    """float64 [N]: pi_(s, x) -- the walk from s in the graph without the edge {s, x} (x = -1, x == s or x not in G(s): the whole graph)."""
    if 0 <= x < N and x != s and x in nb[s]:
        nb = list(nb)
        nb[s] = nb[s] - {x}
        nb[x] = nb[x] - {s}
    deg = np.array([len(r) for r in nb], np.int64)
    rows = np.repeat(np.arange(N), deg)
    idx = np.array([z for r in nb for z in sorted(r)], np.int64)
    a, b = constants(alpha)
    lone = deg == 0
    p = np.zeros(N, np.float64)
    p[s] = 1.0
    for _ in range(int(iters)):
        q = p / np.maximum(deg, 1)
        m = np.bincount(rows, weights=q[idx], minlength=N)
        m[lone] = p[lone]                                                     # a node without neighbours keeps its mass
        p = b * m
        p[s] += a
    return p


def rooted_pagerank(N, src, dst, sources, alpha=0.15, iters=20, nb=None):
    """-> float64 [m, N]: row r = pi_(sources[r], -1); a source outside [0, N) gives a row of zeros."""
    nb = pair_score_ref.neighbourhoods(N, src, dst) if nb is None else nb
    sources = np.asarray(sources, np.int64).reshape(-1)
    out = np.zeros((len(sources), N), np.float64)
    done = {}
    for r, s in enumerate(sources.tolist()):
        if not 0 <= s < N:
            continue
        if s not in done:
            done[s] = column(N, nb, s, -1, alpha, iters)
        out[r] = done[s]
    return out


def pair_pagerank(N, src, dst, pairs, flags=0, alpha=0.15, iters=20, nb=None):
    """-> float64 [n, 2]: (pi_(u,x)[v], pi_(v,x')[u]) of the canonical pair (u, v) = (min, max); x = v and x' = u with the mask flag, else -1."""
    nb = pair_score_ref.neighbourhoods(N, src, dst) if nb is None else nb
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = np.zeros((len(pairs), 2), np.float64)
    done = {}

    def col(s, x):
        if x >= 0 and (x == s or x not in nb[s]):
            x = -1                                                            # the column's graph is the whole graph: the same vector
        if (s, x) not in done:
            done[(s, x)] = column(N, nb, s, x, alpha, iters)
        return done[(s, x)]
    for k, (p, q) in enumerate(pairs.tolist()):
        if not (0 <= p < N and 0 <= q < N):
            continue                                                          # a node outside the graph: two zeros
        u, v = min(p, q), max(p, q)
        cut = bool(flags & MASK_TARGET)
        out[k, 0] = col(u, v if cut else -1)[v]
        out[k, 1] = col(v, u if cut else -1)[u]
    return out


def bound(want, iters, d_max):
    """The fp32 device result's distance from the float64 restatement, entry by entry.  Every quantity of the iteration is non-negative, so relative
    rounding errors add up and never grow: per iteration an entry passes through at most d_max + 8 roundings of 2^-24 (the rounded 1 / deg, the scale,
    d_max - 1 adds in any order, a, b, the product, the final add, slack).  The absolute term covers underflow."""
    return 1.01 * iters * (d_max + 8) * 2.0 ** -24 * np.asarray(want, np.float64) + 2.0 ** -100
