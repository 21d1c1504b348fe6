"""Restatement of the PageRank-candidate definition of include/gmeta_hip.h (gm_store_pagerank_candidates), literally: the candidate set R(a), the ranking as
the descending order of the integer key the definition names (candidate_ref.keys: the key of gm_store_pair_candidates) and the padding, applied to a GIVEN
[m, N] score matrix plus the neighbourhoods of pair_score_ref.neighbourhoods.  The scores are NOT restated here: the definition makes them the bits of
gm_store_rooted_pagerank's rows, so the GPU tests feed the device's own rows (which that export's tests hold against float64), and pagerank_ref's float64
rows where a tolerance is derived.  Pure numpy."""
import numpy as np

import candidate_ref

MAX_K = candidate_ref.MAX_K


def candidates(N, nb, a, row):
    """R(a) = { w : w != a, w not in G(a), row[w] > 0 } as an ascending int64 array; empty for a source outside [0, N).  For a float32 row `> 0` is the test
    on the bits: every entry is +0 or a positive finite number."""
    a = int(a)
    if not 0 <= a < N:
        return np.zeros(0, np.int64)
    row = np.asarray(row)
    assert row.shape == (N,) and not (row < 0).any()
    keep = row > 0
    keep[a] = False
    keep[sorted(nb[a])] = False
    return np.nonzero(keep)[0].astype(np.int64)


def top_k(N, nb, sources, rows, k):
    """sources [m], rows [m, N] float32 (row r: the scores seen from sources[r]) -> (nodes int64 [m, k], scores float32 [m, k], totals int64 [m]): row r
    holds the first min(k, |R|) candidates in descending key order, then -1 / 0.0."""
    assert 1 <= k <= MAX_K
    sources = np.asarray(sources, np.int64).reshape(-1)
    rows = np.ascontiguousarray(rows, np.float32).reshape(len(sources), N)
    m = len(sources)
    nodes = np.full((m, k), -1, np.int64); sc = np.zeros((m, k), np.float32); tot = np.zeros(m, np.int64)
    for r, a in enumerate(sources.tolist()):
        c = candidates(N, nb, a, rows[r])
        tot[r] = len(c)
        if len(c):
            nodes[r], sc[r] = candidate_ref.rank(c, rows[r][c], k)
    return nodes, sc, tot


def path_case(n=12):
    """0 - 1 - ... - (n - 1)."""
    return n, np.arange(n - 1, dtype=np.int64), np.arange(1, n, dtype=np.int64)


def star_case(leaves=70, tail=4):
    """Node 0 joined to the leaves 1 .. leaves (more than a wave of them), and a tail leaves + 1 .. leaves + tail hanging off leaf 1 in a line.  Seen from a
    leaf other than 1, every other such leaf is reached by the same walks through the centre: the same expression, the same fp32 bits."""
    src = [0] * leaves + [1] + list(range(leaves + 1, leaves + tail))
    dst = list(range(1, leaves + 1)) + [leaves + 1] + list(range(leaves + 2, leaves + tail + 1))
    return leaves + tail + 1, np.asarray(src, np.int64), np.asarray(dst, np.int64)


def random_connected_case(N=3001, extra=6000, seed=77):
    """A random spanning tree (node v joined to a random earlier node) plus `extra` random edges: connected, mean distinct degree about 2 (N - 1 + extra) / N."""
    rng = np.random.default_rng(seed)
    v = np.arange(1, N, dtype=np.int64)
    u = (rng.random(N - 1) * v).astype(np.int64)
    return N, np.concatenate([u, rng.integers(0, N, extra)]).astype(np.int64), np.concatenate([v, rng.integers(0, N, extra)]).astype(np.int64)
