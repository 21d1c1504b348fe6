"""Restatement of the held-out-edge definitions of include/gmeta_hip.h (gm_store_without_edges, gm_store_split_edges) in numpy / pure Python on the oracle's
lowbias32 / sample_salt.  A graph is its in-edge CSR (ptr int64 [N + 1], idx int32 [E], w float32 [E] or None): row v lists the sources of v's in-edges in stored
order (GraphStore.host_csr / host_weights).  The GPU tests compare bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gmeta_oracle as orc      # noqa: E402

TAG = 0x53504C54


def pair_keys(N, pairs):
    """canonical keys min * N + max of [m, 2] pairs: sorted, unique int64"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.unique(np.minimum(p[:, 0], p[:, 1]) * N + np.maximum(p[:, 0], p[:, 1]))


def out_csr(ptr, idx, w=None):
    """The by-source CSR the store derives from an in-CSR: a stable counting sort by source, so a row's destinations keep the in-CSR's (ascending
    destination) order and a weight travels with its edge."""
    N = len(ptr) - 1
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(ptr))
    order = np.argsort(np.asarray(idx, np.int64), kind='stable')
    optr = np.zeros(N + 1, np.int64)
    optr[1:] = np.cumsum(np.bincount(np.asarray(idx, np.int64), minlength=N))
    return optr, dst[order].astype(np.int32), None if w is None else np.asarray(w, np.float32)[order]


def filter_in_csr(ptr, idx, w, keys):
    """The in-CSR with every entry whose canonical pair is in `keys` deleted and the stored order otherwise kept."""
    N = len(ptr) - 1
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(ptr))
    src = np.asarray(idx, np.int64)
    keep = ~np.isin(np.minimum(src, dst) * N + np.maximum(src, dst), np.asarray(keys, np.int64))
    nptr = np.zeros(N + 1, np.int64)
    nptr[1:] = np.cumsum(np.bincount(dst[keep], minlength=N))
    return nptr, np.ascontiguousarray(np.asarray(idx, np.int32)[keep]), None if w is None else np.ascontiguousarray(np.asarray(w, np.float32)[keep])


def without_edges(graphs, keys):
    """graphs: [(ptr, idx, w)], keys: one sorted key list per graph -> per graph {'in': (ptr, idx, w), 'out': (ptr, idx, w)} of the derived store, and its
    symmetric flag: at least one edge, and the two orientations equal word for word in every graph (what gm_store_create decides on its staging arrays)."""
    out, sym, edges = [], True, 0
    for (ptr, idx, w), k in zip(graphs, keys):
        a = filter_in_csr(ptr, idx, w, k)
        b = out_csr(*a)
        out.append({'in': a, 'out': b})
        edges += len(a[1])
        sym = sym and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (w is None or np.array_equal(a[2], b[2]))
    return out, bool(sym and edges > 0)


def edge_list(ptr, idx):
    """(src, dst) of an in-CSR, in stored order"""
    return np.asarray(idx, np.int64), np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))


def neighbour_rows(ptr, idx):
    """The neighbour index: per node the ascending distinct neighbours in either direction, itself aside."""
    N = len(ptr) - 1
    rows = [set() for _ in range(N)]
    src, dst = edge_list(ptr, idx)
    for a, b in zip(src.tolist(), dst.tolist()):
        if a != b:
            rows[a].add(b); rows[b].add(a)
    return [sorted(r) for r in rows]


def thresholds(val, test):
    """floor(fraction * 2^32) in exact arithmetic -> (t_test, t_val)"""
    from fractions import Fraction
    fv, ft = Fraction(val), Fraction(test)
    return int(ft * 2 ** 32), int((ft + fv) * 2 ** 32)


def link_hash(s0, u, v):
    with np.errstate(over='ignore'):
        return int(orc.lowbias32(orc.lowbias32(np.uint32((int(s0) + int(u)) & 0xffffffff)) + np.uint32(v)))


def split_edges(ptr, idx, g, seed, t_test, t_val):
    """-> (pairs int64 [n, 2] ascending by u * N + v, classes uint8 [n], counts (links, val, test)): the walk over the distinct-neighbour rows, one link at a time."""
    assert 0 <= t_test <= t_val <= 2 ** 32
    s0 = int(orc.sample_salt(int(seed), int(g), TAG, 0))
    pairs, cls, links = [], [], 0
    for u, row in enumerate(neighbour_rows(ptr, idx)):
        for v in row:
            if u < v:
                links += 1
                h = link_hash(s0, u, v)
                c = 2 if h < t_test else 1 if h < t_val else 0
                if c:
                    pairs.append((u, v)); cls.append(c)
    cls = np.asarray(cls, np.uint8)
    return np.asarray(pairs, np.int64).reshape(-1, 2), cls, (links, int((cls == 1).sum()), int((cls == 2).sum()))


def multigraph(N, E, rng, loops=3, isolated=3, weighted=False):
    """A directed multigraph in the tests' shape: parallel edges, self loops, one-directional edges, pairs stored in both directions and `isolated` nodes without
    any edge (the last ids) -> (N, src, dst, w or None)."""
    M = N - isolated
    a, b = rng.integers(0, M, E), rng.integers(0, M, E)
    both = rng.random(E) < 0.5                                   # half of the pairs in both directions, the rest one-directional
    twice = rng.random(E) < 0.15                                 # parallel copies
    src = np.concatenate([a, b[both], a[twice], np.arange(loops)])
    dst = np.concatenate([b, a[both], b[twice], np.arange(loops)])
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    w = (rng.integers(1, 9, len(src)) / 4.0).astype(np.float32) if weighted else None
    return N, src.astype(np.int64), dst.astype(np.int64), w
