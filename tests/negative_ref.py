"""Restatement of the negative-pair definition of include/gmeta_hip.h (gm_store_negative_pairs), literally: one candidate at a time, a Python set
for adjacency, a dict for the first k of every pair.  Pure numpy on the oracle's lowbias32 / sample_salt.  The GPU tests compare bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gmeta_oracle as orc      # noqa: E402

TAG = 0x6E454721
MODES = {'uniform': 0, 'two_hop': 1}


def budget(n):
    return 64 * n + 4096


def words(salt, k0, count):
    """r(k, c) = lowbias32(salt + 4 k + c), 32-bit wrap-around, for k in [k0, k0 + count): int lists [count][4]."""
    x = (int(salt) + 4 * k0 + np.arange(4 * count, dtype=np.uint64)) & np.uint64(0xffffffff)
    return orc.lowbias32(x.astype(np.uint32)).reshape(count, 4).tolist()


def pick(r, n):
    return (int(r) * int(n)) >> 32


def out_rows(N, src, dst):
    """The store's out-CSR rows: the in-CSR (stable by destination) re-grouped by source with a stable sort -- destinations in in-CSR order."""
    src = np.asarray(src, np.int64); dst = np.asarray(dst, np.int64)
    by_dst = np.argsort(dst, kind='stable')
    s, d = src[by_dst], dst[by_dst]
    by_src = np.argsort(s, kind='stable')
    s, d = s[by_src], d[by_src]
    ptr = np.searchsorted(s, np.arange(N + 1))
    return [d[ptr[a]:ptr[a + 1]].tolist() for a in range(N)]


def candidate(N, out, m, r):
    """Candidate of the random words r[0..3]: (a, w, b) -- w is None in uniform mode -- or None where a walk meets out-degree 0."""
    a = pick(r[0], N)
    if m == 0:
        return a, None, pick(r[1], N)
    if not out[a]:
        return None
    w = out[a][pick(r[1], len(out[a]))]
    if not out[w]:
        return None
    return a, w, out[w][pick(r[2], len(out[w]))]


def negative_pairs(N, src, dst, g, n, seed=222, mode='uniform', exclude=None, trace=None):
    """-> int64 [found, 2], found <= n.  trace (a list): receives (k, a, w, b) of every pair that was kept."""
    m = MODES[mode]
    assert N >= 2 and n >= 0
    salt = int(orc.sample_salt(int(seed), int(g), TAG, m))
    adj = set(zip(np.asarray(src).tolist(), np.asarray(dst).tolist()))
    out = out_rows(N, src, dst) if m == 1 else None
    excl = set() if exclude is None else {min(a, b) * N + max(a, b) for a, b in np.asarray(exclude, np.int64).reshape(-1, 2).tolist()}
    first, res = {}, []
    B, CH = budget(n), 1 << 15
    for k0 in range(0, B, CH):
        w4 = words(salt, k0, min(CH, B - k0))
        for i, r in enumerate(w4):
            if len(res) == n:
                break
            c = candidate(N, out, m, r)
            if c is None:
                continue
            a, w, b = c
            u, v = min(a, b), max(a, b)
            if u == v or (u, v) in adj or (v, u) in adj:
                continue
            key = u * N + v
            if key in excl or key in first:
                continue
            first[key] = k0 + i
            res.append((u, v))
            if trace is not None:
                trace.append((k0 + i, a, w, b))
        if len(res) == n:
            break
    return np.asarray(res, np.int64).reshape(-1, 2), len(res)


def free_pairs(N, src, dst):
    """Brute force: every unordered pair u < v without an edge in either direction."""
    A = np.zeros((N, N), bool)
    A[np.asarray(src), np.asarray(dst)] = True
    A |= A.T
    u, v = np.nonzero(np.triu(~A, 1))
    return set(zip(u.tolist(), v.tolist()))


class HostStore:
    """GraphStore's negative_pairs / has_edges on the restatement (host logic tests; no GPU)."""

    def __init__(self, graphs):
        self.graphs = [(int(g[0]), np.asarray(g[1], np.int64), np.asarray(g[2], np.int64)) for g in graphs]
        self.n_graphs, self.n_nodes = len(self.graphs), [g[0] for g in self.graphs]
        self.calls = []

    def negative_pairs(self, g, n, seed=222, mode='uniform', exclude=None):
        self.calls.append((g, n, seed, mode, None if exclude is None else np.array(exclude)))
        N, src, dst = self.graphs[g]
        p, found = negative_pairs(N, src, dst, g, n, seed, mode, exclude)
        if found < n:
            raise ValueError('only %d' % found)
        return p

    def has_edges(self, g, pairs):
        N, src, dst = self.graphs[g]
        adj = set(zip(src.tolist(), dst.tolist()))
        return np.array([(a, b) in adj or (b, a) in adj for a, b in np.asarray(pairs).reshape(-1, 2).tolist()], bool)


# ---------------------------------------------------------------------------------------------------- shared cases
def multigraph_case():
    """300 nodes, directed: parallel edges, self loops, isolated nodes (290..299), sinks (280..289: in-edges only), node 0 with out-degree 400 (a long
    row for the search, parallel copies inside), node 1 with in-degree 400."""
    rng = np.random.default_rng(31)
    N = 300
    src = rng.integers(2, 280, 900); dst = rng.integers(2, 290, 900)                     # body; 280..289 only ever destinations
    par = rng.choice(900, 60, replace=False)
    hub_out = rng.integers(1, 290, 400); hub_in = rng.integers(2, 280, 400)
    loops = np.array([5, 5, 17, 0, 1, 100])
    s = np.concatenate([src, src[par], np.zeros(400, np.int64), hub_in, loops])
    d = np.concatenate([dst, dst[par], hub_out, np.ones(400, np.int64), loops])
    order = rng.permutation(len(s))
    s, d = s[order].astype(np.int64), d[order].astype(np.int64)
    outdeg, indeg = np.bincount(s, minlength=N), np.bincount(d, minlength=N)
    assert outdeg[0] >= 400 and indeg[1] >= 400
    assert (outdeg[280:290] == 0).all() and (indeg[280:290] > 0).any() and (outdeg[290:] == 0).all() and (indeg[290:] == 0).all()
    assert len(set(zip(s.tolist(), d.tolist()))) < len(s) and (s == d).sum() >= 6
    return N, s, d


def dense_case():
    """40 nodes: every pair adjacent (one direction, by parity) except those with (u + v) % 7 == 0."""
    N = 40
    e = [(u, v) if (u + v) % 2 else (v, u) for u in range(N) for v in range(u + 1, N) if (u + v) % 7 != 0]
    e = np.asarray(e, np.int64)
    return N, e[:, 0].copy(), e[:, 1].copy()


def big_case():
    """70,000 nodes, 200,000 random edges: keys u * N + v above 2^32."""
    rng = np.random.default_rng(7)
    N = 70_000
    return N, rng.integers(0, N, 200_000).astype(np.int64), rng.integers(0, N, 200_000).astype(np.int64)
