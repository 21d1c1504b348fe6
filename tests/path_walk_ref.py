"""Restatement of the walk-count definition of include/gmeta_hip.h (gm_store_pair_walks), literally: Python sets for the neighbourhoods (those of
pair_score_ref), one pair at a time, Python integers.  The mask flag is restated as the definition states it -- the walks of the graph WITHOUT the edge
{u, v} -- not through the closed form the device uses.  The GPU tests hold the device result against it for equality."""
import numpy as np

import pair_score_ref

MASK_TARGET = 1
COLS = ('w1', 'w2', 'w3')


def pair_walks(N, src, dst, pairs, flags=0, nb=None):
    """-> int64 [n, 3]: the numbers of walks of length 1, 2 and 3 from u to v in the symmetric 0 / 1 matrix of the neighbourhoods."""
    nb = pair_score_ref.neighbourhoods(N, src, dst) if nb is None else nb
    out = np.zeros((len(pairs), 3), np.int64)
    for k, (a, b) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2).tolist()):
        if not (0 <= a < N and 0 <= b < N):
            continue                                                        # a node outside the graph: three zeros
        u, v = min(a, b), max(a, b)
        cut = bool(flags & MASK_TARGET) and u != v and v in nb[u]
        if cut:                                                             # the graph without the edge {u, v}: only the rows of u and v change
            gu, gv = nb[u] - {v}, nb[v] - {u}
            row = lambda z: gu if z == u else gv if z == v else nb[z]      # noqa: E731
        else:
            gu, gv = nb[u], nb[v]
            row = lambda z: nb[z]                                           # noqa: E731
        out[k, 0] = 1 if v in gu else 0
        out[k, 1] = sum(1 for z in gu if z in gv)
        out[k, 2] = sum(len(row(z) & gv) for z in gu)
    return out


# ---------------------------------------------------------------------------------------------------- shared case
HUB_ROW = 3000
END_ROWS = (0, 1, 15, 16, 17, 63, 64, 65, 129)      # endpoints: the row lengths around every lane width and the default chunk
MID_ROWS = (64, 65, 129, 300)                       # middle nodes: INNER rows of these lengths lie on the walks between the endpoints


def walk_case():
    """A directed graph of 3,300 nodes whose planted nodes have Gamma rows of exactly these lengths (by construction, asserted):
        0, 1                  two ADJACENT hubs of HUB_ROW distinct neighbours each, from overlapping windows of the pool
        2 .. 10               endpoints of END_ROWS[k] neighbours: the four middle nodes first, then a window of the pool (the leaf hangs off the 300-row middle node)
        11 .. 14              middle nodes of MID_ROWS[k] neighbours: both hubs, every endpoint of 15 or more, then pool nodes
    The pool (15 .. 3299) also holds random edges of its own (mean degree about 6), so inner rows of ordinary nodes are not trivial.  Edges point in a random
    direction; parallel copies, reverse copies and self loops are sprinkled in (none changes a neighbourhood).
    -> (N, src, dst, endpoints): the planted nodes, the middle nodes and ten ordinary pool nodes."""
    rng = np.random.default_rng(8)
    E, M = len(END_ROWS), len(MID_ROWS)
    ends = list(range(2, 2 + E)); mids = list(range(2 + E, 2 + E + M))
    first = 2 + E + M
    N = 3300
    pool = np.arange(first, N)
    und = [(0, 1)]
    for k, want in zip(ends, END_ROWS):
        if want == 1:
            und.append((k, mids[-1]))
        elif want:
            und.extend((k, m) for m in mids)
            span = pool[:max(2 * (want - M), 40)]                           # overlapping windows: shorter rows are thinned subsets of longer ones
            und.extend((k, int(z)) for z in np.sort(rng.choice(span, want - M, replace=False)))
    have = {m: sum(1 for a, b in und if b == m) for m in mids}
    for m, want in zip(mids, MID_ROWS):
        und.extend([(0, m), (1, m)])
        need = want - 2 - have[m]
        und.extend((m, int(z)) for z in np.sort(rng.choice(pool[100:1500], need, replace=False)))
    rest = HUB_ROW - 1 - M
    und.extend((0, int(z)) for z in pool[:rest])
    und.extend((1, int(z)) for z in pool[len(pool) - rest:])
    a, b = rng.integers(0, len(pool), 3 * len(pool)), rng.integers(0, len(pool), 3 * len(pool))
    und.extend((int(pool[x]), int(pool[y])) for x, y in zip(a, b) if x != y)
    src, dst = [], []
    for x, y in und:
        if rng.random() < 0.5:
            x, y = y, x
        src.append(x); dst.append(y)
        r = rng.random()
        if r < 0.05:                                                        # a parallel copy
            src.append(x); dst.append(y)
        elif r < 0.10:                                                      # the reverse edge
            src.append(y); dst.append(x)
    loops = [0, 1, 2, 2, mids[0], int(pool[7]), int(pool[-1])]              # self loops: never a neighbour (node 2 stays isolated)
    src.extend(loops); dst.extend(loops)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    deg = pair_score_ref.degrees(N, src, dst)
    assert tuple(deg[:2].tolist()) == (HUB_ROW, HUB_ROW), deg[:2]
    assert tuple(deg[ends].tolist()) == END_ROWS, deg[ends]
    assert tuple(deg[mids].tolist()) == MID_ROWS, deg[mids]
    assert 5.0 < deg[first:].mean() - 2.0 * rest / len(pool) < 7.0          # the pool's own edges
    ordinary = [int(z) for z in pool[[3, 50, 290, 291, 1000, 1499, 2000, 2994, 3100, len(pool) - 1]]]
    return N, src, dst, [0, 1] + ends + mids + ordinary
