"""Graphs with chosen degrees and the fp64 reference of the aggregate kernels (agg.hip, agg_stream.hip), for test_agg_ref.py (CPU) and
test_hip_agg_numerics.py (GPU).  No GPU and no library needed here.

The degree-ladder graph: one directed multigraph of N = 2,048 nodes.  Node i < len(LADDER) (block A) has in-degree LADDER[i]; node len(LADDER) + i
(block B) has out-degree LADDER[i]; the degrees sit on both sides of every threshold of the kernels (the third edge of a window row, the hub
thresholds 32 / 64, the split of a hub row at 192 = 1.5 parts, 2.5 parts at 320, 8 parts at 1,000).  Every other node gets a target in-degree
(`filler`); B's out-edge stubs are matched to a random subset of all in-edge stubs, the remaining in-edge stubs get random sources outside B.  Node 0
(in-degree 0) is nobody's source and the last node nobody's destination.  A batch takes the whole graph as every subgraph, so its induced edges are
exactly these edges, parallel edges and self-loops included."""
import numpy as np
import torch

N = 2048
LADDER = list(range(10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 191, 192, 193, 255, 319, 320, 321, 448, 1000]
SET_SUBS = [1, 2, 1]                 # subgraphs per set: 8,192 rows, set boundaries at rows 2,048 and 6,144
GIANT = 5000
# variant -> (largest ladder entry kept, filler in-degrees, giant row)
VARIANTS = {
    'sparse': (1000, (0, 3), False),     # edges <= 8 rows: hub threshold 32, hub parts of 128 edges
    'dense': (1000, (9, 15), False),     # edges > 8 rows: hub threshold 64, 4-row windows, never stream-eligible
    'giant': (1000, (0, 3), True),       # sparse + GIANT parallel edges g_out -> g_in: hub parts of 160 edges
    'flat': (20, (0, 3), False),         # no row above 20 edges in either orientation: no hub list, no schedule
    'unsplit': (191, (0, 3), False),     # hub rows, none of 1.5 parts: scheduled, not split
}


class Graph:
    pass


def build_graph(variant, seed=0, weighted=False):
    """The ladder graph of a variant: .src / .dst (int64 [E], in edge-id order), .w (float32 [E], fractional, or None), .lad (the ladder kept),
    .a0 / .b0 (first node of the blocks), .g_in / .g_out (the giant pair or None)."""
    top, (f_lo, f_hi), giant = VARIANTS[variant]
    rng = np.random.default_rng(1000 + seed)
    lad = [d for d in LADDER if d <= top]
    L = len(lad)
    g = Graph()
    g.variant, g.lad, g.a0, g.b0, g.n = variant, lad, 0, L, N
    indeg = np.zeros(N, np.int64)
    indeg[:L] = lad
    indeg[L:N - 1] = rng.integers(f_lo, f_hi + 1, N - 1 - L)             # B and the remaining nodes; the last node keeps 0
    g.g_in = g.g_out = None
    if giant:
        g.g_in, g.g_out = 2 * L + 100, 2 * L + 900
        indeg[g.g_in] = 0
    dst = np.repeat(np.arange(N), indeg)
    E = len(dst)
    src = np.full(E, -1, np.int64)
    b_stubs = np.repeat(np.arange(L, 2 * L), lad)
    assert len(b_stubs) <= E
    slots = rng.permutation(E)
    src[slots[:len(b_stubs)]] = rng.permutation(b_stubs)
    pool = np.concatenate([np.arange(1, L), np.arange(2 * L, N)])         # not node 0, not B
    if giant:
        pool = pool[pool != g.g_out]
    rest = slots[len(b_stubs):]
    src[rest] = rng.choice(pool, len(rest))
    if top > 32:                                                           # a self-loop on the largest hub of block A (replaces an edge from outside B)
        hub = L - 1
        k = rest[dst[rest] == hub][0]
        src[k] = hub
    if giant:
        src = np.concatenate([src, np.full(GIANT, g.g_out)])
        dst = np.concatenate([dst, np.full(GIANT, g.g_in)])
    order = rng.permutation(len(src))                                      # edge ids in no particular order
    g.src, g.dst = src[order], dst[order]
    g.w = None
    if weighted:
        g.w = (0.25 + 1.5 * rng.random(len(g.src))).astype(np.float32)
    return g


def degrees(g):
    return np.bincount(g.dst, minlength=g.n), np.bincount(g.src, minlength=g.n)


def batch_edges(g, subs=sum(SET_SUBS)):
    """(src row, dst row, weight) of every edge of a batch whose `subs` subgraphs are all the whole graph (row = subgraph * N + node)"""
    off = (np.arange(subs) * g.n)[:, None]
    w = None if g.w is None else np.tile(g.w, subs)
    return (g.src[None, :] + off).reshape(-1), (g.dst[None, :] + off).reshape(-1), w


def set_of_rows(g, set_subs=SET_SUBS):
    return np.repeat(np.arange(len(set_subs)), np.asarray(set_subs) * g.n)


# ---------------------------------------------------------------------------------------------------- host restatements
def heavy_deg_for(rows, edges):
    """gm_heavy_deg_for (common.hip): rows with more edges than this are hub rows"""
    return 32 if edges <= 8 * rows else 64


def hub_part_for(maxdeg):
    """gm_agg_schedule (agg.hip): edges per hub part -- 128, or more (a multiple of 16) so that the widest row has at most 32 parts"""
    return max(128, ((maxdeg + 31) // 32 + 15) // 16 * 16)


def hub_parts(deg, hub_part):
    """parts of a hub row: nearest, a row is split from 1.5 parts upwards (the last part takes the remainder)"""
    return max(1, (deg + hub_part // 2) // hub_part)


def agg_window(rows, edges):
    """gm_agg_window (agg.hip): rows per wave window of the scheduled launch"""
    dense = edges > 8 * rows
    min_waves, min_win = (16384, 4) if dense else (32768, 2)
    win = 64
    while win > min_win and rows // win < min_waves:
        win >>= 1
    return win


def expected_hubs(deg, rows, edges):
    """(threshold, hub rows ascending, edges per part or 0 when nothing is split, parts) of one orientation with per-row degrees `deg`"""
    th = heavy_deg_for(rows, edges)
    hubs = np.nonzero(deg > th)[0]
    if len(hubs) == 0:
        return th, hubs, 0, 0
    hp = hub_part_for(int(deg[hubs].max()))
    parts = sum(hub_parts(int(d), hp) for d in deg[hubs])
    if parts == len(hubs):
        return th, hubs, 0, parts
    return th, hubs, hp, parts


# ---------------------------------------------------------------------------------------------------- the reference
def edge_sums(rows, src, dst, w, x):
    """fp64 from an edge list: sum_{e: dst_e = v} w_e x[src_e], the same sum of magnitudes, and the per-row term count d (int64 [rows])"""
    xd = x.double()
    width = xd.shape[1]
    t = xd[src]
    if w is not None:
        t = t * w.double()[:, None]
    acc = torch.zeros(rows, width, dtype=torch.float64, device=xd.device).index_add_(0, dst, t)
    sab = torch.zeros(rows, width, dtype=torch.float64, device=xd.device).index_add_(0, dst, t.abs())
    return acc, sab, torch.bincount(dst, minlength=rows)


def epilogue(acc, sab, s_out=None, bias=None, relu=False, mask=None):
    """epi(|s_out| acc + bias) with epi = ReLU, then the mask (False: 0); and the condition scale |s_out| sab + |bias|"""
    if s_out is not None:
        so = s_out.double().abs()[:, None]
        acc, sab = acc * so, sab * so
    if bias is not None:
        acc, sab = acc + bias.double(), sab + bias.double().abs()
    if relu:
        acc = acc.clamp_min(0)
    if mask is not None:
        acc = torch.where(mask, acc, torch.zeros_like(acc))
    return acc, sab


def reference(rows, src, dst, w, x, s_out=None, bias=None, relu=False, mask=None):
    """fp64, from an edge list:  out[v] = epi(|s_out[v]| sum_{e: dst_e = v} w_e x[src_e] + bias[v]),  epi = ReLU then the mask (False: 0).
    src / dst: int64 tensors [E] (rows of x / of out); w: [E] or None (1); x: [*, width]; s_out: [rows] or None; bias: [rows, width] (the row's set's
    bias) or None; mask: bool [rows, width] or None.  Inputs are taken at their fp32 values, converted to fp64.  Returns out, the per-element condition
    scale |s_out| sum |w_e||x[src_e]| + |bias| and the per-row term count d."""
    acc, sab, d = edge_sums(rows, src, dst, w, x)
    out, scale = epilogue(acc, sab, s_out, bias, relu, mask)
    return out, scale, d
