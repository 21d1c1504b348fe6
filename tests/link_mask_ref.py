"""Restatement of target-link masking (GM_LINK_MASK_TARGET, include/gmeta_hip.h) out of the oracle's own pieces, and the inputs the tests of the flag
share (tests/test_link_mask_restatement.py on the CPU, tests/test_hip_link_mask.py on the GPU).

    node list of (g, i, j)  = the UNMASKED graph's: orc.linkpred_nodes (reference pairs) or link_sym_ref.nodes (symmetric pairs) -> orc.sample_nodes
    CSR of the subgraph     = orc.induce(masked_graph(G, i, j), node list): G without every edge i -> j and j -> i (i == j: without i's self loops)

Everything else is the oracle's: a masked batch is an orc.Batch (edge_weight_ref.Batch on weighted graphs) whose subgraph s was induced from ITS pair's
masked graph, so orc.classifier_forward / orc.meta_step, hop_label_ref and edge_weight_ref take it as it is."""
import copy

import numpy as np

import gmeta_oracle as orc
import edge_weight_ref as ewr
import link_sym_ref as sym

RNG_SEED = sym.RNG_SEED
MASK = 4            # GM_LINK_MASK_TARGET
MODES = (1, 2)      # reference pairs, GM_LINK_SYMMETRIC


def target_edges(src, dst, i, j):
    """Boolean mask over the edge list: the edges with (src, dst) in {(i, j), (j, i)}."""
    src = np.asarray(src, np.int64); dst = np.asarray(dst, np.int64)
    return ((src == i) & (dst == j)) | ((src == j) & (dst == i))


def masked_graph(n, src, dst, i, j, w=None):
    """The parent graph without the target link of (i, j), order of the other edges kept (w: the weights, filtered alike -> edge_weight_ref.Graph)."""
    keep = ~target_edges(src, dst, i, j)
    src = np.asarray(src, np.int64)[keep]; dst = np.asarray(dst, np.int64)[keep]
    return orc.Graph(n, src, dst) if w is None else ewr.Graph(n, src, dst, np.asarray(w, np.float32)[keep])


def masked_from(G, i, j):
    """masked_graph from the built orc.Graph / edge_weight_ref.Graph: only rows i and j of the in-edge CSR change (row i loses its sources j, row j its
    sources i), and the graph's edge sort is stable, so this is masked_graph(...) without sorting the whole edge list again (held equal to it by
    tests/test_link_mask_restatement.py)."""
    i, j = int(i), int(j)
    drop = np.zeros(len(G.indices), bool)
    for v, u in ((i, j), (j, i)):
        a, b = int(G.indptr[v]), int(G.indptr[v + 1])
        drop[a:b] |= G.indices[a:b] == u
    if not drop.any():
        return G
    M = copy.copy(G)
    M.indices = G.indices[~drop]
    cut = np.zeros(G.n + 1, np.int64)
    for v in {i, j}:
        cut[v + 1] = int(drop[G.indptr[v]:G.indptr[v + 1]].sum())
    M.indptr = G.indptr - np.cumsum(cut)
    if hasattr(G, 'w'):
        M.w = G.w[~drop]
    return M


def unmasked_nodes(G, i, j, h, mode):
    return orc.linkpred_nodes(G, int(i), int(j)) if mode == 1 else sym.nodes(G, i, j, h)


def node_lists(og, seeds, h, sample_n, mode, rng_seed=RNG_SEED):
    """Per seed: the node list of the UNMASKED graph, thinned by the oracle's keyed permutation (both centres re-added)."""
    return [orc.sample_nodes(unmasked_nodes(og[g], i, j, h, mode), sample_n, rng_seed, int(g), int(i), int(j)) for g, i, j in np.asarray(seeds).tolist()]


def masked_node_lists(og, seeds, h, sample_n, mode, rng_seed=RNG_SEED):
    """The same with the expansion actually run on each pair's masked graph (the header's remark says these are node_lists(...))."""
    return [orc.sample_nodes(unmasked_nodes(masked_from(og[g], i, j), i, j, h, mode), sample_n, rng_seed, int(g), int(i), int(j))
            for g, i, j in np.asarray(seeds).tolist()]


def batch_from_lists(og, seeds, lists):
    """The oracle's Batch whose subgraph s is induced from the masked graph of ITS pair: graph s of the list handed to the oracle is pair s's masked
    graph; graph_id is put back afterwards (features() reads it).  Weighted graphs (edge_weight_ref.Graph) give an edge_weight_ref.Batch."""
    seeds = [tuple(int(x) for x in s) for s in np.asarray(seeds).tolist()]
    assert all(j >= 0 for _, _, j in seeds), 'target-link masking is defined for pairs'
    mg = [masked_from(og[g], i, j) for g, i, j in seeds]
    cls = ewr.Batch if seeds and hasattr(og[seeds[0][0]], 'w') else orc.Batch
    b = cls(mg, [(s, i, j) for s, (_, i, j) in enumerate(seeds)], lists)
    b.graph_id = np.concatenate([np.full(len(l), g, np.int64) for (g, _, _), l in zip(seeds, lists)] + [np.zeros(0, np.int64)])
    return b


def extract_batch(og, seeds, h, sample_n, mode, rng_seed=RNG_SEED):
    return batch_from_lists(og, seeds, node_lists(og, seeds, h, sample_n, mode, rng_seed))


def unmasked_batch(og, seeds, h, sample_n, mode, rng_seed=RNG_SEED):
    if mode == 1:
        return orc.extract_batch(og, seeds, h, sample_n, rng_seed, True)
    return sym.extract_batch(og, seeds, h, sample_n, rng_seed)


def header_norm(b):
    """GM_F_NORM as include/gmeta_hip.h states it, on the restated batch: 1 / sqrtf(d > 0 ? d : 1) with d the in-degree, or on a weighted batch the in-edge
    weights summed in edge order in fp32 -- one correctly rounded square root and one correctly rounded division, the same two IEEE operations on the host
    and on the device, so the comparison is bitwise.  (The oracle's own `norm` is np.power(d, -0.5), which numpy does not round correctly: it is one ulp
    off for some degrees, which is why tests/test_hip_parity.py compares the norms of UNMASKED batches within 2e-7.)"""
    if hasattr(b, 'ew'):
        d = np.zeros(b.n, np.float32)
        np.add.at(d, np.repeat(np.arange(b.n), np.diff(b.indptr)), np.asarray(b.ew, np.float32))
    else:
        d = np.diff(b.indptr).astype(np.float32)
    d = np.where(d > 0, d, np.float32(1)).astype(np.float32)
    out = (np.float32(1) / np.sqrt(d, dtype=np.float32)).astype(np.float32)
    assert np.allclose(out, b.norm, rtol=2e-7, atol=0)
    return out


def by_source(b):
    """(indptr_t, destinations) of a batch, destinations in edge order: the GM_F_INDPTR_T / GM_F_INDICES_T the device builds."""
    return orc._by_source(b)


def brute_force_csr(G_edges, nodes, i, j):
    """Local in-edge CSR of the induced subgraph by filtering the EDGE LIST (n, src, dst): inside the node set, not a target edge, grouped by
    destination in edge order -- no oracle code on the path."""
    n, src, dst = G_edges
    src = np.asarray(src, np.int64); dst = np.asarray(dst, np.int64)
    nodes = np.asarray(nodes, np.int64)
    lut = np.full(n, -1, np.int64); lut[nodes] = np.arange(len(nodes))
    rows = [[] for _ in nodes]
    for s, d in zip(src.tolist(), dst.tolist()):
        if lut[s] < 0 or lut[d] < 0 or (s, d) in ((i, j), (j, i)):
            continue
        rows[lut[d]].append(int(lut[s]))
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    return indptr, np.array([u for r in rows for u in r], np.int32)


def adjacent(G, i, j):
    """Number of target edges of (i, j) in G (i == j: its self loops)."""
    i, j = int(i), int(j)
    return int((G.preds(i) == j).sum()) + (int((G.preds(j) == i).sum()) if i != j else 0)


# ---------------------------------------------------------------------------------------------------- shared inputs
PLANTED = ('only_ij', 'only_ji', 'both', 'triple_ij', 'self_two_loops', 'non_adjacent', 'isolated_j', 'via_third')


def fuzz_case(seed):
    """link_sym_ref.fuzz_case's graphs (25-160 nodes, hub, parallel edges, self loops, isolated nodes) and its pairs, plus pairs PLANTED in graph 0 so
    that the mask has work.  Eighteen fresh nodes are appended to graph 0 and wired as the plan says (each hangs on to the old graph through one edge
    from a random old node, so their neighbourhoods are not trivial):
        only_ij   a -> b once                 only_ji         b -> a once (seeded as (a, b))       both          a -> b and b -> a
        triple_ij a -> b three times          self_two_loops  a -> a twice, seeded (a, a)          non_adjacent  no edge between a and b
        isolated_j b has no edge at all       via_third       a -> t -> b and b -> t -> a only
    `planted` maps the name to the index of its seed; assert_planted checks every property on the generated parent."""
    c = sym.fuzz_case(seed)
    rng = np.random.default_rng(9000 + seed)
    n0, src, dst = c['graphs'][0]
    src, dst = list(np.asarray(src).tolist()), list(np.asarray(dst).tolist())
    new = iter(range(n0, n0 + 18))
    es, seeds, planted = [], [], {}

    def node(anchor=True):
        v = next(new)
        if anchor:
            es.append((int(rng.integers(0, n0)), v))
        return v

    def plant(name, a, b):
        planted[name] = len(c['seeds']) + len(seeds)
        seeds.append((0, a, b))
    a, b = node(), node(); es += [(a, b)]; plant('only_ij', a, b)
    a, b = node(), node(); es += [(b, a)]; plant('only_ji', a, b)
    a, b = node(), node(); es += [(a, b), (b, a)]; plant('both', a, b)
    a, b = node(), node(); es += [(a, b), (int(rng.integers(0, n0)), b), (a, b), (a, b)]; plant('triple_ij', a, b)
    a = node(); es += [(a, a), (int(rng.integers(0, n0)), a), (a, a)]; plant('self_two_loops', a, a)
    a, b = node(), node(); plant('non_adjacent', a, b)
    a, b = node(), node(anchor=False); plant('isolated_j', a, b)
    a, b, t = node(), node(), node(); es += [(a, t), (t, b), (b, t), (t, a)]; plant('via_third', a, b)
    extra = np.array(es, np.int64)
    g0 = (n0 + 18, np.concatenate([np.asarray(src, np.int64), extra[:, 0]]), np.concatenate([np.asarray(dst, np.int64), extra[:, 1]]))
    graphs = [g0] + list(c['graphs'][1:])
    out = dict(graphs=graphs, og=[orc.Graph(*g) for g in graphs], seeds=np.concatenate([c['seeds'], np.array(seeds, np.int32)]), h=c['h'],
               sample_n=c['sample_n'], planted=planted)
    assert_planted(out)
    return out


def assert_planted(c):
    """Every planted property holds on the generated parent (a case cannot silently degenerate)."""
    G = c['og'][0]
    n, src, dst = c['graphs'][0]
    cnt = lambda s, d: int(((np.asarray(src) == s) & (np.asarray(dst) == d)).sum())      # noqa: E731
    sd = {k: tuple(int(x) for x in c['seeds'][v]) for k, v in c['planted'].items()}
    assert set(sd) == set(PLANTED)
    _, a, b = sd['only_ij']; assert (cnt(a, b), cnt(b, a)) == (1, 0)
    _, a, b = sd['only_ji']; assert (cnt(a, b), cnt(b, a)) == (0, 1)
    _, a, b = sd['both']; assert (cnt(a, b), cnt(b, a)) == (1, 1)
    _, a, b = sd['triple_ij']; assert (cnt(a, b), cnt(b, a)) == (3, 0) and len(G.preds(b)) == 5      # (the copies are not adjacent in b's list)
    _, a, b = sd['self_two_loops']; assert a == b and cnt(a, a) == 2 and len(G.preds(a)) == 4
    _, a, b = sd['non_adjacent']; assert a != b and cnt(a, b) == cnt(b, a) == 0 and adjacent(G, a, b) == 0
    _, a, b = sd['isolated_j']; assert len(G.preds(b)) == 0 and not (np.asarray(src) == b).any()
    _, a, b = sd['via_third']
    assert cnt(a, b) == cnt(b, a) == 0 and len(np.intersect1d(G.preds(a), G.preds(b))) >= 1
    assert sum(adjacent(G, i, j) > 0 for g, i, j in c['seeds'].tolist() if g == 0) >= 5


def weighted(c, seed=5):
    """The case on weighted graphs: log-uniform weights in [0.25, 4], one per edge (parallel copies differ), as edge_weight_ref.Graph."""
    rng = np.random.default_rng(seed)
    wg = [(n, s, d, np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(s))).astype(np.float32)) for n, s, d in c['graphs']]
    return wg, [ewr.Graph(*g) for g in wg]


EX_BIG_DEG = 256      # extract.hip: rows with more parent neighbours are walked by a whole wave (256 ids per iteration), the others by eight lanes (32 ids)


def boundary_graph(deg, positions, symmetric, side='in', j_extra=0):
    """Hand-built graph for the walker boundaries.  Centre I has `deg` in-edges (side='out': out-edges) in parent edge order; the neighbour at the list
    positions `positions` is J (parallel copies), every other position k holds the filler node k.  J = min(positions), I = deg; the fillers are chained
    (k -> k + 1) so that other rows have edges too.  j_extra: that many further in-edges of J from fresh nodes (a hub J).
    symmetric: every edge is stored in both directions and the edge list is sorted by (dst, src) -- rows ascending, the layout the store recognises as
    symmetric; J's copies must then be adjacent (`positions` contiguous), and row J meets I as often.
    Positions follow parent edge order because the store's sort by destination is stable.  Returns ((n, src, dst), I, J)."""
    positions = sorted(positions)
    J, I = positions[0], deg
    assert not symmetric or (positions == list(range(J, J + len(positions))) and side == 'in')
    nb = [J if k in positions else k for k in range(deg)]
    n = deg + 1 + j_extra
    es = [(u, I) if side == 'in' else (I, u) for u in nb]
    fill = [k for k in range(deg) if k not in positions]
    es += [(a, b) for a, b in zip(fill[:-1], fill[1:])]
    es += [(deg + 1 + k, J) for k in range(j_extra)]
    if side == 'out':
        es += [(fill[0], I)]                                   # in-degree small
    e = np.array(es, np.int64)
    if symmetric:
        e = np.concatenate([e, e[:, ::-1]])
        e = e[np.lexsort((e[:, 0], e[:, 1]))]
    return (n, e[:, 0].copy(), e[:, 1].copy()), I, J


def list_positions(G_edges, v, u, side='in'):
    """Positions of neighbour u in v's parent in-list (side='out': out-list), in edge order."""
    n, src, dst = G_edges
    a, b = (src, dst) if side == 'in' else (dst, src)
    return np.nonzero(np.asarray(a)[np.asarray(b) == v] == u)[0].tolist()
