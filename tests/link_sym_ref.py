"""Restatement of the symmetric pair mode (GM_LINK_SYMMETRIC, include/gmeta_hip.h) out of the oracle's own pieces, and the inputs the tests of that
mode share (tests/test_link_symmetric_restatement.py on the CPU, tests/test_hip_link_symmetric.py on the GPU).

    nodes(G, i, j, h) = khop_nodes(G, i, h) U khop_nodes(G, j, h)  ->  orc.sample_nodes(., g, i, j)  ->  orc.extract_batch(link_pred=True, replay_nodes=.)

Nothing downstream of the node set differs from the reference's pair mode, so the oracle's Batch / meta_step take the restated batches as they are."""
import numpy as np

import gmeta_oracle as orc

RNG_SEED = 222


def nodes(G, i, j, h):
    """{v : in-hop distance to i <= h} U {v : in-hop distance to j <= h}, ascending."""
    return np.union1d(orc.khop_nodes(G, int(i), h), orc.khop_nodes(G, int(j), h)).astype(np.int32)


def node_lists(graphs, seeds, h, sample_n, rng_seed=RNG_SEED):
    """Per seed (g, i, j): the node set, thinned by the oracle's keyed permutation when it holds more than sample_n nodes (both centres re-added)."""
    return [orc.sample_nodes(nodes(graphs[g], i, j, h), sample_n, rng_seed, int(g), int(i), int(j)) for g, i, j in np.asarray(seeds).tolist()]


def extract_batch(graphs, seeds, h, sample_n, rng_seed=RNG_SEED):
    return orc.extract_batch(graphs, seeds, h, sample_n, rng_seed, True, replay_nodes=node_lists(graphs, seeds, h, sample_n, rng_seed))


def differs_from_reference_mode(graphs, seeds, h, sample_n, rng_seed=RNG_SEED):
    """Number of subgraphs whose FINAL node list (after sampling) is not the one the reference's pair mode gives (orc.linkpred_nodes: i two hops, j one,
    h ignored).  A case where this is zero could not tell a build that ignores the mode from one that honours it."""
    sym = node_lists(graphs, seeds, h, sample_n, rng_seed)
    ref = [orc.sample_nodes(orc.linkpred_nodes(graphs[g], int(i), int(j)), sample_n, rng_seed, int(g), int(i), int(j)) for g, i, j in np.asarray(seeds).tolist()]
    return sum(not np.array_equal(a, b) for a, b in zip(sym, ref))


def assert_batch_matches(hb, obs):
    """Integer work of a device batch `hb` against the oracle batches `obs` of its consecutive sets, bit for bit: node lists, in-edge CSR, centre
    indices (as tests/test_hip_fuzz.py:71-80)."""
    assert np.array_equal(hb.parent(), np.concatenate([b.parent for b in obs]))
    ip, ix = hb.csr()
    r0 = e0 = 0
    for b in obs:
        assert np.array_equal(ip[r0:r0 + b.n + 1] - e0, b.indptr) and np.array_equal(ix[e0:e0 + len(b.indices)] - r0, b.indices)
        r0 += b.n; e0 += len(b.indices)
    cen = np.concatenate([(b.centre_rows - b.sub_off[:-1, None]).reshape(-1) for b in obs])      # local index inside each subgraph
    assert hb.centres == 2 and np.array_equal(hb._read(8, hb.subs * hb.centres, np.int32), cen)


# ---------------------------------------------------------------------------------------------------- shared inputs
FUZZ_SEEDS = list(range(9))            # h = 1 + seed % 3, sample_n = (6, 40, 10000)[seed // 3]: the full grid


def fuzz_case(seed):
    """Random ragged multigraphs of tests/test_hip_fuzz.py (25-160 nodes, 1-3 graphs, a hub, parallel self loops, isolated nodes): eight random pairs
    plus, in graph 0, an isolated j, a j inside i's neighbourhood, a pair with disjoint neighbourhoods and (seed 0 only) one i == j pair."""
    from test_hip_fuzz import _graph
    rng = np.random.default_rng(5000 + seed)
    h, sample_n = 1 + seed % 3, (6, 40, 10000)[(seed // 3) % 3]
    graphs = [_graph(rng, int(rng.integers(25, 160))) for _ in range(int(rng.integers(1, 4)))]
    og = [orc.Graph(*g) for g in graphs]
    seeds = []
    for _ in range(8):
        g = int(rng.integers(0, len(graphs))); n = graphs[g][0]
        i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
        seeds.append((g, i, j if j != i else (i + 1) % n))
    G = og[0]
    deg_in = np.diff(G.indptr); deg_out = np.bincount(G.indices, minlength=G.n)
    iso = np.nonzero((deg_in == 0) & (deg_out == 0))[0]
    inner = [(int(v), int(u)) for v in np.nonzero(deg_in > 0)[0] for u in G.preds(v)[:1] if u != v]
    i0, j_in = inner[int(rng.integers(len(inner)))]
    special = {'isolated_j': len(seeds), 'j_inside': len(seeds) + 1, 'disjoint': len(seeds) + 2}
    seeds += [(0, i0, int(iso[0])), (0, i0, j_in)]
    # disjoint neighbourhoods: among the nodes with predecessors, the pair without a common node whose smaller side is largest
    cand = np.nonzero(deg_in > 0)[0]
    M = np.zeros((len(cand), G.n), np.int32)
    for k, v in enumerate(cand):
        M[k, orc.khop_nodes(G, int(v), h)] = 1
    size = M.sum(1)
    free = (M @ M.T) == 0
    score = np.where(free, np.minimum(size[:, None], size[None, :]), -1)
    a, b = np.unravel_index(int(score.argmax()), score.shape)
    nontrivial = bool(score[a, b] > 0)
    seeds.append((0, int(cand[a]), int(cand[b])) if nontrivial else (0, int(iso[0]), i0))      # (else: an isolated i against any j)
    if seed == 0:
        special['self_pair'] = len(seeds)
        seeds.append((0, i0, i0))
    return dict(graphs=graphs, og=og, seeds=np.array(seeds, np.int32), h=h, sample_n=sample_n, special=special, disjoint_nontrivial=nontrivial)


HUB_CASES = [(2, 10000), (3, 10000), (2, 150)]          # (h, sample_n)


def hub_case():
    """One 600-node graph with two nodes of in-degree ~400 (> EX_BIG_DEG = 256: walked by a whole wave from the hub list): hub A is an in-neighbour of i,
    hub B of j, and neither hub is within one hop of the other side, so B is first reached from j -- after the hub list was reset.  i2 has A as
    in-neighbour too: as second root of (i, i2) it finds A already expanded."""
    rng = np.random.default_rng(77)
    n, A, B, i, j, i2 = 600, 10, 20, 300, 400, 500
    src = rng.integers(0, n, 1200); dst = rng.integers(0, n, 1200)
    keep = ~np.isin(src, [A, B]) & ~np.isin(dst, [A, B, i, j, i2])          # the hubs' edges and the centres' in-edges are the planted ones only
    src, dst = src[keep], dst[keep]
    others = np.setdiff1d(np.arange(n), [A, B, i, j, i2])
    pa, pb = rng.choice(others, 400, replace=False), rng.choice(others, 395, replace=False)
    low = others[:3]
    src = np.concatenate([src, pa, pb, [A, low[0], B, low[1], A, low[2]]])
    dst = np.concatenate([dst, np.full(400, A), np.full(395, B), [i, i, j, j, i2, i2]])
    graphs = [(n, src.astype(np.int64), dst.astype(np.int64))]
    seeds = np.array([(0, i, j), (0, j, i), (0, i, i2), (0, 50, j), (0, i, 51)], np.int32)
    return dict(graphs=graphs, og=[orc.Graph(*g) for g in graphs], seeds=seeds, hubs=(A, B), centres=(i, j, i2))


def large_case():
    """The 800k-node preferential-attachment graph of tests/test_hip_large_graph.py (too large for the LDS bitmaps: the global-memory bitmap path), eight
    pairs, two of them with a hub (nodes 0..3) on one side."""
    from gmeta_amd import synth
    n = 800_000
    rng = np.random.default_rng(3)
    e = synth.pa_edges(n, 3, rng)
    src = np.concatenate([e[:, 0], e[:, 1]]); dst = np.concatenate([e[:, 1], e[:, 0]])
    r = rng.integers(0, n, 14)
    seeds = np.array([(0, int(r[2 * k]), int(r[2 * k + 1])) for k in range(6)] + [(0, int(r[12]), 1), (0, 2, int(r[13]))], np.int32)
    return dict(graphs=[(n, src, dst)], seeds=seeds, h=2, sample_n=500)


WHOLE_PATH_SEEDS = list(range(4))


def whole_path_case(seed):
    """Inputs of one meta-step in the new mode with an h-layer model: T tasks of C classes on random multigraphs, every pair with j != i."""
    from test_hip_fuzz import _graph
    rng = np.random.default_rng(7000 + seed)
    h = (2, 3, 1, 3)[seed]
    sample_n = (10000, 40, 6, 10000)[seed]
    n_graphs = int(rng.integers(1, 4))
    F0 = int(rng.choice([5, 12, 32]))
    graphs = [_graph(rng, int(rng.integers(25, 160))) for _ in range(n_graphs)]
    feats = [rng.standard_normal((g[0], F0)).astype(np.float32) for g in graphs]
    T, C = int(rng.integers(1, 4)), int(rng.integers(2, 4))
    k_spt, k_qry = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    dims = [F0] + [int(rng.choice([8, 16, 20, 32, 64])) for _ in range(h)]

    def seeds_for(count):
        out = []
        for _ in range(count):
            g = int(rng.integers(0, n_graphs)); n = graphs[g][0]
            i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
            out.append((g, i, j if j != i else (i + 1) % n))
        return np.array(out, np.int32)
    spt = [seeds_for(C * k_spt) for _ in range(T)]
    qry = [seeds_for(C * k_qry) for _ in range(T)]
    return dict(graphs=graphs, og=[orc.Graph(*g) for g in graphs], feats=feats, h=h, sample_n=sample_n, T=T, C=C, k_spt=k_spt, k_qry=k_qry, dims=dims,
                spt_seeds=spt, qry_seeds=qry, rng=rng)


SURFACE_HOPS = (1, 3)
SURFACE = dict(n_graphs=3, n=120, m=2, F0=5, n_way=2, k_spt=2, k_qry=3, tasks=3, sample_nodes=20)


def surface_dataset():
    from gmeta_amd import synth
    s = SURFACE
    return synth.link_dataset(s['n_graphs'], s['n'], s['m'], s['F0'], seed=11)


def surface_query_names(d):
    """Unlabelled pairs for Subgraphs.query_batch: per task, seven query names of one graph."""
    names = d['tables']['train_qry'][0]
    return [[nm for nm in names if nm.startswith('%d_' % g)][:7] for g in range(SURFACE['tasks'])]
