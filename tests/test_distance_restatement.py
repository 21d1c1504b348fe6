"""CPU (-m "not gpu"): the restatement of the shortest-path-distance definition (tests/distance_ref.py) against closed forms and against the walk counts of
path_walk_ref, the level-1 shortcut the kernels use for a masked column against the search with the edge really removed, the host helpers that turn the
bytes into a score and an AUC, and the declarations, knobs and driver flag of the feature.  No compute call of the library: that needs a GPU
(tests/test_hip_pair_distance.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import distance_ref as ref
import negative_ref
import pair_score_ref
import path_walk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ref.UNREACHED


def _both(e):
    return np.array([a for a, _ in e], np.int64), np.array([b for _, b in e], np.int64)


def test_a_path_a_star_two_components_and_a_single_node():
    N = 12
    src, dst = _both([(k + 1, k) if k % 2 else (k, k + 1) for k in range(N - 1)])
    for max_dist in (1, 5, 11, 254):
        want = np.abs(np.arange(N)[:, None] - np.arange(N)[None, :])
        want = np.where(want > max_dist, U, want).astype(np.uint8)
        assert np.array_equal(ref.node_distances(N, src, dst, np.arange(N), max_dist), want)
    pairs = np.array([(a, b) for a in range(N) for b in range(N)])
    plain, masked = ref.pair_distance(N, src, dst, pairs, 0, 254), ref.pair_distance(N, src, dst, pairs, 1, 254)
    adj = np.abs(pairs[:, 0] - pairs[:, 1]) == 1
    assert np.array_equal(plain, np.abs(pairs[:, 0] - pairs[:, 1])) and (masked[adj] == U).all() and np.array_equal(masked[~adj], plain[~adj])      # every edge a bridge
    # a star: centre 0
    src, dst = _both([(0, k) for k in range(1, 7)])
    d = ref.node_distances(7, src, dst, [0, 3], 8)
    assert d[0].tolist() == [0, 1, 1, 1, 1, 1, 1] and d[1].tolist() == [1, 2, 2, 0, 2, 2, 2]
    assert ref.node_distances(7, src, dst, [3], 1)[0].tolist() == [1, U, U, 0, U, U, U]
    assert ref.pair_distance(7, src, dst, [(0, 3), (3, 4), (3, 3)], 1).tolist() == [U, 2, 0]
    # two components, self loops and a doubled edge
    src, dst = _both([(0, 1), (1, 0), (1, 2), (3, 4), (4, 4), (2, 2)])
    d = ref.node_distances(5, src, dst, np.arange(5), 8)
    assert d.tolist() == [[0, 1, 2, U, U], [1, 0, 1, U, U], [2, 1, 0, U, U], [U, U, U, 0, 1], [U, U, U, 1, 0]]
    assert ref.pair_distance(5, src, dst, [(4, 4), (2, 2)], 1).tolist() == [0, 0]                  # a == b: 0 with either flag, a self loop is no edge
    # one node
    none = np.zeros(0, np.int64)
    assert ref.node_distances(1, none, none, [0, 0, 1, -1], 3).tolist() == [[0], [0], [U], [U]]
    assert ref.pair_distance(1, none, none, [(0, 0), (0, 1)], 1, 3).tolist() == [0, U]
    assert ref.node_distances(1, none, none, [], 3).shape == (0, 1) and ref.pair_distance(1, none, none, np.zeros((0, 2)), 0, 3).shape == (0,)


@pytest.mark.parametrize('L', [3, 4, 9])
def test_a_cycle_and_its_masked_edges(L):
    src, dst = _both([(k, (k + 1) % L) for k in range(L)])
    ring = np.minimum(np.arange(L), L - np.arange(L))
    assert np.array_equal(ref.node_distances(L, src, dst, [0], 254)[0], ring)
    for k in range(L):
        pair = [(k, (k + 1) % L)]
        assert ref.pair_distance(L, src, dst, pair, 0, 254).tolist() == [1]
        assert ref.pair_distance(L, src, dst, pair, 1, 254).tolist() == [L - 1]                    # the long way round
        assert ref.pair_distance(L, src, dst, pair, 1, L - 1).tolist() == [L - 1] and (L == 3 or ref.pair_distance(L, src, dst, pair, 1, L - 2).tolist() == [U])


def test_the_chain_case_holds_every_class():
    N, src, dst, L = ref.chain_case()
    assert N % 64 != 0 and L == 67
    d = ref.node_distances(N, src, dst, [0], 254)[0]
    assert d[:255].tolist() == list(range(255)) and (d[255:260] == U).all() and d[327] == 1 and (d[329:] == U).all()      # 254 reads 254, 255 .. 259 unreached
    assert ref.node_distances(N, src, dst, [259], 254)[0][0] == U and ref.node_distances(N, src, dst, [259], 254)[0][5] == 254
    assert ref.pair_distance(N, src, dst, [(40, 41), (100, 260), (0, 327)], 1, 254).tolist() == [U, U, U]                    # bridges
    assert ref.pair_distance(N, src, dst, [(270, 271), (260, 326)], 1, 254).tolist() == [L - 1, L - 1]                       # cycle edges
    assert ref.pair_distance(N, src, dst, [(328, 100)], 0, 254).tolist() == [1 + 30 + 1]


def test_against_the_walk_counts_on_the_multigraph():
    """d == k for k in 1..3 exactly when the first non-zero walk count is w_k; d > 3 or unreached exactly when all three are zero (u != v)."""
    N, src, dst = negative_ref.multigraph_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    pairs = np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing='ij'), -1).reshape(-1, 2)
    off = pairs[:, 0] != pairs[:, 1]
    counts = {}
    for flags in (0, 1):
        w = path_walk_ref.pair_walks(N, src, dst, pairs, flags, nb)
        d = ref.pair_distance(N, src, dst, pairs, flags, 254, nb)
        first = np.where(w[:, 0] > 0, 1, np.where(w[:, 1] > 0, 2, np.where(w[:, 2] > 0, 3, 0)))
        assert np.array_equal(np.where(d[off] <= 3, d[off], 0), first[off]) and not d[~off].any()
        for max_dist in (1, 2, 3):
            assert np.array_equal(ref.pair_distance(N, src, dst, pairs, flags, max_dist, nb), np.where(d <= max_dist, d, U))
        counts[flags] = d
    d = counts[0][off]
    assert [int((d == k).sum()) for k in (1, 2, 3, 4)] == [2612, 65896, 15104, 198] and int((d == U).sum()) == 5890 and d[d != U].max() == 4
    m = counts[1][off][d == 1]
    assert len(m) == 2 * 1306 and [int((m == k).sum()) for k in (2, 3, 4)] == [2 * 1137, 2 * 166, 2 * 3]


def test_the_level_one_shortcut_of_the_kernels_is_the_search_without_the_edge():
    """pair_distance.hip searches a masked column (s, x) in the WHOLE graph and clears x's bit in next and seen behind level 1 (the proof is in its header
    comment).  The same levels on boolean matrices, every adjacent ordered pair of the multigraph and of the chain as a column, against the restatement."""
    for N, src, dst in (negative_ref.multigraph_case(), ref.chain_case()[:3]):
        nb = pair_score_ref.neighbourhoods(N, src, dst)
        S = np.zeros((N, N), bool)
        for v, row in enumerate(nb):
            S[v, list(row)] = True
        cols = [(s, x) for s in range(N) for x in sorted(nb[s])]
        cs, cx = np.array([c[0] for c in cols]), np.array([c[1] for c in cols])
        k = np.arange(len(cols))
        seen = np.zeros((N, len(cols)), bool)
        seen[cs, k] = True
        front, d = seen.copy(), np.full((N, len(cols)), U, np.uint8)
        d[cs, k] = 0
        for t in range(1, 255):
            nxt = (S.astype(np.float32) @ front.astype(np.float32) > 0) & ~seen
            if t == 1:
                nxt[cx, k] = False
            if not nxt.any():
                break
            seen |= nxt
            d[nxt] = t
            front = nxt
        want = np.stack([ref.column(N, nb, s, x, 254) for s, x in cols], 1)
        assert np.array_equal(d, want)


def test_graph_distance_index_ranks_closer_higher_and_unreached_last():
    import gmeta_amd
    assert gmeta_amd.DISTANCE_SCORES == ('graph_distance',) and gmeta_amd.DIST_UNREACHED == U == 255
    for name in ('DISTANCE_SCORES', 'DIST_UNREACHED', 'graph_distance_index', 'link_distance_scores', 'link_distance_auc'):
        assert name in gmeta_amd.__all__ and hasattr(gmeta_amd, name)
    got = gmeta_amd.graph_distance_index(np.array([0, 1, 8, 255, 3], np.uint8), 8)
    assert got.dtype == np.float64 and got.tolist() == [0.0, -1.0, -8.0, -9.0, -3.0]
    assert gmeta_amd.graph_distance_index(np.array([254, 255], np.uint8), 254).tolist() == [-254.0, -255.0]
    assert gmeta_amd.graph_distance_index(np.zeros(0, np.uint8), 8).shape == (0,)
    assert gmeta_amd.PAIR_SCORES == ('cn', 'jaccard', 'adamic_adar', 'resource_allocation', 'pref_attachment') and gmeta_amd.PATH_SCORES == ('local_path', 'katz')
    assert gmeta_amd.PAGERANK_SCORES == ('rooted_pagerank',)


class _HostStore:
    """GraphStore.pair_distance on the restatement (host logic of link_distance_auc; no GPU)."""

    def __init__(self, graphs):
        self.graphs, self.calls = graphs, []

    def pair_distance(self, g, pairs, mask_target=False, max_dist=8):
        self.calls.append((g, len(pairs), mask_target, max_dist))
        N, src, dst = self.graphs[g]
        return ref.pair_distance(N, src, dst, pairs, 1 if mask_target else 0, max_dist)


def test_link_distance_auc_scores_each_graph_once_and_keeps_the_order():
    import gmeta_amd
    rng = np.random.default_rng(2)
    graphs = [(30, rng.integers(0, 30, 40), rng.integers(0, 30, 40)), (20, rng.integers(0, 20, 25), rng.integers(0, 20, 25))]
    names, labels, rows = [], [], []
    for k in range(90):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, graphs[g][0], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b)); labels.append(str(k % 2))
        rows.append(ref.pair_distance(*graphs[g], [(a, b)], 1, 3)[0])
    rows = np.asarray(rows, np.uint8)
    assert (rows == U).any() and (rows == 2).any()
    store = _HostStore(graphs)
    got = gmeta_amd.link_distance_scores(store, names, mask_target=True, max_dist=3)
    assert got.dtype == np.uint8 and np.array_equal(got, rows)
    store.calls.clear()
    auc = gmeta_amd.link_distance_auc(store, names, labels, mask_target=True, max_dist=3)
    assert sorted(c[0] for c in store.calls) == [0, 1] and all(c[2:] == (True, 3) for c in store.calls) and sum(c[1] for c in store.calls) == 90
    assert tuple(auc) == gmeta_amd.DISTANCE_SCORES
    score = gmeta_amd.graph_distance_index(rows, 3)
    assert auc['graph_distance'] == gmeta_amd.link_auc(score, labels) == pytest.approx(pair_score_ref.auc_by_pair_count(score, labels), abs=1e-12)      # ties: one half
    store.calls.clear()
    gmeta_amd.link_distance_auc(store, names, labels)
    assert all(c[2:] == (False, 8) for c in store.calls)
    with pytest.raises(ValueError, match='g_i_j'):
        gmeta_amd.link_distance_auc(store, ['0_1'], ['1'])
    with pytest.raises(ValueError, match='both labels'):
        gmeta_amd.link_distance_auc(store, names[:4], ['1'] * 4)


def test_graphstore_methods_refuse_bad_arguments_before_the_library():
    """No GPU and no store behind the object: the checks come first."""
    import gmeta_amd
    store = object.__new__(gmeta_amd.GraphStore)
    store.handle, store.n_graphs, store.n_nodes = None, 1, [10]
    for max_dist in (0, 255, -1, 1000):
        with pytest.raises(ValueError, match='max_dist = %d' % max_dist):
            store.node_distances(0, [1], max_dist=max_dist)
        with pytest.raises(ValueError, match='max_dist = %d' % max_dist):
            store.pair_distance(0, [[1, 2]], max_dist=max_dist)
    with pytest.raises(ValueError, match='graph 1'):
        store.node_distances(1, [1])
    with pytest.raises(ValueError, match='outside'):
        store.node_distances(0, [10])
    with pytest.raises(ValueError, match='outside'):
        store.pair_distance(0, [[0, -1]])


def test_the_exports_are_declared_bound_and_tunable():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (('gm_store_node_distances', 7), ('gm_store_pair_distance', 8)):
        assert re.search(r'\b%s\s*\(' % name, code) and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    assert re.search(r'#define\s+GM_DIST_UNREACHED\s+255\b', code) and _lib.DIST_UNREACHED == 255
    assert hasattr(gmeta_amd.GraphStore, 'node_distances') and hasattr(gmeta_amd.GraphStore, 'pair_distance')
    build = open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert build.count("'pair_distance.hip'") == 1 and build.index("'pair_pagerank.hip'") < build.index("'pair_distance.hip'") < build.index("'pair_walks.hip'")
    for name, values in ((b'dist_chunk', (1, 63, 2 ** 30, 0)), (b'dist_cols', (64, 128, 4096, 0))):
        for v in values:
            assert _lib.lib().gm_set_tuning(name, v) == 0 and _lib.lib().gm_get_tuning(name) == v
    assert _lib.lib().gm_set_tuning(b'GM_DIST_CHUNK', 5) == 0 and _lib.lib().gm_get_tuning(b'dist_chunk') == 5
    assert _lib.lib().gm_set_tuning(b'GM_DIST_COLS', 192) == 0 and _lib.lib().gm_get_tuning(b'dist_cols') == 192
    assert _lib.lib().gm_set_tuning(b'dist_chunk', 0) == 0 and _lib.lib().gm_set_tuning(b'dist_cols', 0) == 0


def test_train_flag_takes_the_distance_score():
    import train as drv
    base = ['--data_dir', 'x', '--task_setup', 'Shared']
    assert drv.parse(base + ['--link_pred_mode', 'True', '--distance', '8']).distance == 8
    assert drv.parse(base + ['--link_pred_mode', 'True', '--distance', '254']).distance == 254
    assert drv.parse(base).distance == 0 and drv.parse(base + ['--link_pred_mode', 'True']).distance == 0
    all3 = drv.parse(base + ['--link_pred_mode', 'True', '--distance', '4', '--pagerank', '1', '--heuristics', '2'])
    assert all3.distance == 4 and all3.pagerank == 1 and all3.heuristics == 2          # independent of the other two
    with pytest.raises(SystemExit, match='link_pred_mode'):
        drv.parse(base + ['--distance', '8'])                                         # node tasks have no pairs to score
    for bad in ('255', '-1'):
        with pytest.raises(SystemExit, match='distance'):
            drv.parse(base + ['--link_pred_mode', 'True', '--distance', bad])
    with pytest.raises(SystemExit):
        drv.parse(base + ['--link_pred_mode', 'True', '--pagerank', '2'])             # the pinned choices stay
    with pytest.raises(SystemExit):
        drv.parse(base + ['--link_pred_mode', 'True', '--heuristics', '3'])
