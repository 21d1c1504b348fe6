"""CPU (-m "not gpu"): the restatement of the rooted-PageRank definition (tests/pagerank_ref.py) against the closed form from dense matrix powers, the mask
flag against the restatement on an edge list without the edge, the host helpers that turn the two columns into a score and an AUC, and the declarations,
knobs and driver flag of the feature.  No compute call of the library: that needs a GPU (tests/test_hip_pair_pagerank.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import negative_ref
import pagerank_ref as ref
import pair_score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, ITERS = 0.15, 20


def dense_M(N, src, dst):
    """M[v, z] = 1 / deg z for z in G(v); M[v, v] = 1 for a node without neighbours."""
    S = np.zeros((N, N), np.float64)
    S[np.asarray(src), np.asarray(dst)] = 1.0
    S = np.maximum(S, S.T)
    np.fill_diagonal(S, 0.0)
    deg = S.sum(0)
    M = S / np.maximum(deg, 1.0)[None, :]
    M[deg == 0, deg == 0] = 1.0
    return M, deg.astype(np.int64)


def closed_form(M, alpha, iters):
    """column s = a sum_{t < T} b^t M^t e_s + b^T M^T e_s, for every s at once"""
    a, b = ref.constants(alpha)
    P, acc = np.eye(len(M)), np.zeros_like(M)
    for _ in range(iters):
        acc += a * P
        P = b * (M @ P)
    return acc + P


def mass(alpha, iters):
    """sum_v p_iters[v] of the definition: S_0 = 1, S_{t+1} = a + b S_t"""
    a, b = ref.constants(alpha)
    S = 1.0
    for _ in range(iters):
        S = a + b * S
    return S


@pytest.fixture(scope='module', params=['multigraph', 'dense'])
def case(request):
    N, src, dst = negative_ref.multigraph_case() if request.param == 'multigraph' else negative_ref.dense_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    return request.param, N, src, dst, nb, ref.rooted_pagerank(N, src, dst, np.arange(N), ALPHA, ITERS, nb)


def test_every_source_equals_the_closed_form_and_sums_to_one(case):
    name, N, src, dst, nb, got = case
    M, deg = dense_M(N, src, dst)
    want = closed_form(M, ALPHA, ITERS).T                                     # row s = the vector of source s
    assert got.shape == (N, N) and got.dtype == np.float64
    assert np.abs(got - want).max() < 1e-12
    # The walk keeps the mass: sum p_{t+1} = a + b sum p_t.  b = 1.0f - a is ROUNDED, so for alpha = 0.15 a + b is 1 + 2.9e-8, not 1, and the float64 mass of
    # the definition after 20 steps is 1 + 1.9e-7; with a + b == 1 exactly (alpha = 0.5, 0.25) it is 1.
    assert np.abs(got.sum(1) - mass(ALPHA, ITERS)).max() < 1e-12 and (got >= 0).all() and abs(mass(ALPHA, ITERS) - 1.0) < 2.0 ** -24 / 0.15
    for alpha in (0.5, 0.25):
        exact = ref.rooted_pagerank(N, src, dst, np.arange(N), alpha, ITERS, nb)
        assert mass(alpha, ITERS) == 1.0 and np.abs(exact.sum(1) - 1.0).max() < 1e-12
        if name == 'multigraph':
            assert np.array_equal(exact[290:], np.eye(N)[290:])               # an isolated source: e_s
    if name == 'multigraph':
        assert (deg[290:] == 0).all()
        assert np.array_equal(got[290:], mass(ALPHA, ITERS) * np.eye(N)[290:])      # an isolated source keeps all of the mass
        assert not got[:290, 290:].any()                                      # and nobody reaches it
    for iters in (1, 2, 7):
        few = ref.rooted_pagerank(N, src, dst, [0, 3, N - 1], ALPHA, iters, nb)
        assert np.abs(few - closed_form(M, ALPHA, iters).T[[0, 3, N - 1]]).max() < 1e-12
    other = ref.rooted_pagerank(N, src, dst, [2], 0.5, 9, nb)
    assert np.abs(other[0] - closed_form(M, 0.5, 9)[:, 2]).max() < 1e-12


def test_one_iteration_by_hand(case):
    _, N, src, dst, nb, _ = case
    a, b = ref.constants(ALPHA)
    assert a == float(np.float32(0.15)) and b == float(np.float32(1.0) - np.float32(0.15)) and a != 0.15
    for s in (0, 1, 7, N - 1):
        got = ref.rooted_pagerank(N, src, dst, [s], ALPHA, 1, nb)[0]
        want = np.zeros(N)
        if nb[s]:
            for v in nb[s]:
                want[v] = b * (1.0 / len(nb[s]))                          # p_0[s] / deg s first, as the definition scales
            want[s] = a
        else:
            want[s] = a + b
        assert np.array_equal(got, want)


def test_masked_pairs_equal_the_restatement_without_the_edge(case):
    name, N, src, dst, nb, plain = case
    rng = np.random.default_rng(3)
    adj = [(u, v) for u in range(N) for v in sorted(nb[u]) if u < v]
    assert len(adj) > 300
    some = [adj[k] for k in rng.choice(len(adj), 25, replace=False)] + ([(0, 1)] if 1 in nb[0] else [])
    for u, v in some:
        keep = ~(((src == u) & (dst == v)) | ((src == v) & (dst == u)))       # every copy of the edge, in both directions
        assert keep.sum() < len(src)
        want = ref.pair_pagerank(N, src[keep], dst[keep], [(u, v)], 0, ALPHA, ITERS)
        got = ref.pair_pagerank(N, src, dst, [(u, v)], ref.MASK_TARGET, ALPHA, ITERS, nb)
        assert np.array_equal(got, want), (u, v)
        assert np.array_equal(ref.pair_pagerank(N, src, dst, [(v, u)], ref.MASK_TARGET, ALPHA, ITERS, nb), got)
        assert not np.array_equal(got, ref.pair_pagerank(N, src, dst, [(u, v)], 0, ALPHA, ITERS, nb))


def test_a_leaf_whose_only_edge_is_masked_is_isolated():
    N, src, dst = 5, np.array([0, 1, 2, 1]), np.array([1, 2, 3, 0])           # the path 0 - 1 - 2 - 3 (0 - 1 twice), node 4 alone
    for pair in ((0, 1), (1, 0), (2, 3)):
        assert not ref.pair_pagerank(N, src, dst, [pair], ref.MASK_TARGET, ALPHA, ITERS).any()      # no walk joins the two any more
        assert (ref.pair_pagerank(N, src, dst, [pair], 0, ALPHA, ITERS) > 0).all()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    assert np.array_equal(ref.column(N, nb, 0, 1, ALPHA, 3), ref.column(N, nb, 4, -1, ALPHA, 3)[[4, 1, 2, 3, 0]])      # the cut leaf walks as the lone node does


def test_unmasked_pairs_read_the_vectors_and_non_adjacent_pairs_ignore_the_flag(case):
    _, N, src, dst, nb, plain = case
    rng = np.random.default_rng(5)
    pairs = np.concatenate([rng.integers(0, N, (400, 2)), np.array([(4, 4), (0, 1), (1, 0), (N - 1, N - 1)])])
    got = ref.pair_pagerank(N, src, dst, pairs, 0, ALPHA, ITERS, nb)
    u, v = pairs.min(1), pairs.max(1)
    assert np.array_equal(got[:, 0], plain[u, v]) and np.array_equal(got[:, 1], plain[v, u])
    assert np.array_equal(got, ref.pair_pagerank(N, src, dst, pairs[:, ::-1], 0, ALPHA, ITERS, nb))      # (a, b) equals (b, a)
    masked = ref.pair_pagerank(N, src, dst, pairs, ref.MASK_TARGET, ALPHA, ITERS, nb)
    far = np.array([b not in nb[a] for a, b in pairs.tolist()])
    assert far.any() and (~far).any()
    assert np.array_equal(masked[far], got[far])                              # non-adjacent and self pairs: exactly the unmasked result
    assert (masked[~far] != got[~far]).any(1).all()


def test_ids_outside_the_graph_and_empty_lists():
    N, src, dst = negative_ref.multigraph_case()
    got = ref.pair_pagerank(N, src, dst, [(0, N), (-1, 5), (N, N), (1, 0)])
    assert not got[:3].any() and (got[3] > 0).all()
    vec = ref.rooted_pagerank(N, src, dst, [N, -1, 0, 0])
    assert not vec[:2].any() and np.array_equal(vec[2], vec[3]) and abs(vec[2].sum() - mass(0.15, 20)) < 1e-12
    assert ref.pair_pagerank(N, src, dst, np.zeros((0, 2), np.int64)).shape == (0, 2)
    assert ref.rooted_pagerank(N, src, dst, []).shape == (0, N)


def test_rooted_pagerank_index_is_the_float64_sum():
    import gmeta_amd
    assert gmeta_amd.PAGERANK_SCORES == ('rooted_pagerank',)
    for name in ('PAGERANK_SCORES', 'rooted_pagerank_index', 'link_pagerank_scores', 'link_pagerank_auc'):
        assert name in gmeta_amd.__all__ and hasattr(gmeta_amd, name)
    assert gmeta_amd.PAIR_SCORES == ('cn', 'jaccard', 'adamic_adar', 'resource_allocation', 'pref_attachment') and gmeta_amd.PATH_SCORES == ('local_path', 'katz')
    cols = np.array([[0.25, 0.5], [0.0, 0.0], [1.0, 2.0 ** -30]], np.float32)
    got = gmeta_amd.rooted_pagerank_index(cols)
    assert got.dtype == np.float64 and got.tolist() == [0.75, 0.0, 1.0 + 2.0 ** -30]      # the sum is not rounded to fp32
    assert gmeta_amd.rooted_pagerank_index(np.zeros((0, 2), np.float32)).shape == (0,)


class _HostStore:
    """GraphStore.pair_pagerank on the restatement (host logic of link_pagerank_auc; no GPU)."""

    def __init__(self, graphs):
        self.graphs, self.calls = graphs, []

    def pair_pagerank(self, g, pairs, mask_target=False, alpha=0.15, iters=20):
        self.calls.append((g, len(pairs), mask_target, alpha, iters))
        N, src, dst = self.graphs[g]
        return ref.pair_pagerank(N, src, dst, pairs, 1 if mask_target else 0, alpha, iters).astype(np.float32)


def test_link_pagerank_auc_scores_each_graph_once_and_keeps_the_order():
    import gmeta_amd
    rng = np.random.default_rng(2)
    graphs = [(30, rng.integers(0, 30, 120), rng.integers(0, 30, 120)), (20, rng.integers(0, 20, 70), rng.integers(0, 20, 70))]
    names, labels, rows = [], [], []
    for k in range(90):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, graphs[g][0], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b)); labels.append(str(k % 2))
        rows.append(ref.pair_pagerank(*graphs[g], [(a, b)], 1)[0])
    rows = np.asarray(rows).astype(np.float32)
    store = _HostStore(graphs)
    assert np.array_equal(gmeta_amd.link_pagerank_scores(store, names, mask_target=True), rows)
    store.calls.clear()
    got = gmeta_amd.link_pagerank_auc(store, names, labels, mask_target=True)
    assert sorted(c[0] for c in store.calls) == [0, 1] and all(c[2:] == (True, 0.15, 20) for c in store.calls) and sum(c[1] for c in store.calls) == 90
    assert tuple(got) == gmeta_amd.PAGERANK_SCORES
    score = rows.astype(np.float64).sum(1)
    assert got['rooted_pagerank'] == gmeta_amd.link_auc(score, labels) == pytest.approx(pair_score_ref.auc_by_pair_count(score, labels), abs=1e-12)
    store.calls.clear()
    other = gmeta_amd.link_pagerank_auc(store, names, labels, mask_target=False, alpha=0.5, iters=3)
    assert all(c[2:] == (False, 0.5, 3) for c in store.calls)
    plain = np.asarray([ref.pair_pagerank(*graphs[int(nm.split('_')[0])], [[int(x) for x in nm.split('_')[1:]]], 0, 0.5, 3)[0] for nm in names]).astype(np.float32)
    assert other['rooted_pagerank'] == gmeta_amd.link_auc(plain.astype(np.float64).sum(1), labels)
    with pytest.raises(ValueError, match='g_i_j'):
        gmeta_amd.link_pagerank_auc(store, ['0_1'], ['1'])
    with pytest.raises(ValueError, match='both labels'):
        gmeta_amd.link_pagerank_auc(store, names[:4], ['1'] * 4)


def test_graphstore_methods_refuse_bad_arguments_before_the_library():
    """No GPU and no store behind the object: the checks come first."""
    import gmeta_amd
    store = object.__new__(gmeta_amd.GraphStore)
    store.handle, store.n_graphs, store.n_nodes = None, 1, [10]
    for alpha in (0.0, 1.0, -0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='alpha'):
            store.rooted_pagerank(0, [1], alpha=alpha)
        with pytest.raises(ValueError, match='alpha'):
            store.pair_pagerank(0, [[1, 2]], alpha=alpha)
    for iters in (0, 256, -1):
        with pytest.raises(ValueError, match='iters = %d' % iters):
            store.rooted_pagerank(0, [1], iters=iters)
        with pytest.raises(ValueError, match='iters = %d' % iters):
            store.pair_pagerank(0, [[1, 2]], iters=iters)
    with pytest.raises(ValueError, match='graph 1'):
        store.rooted_pagerank(1, [1])
    with pytest.raises(ValueError, match='outside'):
        store.rooted_pagerank(0, [10])


def test_the_exports_are_declared_bound_and_tunable():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (('gm_store_rooted_pagerank', 8), ('gm_store_pair_pagerank', 9)):
        assert re.search(r'\b%s\s*\(' % name, code) and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args and ctypes.c_float in _lib.PROTOTYPES[name][1]
    assert hasattr(gmeta_amd.GraphStore, 'rooted_pagerank') and hasattr(gmeta_amd.GraphStore, 'pair_pagerank')
    build = open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert build.count("'pair_pagerank.hip'") == 1 and build.index("'pair_pagerank.hip'") > build.index("'candidates.hip'")      # a translation unit of its own, behind the index's
    for name, values in ((b'ppr_chunk', (1, 63, 2 ** 30, 0)), (b'ppr_cols', (64, 128, 256, 0))):
        for v in values:
            assert _lib.lib().gm_set_tuning(name, v) == 0 and _lib.lib().gm_get_tuning(name) == v
    assert _lib.lib().gm_set_tuning(b'GM_PPR_CHUNK', 5) == 0 and _lib.lib().gm_get_tuning(b'ppr_chunk') == 5
    assert _lib.lib().gm_set_tuning(b'GM_PPR_COLS', 192) == 0 and _lib.lib().gm_get_tuning(b'ppr_cols') == 192
    assert _lib.lib().gm_set_tuning(b'ppr_chunk', 0) == 0 and _lib.lib().gm_set_tuning(b'ppr_cols', 0) == 0


def test_train_flag_takes_the_pagerank_score():
    import train as drv
    base = ['--data_dir', 'x', '--task_setup', 'Shared']
    assert drv.parse(base + ['--link_pred_mode', 'True', '--pagerank', '1']).pagerank == 1
    assert drv.parse(base).pagerank == 0 and drv.parse(base + ['--link_pred_mode', 'True']).pagerank == 0
    both = drv.parse(base + ['--link_pred_mode', 'True', '--pagerank', '1', '--heuristics', '2'])
    assert both.pagerank == 1 and both.heuristics == 2                        # independent of --heuristics
    with pytest.raises(SystemExit, match='link_pred_mode'):
        drv.parse(base + ['--pagerank', '1'])                                 # node tasks have no pairs to score
    with pytest.raises(SystemExit):
        drv.parse(base + ['--link_pred_mode', 'True', '--pagerank', '2'])
    with pytest.raises(SystemExit):
        drv.parse(base + ['--link_pred_mode', 'True', '--heuristics', '3'])   # the heuristics flag keeps its three choices
