"""CPU (-m "not gpu"): the restatement of the walk-count definition (tests/path_walk_ref.py) against the powers of the dense symmetric matrix, the mask flag
against the powers of the matrix with the one edge removed, the planted case's degrees, and the host helpers that turn walk counts into scores and AUCs."""
import ctypes
import os
import re

import numpy as np
import pytest

import negative_ref
import pair_score_ref
import path_walk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense_S(N, src, dst):
    S = np.zeros((N, N), np.float64)
    S[np.asarray(src), np.asarray(dst)] = 1.0
    S = np.maximum(S, S.T)
    np.fill_diagonal(S, 0.0)
    return S


@pytest.fixture(scope='module')
def multigraph():
    N, src, dst = negative_ref.multigraph_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    pairs = np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing='ij'), -1).reshape(-1, 2)
    return N, src, dst, nb, pairs, ref.pair_walks(N, src, dst, pairs, 0, nb)


def test_every_ordered_pair_equals_the_powers_of_the_dense_matrix(multigraph):
    N, src, dst, nb, pairs, got = multigraph
    S = dense_S(N, src, dst)
    S2 = S @ S
    S3 = S2 @ S
    assert S3.max() < 2.0 ** 53                                               # float64 holds every entry exactly
    want = np.stack([S, S2, S3], -1).reshape(-1, 3).astype(np.int64)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    sq = got.reshape(N, N, 3)
    assert np.array_equal(sq, sq.transpose(1, 0, 2))                          # (a, b) and (b, a): the same row
    deg = pair_score_ref.degrees(N, src, dst).astype(np.int64)
    diag = sq[np.arange(N), np.arange(N)]                                     # a == b: (0, deg, sum over z in G(a) of |G(z) & G(a)|)
    assert np.array_equal(diag[:, 0], np.zeros(N, np.int64)) and np.array_equal(diag[:, 1], deg)
    assert np.array_equal(diag[:, 2], np.array([sum(len(nb[z] & nb[a]) for z in nb[a]) for a in range(N)], np.int64))
    iso = np.nonzero(deg == 0)[0]
    assert len(iso) >= 10 and not sq[iso].any() and not sq[:, iso].any()      # an isolated node: zeros against everybody
    assert got[:, 2].max() > 1000 and (got[:, 2] == 0).any()


def test_masked_rows_equal_the_powers_without_the_edge_and_the_closed_form(multigraph):
    N, src, dst, nb, pairs, plain = multigraph
    got = ref.pair_walks(N, src, dst, pairs, ref.MASK_TARGET, nb)
    S = dense_S(N, src, dst)
    deg = S.sum(1).astype(np.int64)
    adj = (S[pairs[:, 0], pairs[:, 1]] > 0) & (pairs[:, 0] != pairs[:, 1])
    assert adj.sum() > 1000
    assert np.array_equal(got[~adj], plain[~adj])                             # non-adjacent and self pairs: untouched
    for k in np.nonzero(adj)[0].tolist():
        a, b = pairs[k].tolist()
        C = S.copy()
        C[a, b] = C[b, a] = 0.0
        r1 = C[a]
        r2 = r1 @ C
        r3 = r2 @ C
        assert got[k].tolist() == [int(r1[b]), int(r2[b]), int(r3[b])], (a, b)
    da, db = deg[pairs[:, 0]], deg[pairs[:, 1]]
    want = plain.copy()
    want[adj, 0] = 0
    want[adj, 2] -= (da + db - 1)[adj]
    assert np.array_equal(got, want)                                          # the closed form of the definition: w1 = 0, w2 unchanged, w3 loses deg u + deg v - 1


def test_ids_outside_the_graph_and_an_empty_list():
    N, src, dst = negative_ref.multigraph_case()
    got = ref.pair_walks(N, src, dst, [(0, N), (-1, 5), (N, N), (1, 0)])
    assert not got[:3].any() and got[3, 0] in (0, 1) and got[3, 2] > 0
    assert ref.pair_walks(N, src, dst, np.zeros((0, 2), np.int64)).shape == (0, 3)


def test_walk_case_meets_its_degrees_and_its_hubs_meet_long_inner_rows():
    N, src, dst, nodes = ref.walk_case()                                      # (asserts its degrees itself)
    deg = pair_score_ref.degrees(N, src, dst)
    E, M = len(ref.END_ROWS), len(ref.MID_ROWS)
    assert 3200 <= N <= 3400 and len(nodes) == 2 + E + M + 10 == len(set(nodes))
    assert deg[nodes[:2]].tolist() == [ref.HUB_ROW] * 2 and tuple(deg[nodes[2:2 + E]].tolist()) == ref.END_ROWS
    assert tuple(deg[nodes[2 + E:2 + E + M]].tolist()) == ref.MID_ROWS
    assert (src == dst).sum() >= 5 and len(set(zip(src.tolist(), dst.tolist()))) < len(src)
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    assert set(nodes[2 + E:2 + E + M]) <= nb[0] & nb[1]                       # the middle hubs lie between the two hubs
    hub = ref.pair_walks(N, src, dst, [(0, 1), (1, 0)], 0, nb)
    cut = ref.pair_walks(N, src, dst, [(0, 1)], 1, nb)
    assert hub[0].tolist() == hub[1].tolist() and hub[0, 0] == 1 and hub[0, 1] > 2000 and hub[0, 2] > 10000
    assert cut[0].tolist() == [0, int(hub[0, 1]), int(hub[0, 2]) - (2 * ref.HUB_ROW - 1)]


def test_path_indices_on_hand_computed_rows():
    import gmeta_amd
    walks = np.array([[1, 2, 10], [0, 0, 0], [0, 3, 200]], np.int64)
    assert gmeta_amd.PATH_SCORES == ('local_path', 'katz')
    lp = gmeta_amd.local_path_index(walks)
    assert lp.dtype == np.float64 and lp.tolist() == [2 + 0.01 * 10, 0.0, 3 + 0.01 * 200]
    assert gmeta_amd.local_path_index(walks, eps=0.5).tolist() == [7.0, 0.0, 103.0]
    kz = gmeta_amd.katz_index(walks)
    b = 0.005
    assert kz.dtype == np.float64 and kz.tolist() == [b * 1 + b ** 2 * 2 + b ** 3 * 10, 0.0, b * 0 + b ** 2 * 3 + b ** 3 * 200]
    assert gmeta_amd.katz_index(walks, beta=0.5).tolist() == [0.5 + 0.5 + 1.25, 0.0, 0.75 + 25.0]
    assert gmeta_amd.katz_index(np.zeros((0, 3), np.int64)).shape == (0,)
    big = np.array([[0, 0, 2 ** 53 + 2]], np.int64)                           # the integers are read as int64, not through float32
    assert gmeta_amd.local_path_index(big, eps=1.0)[0] == float(2 ** 53 + 2)


class _HostStore:
    """GraphStore.pair_walks on the restatement (host logic of link_path_auc; no GPU)."""

    def __init__(self, graphs):
        self.graphs, self.calls = graphs, []

    def pair_walks(self, g, pairs, mask_target=False):
        self.calls.append((g, len(pairs), mask_target))
        N, src, dst = self.graphs[g]
        return ref.pair_walks(N, src, dst, pairs, 1 if mask_target else 0)


def test_link_path_auc_scores_each_graph_once_and_keeps_the_order():
    import gmeta_amd
    rng = np.random.default_rng(2)
    graphs = [(30, rng.integers(0, 30, 120), rng.integers(0, 30, 120)), (20, rng.integers(0, 20, 70), rng.integers(0, 20, 70))]
    names, labels, rows = [], [], []
    for k in range(90):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, graphs[g][0], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b)); labels.append(str(k % 2))
        rows.append(ref.pair_walks(*graphs[g], [(a, b)], 1)[0])
    rows = np.asarray(rows)
    store = _HostStore(graphs)
    assert np.array_equal(gmeta_amd.link_path_scores(store, names, mask_target=True), rows)
    store.calls.clear()
    got = gmeta_amd.link_path_auc(store, names, labels, mask_target=True)
    assert sorted(c[0] for c in store.calls) == [0, 1] and all(c[2] for c in store.calls) and sum(c[1] for c in store.calls) == 90
    assert tuple(got) == gmeta_amd.PATH_SCORES
    assert got['local_path'] == gmeta_amd.link_auc(rows[:, 1] + 0.01 * rows[:, 2], labels)
    assert got['katz'] == gmeta_amd.link_auc(0.005 * rows[:, 0] + 0.005 ** 2 * rows[:, 1] + 0.005 ** 3 * rows[:, 2], labels)
    other = gmeta_amd.link_path_auc(store, names, labels, mask_target=False, eps=0.5, beta=0.3)
    plain = np.asarray([ref.pair_walks(*graphs[int(nm.split('_')[0])], [[int(x) for x in nm.split('_')[1:]]], 0)[0] for nm in names])
    assert other['local_path'] == gmeta_amd.link_auc(plain[:, 1] + 0.5 * plain[:, 2], labels)
    assert other['katz'] == gmeta_amd.link_auc(gmeta_amd.katz_index(plain, 0.3), labels)
    with pytest.raises(ValueError, match='g_i_j'):
        gmeta_amd.link_path_auc(store, ['0_1'], ['1'])
    assert len(gmeta_amd.PAIR_SCORES) == 5                                    # the five-score call keeps its keys


def test_the_export_is_declared_bound_and_tunable():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r'\bgm_store_pair_walks\s*\(', code) and hasattr(lib, 'gm_store_pair_walks')
    assert len(_lib.PROTOTYPES['gm_store_pair_walks'][1]) == 7 and hasattr(gmeta_amd.GraphStore, 'pair_walks')
    assert open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read().rstrip().split('SOURCES += ')[-1].startswith("['pair_walks.hip']")      # last in the list
    for name, values in ((b'walk_chunk', (1, 63, 2 ** 30, 0)), (b'walk_lanes', (32, 64, 0))):
        for v in values:
            assert _lib.lib().gm_set_tuning(name, v) == 0 and _lib.lib().gm_get_tuning(name) == v
    assert _lib.lib().gm_set_tuning(b'GM_WALK_CHUNK', 5) == 0 and _lib.lib().gm_get_tuning(b'walk_chunk') == 5
    assert _lib.lib().gm_set_tuning(b'walk_chunk', 0) == 0


def test_train_flag_takes_the_path_scores():
    import train as drv
    base = ['--data_dir', 'x', '--task_setup', 'Shared']
    assert drv.parse(base + ['--link_pred_mode', 'True', '--heuristics', '2']).heuristics == 2
    assert drv.parse(base + ['--heuristics', '1']).heuristics == 1 and drv.parse(base).heuristics == 0
    with pytest.raises(SystemExit, match='link_pred_mode'):
        drv.parse(base + ['--heuristics', '2'])                               # node tasks have no pairs to score
    with pytest.raises(SystemExit):
        drv.parse(base + ['--link_pred_mode', 'True', '--heuristics', '3'])
