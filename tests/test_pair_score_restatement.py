"""CPU (-m "not gpu"): the restatement of the pair-score definition (tests/pair_score_ref.py) against a brute-force dense matrix and hand-computed
cases; the mask flag; link_auc against the O(n^2) pair count; the C ABI surface and the driver flag."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import negative_ref
import pair_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CN, JAC, AA, RA, PA = range(5)


def dense_scores(N, src, dst, pairs, flags=0):
    """Independent of pair_score_ref.pair_scores: S = (A or A^T) with a zero diagonal; cn = (S S)[a, b], the weighted sums = (S diag(w) S)[a, b]."""
    S = np.zeros((N, N), np.float64)
    S[np.asarray(src), np.asarray(dst)] = 1.0
    S = np.maximum(S, S.T)
    np.fill_diagonal(S, 0.0)
    deg = S.sum(1).astype(np.int64)
    aa = np.array([ref.w_aa(int(d)) for d in deg]); ra = np.array([ref.w_ra(int(d)) for d in deg])
    C, A, R = S @ S, (S * aa) @ S, (S * ra) @ S
    out = np.zeros((len(pairs), 5))
    for k, (a, b) in enumerate(np.asarray(pairs).tolist()):
        adj = a != b and S[a, b] > 0 and (flags & 1)
        da, db = deg[a] - (1 if adj else 0), deg[b] - (1 if adj else 0)
        U = deg[a] if a == b else da + db - C[a, b]
        out[k] = (C[a, b], C[a, b] / U if U else 0.0, A[a, b], R[a, b], float(np.float32(int(da) * int(db))))
    return out, deg


def random_multigraph():
    rng = np.random.default_rng(17)
    N = 60
    src = rng.integers(0, N - 3, 420); dst = rng.integers(0, N - 3, 420)       # 57 .. 59 isolated; self loops and parallel edges by chance
    assert (src == dst).any() and len(set(zip(src.tolist(), dst.tolist()))) < len(src)
    return N, src.astype(np.int64), dst.astype(np.int64)


@pytest.mark.parametrize('case', ['multigraph', 'random'])
@pytest.mark.parametrize('flags', [0, 1])
def test_restatement_against_the_dense_matrix(case, flags):
    N, src, dst = negative_ref.multigraph_case() if case == 'multigraph' else random_multigraph()
    pairs = np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing='ij'), -1).reshape(-1, 2)
    got = ref.pair_scores(N, src, dst, pairs, flags)
    want, deg = dense_scores(N, src, dst, pairs, flags)
    assert np.array_equal(got[:, CN], want[:, CN]) and np.array_equal(got[:, PA], want[:, PA])
    np.testing.assert_allclose(got[:, [JAC, AA, RA]], want[:, [JAC, AA, RA]], rtol=1e-12, atol=0)
    assert np.array_equal(ref.degrees(N, src, dst), deg)
    assert got[:, CN].max() > 3 and (got[:, CN] == 0).any()
    # orientation: (a, b) and (b, a) are the same pair
    assert np.array_equal(got.reshape(N, N, 5), got.reshape(N, N, 5).transpose(1, 0, 2))
    if flags:
        plain = ref.pair_scores(N, src, dst, pairs, 0)
        assert np.array_equal(plain[:, [CN, AA, RA]], got[:, [CN, AA, RA]]) and (plain[:, PA] != got[:, PA]).any()


def _sc(N, e, pairs, flags=0):
    e = np.asarray(e, np.int64).reshape(-1, 2)
    return ref.pair_scores(N, e[:, 0], e[:, 1], pairs, flags)


def test_six_clique():
    e = [(u, v) for u in range(6) for v in range(u + 1, 6)]
    s = _sc(6, e, [(0, 1), (4, 2)])
    w = np.float32(1 / math.log(5))
    for row in s:
        assert row[CN] == 4 and row[JAC] == 4 / (5 + 5 - 4) and row[PA] == 25
        assert row[AA] == pytest.approx(4 * float(w), rel=1e-15) and row[RA] == pytest.approx(4 * float(np.float32(0.2)), rel=1e-15)
    m = _sc(6, e, [(0, 1)], 1)[0]
    assert m[CN] == 4 and m[JAC] == 4 / (4 + 4 - 4) and m[PA] == 16 and m[AA] == s[0][AA]


def test_star_leaves_share_the_centre():
    n = 9
    e = [(0, k) for k in range(1, n)]
    s = _sc(n, e, [(3, 7), (0, 3)])
    assert s[0][CN] == 1 and s[0][JAC] == 1 / (1 + 1 - 1) and s[0][PA] == 1
    assert s[0][AA] == float(np.float32(1 / math.log(n - 1))) and s[0][RA] == float(np.float32(1 / (n - 1)))
    assert s[1].tolist() == [0, 0, 0, 0, float(n - 1)]                       # centre and leaf: adjacent, nothing in common
    assert _sc(n, e, [(0, 3)], 1)[0].tolist() == [0, 0, 0, 0, 0.0]            # masked: the leaf has no neighbour left


def test_directed_path_through_a_common_sink():
    """a -> z <- b: z is common although no row of the in-CSR or of the out-CSR lists both a and b's edges."""
    s = _sc(4, [(0, 2), (1, 2), (2, 3)], [(0, 1), (1, 0)])
    assert s[0].tolist() == s[1].tolist() == [1, 1.0, float(np.float32(1 / math.log(3))), float(np.float32(1 / 3)), 1.0]


def test_self_pair_and_isolated_node():
    e = [(0, 1), (1, 0), (0, 2), (2, 2), (3, 0), (1, 2)]                      # node 4 isolated; 2 has a self loop; 0-1 in both directions
    s = _sc(5, e, [(0, 0), (4, 4), (4, 0), (2, 2), (0, 5), (-1, 2)])
    d = ref.degrees(5, *np.asarray(e).T)
    assert d.tolist() == [3, 2, 2, 1, 0]
    w2 = float(np.float32(1 / math.log(2)))
    assert s[0].tolist() == [3, 1.0, pytest.approx(2 * w2), pytest.approx(0.5 + 0.5 + 1.0), 9.0]      # I = Gamma(0) = {1, 2, 3}; deg 3 of node 3 is 1: w_aa = 0
    assert s[1].tolist() == [0, 0, 0, 0, 0] and s[2].tolist() == [0, 0, 0, 0, 0]
    assert s[3].tolist() == [2, 1.0, pytest.approx(float(np.float32(1 / math.log(3))) + w2), pytest.approx(float(np.float32(1 / 3)) + 0.5), 4.0]
    assert s[4].tolist() == [0] * 5 and s[5].tolist() == [0] * 5              # ids outside the graph
    assert np.array_equal(_sc(5, e, [(0, 0), (2, 2), (4, 4)], 1), s[[0, 3, 1]])      # the mask never touches a self pair


def test_mask_flag_takes_one_from_each_degree_of_an_adjacent_pair_only():
    N, src, dst = negative_ref.multigraph_case()
    nb = ref.neighbourhoods(N, src, dst)
    rng = np.random.default_rng(3)
    pairs = rng.integers(0, N, (4000, 2))
    plain, masked = ref.pair_scores(N, src, dst, pairs, 0, nb), ref.pair_scores(N, src, dst, pairs, 1, nb)
    adj = np.array([a != b and b in nb[a] for a, b in pairs.tolist()])
    assert 50 < adj.sum() < len(adj) - 50
    assert np.array_equal(plain[~adj], masked[~adj])
    deg = ref.degrees(N, src, dst).astype(np.int64)
    da, db = deg[pairs[:, 0]], deg[pairs[:, 1]]
    assert np.array_equal(masked[adj][:, PA], ((da - 1) * (db - 1))[adj].astype(np.float64))
    assert np.array_equal(plain[:, PA], (da * db).astype(np.float64))
    U = (da - 1) + (db - 1) - masked[:, CN]
    ok = adj & (U > 0)
    assert np.array_equal(masked[ok][:, JAC], (masked[:, CN] / np.where(U > 0, U, 1))[ok]) and (masked[adj & (U == 0)][:, JAC] == 0).all()


def test_planted_case_has_the_rows_it_names():
    N, src, dst, nodes = ref.planted_case()
    deg = ref.degrees(N, src, dst)
    assert tuple(deg[nodes].tolist()) == ref.PLANTED_ROWS
    pairs = [(a, b) for a in nodes for b in nodes]
    s = ref.pair_scores(N, src, dst, pairs)
    assert (s[:, CN] > 0).sum() > 50 and s[:, CN].max() >= 129               # the rows overlap: every length meets a non-empty intersection


def test_link_auc_against_the_pair_count():
    import gmeta_amd
    rng = np.random.default_rng(1)
    for n, levels in ((40, 5), (200, 12), (151, 1000), (30, 1)):
        s = rng.integers(0, levels, n).astype(np.float64) / 3.0                # many ties
        y = rng.integers(0, 2, n)
        y[0], y[1] = 0, 1
        assert gmeta_amd.link_auc(s, y) == pytest.approx(ref.auc_by_pair_count(s, y), abs=1e-12)
        assert gmeta_amd.link_auc(s, [str(v) for v in y]) == gmeta_amd.link_auc(s, y)      # the tables' string labels
    assert gmeta_amd.link_auc([3, 2, 1, 0], [1, 1, 0, 0]) == 1.0 and gmeta_amd.link_auc([0, 1, 2, 3], [1, 1, 0, 0]) == 0.0
    assert gmeta_amd.link_auc([1, 1, 1, 1], [1, 0, 1, 0]) == 0.5
    assert gmeta_amd.link_auc([2, 1, 1, 0], [1, 1, 0, 0]) == (2 + 1 + 0.5) / 4
    for bad in ([1, 1, 1], [0, 0]):
        with pytest.raises(ValueError, match='both labels'):
            gmeta_amd.link_auc(np.arange(len(bad)), bad)
    with pytest.raises(ValueError):
        gmeta_amd.link_auc([1.0, 2.0], [0, 2])
    with pytest.raises(ValueError):
        gmeta_amd.link_auc([1.0, 2.0, 3.0], [0, 1])


class _HostStore:
    """GraphStore.pair_scores on the restatement (host logic of link_heuristic_auc; no GPU)."""

    def __init__(self, graphs):
        self.graphs, self.calls = graphs, []

    def pair_scores(self, g, pairs, mask_target=False):
        self.calls.append((g, len(pairs), mask_target))
        N, src, dst = self.graphs[g]
        return ref.pair_scores(N, src, dst, pairs, 1 if mask_target else 0).astype(np.float32)


def test_link_heuristic_auc_scores_each_graph_once_and_keeps_the_order():
    import gmeta_amd
    rng = np.random.default_rng(2)
    graphs = [(30, rng.integers(0, 30, 120), rng.integers(0, 30, 120)), (20, rng.integers(0, 20, 70), rng.integers(0, 20, 70))]
    names, labels, rows = [], [], []
    for k in range(90):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, graphs[g][0], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b)); labels.append(str(k % 2))
        rows.append(ref.pair_scores(*graphs[g], [(a, b)], 1)[0].astype(np.float32))
    store = _HostStore(graphs)
    got = gmeta_amd.link_heuristic_auc(store, names, labels, mask_target=True)
    assert sorted(c[0] for c in store.calls) == [0, 1] and all(c[2] for c in store.calls) and sum(c[1] for c in store.calls) == 90
    assert tuple(got) == gmeta_amd.PAIR_SCORES == ref.COLS
    rows = np.asarray(rows)
    for k, nm in enumerate(ref.COLS):
        assert got[nm] == gmeta_amd.link_auc(rows[:, k], labels) and 0.0 <= got[nm] <= 1.0
    with pytest.raises(ValueError, match='g_i_j'):
        gmeta_amd.link_heuristic_auc(store, ['0_1'], ['1'])


def test_exports_are_declared_and_bound():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gm_store_pair_scores', 'gm_store_neighbour_degrees'):
        assert re.search(r'\b%s\s*\(' % name, code) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES['gm_store_pair_scores'][1]) == 7 and len(_lib.PROTOTYPES['gm_store_neighbour_degrees'][1]) == 4
    assert re.search(r'#define GM_PAIR_MASK_TARGET 1\b', code) and _lib.PAIR_MASK_TARGET == 1 == ref.MASK_TARGET
    assert hasattr(gmeta_amd.GraphStore, 'pair_scores') and hasattr(gmeta_amd.GraphStore, 'neighbour_degrees')
    assert open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read().count("'pair_scores.hip']") == 1      # appended last
    for lanes in (16, 32, 64, 0):
        assert _lib.lib().gm_set_tuning(b'pair_lanes', lanes) == 0 and _lib.lib().gm_get_tuning(b'pair_lanes') == lanes


def test_train_flag_parses_and_defaults_to_off():
    import train as drv
    base = ['--data_dir', 'x', '--task_setup', 'Shared']
    assert drv.parse(base).heuristics == 0 and drv.parse(base + ['--heuristics', '1']).heuristics == 1
    with pytest.raises(SystemExit):
        drv.parse(base + ['--heuristics', '2'])
