"""CPU (-m "not gpu"): the restatement of the held-out-edge definitions (tests/holdout_ref.py; the definition itself is in include/gmeta_hip.h) against a
brute-force version on Python sets and lists, the properties of the hashed split that the definition promises, and the driver's flag checks."""
import math

import numpy as np
import pytest

import holdout_ref as ref
from gmeta_amd.graphstore import edges_to_in_csr


def _csr(N, src, dst, w):
    got = edges_to_in_csr(N, src, dst, w)
    return got if w is not None else got + (None,)


def _brute(ptr, idx, w, pairs):
    """rows as Python lists, the removed pairs as a set of frozensets -> the filtered rows in both orientations"""
    N = len(ptr) - 1
    gone = {frozenset(p) for p in pairs}
    rows_in = [[] for _ in range(N)]
    for v in range(N):
        for e in range(ptr[v], ptr[v + 1]):
            if frozenset((int(idx[e]), v)) not in gone:
                rows_in[v].append((int(idx[e]), None if w is None else float(w[e])))
    rows_out = [[] for _ in range(N)]
    for v in range(N):                       # destinations ascending, a row's stored order inside: the stable order of the store's by-source CSR
        for u, x in rows_in[v]:
            rows_out[u].append((v, x))
    return rows_in, rows_out


def _rows(ptr, idx, w):
    return [[(int(idx[e]), None if w is None else float(w[e])) for e in range(ptr[v], ptr[v + 1])] for v in range(len(ptr) - 1)]


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_filter_equals_the_brute_force_version_on_random_multigraphs(seed, weighted):
    rng = np.random.default_rng(seed)
    N, src, dst, w = ref.multigraph(40 + 7 * seed, 150, rng, weighted=weighted)
    ptr, idx, w = _csr(N, src, dst, w)
    pick = rng.choice(len(src), 40, replace=False)
    pairs = np.stack([dst[pick], src[pick]], axis=1)                                            # named against the stored direction
    pairs = np.concatenate([pairs, pairs[:5, ::-1], [[0, 0], [N - 1, N - 2], [5, 5]]])          # duplicates, a self loop, pairs that name no edge
    keys = ref.pair_keys(N, pairs)
    assert np.all(np.diff(keys) > 0)
    got, sym = ref.without_edges([(ptr, idx, w)], [keys])
    want_in, want_out = _brute(ptr, idx, w, pairs.tolist())
    assert _rows(*got[0]['in']) == want_in and _rows(*got[0]['out']) == want_out
    assert sym == (want_in == want_out and any(want_in))
    assert len(got[0]['in'][1]) < len(idx)
    # nothing removed: the graph itself, and the by-source CSR is the one GraphStore.symmetric() derives
    same, _ = ref.without_edges([(ptr, idx, w)], [np.zeros(0, np.int64)])
    assert np.array_equal(same[0]['in'][0], ptr) and np.array_equal(same[0]['in'][1], idx)


def test_symmetric_flag_follows_the_filtered_arrays():
    und = np.array([[0, 1], [1, 2], [2, 3], [0, 3]])
    src, dst = np.concatenate([und[:, 0], und[:, 1], [4]]), np.concatenate([und[:, 1], und[:, 0], [2]])      # an undirected cycle and one arc 4 -> 2
    order = np.lexsort((src, dst))                                                                            # rows of ascending sources, as the flag asks
    src, dst = src[order], dst[order]
    ptr, idx, w = _csr(6, src, dst, None)
    assert not ref.without_edges([(ptr, idx, None)], [[]])[1]
    assert ref.without_edges([(ptr, idx, None)], [ref.pair_keys(6, [[2, 4]])])[1]                              # the arc gone: symmetric
    every = ref.pair_keys(6, np.stack([src, dst], axis=1))
    got, sym = ref.without_edges([(ptr, idx, None)], [every])
    assert not sym and len(got[0]['in'][1]) == 0 and not got[0]['in'][0].any()                                # no edge left: false


def _graph(seed, N=400, E=1600):
    N, src, dst, _ = ref.multigraph(N, E, np.random.default_rng(seed))
    return N, src, dst


def test_split_ignores_orientation_and_multiplicity_and_follows_the_seed():
    N, src, dst = _graph(3)
    t = ref.thresholds(0.05, 0.10)
    a = ref.split_edges(*edges_to_in_csr(N, src, dst), 1, 222, *t)
    b = ref.split_edges(*edges_to_in_csr(N, dst, src), 1, 222, *t)                                            # every edge reversed
    c = ref.split_edges(*edges_to_in_csr(N, np.concatenate([src, dst, src]), np.concatenate([dst, src, dst])), 1, 222, *t)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2] == other[2]
    again = ref.split_edges(*edges_to_in_csr(N, src, dst), 1, 222, *t)
    assert np.array_equal(a[0], again[0]) and np.array_equal(a[1], again[1])
    for seed, g in ((223, 1), (222, 0), (222 + (1 << 32), 1)):                                                  # the seed (both halves) and the graph index enter the hash
        other = ref.split_edges(*edges_to_in_csr(N, src, dst), g, seed, *t)
        assert not np.array_equal(a[0], other[0])
    keys = a[0][:, 0] * N + a[0][:, 1]
    assert np.all(a[0][:, 0] < a[0][:, 1]) and np.all(np.diff(keys) > 0)
    # the classes nest: raising the validation threshold moves no test link
    wide = ref.split_edges(*edges_to_in_csr(N, src, dst), 1, 222, t[0], 2 * t[1])
    assert np.array_equal(wide[0][wide[1] == 2], a[0][a[1] == 2]) and wide[2][1] > a[2][1]


SEEDS = (222, 1, 2, 3, 4, 5)
SIGMAS = 5.0      # a binomial count leaves +-5 standard deviations with probability < 6e-7: twelve checks below, so a correct hash fails once in > 10^5 seed choices


def test_split_counts_stay_within_five_standard_deviations_of_the_binomial_expectation():
    N, src, dst = _graph(4)
    ptr, idx = edges_to_in_csr(N, src, dst)
    val, test = 0.05, 0.10
    for seed in SEEDS:
        _, _, (links, n_val, n_test) = ref.split_edges(ptr, idx, 0, seed, *ref.thresholds(val, test))
        assert links > 1500
        for name, n, f in (('val', n_val, val), ('test', n_test, test)):
            sd = math.sqrt(links * f * (1 - f))
            print('seed %d %s: %d of %d links, expectation %.1f, %.2f sd' % (seed, name, n, links, links * f, (n - links * f) / sd))
            assert abs(n - links * f) <= SIGMAS * sd


def test_split_thresholds_at_their_ends():
    N, src, dst = _graph(5, 120, 400)
    ptr, idx = edges_to_in_csr(N, src, dst)
    pairs, cls, (links, n_val, n_test) = ref.split_edges(ptr, idx, 0, 222, 0, 0)
    assert len(pairs) == 0 and (n_val, n_test) == (0, 0) and links > 0
    pairs, cls, cnt = ref.split_edges(ptr, idx, 0, 222, 0, 2 ** 32)
    assert cnt == (links, links, 0) and np.all(cls == 1)
    rows = ref.neighbour_rows(ptr, idx)
    assert pairs.tolist() == [[u, v] for u in range(N) for v in rows[u] if u < v]
    pairs, cls, cnt = ref.split_edges(ptr, idx, 0, 222, 2 ** 32, 2 ** 32)
    assert cnt == (links, 0, links) and np.all(cls == 2)
    assert ref.thresholds(0, 0) == (0, 0) and ref.thresholds(0.5, 0.5) == (2 ** 31, 2 ** 32) and ref.thresholds(0, 1) == (2 ** 32, 2 ** 32)


def test_driver_flag_needs_pairs_and_a_family():
    import train as drv
    base = ['--data_dir', 'x/', '--task_setup', 'Shared']
    assert drv.parse(base).holdout == 0
    assert drv.parse(base + ['--link_pred_mode', 'True', '--holdout', '1', '--buddy', '2']).holdout == 1
    with pytest.raises(SystemExit, match='link_pred_mode'):
        drv.parse(base + ['--holdout', '1', '--heuristics', '1'])
    with pytest.raises(SystemExit, match='--heuristics, --pagerank, --distance or --buddy'):
        drv.parse(base + ['--link_pred_mode', 'True', '--holdout', '1'])
