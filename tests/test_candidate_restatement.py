"""CPU (-m "not gpu"): the restatement of the candidate-partner definition (tests/candidate_ref.py) against the dense boolean S S with S and the diagonal
removed; the ranking against np.lexsort under heavy ties; candidate_names; the ValueErrors of GraphStore.link_candidates; the C ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import candidate_ref as ref
import negative_ref
import pair_score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense_candidates(N, src, dst):
    """Independent of candidate_ref: S = (A or A^T) without the diagonal; C = (S S > 0) and not S and not I, as a boolean matrix."""
    S = np.zeros((N, N), bool)
    S[np.asarray(src), np.asarray(dst)] = True
    S |= S.T
    np.fill_diagonal(S, False)
    two = (S.astype(np.float32) @ S.astype(np.float32)) > 0                   # counts below 2^24: exact in fp32
    C = two & ~S
    np.fill_diagonal(C, False)
    return C


def _random_graph(seed, N, E):
    rng = np.random.default_rng(seed)
    return N, rng.integers(0, N, E).astype(np.int64), rng.integers(0, N, E).astype(np.int64)


CASES = {
    'multigraph': negative_ref.multigraph_case,
    'dense': negative_ref.dense_case,
    'planted': lambda: pair_score_ref.planted_case()[:3],
    'words': ref.word_boundary_case,
    'random_sparse': lambda: _random_graph(1, 97, 120),
    'random_mid': lambda: _random_graph(2, 64, 400),
    'random_loops': lambda: _random_graph(3, 33, 40),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_candidate_sets_against_the_dense_matrix(case):
    N, src, dst = CASES[case]()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    C = dense_candidates(N, src, dst)
    total = 0
    for a in range(N):
        got = ref.candidates(N, src, dst, a, nb)
        assert got == np.nonzero(C[a])[0].tolist(), (case, a)
        assert a not in got and not (set(got) & nb[a])
        total += len(got)
    assert total == int(C.sum()) and total > 0
    assert ref.candidates(N, src, dst, -1, nb) == [] and ref.candidates(N, src, dst, N, nb) == []
    if case == 'multigraph':
        assert total == 65896 and sum(1 for a in range(N) if not C[a].any()) == 10
    if case == 'dense':
        assert sorted({int(c) for c in C.sum(1)}) == [5, 6]
    if case == 'planted':
        pool = C[13:].sum(1)
        assert pool.max() == 3014


def test_word_boundary_case_sits_on_the_boundaries():
    N, src, dst = ref.word_boundary_case()
    assert N % 32 != 0
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    edge_ids = {0, 31, 32, 63, 64, N - 1}
    cand = set().union(*[set(ref.candidates(N, src, dst, a, nb)) for a in range(N)])
    blocked = set().union(*[nb[a] for a in range(N) if ref.candidates(N, src, dst, a, nb)])
    assert edge_ids <= cand and edge_ids <= blocked
    assert ref.candidates(N, src, dst, 5, nb) == [0, 32, 63, 69]              # 31 and 64 share node 10 with 5 but are adjacent to it


def test_ranking_against_lexsort_with_heavy_ties():
    rng = np.random.default_rng(4)
    for n, levels, k in ((1, 1, 3), (50, 3, 7), (700, 4, 64), (3000, 5, 1024), (1500, 1500, 1024), (40, 2, 40)):
        w = np.sort(rng.choice(5000, n, replace=False))
        sc = (rng.integers(1, levels + 1, n).astype(np.float32) / np.float32(3.0))      # positive fp32 with many equal values
        nodes, out = ref.rank(w.tolist(), sc, k)
        order = np.lexsort((w, -sc.astype(np.float64)))[:k]                    # descending score, then ascending node id
        t = len(order)
        assert np.array_equal(nodes[:t], w[order]) and np.array_equal(out[:t].view(np.uint32), sc[order].view(np.uint32))
        assert (nodes[t:] == -1).all() and (out[t:] == 0).all() and nodes.dtype == np.int64 and out.dtype == np.float32
    # positive fp32 order like their bit patterns: the key's upper half ranks by score
    x = np.sort(np.abs(rng.standard_normal(1000)).astype(np.float32) + np.float32(1e-30))
    assert (np.diff(x.view(np.uint32).astype(np.int64)) >= 0).all()
    key = ref.keys([7, 3], np.array([1.5, 1.5], np.float32))
    assert int(key[1]) > int(key[0]) and int(key[0]) == (0x3FC00000 << 32) | (0xFFFFFFFF - 7)


def test_top_k_walks_the_pairs_in_order():
    N, src, dst = negative_ref.dense_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    sources = [3, 3, -1, 11, N]
    sets = [ref.candidates(N, src, dst, a, nb) for a in sources]
    pairs = ref.pairs_of(sources, sets)
    assert len(pairs) == sum(len(c) for c in sets) and (pairs[:len(sets[0]), 0] == 3).all()
    sc = pair_score_ref.pair_scores(N, src, dst, pairs, 0, nb)[:, 2].astype(np.float32)
    nodes, out, tot = ref.top_k(sources, sets, sc, 8)
    assert tot.tolist() == [len(c) for c in sets] and tot[2] == tot[4] == 0 and (nodes[2] == -1).all()
    assert np.array_equal(nodes[0], nodes[1]) and set(nodes[0][nodes[0] >= 0].tolist()) == set(sets[0]) and (nodes[0][tot[0]:] == -1).all()
    assert (np.diff(out[0][:tot[0]]) <= 0).all()


def test_candidate_names():
    import gmeta_amd
    part = np.array([[5, 9, -1], [-1, -1, -1], [0, 2, 1]], np.int64)
    assert gmeta_amd.candidate_names(2, [7, 8, 7], part) == [['2_7_5', '2_7_9'], [], ['2_7_0', '2_7_2', '2_7_1']]
    assert gmeta_amd.candidate_names(0, [], np.zeros((0, 4), np.int64)) == []
    with pytest.raises(ValueError, match='partners'):
        gmeta_amd.candidate_names(0, [1, 2], part)
    assert 'candidate_names' in gmeta_amd.__all__


def test_link_candidates_refuses_bad_arguments_before_the_library():
    """No GPU and no store behind the object: the checks come first."""
    import gmeta_amd
    store = object.__new__(gmeta_amd.GraphStore)
    store.handle, store.n_graphs, store.n_nodes = None, 1, [10]
    with pytest.raises(ValueError, match='score'):
        store.link_candidates(0, [1], score='katz')
    for k in (0, -3, 1025):
        with pytest.raises(ValueError, match='k = %d' % k):
            store.link_candidates(0, [1], k=k)
    with pytest.raises(ValueError, match='graph 1'):
        store.link_candidates(1, [1])
    with pytest.raises(ValueError, match='outside'):
        store.link_candidates(0, [10])


def test_export_is_declared_and_bound():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = 'gm_store_pair_candidates'
    assert re.search(r'\b%s\s*\(' % name, code) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES[name][1]) == 10
    assert hasattr(gmeta_amd.GraphStore, 'link_candidates')
    src = open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert src.count("'candidates.hip'") == 1 and src.index("'candidates.hip'") > src.index("'pair_scores.hip'")      # last
    for knob, values in ((b'cand_round', (1, 4096, 0)), (b'cand_bitmap', (1, 2, 0))):
        for v in values:
            assert _lib.lib().gm_set_tuning(knob, v) == 0 and _lib.lib().gm_get_tuning(knob) == v
