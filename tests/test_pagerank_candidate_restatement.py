"""CPU (-m "not gpu"): the restatement of the PageRank-candidate definition (tests/pagerank_candidate_ref.py) on hand answers -- a path, a star with ties, a
k above the total --, its agreement with an independent lexsort, the ValueErrors of GraphStore.pagerank_candidates, the C ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import negative_ref
import pagerank_candidate_ref as ref
import pagerank_ref
import pair_score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_path_far_side_in_order_of_distance():
    N, src, dst = ref.path_case(8)
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    rows = pagerank_ref.rooted_pagerank(N, src, dst, [0, 3], 0.15, 60, nb).astype(f32)      # 60 steps: the mass still moving (0.85^60) is far below the far end's
    assert (rows > 0).all()
    nodes, sc, tot = ref.top_k(N, nb, [0, 3], rows, 6)
    assert nodes[0].tolist() == [2, 3, 4, 5, 6, 7] and tot[0] == N - 2         # not 0 itself, not its neighbour 1
    assert tot[1] == N - 3 and not set(nodes[1].tolist()) & {2, 3, 4} and nodes[1, 5] == -1 and sc[1, 5] == 0
    right = [w for w in nodes[1].tolist() if w > 3]
    left = [w for w in nodes[1].tolist() if 0 <= w < 3]
    assert right == [5, 6, 7] and left == [1, 0]                               # each side in order of distance
    assert (np.diff(sc.astype(np.float64), axis=1) <= 0).all() and np.array_equal(sc[0], rows[0][nodes[0]])
    whole = ref.top_k(N, nb, [0], rows[:1], N)
    assert whole[0][0, :N - 2].tolist() == list(range(2, N)) and (whole[0][0, N - 2:] == -1).all() and (whole[1][0, N - 2:] == 0).all()


def test_star_ties_in_ascending_id_and_padding():
    N = 7                                                                       # centre 0, leaves 1 .. 6
    src, dst = np.zeros(6, np.int64), np.arange(1, 7, dtype=np.int64)
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    row = np.array([0.5, 0.2, 0.05, 0.1, 0.05, 0.05, 0.05], f32)                # seen from leaf 1: the centre is adjacent, 3 stands out, 2 4 5 6 tie
    nodes, sc, tot = ref.top_k(N, nb, [1, 1, -1, N], np.stack([row, row, row, row]), 3)
    assert nodes[0].tolist() == [3, 2, 4] and sc[0].tolist() == [f32(0.1), f32(0.05), f32(0.05)] and tot.tolist() == [5, 5, 0, 0]
    assert np.array_equal(nodes[1], nodes[0]) and (nodes[2:] == -1).all() and not sc[2:].any()
    nodes, sc, tot = ref.top_k(N, nb, [1], row[None], 8)                        # k above the total: padded
    assert nodes[0].tolist() == [3, 2, 4, 5, 6, -1, -1, -1] and sc[0, 5:].tolist() == [0, 0, 0] and sc.dtype == f32 and nodes.dtype == np.int64
    zero = row.copy(); zero[4] = 0                                              # an entry that underflowed to zero is no candidate
    assert ref.top_k(N, nb, [1], zero[None], 8)[0][0].tolist() == [3, 2, 5, 6, -1, -1, -1, -1]
    lone = np.zeros(N, f32); lone[0] = 1                                        # an isolated source keeps its mass: nothing else is positive
    assert ref.top_k(N, [set() for _ in range(N)], [0], lone[None], 2)[2].tolist() == [0]


def test_against_lexsort_on_the_multigraph_rows():
    N, src, dst = negative_ref.multigraph_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    sources = np.array([0, 1, 5, 17, 150, 285, 295])
    rows = pagerank_ref.rooted_pagerank(N, src, dst, sources, 0.15, 2, nb).astype(f32)      # two steps: many zeros, many equal entries
    for k in (1, 7, 1024):
        nodes, sc, tot = ref.top_k(N, nb, sources, rows, k)
        for r, a in enumerate(sources.tolist()):
            ok = rows[r] > 0
            ok[[a] + sorted(nb[a])] = False
            w = np.nonzero(ok)[0]
            order = w[np.lexsort((w, -rows[r][w].astype(np.float64)))][:k]
            t = len(order)
            assert tot[r] == len(w) and np.array_equal(nodes[r, :t], order) and (nodes[r, t:] == -1).all()
            assert np.array_equal(sc[r, :t].view(np.uint32), rows[r][order].view(np.uint32)) and (sc[r, t:].view(np.uint32) == 0).all()
    assert ref.top_k(N, nb, sources, rows, 1024)[2][-1] == 0 and ref.top_k(N, nb, sources, rows, 1024)[2][0] > 0      # 295 is isolated


def test_the_cases_are_what_the_gpu_tests_need():
    N, src, dst = ref.star_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    assert N == 75 and len(nb[0]) == 70 > 64 and nb[1] == {0, 71} and nb[74] == {73} and all(nb[w] == {0} for w in range(2, 71))
    N, src, dst = ref.random_connected_case()
    deg = pair_score_ref.degrees(N, src, dst)
    assert N == 3001 and N % 64 != 0 and deg.min() >= 1 and 5.5 < deg.mean() < 6.5
    seen, front = {0}, [0]
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    while front:
        front = [z for x in front for z in nb[x] if z not in seen and not seen.add(z)]
    assert len(seen) == N                                                       # connected


def test_pagerank_candidates_refuses_bad_arguments_before_the_library():
    """No GPU and no store behind the object: the checks come first."""
    import gmeta_amd
    store = object.__new__(gmeta_amd.GraphStore)
    store.handle, store.n_graphs, store.n_nodes = None, 1, [10]
    for k in (0, -3, 1025):
        with pytest.raises(ValueError, match='k = %d' % k):
            store.pagerank_candidates(0, [1], k=k)
    for alpha in (0.0, 1.0, float('nan')):
        with pytest.raises(ValueError, match='alpha'):
            store.pagerank_candidates(0, [1], alpha=alpha)
    for iters in (0, 256):
        with pytest.raises(ValueError, match='iters = %d' % iters):
            store.pagerank_candidates(0, [1], iters=iters)
    with pytest.raises(ValueError, match='graph 1'):
        store.pagerank_candidates(1, [1])
    with pytest.raises(ValueError, match='outside'):
        store.pagerank_candidates(0, [10])
    with pytest.raises(ValueError, match='outside'):
        store.pagerank_candidates(0, [-1])


def test_export_is_declared_and_bound():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = 'gm_store_pagerank_candidates'
    assert re.search(r'\b%s\s*\(' % name, code) and name in _lib.PROTOTYPES and hasattr(lib, name)
    res, args = _lib.PROTOTYPES[name]
    # s, g, d_nodes, m, k, alpha, iters, d_out_nodes, d_out_scores, d_out_total, stream: alpha is the one float passed by value (the scores leave through a pointer)
    assert res is ctypes.c_int32 and len(args) == 11 and [k for k, t in enumerate(args) if t is ctypes.c_float] == [5]
    assert args[3] is ctypes.c_int64 and args[4] is ctypes.c_int32 and args[6] is ctypes.c_int32
    assert hasattr(gmeta_amd.GraphStore, 'pagerank_candidates')
    build = open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert build.count("'pagerank_candidates.hip'") == 1
    # the existing surface is as it was
    assert gmeta_amd.PAIR_SCORES == ('cn', 'jaccard', 'adamic_adar', 'resource_allocation', 'pref_attachment') and gmeta_amd.PAGERANK_SCORES == ('rooted_pagerank',)
