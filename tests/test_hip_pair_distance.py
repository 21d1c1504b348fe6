"""GPU (-m gpu): gm_store_node_distances, gm_store_pair_distance and the Python layers above them against the restatement of the definition
(tests/distance_ref.py: a plain breadth-first search; the definition itself is in include/gmeta_hip.h).  Distances are integers: everything is EQUAL, there
is no tolerance.  The restatement at a smaller max_dist is the one at 254 with the entries above max_dist unreached; test_distance_restatement.py checks
that on the CPU, so the references are searched once."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import distance_ref as ref
import negative_ref
import pair_score_ref
import path_walk_ref
from test_hip_pair_pagerank import _stream, tuning
from test_hip_pair_scores import DRIVER, _positives_only, _splits, _store

pytestmark = pytest.mark.gpu
U = ref.UNREACHED
POISON = 0xAB
MAX_DISTS = (1, 2, 3, 4, 8, 254)
CHUNKS = (0, 1, 7, 2 ** 30)                   # 0: the library's choice; 1: every row of two or more entries is cut; 2^30: none is
COLS = (0, 64, 128, 4096)                     # 0: the library's choice; 4096: the bound


def _raw_vec(store, g, sources, max_dist=8, stream=None):
    """The C ABI itself: uint8 [m, N].  The row behind m is poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    a = np.ascontiguousarray(np.asarray(sources, np.int64).reshape(-1), np.int32)
    m, N = len(a), store.n_nodes[g]
    d_a = torch.from_numpy(a).cuda() if m else None
    out = torch.full((m + 1, N), POISON, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_store_node_distances(store.handle, g, _lib.ptr(d_a), m, max_dist, _lib.ptr(out), _stream(stream)), 'gm_store_node_distances')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.dtype == np.uint8 and (out[m:] == POISON).all()
    return out[:m]


def _raw(store, g, pairs, flags=0, max_dist=8, stream=None):
    """The C ABI itself: uint8 [n], the 64 entries behind n poisoned."""
    from gmeta_amd import _lib
    p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
    n = len(p)
    d_p = torch.from_numpy(p).cuda() if n else None
    out = torch.full((n + 64,), POISON, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_store_pair_distance(store.handle, g, _lib.ptr(d_p), n, flags, max_dist, _lib.ptr(out), _stream(stream)), 'gm_store_pair_distance')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.dtype == np.uint8 and (out[n:] == POISON).all()
    return out[:n]


def cap(d, max_dist):
    return np.where(d <= max_dist, d, U).astype(np.uint8)


def _all_pairs(N):
    return np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing='ij'), -1).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------- shared references, computed once
class Case:
    """A graph, its store, and the restatement at max_dist 254 of every source's vector and of every ordered pair with both flags."""

    def __init__(self, N, src, dst):
        self.N, self.src, self.dst = N, src, dst
        self.nb = pair_score_ref.neighbourhoods(N, src, dst)
        self.store = _store([(N, src, dst)])
        self.pairs = _all_pairs(N)
        self.vec = ref.node_distances(N, src, dst, np.arange(N), 254, self.nb)
        self.want = {f: ref.pair_distance(N, src, dst, self.pairs, f, 254, self.nb) for f in (0, 1)}
        self.adj = np.array([b in self.nb[a] for a, b in self.pairs.tolist()])
        for w in (self.vec, self.want[0], self.want[1]):
            w.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case_a():
    return Case(*negative_ref.multigraph_case())


@functools.lru_cache(maxsize=None)
def case_c():
    return Case(*ref.chain_case()[:3])


@functools.lru_cache(maxsize=None)
def case_w():
    """The planted hubs of path_walk_ref: two adjacent rows of 3,000 entries.  -> store, N, the planted nodes, the restated vectors of 200 sources (the planted
    nodes among them) at max_dist 8, the pairs among the planted nodes and their restated distances with both flags."""
    N, src, dst, nodes = path_walk_ref.walk_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    assert max(len(r) for r in nb) == path_walk_ref.HUB_ROW
    sample = np.concatenate([np.asarray(nodes), np.random.default_rng(4).choice(N, 200 - len(nodes), replace=False)])
    vec = ref.node_distances(N, src, dst, sample, 8, nb)
    pairs = np.array([(a, b) for a in nodes for b in nodes], np.int64)
    want = {f: ref.pair_distance(N, src, dst, pairs, f, 8, nb) for f in (0, 1)}
    return _store([(N, src, dst)]), N, nodes, sample, vec, pairs, want


# ---------------------------------------------------------------------------------------------------- the multigraph: every source, every ordered pair
@pytest.mark.parametrize('max_dist', MAX_DISTS)
def test_multigraph_every_source_and_every_ordered_pair(max_dist):
    a = case_a()
    d = a.want[0][a.pairs[:, 0] != a.pairs[:, 1]]
    assert a.N == 300 and max(len(r) for r in a.nb) == 211 and d[d != U].max() == 4 and (d == U).sum() == 5890      # 3 and 4 straddle the largest finite distance
    vec = _raw_vec(a.store, 0, np.arange(a.N), max_dist)
    assert np.array_equal(vec, cap(a.vec, max_dist))
    assert (vec[290:] == np.where(np.eye(a.N, dtype=bool), 0, U)[290:]).all()                       # an isolated source reaches itself alone
    plain = _raw(a.store, 0, a.pairs, 0, max_dist)
    assert np.array_equal(plain, cap(a.want[0], max_dist))
    assert np.array_equal(plain, vec[a.pairs.min(1), a.pairs.max(1)])                              # the entries of the vector call
    assert int(a.adj.sum()) == 2 * 1306                                                            # more than 1,300 distinct masked columns
    with tuning(dist_cols=64):                                                                     # 20-odd rounds, the last one partial
        masked = _raw(a.store, 0, a.pairs, 1, max_dist)
    assert np.array_equal(masked, cap(a.want[1], max_dist))
    assert np.array_equal(masked[~a.adj], plain[~a.adj]) and (masked[a.adj] != 1).all()
    for got in (plain, masked):
        assert np.array_equal(got.reshape(a.N, a.N), got.reshape(a.N, a.N).T)                      # (a, b) against (b, a)
    assert np.array_equal(_raw(a.store, 0, a.pairs, 1, max_dist), masked)                          # the library's columns per round


# ---------------------------------------------------------------------------------------------------- the chain: long distances, bridges, a cycle
@pytest.mark.parametrize('max_dist', [254, 66, 65, 8])
def test_chain_bridges_cycle_and_the_last_level(max_dist):
    c = case_c()
    N, L = c.N, ref.chain_case()[3]
    assert N == 331 and N % 64 and L == 67
    far = c.vec[0]
    assert far[254] == 254 and (far[255:260] == U).all() and (c.vec[259][:5] == U).all() and c.vec[259][5] == 254      # 254 reads 254, 255 .. 259 unreached
    m = c.want[1][c.adj]
    assert (m == U).sum() == 2 * (259 + 3) and (m == L - 1).sum() == 2 * L and len(m) == 2 * (259 + 3 + L)               # bridges and cycle edges, nothing else
    assert (c.vec[329:] == np.where(np.eye(N, dtype=bool), 0, U)[329:]).all()
    vec = _raw_vec(c.store, 0, np.arange(N), max_dist)
    assert np.array_equal(vec, cap(c.vec, max_dist))
    for flags in (0, 1):
        got = _raw(c.store, 0, c.pairs, flags, max_dist)
        assert np.array_equal(got, cap(c.want[flags], max_dist)), flags
    cyc = got[c.adj & (c.pairs.min(1) >= 260) & (c.pairs.max(1) < 327)]
    assert len(cyc) == 2 * L and (cyc == (L - 1 if max_dist >= L - 1 else U)).all()                # 66 and 65 straddle the detour
    with tuning(dist_cols=64, dist_chunk=1):
        assert np.array_equal(_raw_vec(c.store, 0, np.arange(N), max_dist), vec) and np.array_equal(_raw(c.store, 0, c.pairs, 1, max_dist), got)


# ---------------------------------------------------------------------------------------------------- a planted hub: the cut and the widths of a row
@pytest.mark.parametrize('chunk', CHUNKS)
def test_planted_hub_under_every_cut_and_width(chunk):
    store, N, nodes, sample, want_vec, pairs, want = case_w()
    sources = np.arange(2100)                                                                      # more than 2,048 columns: a row as wide as a wave
    base = None
    for cols in COLS:
        with tuning(dist_chunk=chunk, dist_cols=cols):
            got = (_raw_vec(store, 0, sources), _raw_vec(store, 0, sample), _raw(store, 0, pairs, 0), _raw(store, 0, pairs, 1))
        assert np.array_equal(got[1], want_vec) and np.array_equal(got[2], want[0]) and np.array_equal(got[3], want[1]), (chunk, cols)
        at = sample < 2100
        assert np.array_equal(got[0][sample[at]], want_vec[at]), (chunk, cols)
        base = got if base is None else base
        assert all(np.array_equal(x, y) for x, y in zip(got, base)), (chunk, cols)                 # byte-identical under every combination
    assert pairs[1].tolist() == [0, 1] and want[0][1] == 1 and want[1][1] == 2                      # the two adjacent hubs: a detour of 2
    leaf, stem = nodes[3], nodes[-11]                                                              # the 1-entry endpoint and the node it hangs off: a bridge
    k = nodes.index(leaf) * len(nodes) + nodes.index(stem)
    assert pairs[k].tolist() == [leaf, stem] and want[0][k] == 1 and want[1][k] == U


def test_planted_hub_equal_across_the_cuts():
    store, N, nodes, sample, want_vec, pairs, want = case_w()
    got = []
    for chunk in CHUNKS + (63, 64, 65):
        with tuning(dist_chunk=chunk):
            got.append(_raw_vec(store, 0, np.arange(700, 1500), 3))
    assert all(np.array_equal(g, got[0]) for g in got) and (got[0] == U).any() and (got[0] == 3).any()


# ---------------------------------------------------------------------------------------------------- stores, streams, independence
def test_second_graph_of_a_store_and_degenerate_stores():
    a = case_a()
    rng = np.random.default_rng(2)
    g0 = (50, rng.integers(0, 50, 333).astype(np.int64), rng.integers(0, 50, 333).astype(np.int64))
    store = _store([g0, (a.N, a.src, a.dst)])
    assert np.array_equal(_raw_vec(store, 1, np.arange(a.N), 8), cap(a.vec, 8))                    # an offset slip would read graph 0's rows
    for flags in (0, 1):
        assert np.array_equal(_raw(store, 1, a.pairs[::3], flags, 8), cap(a.want[flags][::3], 8))
    assert np.array_equal(_raw_vec(store, 0, np.arange(50), 8), ref.node_distances(*g0, np.arange(50), 8))
    none = np.zeros(0, np.int64)
    one = _store([(1, none, none)])
    assert _raw_vec(one, 0, [0, 0, 1, -1], 3).tolist() == [[0], [0], [U], [U]]
    assert _raw(one, 0, [(0, 0), (0, 1)], 1, 3).tolist() == [0, U]
    bare = _store([(70, none, none)])                                                              # no edge at all
    assert np.array_equal(_raw_vec(bare, 0, np.arange(70), 254), np.where(np.eye(70, dtype=bool), 0, U))
    assert _raw(bare, 0, [(3, 3), (3, 4), (69, 0)], 1, 254).tolist() == [0, U, U]


@pytest.mark.parametrize('flags', [0, 1])
def test_a_result_depends_on_its_own_pair_or_source_alone(flags):
    a = case_a()
    N = a.N
    rng = np.random.default_rng(12)
    pairs = np.concatenate([rng.integers(0, N, (700, 2)), np.stack([rng.integers(0, 2, 60), rng.integers(0, N, 60)], 1)])
    base = _raw(a.store, 0, pairs, flags)
    assert np.array_equal(base, cap(a.want[flags][pairs[:, 0] * N + pairs[:, 1]], 8))
    perm = rng.permutation(len(pairs))
    assert np.array_equal(_raw(a.store, 0, pairs[perm], flags), base[perm])                        # shuffled
    dup = rng.integers(0, len(pairs), 2000)
    assert np.array_equal(_raw(a.store, 0, pairs[dup], flags), base[dup])                          # with duplicates
    cut = np.concatenate([_raw(a.store, 0, part, flags) for part in (pairs[:100], pairs[100:101], pairs[101:])])
    assert np.array_equal(cut, base)                                                               # a sub-list at a time
    assert np.array_equal(_raw(a.store, 0, pairs[:, ::-1], flags), base)                           # the other orientation
    assert np.array_equal(_raw(a.store, 0, pairs, flags, stream=torch.cuda.Stream()), base)        # a second stream
    odd = _raw(a.store, 0, [(0, N), (-1, 5), (N, N), (2 ** 31 - 1, 0), (0, 1), (7, 7)], flags)
    assert odd.tolist() == [U, U, U, U, int(cap(a.want[flags][1:2], 8)[0]), 0]
    if flags:
        return
    sources = np.concatenate([rng.integers(0, N, 150), [0, 0, 1, 299, 299], rng.integers(0, N, 40)])
    whole = cap(a.vec, 8)
    assert np.array_equal(_raw_vec(a.store, 0, sources), whole[sources])                           # every row on its own, whatever the list
    assert np.array_equal(_raw_vec(a.store, 0, sources[:17], stream=torch.cuda.Stream()), whole[sources[:17]])
    odd = _raw_vec(a.store, 0, [5, N, -1, 5, 2 ** 31 - 1])
    assert (odd[[1, 2, 4]] == U).all() and np.array_equal(odd[0], whole[5]) and np.array_equal(odd[3], whole[5])
    assert (_raw_vec(a.store, 0, [N, -3]) == U).all() and _raw_vec(a.store, 0, []).shape == (0, N)


def test_against_the_walk_counts_of_the_device():
    """GraphStore.pair_walks against pair_distance: d == k for k in 1..3 exactly when the first non-zero walk count is w_k."""
    a = case_a()
    off = a.pairs[:, 0] != a.pairs[:, 1]
    for mask in (False, True):
        w = a.store.pair_walks(0, a.pairs, mask_target=mask)
        d = a.store.pair_distance(0, a.pairs, mask_target=mask, max_dist=3)
        first = np.where(w[:, 0] > 0, 1, np.where(w[:, 1] > 0, 2, np.where(w[:, 2] > 0, 3, U)))
        assert np.array_equal(d[off], first[off]) and not d[~off].any(), mask


# ---------------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_and_n_zero():
    from gmeta_amd import _lib
    a = case_a()
    store, lib, N = a.store, _lib.lib(), a.N
    assert _raw(store, 0, np.zeros((0, 2))).shape == (0,)                     # n == 0: the poisoned entries stay
    null, st = C.c_void_p(0), _lib.stream_ptr()
    assert lib.gm_store_pair_distance(store.handle, 0, null, 0, 0, 8, null, st) == 0      # n == 0 with NULL pointers
    assert lib.gm_store_node_distances(store.handle, 0, null, 0, 8, null, st) == 0
    out = torch.zeros((4, N), dtype=torch.uint8, device='cuda')
    d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')

    def pair(g=0, n=4, flags=0, max_dist=8, p=_lib.ptr(d_p), o=_lib.ptr(out), s=store.handle):
        return lib.gm_store_pair_distance(s, g, p, n, flags, max_dist, o, st)

    def vec(g=0, n=4, flags=0, max_dist=8, p=_lib.ptr(d_p), o=_lib.ptr(out), s=store.handle):
        return lib.gm_store_node_distances(s, g, p, n, max_dist, o, st)
    for call, name in ((pair, 'gm_store_pair_distance'), (vec, 'gm_store_node_distances')):
        cnt = 'n' if call is pair else 'm'
        bad = [(dict(g=1), 'graph 1'), (dict(g=-1), 'graph -1'), (dict(n=-1), '%s = -1' % cnt), (dict(n=2 ** 31), '%s = 2147483648' % cnt),
               (dict(max_dist=0), 'max_dist = 0'), (dict(max_dist=255), 'max_dist = 255'), (dict(max_dist=-3), 'max_dist = -3'),
               (dict(p=null), 'NULL argument'), (dict(o=null), 'NULL argument'), (dict(s=null), 'store is NULL')]
        if call is pair:
            bad += [(dict(flags=2), 'flag bits 0x2'), (dict(flags=5), 'flag bits 0x5')]
        for kw, word in bad:
            with pytest.raises(ValueError, match=word):
                _lib.check(call(**kw), name)
        for knob, value, word in (('dist_cols', 48, 'dist_cols = 48'), ('dist_cols', -64, 'dist_cols = -64'), ('dist_cols', 4160, 'dist_cols = 4160'),
                                  ('dist_chunk', -1, 'dist_chunk = -1')):
            with tuning(**{knob: value}):
                with pytest.raises(ValueError, match=word):
                    _lib.check(call(), name)
        assert call(n=0) == 0 and call() == 0 and call(max_dist=1) == 0 and call(max_dist=254) == 0
    assert pair(flags=1) == 0
    torch.cuda.synchronize()
    assert store.pair_distance(0, np.zeros((0, 2))).shape == (0,) and store.pair_distance(0, []).dtype == np.uint8
    assert store.node_distances(0, []).shape == (0, N) and store.node_distances(0, []).dtype == np.uint8
    for max_dist in (0, 255):
        with pytest.raises(ValueError, match='max_dist = %d' % max_dist):
            store.pair_distance(0, [[0, 1]], max_dist=max_dist)
        with pytest.raises(ValueError, match='max_dist = %d' % max_dist):
            store.node_distances(0, [0], max_dist=max_dist)
    with pytest.raises(ValueError, match='graph'):
        store.pair_distance(1, [[0, 1]])
    with pytest.raises(ValueError, match='outside'):
        store.pair_distance(0, [[0, N]])
    with pytest.raises(ValueError, match='outside'):
        store.node_distances(0, [-1])


def test_graphstore_methods_equal_the_raw_calls():
    a, c = case_a(), case_c()
    for mask in (False, True):
        got = a.store.pair_distance(0, a.pairs[:5000], mask_target=mask)
        assert got.dtype == np.uint8 and got.shape == (5000,) and np.array_equal(got, _raw(a.store, 0, a.pairs[:5000], 1 if mask else 0, 8))
        assert np.array_equal(c.store.pair_distance(0, c.pairs[::7], mask_target=mask, max_dist=100), cap(c.want[1 if mask else 0][::7], 100))
    vec = a.store.node_distances(0, [3, 3, 299])
    assert vec.dtype == np.uint8 and vec.shape == (3, a.N) and np.array_equal(vec, cap(a.vec[[3, 3, 299]], 8))
    assert np.array_equal(c.store.node_distances(0, [0, 259], max_dist=254), c.vec[[0, 259]])
    s2 = torch.cuda.Stream()
    with torch.cuda.stream(s2):
        assert np.array_equal(a.store.pair_distance(0, a.pairs[:5000], mask_target=True), got)


# ---------------------------------------------------------------------------------------------------- AUC over completed tables, driver
@pytest.mark.parametrize('mask', [False, True])
def test_link_distance_auc_equals_the_auc_of_the_restated_distances(mask):
    import gmeta_amd
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, pos, info1)
    names, labels = tables['train']
    want = np.zeros(len(names), np.uint8)
    for k, nm in enumerate(names):
        g, a, b = (int(x) for x in nm.split('_'))
        want[k] = ref.pair_distance(*d['graphs'][g], [(a, b)], 1 if mask else 0, 8)[0]
    got = gmeta_amd.link_distance_scores(store, names, mask_target=mask)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    auc = gmeta_amd.link_distance_auc(store, names, labels, mask_target=mask)
    assert tuple(auc) == gmeta_amd.DISTANCE_SCORES and auc['graph_distance'] == gmeta_amd.link_auc(gmeta_amd.graph_distance_index(want, 8), labels)
    if not mask:
        assert auc['graph_distance'] == 1.0 and (want[np.asarray(labels) == '1'] == 1).all()         # unmasked, every positive is an edge
    print('mask %s: AUC graph_distance %.6f' % (mask, auc['graph_distance']))


def test_train_driver_reports_the_distance_auc(tmp_path, capsys):
    import gmeta_amd
    from gmeta_amd import datadir, synth
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric']
    res = drv.main(drv.parse(base + ['--distance', '8']))
    text = capsys.readouterr().out
    auc = res['distance_auc']
    assert tuple(auc) == gmeta_amd.DISTANCE_SCORES and 0.0 <= auc['graph_distance'] <= 1.0, auc
    assert 'Distance test AUC: graph_distance %.4f' % auc['graph_distance'] in text and 'PageRank test AUC' not in text and 'pagerank_auc' not in res
    # over the completed test table, with the mask: the same call by hand
    from gmeta_amd.negatives import read_link_tables
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root + '/'), info1, mode='uniform')
    assert auc == gmeta_amd.link_distance_auc(store, *tables['test'], mask_target=True, max_dist=8)
    every = drv.main(drv.parse(base + ['--distance', '8', '--pagerank', '1', '--heuristics', '2']))
    text = capsys.readouterr().out
    assert text.index('Heuristic test AUC:') < text.index('Path test AUC:') < text.index('PageRank test AUC:') < text.index('Distance test AUC:')
    assert every['distance_auc'] == auc and {k: v for k, v in every.items() if k not in ('heuristic_auc', 'path_auc', 'pagerank_auc')} == res
    plain = drv.main(drv.parse(base + ['--pagerank', '1', '--heuristics', '2']))
    text = capsys.readouterr().out
    assert 'Distance test AUC' not in text and 'distance_auc' not in plain
    assert plain == {k: v for k, v in every.items() if k != 'distance_auc'}      # the flag changes nothing else
