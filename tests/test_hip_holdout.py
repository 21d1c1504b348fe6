"""GPU (-m gpu): gm_store_without_edges / gm_store_split_edges / gm_store_dims / gm_store_read_csr and the Python layers above them, bit for bit against the
restatement of the definition (tests/holdout_ref.py; the definition itself is in include/gmeta_hip.h): the read-back of derived stores over a three-graph
multigraph store with every edge case of the removal list, the scan's block boundaries, a derived store against the store the constructor builds from the
filtered edges through the calls that read it, agreement with mask_target on single pairs, the hashed split, store lifetimes and the driver's flag."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import holdout_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
CHUNK = 1024      # slots per block of the flag / compact kernels (GM_HO_CHUNK, csrc/holdout.hip)
SIZES = (150, 260, 90)


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def host_graphs(weighted):
    """three multigraphs (parallel edges, self loops, one-directional edges, isolated nodes) -> [(N, src, dst, w)], [(ptr, idx, w)], features"""
    from gmeta_amd.graphstore import edges_to_in_csr
    rng = np.random.default_rng(7)
    raw = [ref.multigraph(N, 4 * N, rng, weighted=weighted) for N in SIZES]
    csr = []
    for N, src, dst, w in raw:
        got = edges_to_in_csr(N, src, dst, w)
        csr.append(got if weighted else got + (None,))
    feats = [rng.standard_normal((N, 6)).astype(f32) for N in SIZES]
    return raw, csr, feats


@functools.lru_cache(maxsize=None)
def parent(weighted):
    import gmeta_amd
    raw, csr, feats = host_graphs(weighted)
    store = gmeta_amd.GraphStore([(p, i) for p, i, _ in csr], feats, edge_weights=[w for _, _, w in csr] if weighted else None)
    assert store.n_edges == [len(i) for _, i, _ in csr]
    return store


def built(csr_list, feats, weighted):
    """the store the constructor builds on the host from in-CSRs"""
    import gmeta_amd
    return gmeta_amd.GraphStore([(p, i) for p, i, _ in csr_list], feats, edge_weights=[w for _, _, w in csr_list] if weighted else None)


def assert_store_is(store, want, sym):
    """every graph of `store`, read back in both orientations, equals the restated arrays bit for bit; so do the dims and the flag"""
    for g, w in enumerate(want):
        n, e, s = store.dims(g)
        assert (n, e) == (len(w['in'][0]) - 1, len(w['in'][1])) and store.n_nodes[g] == n and store.n_edges[g] == e
        assert s == (sym and 'GM_EXTRACT_NO_SYM' not in os.environ)
        for o, key in ((0, 'in'), (1, 'out')):
            ptr, idx, wt = store.read_csr(g, o)
            assert np.array_equal(ptr, w[key][0]) and np.array_equal(idx, w[key][1]), (g, key)
            assert (wt is None) == (w[key][2] is None) and (wt is None or np.array_equal(bits(wt), bits(w[key][2]))), (g, key)


def edge_pairs(csr, g):
    src, dst = ref.edge_list(csr[g][0], csr[g][1])
    return np.stack([src, dst], axis=1)


def removal(name, csr):
    """the removal lists of the named case, one per graph (None: nothing)"""
    rng = np.random.default_rng(11)
    some = lambda g, k: edge_pairs(csr, g)[rng.choice(len(csr[g][1]), k, replace=False)][:, ::-1]      # noqa: E731  (named against the stored direction)
    N1 = SIZES[1]
    if name == 'empty':
        return [None, None, None]
    if name == 'middle':
        return [None, some(1, 120), None]
    if name == 'mixed':
        return [np.concatenate([some(0, 60), some(0, 60)]), some(1, 300), some(2, 40)]                   # duplicates among them
    if name == 'missing':                                                                                 # isolated nodes: these keys name no edge
        return [np.array([[SIZES[0] - 1, SIZES[0] - 2], [SIZES[0] - 1, SIZES[0] - 1]]), np.array([[N1 - 1, 0]]), None]
    if name == 'loops':                                                                                   # (a, a): the self loops of 0, 1, 2 of every graph
        return [np.array([[0, 0], [1, 1]]), np.array([[2, 2]]), np.array([[0, 0], [1, 1], [2, 2]])]
    if name == 'row':                                                                                     # every edge at node 5 of graph 1, either direction: its rows empty
        e = edge_pairs(csr, 1)
        return [None, e[(e[:, 0] == 5) | (e[:, 1] == 5)], None]
    if name == 'all':
        return [edge_pairs(csr, g) for g in range(3)]
    raise KeyError(name)


CASES = ('empty', 'middle', 'mixed', 'missing', 'loops', 'row', 'all')


# ---------------------------------------------------------------------------------------------------- 1. read-back equals the restatement
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('name', CASES)
def test_read_back_equals_the_restatement(name, weighted):
    _, csr, feats = host_graphs(weighted)
    store = parent(weighted)
    removed = removal(name, csr)
    keys = [ref.pair_keys(N, [] if r is None else r) for N, r in zip(SIZES, removed)]
    want, sym = ref.without_edges(csr, keys)
    got = store.without_edges(removed if name != 'middle' else {1: removed[1]})
    try:
        assert got.n_graphs == 3 and got.feat_dim == 6 and got.weighted == weighted
        assert_store_is(got, want, sym)
        if name == 'empty':
            assert got.n_edges == store.n_edges
            for g in range(3):
                for a, b in zip(got.read_csr(g, 1), store.read_csr(g, 1)):
                    assert (a is None and b is None) or np.array_equal(a, b)
        if name == 'row':
            assert want[1]['in'][0][5] == want[1]['in'][0][6] and want[1]['out'][0][5] == want[1]['out'][0][6] and csr[1][0][6] > csr[1][0][5]
        if name == 'all':
            assert got.n_edges == [0, 0, 0] and not sym and not got.has_edges(1, [[0, 1], [2, 2]]).any()
        if name == 'loops':
            e = [edge_pairs(csr, g) for g in range(3)]
            lost = sum(int(((e[g][:, 0] == a) & (e[g][:, 1] == a)).sum()) for g in range(3) for a in np.asarray(removed[g])[:, 0])
            assert store.has_edges(0, [[0, 0]])[0] and not got.has_edges(0, [[0, 0]])[0] and sum(store.n_edges) - sum(got.n_edges) == lost >= 6
        # the lazily read host copy is the in-CSR, and symmetric() answers from it
        for g in range(3):
            assert np.array_equal(got.host_csr[g][0], want[g]['in'][0]) and np.array_equal(got.host_csr[g][1], want[g]['in'][1])
            if weighted:
                assert np.array_equal(bits(got.host_weights[g]), bits(want[g]['in'][2]))
        assert got.host_weights is None or weighted
        assert got.symmetric() == sym or sum(got.n_edges) == 0
    finally:
        got.close()


@pytest.mark.parametrize('weighted', [False, True])
def test_a_removal_can_make_the_store_symmetric(weighted, monkeypatch):
    import gmeta_amd
    from gmeta_amd.graphstore import edges_to_in_csr
    rng = np.random.default_rng(3)
    N = 300
    und = np.unique(np.sort(rng.integers(0, N - 4, (900, 2)), axis=1), axis=0)
    und = und[und[:, 0] != und[:, 1]]
    arcs = np.array([[N - 1, 0], [N - 2, 7], [3, N - 3]])                                           # one-directional, to or from nodes no other edge touches
    src, dst = np.concatenate([und[:, 0], und[:, 1], arcs[:, 0]]), np.concatenate([und[:, 1], und[:, 0], arcs[:, 1]])
    order = np.lexsort((src, dst))
    src, dst = src[order], dst[order]
    w = None
    if weighted:                                                                                     # w_uv == w_vu, as the flag asks of a weighted store
        w = (1.0 + ((np.minimum(src, dst) * 31 + np.maximum(src, dst)) % 13) / 8.0).astype(f32)
    got = edges_to_in_csr(N, src, dst, w)
    csr = [got if weighted else got + (None,)]
    feats = [rng.standard_normal((N, 4)).astype(f32)]
    store = built(csr, feats, weighted)
    assert not store.dims(0)[2] and not store.symmetric()
    want, sym = ref.without_edges(csr, [ref.pair_keys(N, arcs)])
    assert sym
    held = store.without_edges([arcs])
    assert_store_is(held, want, True)
    assert held.symmetric()
    same = built([want[0]['in']], feats, weighted)
    assert same.dims(0) == held.dims(0)
    two = store.without_edges([arcs[:2]])                                                            # one arc left: still not symmetric
    assert not two.dims(0)[2]
    monkeypatch.setenv('GM_EXTRACT_NO_SYM', '1')                                                     # the override of gm_store_create holds here too
    off = store.without_edges([arcs])
    assert not off.dims(0)[2]
    for s in (held, same, two, off, store):
        s.close()


def _raw(store, keys, off):
    from gmeta_amd import _lib
    d_keys = torch.from_numpy(np.asarray(keys, np.int64)).cuda() if len(keys) else None
    h = C.c_void_p()
    off = np.asarray(off, np.int64)
    _lib.check(_lib.lib().gm_store_without_edges(store.handle, _lib.ptr(d_keys), _lib.ptr(off), C.byref(h), _lib.stream_ptr()), 'gm_store_without_edges')
    return h


def test_bad_lists_are_refused():
    from gmeta_amd import _lib
    store = parent(False)
    N0, N1 = SIZES[0], SIZES[1]
    for keys, off, text in (([5, 3], [0, 2, 2, 2], 'ascending'), ([5, 5], [0, 2, 2, 2], 'ascending'), ([N0 * N0], [0, 1, 1, 1], 'outside'), ([-1], [0, 1, 1, 1], 'outside'),
                            ([3, N1 * N1], [0, 1, 2, 2], 'outside'), ([3], [0, 1, 0, 1], 'monotone'), ([3], [1, 1, 1, 1], 'h_key_off')):
        with pytest.raises(ValueError, match=text):
            _raw(store, keys, off)
    # a key that falls under its predecessor only across a list boundary is fine: each list ascends on its own
    h = _raw(store, [9, 3], [0, 1, 2, 2])
    _lib.lib().gm_store_destroy(h)
    with pytest.raises(ValueError, match='node id outside'):
        store.without_edges({0: [[0, N0]]})
    with pytest.raises(ValueError, match='graph'):
        store.without_edges({3: [[0, 1]]})
    with pytest.raises(ValueError, match='entries'):
        store.without_edges([None, None])
    assert np.array_equal(store.pair_keys(1, [[4, 2], [2, 4], [7, 7], [0, 1]]), np.array([1, 2 * N1 + 4, 7 * N1 + 7]))


# ---------------------------------------------------------------------------------------------------- 2. scan boundaries
def test_a_hub_row_longer_than_several_blocks():
    from gmeta_amd.graphstore import edges_to_in_csr
    N = 6000
    leaves = np.arange(1, N)
    ring = np.stack([leaves, np.roll(leaves, 1)], axis=1)                                            # the leaves joined one way round, so that rows differ
    src = np.concatenate([np.zeros(N - 1, np.int64), leaves, ring[:, 0]])
    dst = np.concatenate([leaves, np.zeros(N - 1, np.int64), ring[:, 1]])
    csr = [edges_to_in_csr(N, src, dst) + (None,)]
    assert csr[0][0][1] - csr[0][0][0] == N - 1 > 5 * CHUNK
    store = built(csr, [np.zeros((N, 4), f32)], False)
    rng = np.random.default_rng(5)
    cut = np.concatenate([[1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, N - 1], rng.choice(leaves, 700, replace=False)])      # hub slots at the block edges among them
    removed = np.concatenate([np.stack([np.zeros_like(cut), cut], axis=1), ring[rng.choice(len(ring), 300, replace=False)]])
    want, sym = ref.without_edges(csr, [ref.pair_keys(N, removed)])
    got = store.without_edges([removed])
    assert_store_is(got, want, sym)
    assert not got.has_edges(0, removed).any()
    got.close(); store.close()


@pytest.mark.parametrize('E', [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_edge_counts_at_a_block_boundary(E):
    from gmeta_amd.graphstore import edges_to_in_csr
    rng = np.random.default_rng(E)
    N = 120
    code = rng.choice(N * N, E, replace=False)                                                      # E distinct directed edges, self loops among them
    src, dst = code // N, code % N
    w = (rng.integers(1, 9, E) / 4.0).astype(f32)
    csr = [edges_to_in_csr(N, src, dst, w)]
    store = built(csr, [np.zeros((N, 4), f32)], True)
    assert store.n_edges == [E]
    slots = lambda ptr, idx, at: np.stack([idx[at].astype(np.int64), np.searchsorted(ptr, at, side='right') - 1], axis=1)      # noqa: E731
    optr, oidx, _ = ref.out_csr(*csr[0])
    for name, at in (('first and last slot of every block', [s for b in range(0, E, CHUNK) for s in (b, min(b + CHUNK, E) - 1)]),
                     ('the slots either side of every block edge', [s for b in range(CHUNK, E, CHUNK) for s in (b - 1, b)] or [0]),
                     ('nothing', [])):
        at = np.asarray(at, np.int64)
        for ptr, idx in ((csr[0][0], csr[0][1]), (optr, oidx)):                                      # the slots named in the in-CSR, then in the by-source CSR
            removed = slots(ptr, idx, at)
            want, sym = ref.without_edges(csr, [ref.pair_keys(N, removed)])
            got = store.without_edges([removed])
            assert_store_is(got, want, sym)
            assert len(at) == 0 or got.n_edges[0] < E, name
            got.close()
    store.close()


# ---------------------------------------------------------------------------------------------------- 3. derived equals host-built
@pytest.mark.parametrize('weighted', [False, True])
def test_a_derived_store_behaves_as_the_store_built_on_the_host(weighted):
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    _, csr, feats = host_graphs(weighted)
    store = parent(weighted)
    removed = removal('mixed', csr)
    want, _ = ref.without_edges(csr, [ref.pair_keys(N, r) for N, r in zip(SIZES, removed)])
    a, b = store.without_edges(removed), built([w['in'] for w in want], feats, weighted)
    rng = np.random.default_rng(2)
    try:
        assert a.n_nodes == b.n_nodes and a.n_edges == b.n_edges and a.symmetric() == b.symmetric()
        for g, N in enumerate(SIZES):
            pairs = np.concatenate([rng.integers(0, N, (200, 2)), removed[g][:40], edge_pairs(csr, g)[:60]])
            pairs = pairs[pairs[:, 0] != pairs[:, 1]]
            for mask in (False, True):
                assert np.array_equal(bits(a.pair_scores(g, pairs, mask)), bits(b.pair_scores(g, pairs, mask)))
                assert np.array_equal(a.pair_walks(g, pairs, mask), b.pair_walks(g, pairs, mask))
            assert np.array_equal(a.has_edges(g, pairs), b.has_edges(g, pairs))
            assert np.array_equal(a.neighbour_degrees(g), b.neighbour_degrees(g))
            assert np.array_equal(a.negative_pairs(g, 100, seed=9, mode='two_hop', exclude=removed[g]), b.negative_pairs(g, 100, seed=9, mode='two_hop', exclude=removed[g]))
            assert np.array_equal(a.negative_pairs(g, 150, seed=9), b.negative_pairs(g, 150, seed=9))
            nodes = np.arange(N)
            with a.sketches(g, hops=2, p=6, k=32) as sa, b.sketches(g, hops=2, p=6, k=32) as sb:
                for level in (1, 2):
                    for x, y in zip(sa.registers(nodes, level), sb.registers(nodes, level)):
                        assert np.array_equal(x, y)
            with a.propagated_features(g, hops=2) as pa, b.propagated_features(g, hops=2) as pb:
                for level in (0, 1, 2):
                    assert np.array_equal(bits(pa.rows(nodes, level)), bits(pb.rows(nodes, level)))
        # one extracted batch of pair subgraphs over all three graphs: the same nodes, the same induced edges, the same features
        seeds = []
        for g, N in enumerate(SIZES):
            i = rng.integers(0, N - 3, 6)
            seeds.append(np.column_stack([np.full(6, g), i, (i + 1 + rng.integers(0, N - 5, 6)) % (N - 3)]))      # i != j, both among the nodes that have edges
        seeds = np.concatenate(seeds).astype(np.int32)
        for mode in (_lib.LINK_SYMMETRIC, _lib.LINK_SYMMETRIC | _lib.LINK_MASK_TARGET):
            ba = SubgraphBatch.extract(a, seeds, [0, 9, 18], 2, 40, 222, mode)
            bb = SubgraphBatch.extract(b, seeds, [0, 9, 18], 2, 40, 222, mode)
            assert ba.rows == bb.rows and ba.edges == bb.edges and ba.rows > len(seeds)
            assert np.array_equal(ba.parent(), bb.parent())
            for t in (False, True):
                for x, y in zip(ba.csr(t), bb.csr(t)):
                    assert np.array_equal(x, y)
            del ba, bb
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------- 4. agreement with mask_target
def test_removing_one_pair_scores_it_as_mask_target_scores_it():
    _, csr, _ = host_graphs(False)
    store = parent(False)
    rng = np.random.default_rng(4)
    seen = 0
    for g in (0, 1, 2):
        e = edge_pairs(csr, g)
        e = e[e[:, 0] != e[:, 1]]
        for p in e[rng.choice(len(e), 4, replace=False)].tolist():
            held = store.without_edges({g: [p]})
            try:
                assert store.has_edges(g, [p])[0] and not held.has_edges(g, [p])[0]
                assert np.array_equal(held.pair_walks(g, [p]), store.pair_walks(g, [p], mask_target=True))
                assert np.array_equal(held.pair_distance(g, [p]), store.pair_distance(g, [p], mask_target=True))
                a, b = held.pair_scores(g, [p]), store.pair_scores(g, [p], mask_target=True)
                for col in (0, 4):                                                                   # cn and pref_attachment: exact in both
                    assert bits(a[:, col]) == bits(b[:, col])
                seen += 1
            finally:
                held.close()
    assert seen == 12


# ---------------------------------------------------------------------------------------------------- 5. the split
def _split_raw(store, g, seed, t_test, t_val, capacity=None):
    from gmeta_amd import _lib
    cnt = (C.c_int64 * 3)()
    call = lambda p, c, cap: _lib.lib().gm_store_split_edges(store.handle, g, seed, t_test, t_val, _lib.ptr(p), _lib.ptr(c), cap, cnt, _lib.stream_ptr())      # noqa: E731
    assert call(None, None, 0) == 0
    counts = tuple(cnt)
    n = counts[1] + counts[2]
    cap = n if capacity is None else capacity
    pairs = torch.full((n + 1, 2), -7, dtype=torch.int32, device='cuda')
    cls = torch.full((n + 1,), 9, dtype=torch.uint8, device='cuda')
    rc = call(pairs, cls, cap)
    return rc, counts, pairs.cpu().numpy(), cls.cpu().numpy()


@pytest.mark.parametrize('weighted', [False, True])
def test_split_equals_the_restatement(weighted):
    _, csr, _ = host_graphs(weighted)
    store = parent(weighted)
    for g, seed, val, test in ((0, 222, 0.05, 0.10), (1, 222, 0.05, 0.10), (1, 5 + (3 << 32), 0.3, 0.2), (2, 7, 0.0, 1.0), (2, 7, 1.0, 0.0), (0, 1, 0.0, 0.0)):
        t_test, t_val = ref.thresholds(val, test)
        wp, wc, wcnt = ref.split_edges(csr[g][0], csr[g][1], g, seed, t_test, t_val)
        rc, cnt, pairs, cls = _split_raw(store, g, seed, t_test, t_val)
        n = len(wp)
        assert rc == 0 and cnt == wcnt and np.array_equal(pairs[:n], wp) and np.array_equal(cls[:n], wc)
        assert (pairs[n:] == -7).all() and (cls[n:] == 9).all()                                       # nothing behind the held-out pairs is written
        v, t = store.split_edges(g, val=val, test=test, seed=seed)
        assert np.array_equal(v, wp[wc == 1]) and np.array_equal(t, wp[wc == 2]) and v.dtype == np.int64
        if n:
            assert store.has_edges(g, wp).all()
            assert not set(map(tuple, v.tolist())) & set(map(tuple, t.tolist()))
            rc, _, pairs, _ = _split_raw(store, g, seed, t_test, t_val, capacity=n - 1)
            assert rc == -4 and (pairs == -7).all()                                                   # GM_ERANGE, and nothing written
    from gmeta_amd import _lib
    cnt = (C.c_int64 * 3)()
    assert _lib.lib().gm_store_split_edges(store.handle, 0, 1, 5, 4, None, None, 0, cnt, _lib.stream_ptr()) == -1
    assert _lib.lib().gm_store_split_edges(store.handle, 0, 1, 0, 2 ** 32 + 1, None, None, 0, cnt, _lib.stream_ptr()) == -1
    for bad in (dict(val=-0.1), dict(test=1.5), dict(val=0.6, test=0.5)):
        with pytest.raises(ValueError, match='fractions'):
            store.split_edges(0, **bad)


def test_split_then_hold_out():
    _, csr, _ = host_graphs(False)
    store = parent(False)
    val, test = store.split_edges(1, val=0.1, test=0.2)
    both = np.concatenate([val, test])
    assert len(val) and len(test)
    held = store.without_edges({1: both})
    try:
        assert not held.has_edges(1, both).any()
        rows = ref.neighbour_rows(csr[1][0], csr[1][1])
        links = np.array([[u, v] for u in range(SIZES[1]) for v in rows[u] if u < v])
        gone = set(map(tuple, both.tolist()))
        kept = np.array([p for p in links.tolist() if tuple(p) not in gone])
        assert len(kept) + len(both) == len(links) and held.has_edges(1, kept).all() and held.has_edges(1, kept[:, ::-1]).all()
        # the held-out store splits into nothing it has lost, and the other graphs are untouched
        v2, t2 = held.split_edges(1, val=0.1, test=0.2)
        assert len(v2) == 0 and len(t2) == 0
        assert held.n_edges[0] == store.n_edges[0] and held.n_edges[2] == store.n_edges[2]
    finally:
        held.close()


# ---------------------------------------------------------------------------------------------------- 6. lifetime
def test_parent_and_derived_stores_close_in_any_order():
    _, csr, feats = host_graphs(True)
    removed = removal('mixed', csr)
    want, sym = ref.without_edges(csr, [ref.pair_keys(N, r) for N, r in zip(SIZES, removed)])
    other = removal('middle', csr)
    want2, sym2 = ref.without_edges(csr, [ref.pair_keys(N, [] if r is None else r) for N, r in zip(SIZES, other)])
    pairs = edge_pairs(csr, 1)[:50]
    # the parent goes first
    store = built(csr, feats, True)
    a, b = store.without_edges(removed), store.without_edges(other)                                  # two derived stores of one parent
    expect = a.pair_scores(1, pairs)
    store.close()
    assert_store_is(a, want, sym); assert_store_is(b, want2, sym2)
    assert np.array_equal(bits(a.pair_scores(1, pairs)), bits(expect))
    again = a.without_edges(other)                                                                   # a derived store is a store: it derives another
    a.close()
    assert again.n_edges[1] < b.n_edges[1] and again.n_edges[0] == want[0]['in'][0][-1]
    b.close(); again.close(); again.close()
    # the derived store goes first
    store = built(csr, feats, True)
    before = store.pair_scores(1, pairs)
    a = store.without_edges(removed)
    a.close()
    assert np.array_equal(bits(store.pair_scores(1, pairs)), bits(before))
    assert_store_is(store, ref.without_edges(csr, [[], [], []])[0], False)
    store.close()


# ---------------------------------------------------------------------------------------------------- 7. the driver
def test_train_driver_scores_the_families_on_the_held_out_graphs(tmp_path, capsys):
    import gmeta_amd
    from gmeta_amd import datadir, synth
    from gmeta_amd.negatives import read_link_tables, _pair
    from test_hip_pair_scores import DRIVER, _positives_only, _splits
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric']
    families = ['--heuristics', '2', '--pagerank', '1', '--distance', '4', '--buddy', '2', '--rank_k', '5']
    res = drv.main(drv.parse(base + families + ['--holdout', '1']))
    text = capsys.readouterr().out
    keys = ('heuristic_auc', 'path_auc', 'pagerank_auc', 'distance_auc', 'buddy_auc', 'heuristic_ranking', 'path_ranking', 'pagerank_ranking', 'distance_ranking',
            'buddy_ranking')
    assert all(k + '_holdout' in res and k not in res for k in keys), sorted(res)
    lines = [l for l in text.splitlines() if 'test AUC' in l or 'test Hits@' in l or ' test ' in l and 'MRR' in l]
    assert len(lines) == 10 and all(l.endswith(' (held out)') for l in lines), lines
    assert 'BUDDY test AUC: %.4f (held out)' % res['buddy_auc_holdout'] in text
    plain = drv.main(drv.parse(base + families))
    text = capsys.readouterr().out
    assert 'held out' not in text and set(plain) == {'test_acc', 'early_stopped_test_acc', 'val_best'} | set(keys)
    assert {k: plain[k] for k in ('test_acc', 'early_stopped_test_acc', 'val_best')} == {k: res[k] for k in ('test_acc', 'early_stopped_test_acc', 'val_best')}
    # the derived store of the run, rebuilt by hand, holds no test (or validation) positive and every training positive
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root + '/'), info1, mode='uniform')
    held = gmeta_amd.link_holdout(store, tables)
    only_val = gmeta_amd.link_holdout(store, tables, splits=('val',))
    for split, gone, gone_val in (('test', True, False), ('val', True, True), ('train', False, False)):
        by_graph = {}
        for nm, lab in zip(*tables[split]):
            if lab == '1':
                g, i, j = _pair(nm)
                by_graph.setdefault(g, []).append((i, j))
        for g, p in by_graph.items():
            assert store.has_edges(g, p).all()
            assert held.has_edges(g, p).any() != gone and held.has_edges(g, p).all() != gone
            assert only_val.has_edges(g, p).all() != gone_val
    assert res['heuristic_auc_holdout'] == gmeta_amd.link_heuristic_auc(held, *tables['test'], mask_target=True)
    assert res['buddy_auc_holdout'] == drv.buddy_auc(held, tables['train'], tables['test'], 2)
    for s in (held, only_val, store):
        s.close()
