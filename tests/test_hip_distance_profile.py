"""GPU (-m gpu): gm_store_pair_distance_profile and the Python layers above it against the restatement of the definition (tests/distance_profile_ref.py: two
plain breadth-first searches and a count; the definition itself is in include/gmeta_hip.h) and against the device's own distance and score calls.  The tables
are integers: everything is EQUAL, there is no tolerance.  The references are computed once per (case, flags, max_dist) and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import distance_profile_ref as ref
import path_walk_ref
import pair_score_ref
from test_hip_pair_distance import _raw as _raw_distance
from test_hip_pair_distance import _raw_vec, _store, _stream, case_a, case_c, case_w, tuning

pytestmark = pytest.mark.gpu
POISON = -0x5A5A5A5B
MASKS = (0, 1)


def _raw(store, g, pairs, flags=0, max_dist=3, stream=None):
    """The C ABI itself: int32 [n, D + 2, D + 2].  64 ints behind the last table are poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
    n, E = len(p), (max_dist + 2) ** 2
    d_p = torch.from_numpy(p).cuda() if n else None
    out = torch.full((n * E + 64,), POISON, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_store_pair_distance_profile(store.handle, g, _lib.ptr(d_p), n, flags, max_dist, _lib.ptr(out), _stream(stream)),
               'gm_store_pair_distance_profile')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.dtype == np.int32 and (out[n * E:] == POISON).all()
    return out[:n * E].reshape(n, max_dist + 2, max_dist + 2)


# ---------------------------------------------------------------------------------------------------- shared references, computed once
_COLS = {}                                                                    # per case: the searched columns, shared by every (flags, max_dist)


@functools.lru_cache(maxsize=None)
def want_a(flags, max_dist):
    """The restated tables of every ordered pair of the multigraph."""
    a = case_a()
    w = ref.profile(a.N, a.src, a.dst, a.pairs, flags, max_dist, a.nb, _COLS.setdefault('a', {}))
    w.setflags(write=False)
    return w


CHAIN_NODES = np.concatenate([np.arange(0, 21), np.arange(250, 276), np.arange(320, 331)])


@functools.lru_cache(maxsize=None)
def chain_pairs():
    p = np.array([(a, b) for a in CHAIN_NODES for b in CHAIN_NODES], np.int64)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want_c(flags, max_dist):
    c = case_c()
    w = ref.profile(c.N, c.src, c.dst, chain_pairs(), flags, max_dist, c.nb, _COLS.setdefault('c', {}))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def wide():
    """-> store, N, src, dst, nb, 40 random pairs and 10 adjacent ones"""
    N, src, dst = ref.wide_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    rng = np.random.default_rng(8)
    some = rng.integers(0, N, (40, 2))
    ends = [u for u in rng.permutation(N).tolist() if nb[u]][:10]
    edges = np.array([(u, sorted(nb[u])[0]) if k % 2 else (sorted(nb[u])[0], u) for k, u in enumerate(ends)], np.int64)
    pairs = np.concatenate([some, edges])
    return _store([(N, src, dst)]), N, src, dst, nb, pairs


@functools.lru_cache(maxsize=None)
def hubs():
    """The planted hubs of path_walk_ref: the pairs among the planted nodes and their restated tables at max_dist 3, both flags."""
    store, N, nodes, sample, vec, pairs, dist = case_w()
    _, src, dst, _ = path_walk_ref.walk_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    cols = {}
    return store, pairs, {f: ref.profile(N, src, dst, pairs, f, 3, nb, cols) for f in MASKS}, dist


def one_hot(d, max_dist):
    """int32 [n, D + 2]: a single 1 per row at cap(d)."""
    at = ref.cap(d, max_dist)
    out = np.zeros((len(at), max_dist + 2), np.int32)
    out[np.arange(len(at)), at] = 1
    return out


# ---------------------------------------------------------------------------------------------------- the multigraph: every ordered pair
@pytest.mark.parametrize('max_dist', [1, 2, 3, 4, 7])
def test_multigraph_every_ordered_pair(max_dist):
    a = case_a()
    N, S = a.N, max_dist + 2
    assert N == 300 and max(len(r) for r in a.nb) == 211 and not a.nb[299] and int(a.adj.sum()) == 2 * 1306
    lo, hi = a.pairs.min(1), a.pairs.max(1)
    off = lo != hi
    vec = ref.cap(_raw_vec(a.store, 0, np.arange(N), max_dist), max_dist)                          # the device's own rows
    hist = np.stack([np.bincount(r, minlength=S) for r in vec])
    got = {}
    for flags in MASKS:                                                                            # flags 1: 300 + 2,612 distinct columns in ONE group: rows a wave wide
        P = _raw(a.store, 0, a.pairs, flags, max_dist)
        assert np.array_equal(P, want_a(flags, max_dist)), flags
        assert (P.sum((1, 2)) == N).all()
        row0 = one_hot(_raw_distance(a.store, 0, a.pairs, flags, max_dist), max_dist)              # gm_store_pair_distance
        assert np.array_equal(P[:, 0, :], row0) and np.array_equal(P[:, :, 0], row0)
        cn = a.store.pair_scores(0, a.pairs, mask_target=bool(flags))[:, 0]                        # gm_store_pair_scores
        assert np.array_equal(P[off, 1, 1], cn[off].astype(np.int32))
        plain = ~a.adj if flags else np.ones(len(P), bool)                                         # the columns of gm_store_node_distances
        assert np.array_equal(P.sum(2)[plain], hist[lo][plain]) and np.array_equal(P.sum(1)[plain], hist[hi][plain])
        G = P.reshape(N, N, S, S)
        assert np.array_equal(G, G.transpose(1, 0, 2, 3))                                          # (a, b) and (b, a): the same bits
        same = P[~off]
        assert (same[:, 0, 0] == 1).all() and (same == same * np.eye(S, dtype=np.int32)).all()
        got[flags] = P
    assert np.array_equal(got[1][~a.adj], got[0][~a.adj]) and (got[1][a.adj][:, 0, 1] == 0).all()
    lone = got[0][299 * N + 299]                                                                   # an isolated node with itself
    assert lone[0, 0] == 1 and lone[S - 1, S - 1] == N - 1 and lone.sum() == N
    with tuning(dist_cols=128):                                                                    # hundreds of groups
        for flags in MASKS:
            assert np.array_equal(_raw(a.store, 0, a.pairs, flags, max_dist), got[flags]), flags
    at = np.unique(np.concatenate([np.arange(0, len(a.pairs), 7), np.nonzero(a.adj)[0]]))
    with tuning(dist_cols=64):                                                                     # groups of one word: the columns 63 / 64 of a group
        for flags in MASKS:
            assert np.array_equal(_raw(a.store, 0, a.pairs[at], flags, max_dist), got[flags][at]), flags


# ---------------------------------------------------------------------------------------------------- the chain: N no multiple of 64, bridges, isolated nodes
@pytest.mark.parametrize('flags', MASKS)
def test_chain_bridges_isolated_nodes_and_the_tail_bits(flags):
    c = case_c()
    N, D = c.N, 7
    pairs = chain_pairs()
    assert N == 331 and N % 64
    P = _raw(c.store, 0, pairs, flags, D)
    assert np.array_equal(P, want_c(flags, D))
    assert (P.sum((1, 2)) == N).all()                                                              # the bits behind node 330 never count

    def table(p, q):
        return P[int(np.nonzero((pairs[:, 0] == p) & (pairs[:, 1] == q))[0][0])]
    bridge = table(3, 4)
    assert bridge[0, 8 if flags else 1] == 1 and bridge[0].sum() == 1                              # a masked path edge: its ends never meet again
    two = table(329, 330)                                                                          # two isolated nodes
    assert two[0, 8] == 1 and two[8, 0] == 1 and two[8, 8] == N - 2 and two.sum() == N
    alone = table(330, 330)
    assert alone[0, 0] == 1 and alone[8, 8] == N - 1 and alone.sum() == N
    assert np.array_equal(table(4, 3), bridge) and np.array_equal(table(330, 329), two)
    with tuning(dist_cols=64, dist_chunk=1):
        assert np.array_equal(_raw(c.store, 0, pairs, flags, D), P)


# ---------------------------------------------------------------------------------------------------- more node-words than a wave has lanes
@pytest.mark.parametrize('max_dist', [3, 7])
def test_wide_graph_of_71_node_words(max_dist):
    store, N, src, dst, nb, pairs = wide()
    assert (N + 63) // 64 == 71 and all(b in nb[a] for a, b in pairs[40:].tolist())
    cols = _COLS.setdefault('wide', {})
    for flags in MASKS:
        P = _raw(store, 0, pairs, flags, max_dist)
        assert np.array_equal(P, ref.profile(N, src, dst, pairs, flags, max_dist, nb, cols)), flags
        assert (P.sum((1, 2)) == N).all() and (P[40:, 0, 1] == 1 - flags).all()


# ---------------------------------------------------------------------------------------------------- planted hubs: every cut and width
@pytest.mark.parametrize('chunk', [0, 1, 63, 64, 65, 2 ** 30])
def test_planted_hubs_under_every_cut_and_width(chunk):
    store, pairs, want, dist = hubs()
    base = {f: _raw(store, 0, pairs, f, 3) for f in MASKS}
    for cols in (0, 64, 4096):
        with tuning(dist_chunk=chunk, dist_cols=cols):
            for f in MASKS:
                got = _raw(store, 0, pairs, f, 3)
                assert np.array_equal(got, want[f]), (chunk, cols, f)
                assert got.tobytes() == base[f].tobytes(), (chunk, cols, f)                        # byte-identical to the library's own choice
    assert pairs[1].tolist() == [0, 1] and want[0][1][0, 1] == 1 and want[1][1][0, 2] == 1          # the two adjacent hubs: a detour of 2
    assert np.array_equal(want[0][:, 0, :], one_hot(dist[0], 3)) and np.array_equal(want[1][:, 0, :], one_hot(dist[1], 3))


# ---------------------------------------------------------------------------------------------------- the budget of level planes
def test_plane_budget_forces_small_groups_and_refuses_what_cannot_fit():
    from gmeta_amd import _lib
    a = case_a()
    at = np.arange(0, len(a.pairs), 5)
    planes_64 = 4 * 64 * 5 * 8                                                                     # (D + 1) levels x 64 columns x ceil(300 / 64) words x 8 bytes
    assert planes_64 == 10240
    for flags in MASKS:
        with tuning(dist_plane_kib=16):                                                            # one word of columns fits, two do not: 64-column groups at the default dist_cols
            got = _raw(a.store, 0, a.pairs[at], flags, 3)
        assert np.array_equal(got, want_a(flags, 3)[at]) and np.array_equal(got, _raw(a.store, 0, a.pairs[at], flags, 3))
    with tuning(dist_plane_kib=9):
        with pytest.raises(RuntimeError, match=r'code -4.*N = 300, max_dist = 3; dist_plane_kib = 9'):
            _raw(a.store, 0, a.pairs[:10], 0, 3)
        assert _raw(a.store, 0, a.pairs[:10], 0, 1).shape == (10, 3, 3)                            # two levels of 64 columns take 5 KiB
    with tuning(dist_plane_kib=-1):
        with pytest.raises(ValueError, match='dist_plane_kib = -1'):
            _raw(a.store, 0, a.pairs[:10], 0, 3)
    assert _lib.lib().gm_get_tuning(b'dist_plane_kib') == 0


# ---------------------------------------------------------------------------------------------------- a table depends on its own pair alone
@pytest.mark.parametrize('flags', MASKS)
def test_a_table_depends_on_its_own_pair_alone(flags):
    a = case_a()
    N = a.N
    rng = np.random.default_rng(12)
    pairs = np.concatenate([rng.integers(0, N, (700, 2)), np.stack([rng.integers(0, 2, 60), rng.integers(0, N, 60)], 1)])
    base = _raw(a.store, 0, pairs, flags)
    assert np.array_equal(base, want_a(flags, 3)[pairs[:, 0] * N + pairs[:, 1]])
    perm = rng.permutation(len(pairs))
    assert np.array_equal(_raw(a.store, 0, pairs[perm], flags), base[perm])                        # shuffled
    dup = rng.integers(0, len(pairs), 2000)
    assert np.array_equal(_raw(a.store, 0, pairs[dup], flags), base[dup])                          # with duplicates
    assert np.array_equal(_raw(a.store, 0, pairs[::3], flags), base[::3])                          # a subset
    cut = np.concatenate([_raw(a.store, 0, part, flags) for part in (pairs[:100], pairs[100:101], pairs[101:])])
    assert np.array_equal(cut, base)                                                               # three calls
    assert np.array_equal(_raw(a.store, 0, pairs[:, ::-1], flags), base)                           # the other orientation
    assert np.array_equal(_raw(a.store, 0, pairs, flags, stream=torch.cuda.Stream()), base)        # a second stream
    assert _raw(a.store, 0, pairs, flags).tobytes() == base.tobytes()                              # two runs


# ---------------------------------------------------------------------------------------------------- stores
def test_small_stores_the_third_graph_and_a_weighted_store():
    a = case_a()
    rng = np.random.default_rng(6)
    none = np.zeros(0, np.int64)
    one = _store([(1, none, none)])
    for flags in MASKS:
        P = _raw(one, 0, [(0, 0), (0, 1), (0, 0)], flags, 2)
        assert P[0].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and not P[1].any() and np.array_equal(P[2], P[0])
    graphs = {2: (2, np.array([1], np.int64), np.array([0], np.int64))}
    for N in (64, 65):
        graphs[N] = (N, rng.integers(0, N, 2 * N).astype(np.int64), rng.integers(0, N, 2 * N).astype(np.int64))
    for N, gr in graphs.items():
        store = _store([gr])
        every = np.array([(p, q) for p in range(N) for q in range(N)], np.int64)
        for flags in MASKS:
            for max_dist in (1, 3, 7):
                assert np.array_equal(_raw(store, 0, every, flags, max_dist), ref.profile(*gr, every, flags, max_dist)), (N, flags, max_dist)
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(a.src))).astype(np.float32)
    at = np.arange(0, len(a.pairs), 11)
    for weights in (None, [np.ones(len(graphs[64][1]), np.float32), np.ones(1, np.float32), w]):
        store = _store([graphs[64], graphs[2], (a.N, a.src, a.dst)], weights=weights)
        assert store.weighted == (weights is not None)
        for flags in MASKS:                                                                        # an offset slip would read graph 0's rows; the weights are ignored
            assert np.array_equal(_raw(store, 2, a.pairs[at], flags, 3), want_a(flags, 3)[at]), flags
        assert np.array_equal(_raw(store, 1, [(0, 1), (1, 0), (1, 1)], 1, 1), ref.profile(*graphs[2], [(0, 1), (1, 0), (1, 1)], 1, 1))


# ---------------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_n_zero_and_nodes_outside_the_graph():
    from gmeta_amd import _lib
    a = case_a()
    store, lib, N = a.store, _lib.lib(), a.N
    assert _raw(store, 0, np.zeros((0, 2))).shape == (0, 5, 5)                # n == 0: the poisoned entries stay
    null, st = C.c_void_p(0), _lib.stream_ptr()
    assert lib.gm_store_pair_distance_profile(store.handle, 0, null, 0, 0, 3, null, st) == 0       # n == 0 with NULL pointers
    odd = _raw(store, 0, [(0, N), (-1, 5), (N, N), (2 ** 31 - 1, 0), (0, 1), (7, 7)], 1, 3)
    assert not odd[:4].any() and np.array_equal(odd[4], want_a(1, 3)[1]) and np.array_equal(odd[5], want_a(1, 3)[7 * N + 7])
    out = torch.zeros((4, 25), dtype=torch.int32, device='cuda')
    d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')

    def call(g=0, n=4, flags=0, max_dist=3, p=_lib.ptr(d_p), o=_lib.ptr(out), s=store.handle):
        return lib.gm_store_pair_distance_profile(s, g, p, n, flags, max_dist, o, st)
    name = 'gm_store_pair_distance_profile'
    for kw, word in ((dict(g=1), 'graph 1'), (dict(g=-1), 'graph -1'), (dict(n=-1), 'n = -1'), (dict(n=2 ** 31), 'n = 2147483648'),
                     (dict(max_dist=0), r'max_dist = 0; 1 \.\. 7'), (dict(max_dist=8), r'max_dist = 8; 1 \.\. 7'), (dict(max_dist=-3), 'max_dist = -3'),
                     (dict(flags=2), 'flag bits 0x2'), (dict(flags=5), 'flag bits 0x5'), (dict(p=null), 'NULL argument'), (dict(o=null), 'NULL argument'),
                     (dict(s=null), 'store is NULL')):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**kw), name)
    for knob, value, word in (('dist_cols', 48, 'dist_cols = 48'), ('dist_cols', 4160, 'dist_cols = 4160'), ('dist_chunk', -1, 'dist_chunk = -1')):
        with tuning(**{knob: value}):
            with pytest.raises(ValueError, match=word):
                _lib.check(call(), name)
    assert call(n=0) == 0 and call() == 0 and call(max_dist=1) == 0 and call(max_dist=7) == 0 and call(flags=1) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- Python
def test_graphstore_method_and_link_distance_profiles():
    import gmeta_amd
    a, c = case_a(), case_c()
    for mask in (False, True):
        got = a.store.pair_distance_profile(0, a.pairs[:5000], mask_target=mask)
        assert got.dtype == np.int32 and got.shape == (5000, 5, 5) and np.array_equal(got, _raw(a.store, 0, a.pairs[:5000], 1 if mask else 0, 3))
        seven = c.store.pair_distance_profile(0, chain_pairs()[::5], mask_target=mask, max_dist=7)
        assert seven.shape[1:] == (9, 9) and np.array_equal(seven, want_c(1 if mask else 0, 7)[::5])
    assert a.store.pair_distance_profile(0, [], max_dist=2).shape == (0, 4, 4) and a.store.pair_distance_profile(0, np.zeros((0, 2))).dtype == np.int32
    with pytest.raises(ValueError, match='max_dist = 8'):
        a.store.pair_distance_profile(0, [[0, 1]], max_dist=8)
    with pytest.raises(ValueError, match='outside'):
        a.store.pair_distance_profile(0, [[0, a.N]])
    with torch.cuda.stream(torch.cuda.Stream()):
        assert np.array_equal(a.store.pair_distance_profile(0, a.pairs[:5000], mask_target=True), got)
    # two graphs, names in any orientation, rows in the order of the names
    store = _store([(a.N, a.src, a.dst), (c.N, c.src, c.dst)])
    rng = np.random.default_rng(21)
    trip = [(0, p, q) for p, q in rng.integers(0, a.N, (150, 2)).tolist()] + [(0, q, p) for p, q in a.pairs[a.adj][:40].tolist()]
    trip += [(1, p, q) for p, q in chain_pairs()[rng.integers(0, len(chain_pairs()), 150)].tolist()]
    trip = [trip[k] for k in rng.permutation(len(trip)).tolist()]
    names = ['%d_%d_%d' % t for t in trip]
    for mask in (False, True):
        got = gmeta_amd.link_distance_profiles(store, names, mask_target=mask, max_dist=4)
        assert got.dtype == np.int32 and got.shape == (len(names), 6, 6)
        for g, case in ((0, a), (1, c)):
            rows = [k for k, t in enumerate(trip) if t[0] == g]
            p = np.array([trip[k][1:] for k in rows], np.int64)
            want = ref.oriented(ref.profile(case.N, case.src, case.dst, p, 1 if mask else 0, 4, case.nb, _COLS.setdefault('a' if g == 0 else 'c', {})), p)
            assert np.array_equal(got[rows], want), (mask, g)
        assert any(not np.array_equal(t, t.T) for t in got)
    feats = gmeta_amd.distance_profile_features(got)
    assert feats.shape == (len(names), 36) and np.array_equal(feats, np.log1p((got + got.transpose(0, 2, 1)).astype(np.float64)).reshape(len(names), 36))
