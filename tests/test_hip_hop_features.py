"""GPU (-m gpu): gm_store_propagate_build, gm_prop_rows, gm_prop_pair_features and the Python layers above them against the float64 restatement of the
definition (tests/hop_feature_ref.py; the definition itself is in include/gmeta_hip.h).  The levels are fp32 sums: every level of every node is held to the
DERIVED tolerance ref.bound (a running-error recursion, no measurement), the tests print the worst error / bound ratio.  Everything the definition promises
bit for bit is compared as bits.  The references are computed once per (case, width, weights, flag) at hops = 8 and shared: a level does not depend on the
levels behind it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import distance_ref
import hop_feature_ref as ref
import negative_ref
from test_hip_pair_pagerank import _stream, tuning

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = -7.5
WIDTHS = (5, 64, 100, 128, 300)               # ld 32 (narrower than a wave), 64, 100 (tail columns in the second chunk), 128 (two floats per lane), 300 (four per lane, more than one chunk)
HOPS = (1, 3, 8)
CHUNKS = (0, 1, 7, 64, 2 ** 30)               # 0: the library's choice; 1: every row of two or more entries is cut; 2^30: none is


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def ld_of(F):
    return F if F % 4 == 0 else 32 if F <= 32 else (F + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def graph(which):
    """-> N, src, dst, w (fp32 weights in [0.25, 4) for the weighted stores)"""
    if which == 'hub':
        return ref.hub_case()
    N, src, dst = negative_ref.multigraph_case() if which == 'multigraph' else distance_ref.chain_case()[:3]
    w = np.exp2(np.random.default_rng(41).uniform(-2, 2, len(src))).astype(f32)
    return N, src, dst, w


@functools.lru_cache(maxsize=None)
def made(which, F, weighted):
    """-> store, (ptr, idx, w) as the store holds the graph, X"""
    import gmeta_amd
    N, src, dst, w = graph(which)
    X = ref.features(N, F, 100 + F)
    store = gmeta_amd.GraphStore([(N, src, dst)], [X], edge_weights=[w] if weighted else None)
    ptr, idx = store.host_csr[0]
    g = (ptr, idx, store.host_weights[0] if weighted else None)
    want = ref.csr(N, src, dst, w if weighted else None)
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and (not weighted or np.array_equal(g[2], want[2]))
    return store, g, X


@functools.lru_cache(maxsize=None)
def want(which, F, weighted, self_loops):
    """-> float64 [9, N, F] levels and their tolerance, by the definition at hops = 8"""
    _, g, X = made(which, F, weighted)
    x, E = ref.levels(*g, X, 8, self_loops), ref.bound(*g, X, 8, self_loops)
    x.setflags(write=False); E.setflags(write=False)
    return x, E


class built:
    """gm_store_propagate_build through the C ABI itself, destroyed at the end of the block."""

    def __init__(self, store, g, hops, flags, stream=None):
        from gmeta_amd import _lib
        self.h = C.c_void_p()
        _lib.check(_lib.lib().gm_store_propagate_build(store.handle, g, hops, flags, _stream(stream), C.byref(self.h)), 'gm_store_propagate_build')
        self.hops, self.F, self.N = hops, store.feat_dim, store.n_nodes[g]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from gmeta_amd import _lib
        _lib.lib().gm_prop_destroy(self.h)
        self.h = None
        return False

    def rows(self, level, nodes, stream=None):
        """float32 [m, F]; 64 floats behind the output are poisoned beforehand and must stay so."""
        from gmeta_amd import _lib
        a = np.ascontiguousarray(np.asarray(nodes, np.int64).reshape(-1), np.int32)
        m = len(a)
        d_a = torch.from_numpy(a).cuda() if m else None
        out = torch.full((m * self.F + 64,), POISON, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        _lib.check(_lib.lib().gm_prop_rows(self.h, level, _lib.ptr(d_a), m, _lib.ptr(out), _stream(stream)), 'gm_prop_rows')
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert (out[m * self.F:] == POISON).all()
        return out[:m * self.F].reshape(m, self.F)

    def all_levels(self, stream=None):
        return np.stack([self.rows(t, np.arange(self.N), stream) for t in range(self.hops + 1)])

    def pairs(self, pairs, op, stream=None):
        """float32 [n, hops + 1, F]; 64 poisoned floats behind."""
        from gmeta_amd import _lib
        p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
        n, E = len(p), (self.hops + 1) * self.F
        d_p = torch.from_numpy(p).cuda() if n else None
        out = torch.full((n * E + 64,), POISON, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        _lib.check(_lib.lib().gm_prop_pair_features(self.h, _lib.ptr(d_p), n, op, _lib.ptr(out), _stream(stream)), 'gm_prop_pair_features')
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert (out[n * E:] == POISON).all()
        return out[:n * E].reshape(n, self.hops + 1, self.F)


def levels_of(store, hops, flags, chunk=0, g=0, stream=None):
    with tuning(prop_chunk=chunk):
        with built(store, g, hops, flags, stream) as p:
            return p.all_levels(stream)


# ---------------------------------------------------------------------------------------------------- against the restatement: every level of every node
@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('which', ['multigraph', 'chain', 'hub'])
def test_every_level_of_every_node_within_the_derived_bound(which, F):
    from gmeta_amd import _lib
    N = graph(which)[0]
    worst = 0.0
    for weighted in (False, True):
        store, g, X = made(which, F, weighted)
        longest = int(np.diff(g[0]).max())
        assert longest >= {'multigraph': 400, 'chain': 2, 'hub': 600}[which] and (np.diff(g[0]) == 0).any() and N % 64 != 0
        for flags in (0, 1):
            x, E = want(which, F, weighted, flags)
            for hops in HOPS:
                for chunk in CHUNKS:
                    with tuning(prop_chunk=chunk):
                        with built(store, 0, hops, flags) as p:
                            got = p.all_levels()
                            n, h, f, fl, nb = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
                            assert _lib.lib().gm_prop_dims(p.h, C.byref(n), C.byref(h), C.byref(f), C.byref(fl), C.byref(nb)) == 0
                            assert (n.value, h.value, f.value, fl.value, nb.value) == (N, hops, F, flags, (hops + 1) * N * ld_of(F) * 4)
                    what = (weighted, flags, hops, chunk)
                    assert got.dtype == f32 and got.shape == (hops + 1, N, F) and np.isfinite(got).all(), what
                    assert np.array_equal(bits(got[0]), bits(X)), what                             # level 0 is the store's features
                    err = np.abs(got.astype(np.float64) - x[:hops + 1])
                    ok = err <= E[:hops + 1]
                    assert ok.all(), (what, np.argwhere(~ok)[:5], float((err / np.maximum(E[:hops + 1], 1e-300))[~ok].max()))
                    worst = max(worst, float((err[1:] / np.maximum(E[1:hops + 1], 1e-300)).max()))
            assert x[1].any() and (flags == 0 or x[8].any()) and (E[1:][x[1:] != 0] > 0).all()      # (the chain's edges point one way each: without the self loops its walks die out)
    print('%s F = %d: worst error / bound %.3f' % (which, F, worst))
    assert worst > 0


# ---------------------------------------------------------------------------------------------------- what the definition promises bit for bit
@pytest.mark.parametrize('chunk', [0, 7])
def test_bitwise_promises(chunk):
    import gmeta_amd
    N, src, dst, w = graph('hub')
    store, g, X = made('hub', 100, False)
    side = torch.cuda.Stream()
    for flags in (0, 1):
        a = levels_of(store, 3, flags, chunk)
        b = levels_of(store, 3, flags, chunk, stream=side)                                         # another stream
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(levels_of(store, 3, flags, chunk)))
        assert np.array_equal(bits(a[0]), bits(X))                                                 # level 0 against the store's features
        ones = gmeta_amd.GraphStore([(N, src, dst)], [X], edge_weights=[np.ones(len(src), f32)])   # all weights 1.0: the unweighted bits
        assert ones.weighted and np.array_equal(bits(levels_of(ones, 3, flags, chunk)), bits(a))
        for wt in (None, [w]):                                                                     # a column depends on its own column alone: ld 100 against ld 32
            wide = gmeta_amd.GraphStore([(N, src, dst)], [X], edge_weights=wt)
            five = gmeta_amd.GraphStore([(N, src, dst)], [np.ascontiguousarray(X[:, :5])], edge_weights=wt)
            assert np.array_equal(bits(levels_of(wide, 3, flags, chunk)[:, :, :5]), bits(levels_of(five, 3, flags, chunk)))
        for F in (64, 128, 300):                                                                        # ... and every tiling against the narrowest: ld 64, 128 (two floats per lane), 300 (four)
            XF = ref.features(N, F, 9)
            wideF = gmeta_amd.GraphStore([(N, src, dst)], [XF], edge_weights=[w])
            five = gmeta_amd.GraphStore([(N, src, dst)], [np.ascontiguousarray(XF[:, F - 5:])], edge_weights=[w])
            assert np.array_equal(bits(levels_of(wideF, 2, flags, chunk)[:, :, F - 5:]), bits(levels_of(five, 2, flags, chunk)))
        # the second graph of a two-graph store against the same graph alone
        M, ms, md, mw = graph('multigraph')
        XM = ref.features(M, 100, 5)
        for wts in (None, [mw, w]):
            two = gmeta_amd.GraphStore([(M, ms, md), (N, src, dst)], [XM, X], edge_weights=wts)
            alone = store if wts is None else gmeta_amd.GraphStore([(N, src, dst)], [X], edge_weights=[w])
            assert np.array_equal(bits(levels_of(two, 3, flags, chunk, g=1)), bits(levels_of(alone, 3, flags, chunk)))
            first = gmeta_amd.GraphStore([(M, ms, md)], [XM], edge_weights=None if wts is None else [mw])
            assert np.array_equal(bits(levels_of(two, 3, flags, chunk, g=0)), bits(levels_of(first, 3, flags, chunk)))


def test_the_store_destroyed_first_and_two_handles_alive_together():
    import gmeta_amd
    N, src, dst, w = graph('chain')
    X = ref.features(N, 64, 6)
    store = gmeta_amd.GraphStore([(N, src, dst)], [X])
    with built(store, 0, 2, 1) as one, built(store, 0, 3, 0) as other:
        a, b = one.all_levels(), other.all_levels()
        store.close()
        assert store.handle is None
        assert np.array_equal(bits(one.all_levels()), bits(a)) and np.array_equal(bits(other.all_levels()), bits(b)) and np.array_equal(bits(a[0]), bits(X))
        assert not np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- the row and pair calls
@pytest.mark.parametrize('F', [5, 100, 128])
def test_rows_and_pair_features(F):
    from gmeta_amd import _lib
    store, g, X = made('hub', F, True)
    N = graph('hub')[0]
    rng = np.random.default_rng(2)
    side = torch.cuda.Stream()
    with built(store, 0, 3, 1) as p:
        x = p.all_levels()
        nodes = np.array([3, 3, N, 0, -1, 400, 3, 2 ** 31 - 1, 1])
        for level in (0, 2, 3):
            got = p.rows(level, nodes, stream=side if level == 2 else None)
            inside = (nodes >= 0) & (nodes < N)
            assert not got[~inside].any() and np.array_equal(bits(got[inside]), bits(x[level][nodes[inside]]))
        some = rng.integers(0, N, (300, 2))
        pairs = np.concatenate([some, some[:40, ::-1], [[7, 7], [0, 0], [0, 1], [1, 0], [5, N], [-1, 5], [N, N]]])
        ok = ((pairs >= 0) & (pairs < N)).all(1)
        a, b = np.where(ok, pairs[:, 0], 0), np.where(ok, pairs[:, 1], 0)
        for name, op in (('hadamard', 0), ('abs_diff', 1)):
            got = p.pairs(pairs, op)
            expect = ref.pair_features(x[:, a], x[:, b], name).transpose(1, 0, 2)                    # numpy fp32 on the rows: the same bits
            expect[~ok] = 0
            assert got.shape == (len(pairs), 4, F) and np.array_equal(bits(got), bits(expect)), name
            assert np.array_equal(bits(got[:40]), bits(got[300:340]))                              # both orientations
            assert np.array_equal(bits(got), bits(p.pairs(pairs[:, ::-1], op, stream=side)))
            assert not got[~ok].any() and got[ok].any()
        assert not p.pairs([[7, 7]], 1).any() and np.array_equal(bits(p.pairs([[7, 7]], 0)[0]), bits(x[:, 7] * x[:, 7]))
        # an output pointer that is not 16-byte aligned takes the narrow stores: the same bits
        buf = torch.full((1 + 2 * 4 * F + 64,), POISON, dtype=torch.float32, device='cuda')
        d_p = torch.tensor([[0, 1], [9, 4]], dtype=torch.int32, device='cuda')
        assert _lib.lib().gm_prop_pair_features(p.h, _lib.ptr(d_p), 2, 0, C.c_void_p(buf.data_ptr() + 4), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        buf = buf.cpu().numpy()
        assert buf[0] == POISON and (buf[1 + 8 * F:] == POISON).all() and np.array_equal(bits(buf[1:1 + 8 * F].reshape(2, 4, F)), bits(p.pairs([[0, 1], [9, 4]], 0)))


# ---------------------------------------------------------------------------------------------------- against the library's own GraphConv aggregate
@pytest.mark.parametrize('weighted', [False, True])
def test_level_one_against_gm_aggregate_over_a_batch_of_all_nodes(weighted):
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    store, g, X = made('multigraph', 64, weighted)
    N = graph('multigraph')[0]
    x, E = want('multigraph', 64, weighted, 0)
    B = SubgraphBatch.from_nodes(store, np.array([(0, 0, -1)], np.int32), [0, 1], [np.arange(N)], False)
    assert B.rows == N and B.edges == len(g[1])
    row = B._read(_lib.F_FEAT_ROW, B.rows, np.int32)
    assert sorted(row.tolist()) == list(range(N))
    out = torch.empty(B.rows, 64, dtype=torch.float32, device='cuda')
    nm = B.device_ptr(_lib.F_NORM)
    _lib.check(_lib.lib().gm_aggregate(B.handle, 0, 1, None, 64, nm, nm, _lib.ptr(out), _lib.stream_ptr()), 'gm_aggregate')
    torch.cuda.synchronize()
    agg = out.cpu().numpy()
    got = levels_of(store, 1, 0)[1]
    err = np.abs(got[row].astype(np.float64) - agg.astype(np.float64))
    assert (np.abs(agg.astype(np.float64) - x[1][row]) <= E[1][row]).all()                         # both are fp32 evaluations of the definition ...
    assert (err <= E[1][row]).all()                                                                # ... and stay within the bound of each other
    print('level 1 against gm_aggregate: worst difference / bound %.3f' % float((err / np.maximum(E[1][row], 1e-300)).max()))
    assert agg.any()


# ---------------------------------------------------------------------------------------------------- errors and empty calls
def test_bad_arguments_the_budget_and_empty_calls():
    from gmeta_amd import _lib
    lib = _lib.lib()
    store, g, X = made('hub', 300, False)
    st = _lib.stream_ptr()
    out = C.c_void_p()

    def build(g=0, hops=2, flags=1, o=C.byref(out), s=store.handle):
        return lib.gm_store_propagate_build(s, g, hops, flags, st, o)

    def fails(rc, text, code=-1):
        assert rc == code, rc
        msg = lib.gm_last_error().decode()
        assert text in msg, msg

    fails(build(g=-1), 'graph -1'); fails(build(g=1), 'graph 1'); fails(build(s=None), 'store is NULL'); fails(build(o=None), 'out is NULL')
    fails(build(hops=0), 'hops = 0'); fails(build(hops=9), 'hops = 9'); fails(build(hops=-1), 'hops = -1')
    fails(build(flags=2), 'flag bits 0x2'); fails(build(flags=-1), 'flag bits')
    with tuning(prop_chunk=-1):
        fails(build(), 'prop_chunk = -1')
    with tuning(prop_mib=-2):
        fails(build(), 'prop_mib = -2')
    with tuning(prop_mib=1):                                                                        # 4 x 401 x 300 x 4 = 1.92 MB
        rc = build(hops=3)
        assert rc == -4 and out.value is None
        msg = lib.gm_last_error().decode()
        assert all(t in msg for t in ('1924800 bytes', 'N = 401', 'hops = 3', 'F = 300', 'prop_mib = 1', '1048576')), msg
        with pytest.raises(RuntimeError, match=r'code -4.*N = 401, hops = 3, F = 300; prop_mib = 1'):
            store.propagated_features(0, hops=3)
        assert build(hops=1) == 0 and out.value                                                    # 0.96 MB: fits
        lib.gm_prop_destroy(out)
    assert lib.gm_get_tuning(b'prop_mib') == 0 and lib.gm_get_tuning(b'prop_chunk') == 0
    with built(store, 0, 2, 1) as p:                                                                # after the errors: a good call is unaffected
        d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')
        o = torch.zeros(4 * 3 * 300, dtype=torch.float32, device='cuda')
        P, O = _lib.ptr(d_p), _lib.ptr(o)
        fails(lib.gm_prop_pair_features(None, P, 4, 0, O, st), 'prop is NULL')
        fails(lib.gm_prop_pair_features(p.h, P, -1, 0, O, st), 'n = -1')
        fails(lib.gm_prop_pair_features(p.h, P, 2 ** 31, 0, O, st), 'n = 2147483648')
        fails(lib.gm_prop_pair_features(p.h, P, 4, 2, O, st), 'op = 2')
        fails(lib.gm_prop_pair_features(p.h, P, 4, -1, O, st), 'op = -1')
        fails(lib.gm_prop_pair_features(p.h, None, 4, 0, O, st), 'NULL argument')
        fails(lib.gm_prop_pair_features(p.h, P, 4, 0, None, st), 'NULL argument')
        fails(lib.gm_prop_rows(None, 0, P, 4, O, st), 'prop is NULL')
        fails(lib.gm_prop_rows(p.h, -1, P, 4, O, st), 'level = -1')
        fails(lib.gm_prop_rows(p.h, 3, P, 4, O, st), 'level = 3')
        fails(lib.gm_prop_rows(p.h, 0, P, -5, O, st), 'm = -5')
        fails(lib.gm_prop_rows(p.h, 0, P, 2 ** 31, O, st), 'm = 2147483648')
        fails(lib.gm_prop_rows(p.h, 0, None, 4, O, st), 'NULL argument')
        fails(lib.gm_prop_rows(p.h, 0, P, 4, None, st), 'NULL argument')
        fails(lib.gm_prop_dims(None, None, None, None, None, None), 'prop is NULL')
        assert lib.gm_prop_dims(p.h, None, None, None, None, None) == 0
        assert lib.gm_prop_pair_features(p.h, None, 0, 1, None, st) == 0                            # n == 0 / m == 0: a no-op, with NULL pointers too
        assert lib.gm_prop_rows(p.h, 2, None, 0, None, st) == 0
        torch.cuda.synchronize()
        assert not o.any()                                                                          # nothing was written by a refused call
        assert p.rows(1, []).shape == (0, 300) and p.pairs(np.zeros((0, 2)), 0).shape == (0, 3, 300)
        x, E = want('hub', 300, False, 1)
        assert (np.abs(p.all_levels().astype(np.float64) - x[:3]) <= E[:3]).all()
    lib.gm_prop_destroy(None)                                                                       # NULL: nothing to do


def test_an_edgeless_graph_and_a_two_node_store():
    import gmeta_amd
    X = ref.features(70, 12, 1)
    N, src, dst, _ = graph('chain')
    none = gmeta_amd.GraphStore([(N, src, dst), (70, np.zeros(0, np.int64), np.zeros(0, np.int64))], [ref.features(N, 12, 0), X])
    a = levels_of(none, 2, 0, g=1)
    assert np.array_equal(bits(a[0]), bits(X)) and not a[1:].any()                                  # empty rows give zeros
    b = levels_of(none, 2, 1, g=1)
    assert all(np.array_equal(bits(b[t]), bits(X)) for t in range(3))                               # only the self loop: d = 1, norm = 1
    X2 = ref.features(2, 3, 2)
    two = gmeta_amd.GraphStore([(2, np.array([0]), np.array([1]))], [X2])
    c = levels_of(two, 2, 0)
    assert np.array_equal(bits(c[1][1]), bits(X2[0])) and not c[1][0].any() and not c[2].any()


# ---------------------------------------------------------------------------------------------------- the Python layers
def test_python_layers_equal_the_raw_calls():
    import gmeta_amd
    N, src, dst, w = graph('hub')
    M, ms, md, mw = graph('multigraph')
    X, XM = ref.features(N, 100, 3), ref.features(M, 100, 4)
    store = gmeta_amd.GraphStore([(N, src, dst), (M, ms, md)], [X, XM], edge_weights=[w, mw])
    rng = np.random.default_rng(6)
    pairs = rng.integers(0, N, (55, 2))
    with built(store, 0, 3, 1) as raw:
        want_rows = raw.rows(2, np.arange(0, N, 7))
        want_p = {op: raw.pairs(pairs, code) for op, code in (('hadamard', 0), ('abs_diff', 1))}
    with built(store, 0, 2, 0) as raw:
        want_plain = raw.rows(2, [5, 5, 0])
    pf = store.propagated_features(0, hops=3)
    assert isinstance(pf, gmeta_amd.PropagatedFeatures)
    assert (pf.n_nodes, pf.hops, pf.feat_dim, pf.self_loops, pf.nbytes) == (N, 3, 100, True, 4 * N * 100 * 4)
    got = pf.rows(np.arange(0, N, 7), 2)
    assert got.dtype == f32 and np.array_equal(bits(got), bits(want_rows))
    for op in ref.OPS:
        got = pf.pair_features(pairs, op=op)
        assert isinstance(got, np.ndarray) and got.dtype == f32 and got.shape == (55, 4, 100) and np.array_equal(bits(got), bits(want_p[op]))
        t = pf.pair_features(pairs, op=op, as_torch=True)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (55, 4, 100)
        assert np.array_equal(bits(t.cpu().numpy()), bits(want_p[op]))
    assert np.array_equal(bits(pf.pair_features(pairs)), bits(want_p['hadamard']))                  # the default op
    assert pf.pair_features(np.zeros((0, 2), np.int64)).shape == (0, 4, 100) and pf.rows([], 0).shape == (0, 100)
    assert tuple(pf.pair_features([], as_torch=True).shape) == (0, 4, 100)
    with pytest.raises(ValueError, match='outside'):
        pf.pair_features([[0, N]])
    with store.propagated_features(0, hops=2, self_loops=False) as plain:
        assert (plain.hops, plain.self_loops, plain.nbytes) == (2, False, 3 * N * 100 * 4)
        assert np.array_equal(bits(plain.rows([5, 5, 0], 2)), bits(want_plain))
    assert plain.handle is None
    # link_propagated_features: names of both graphs, in name order, either orientation
    other = store.propagated_features(1, hops=3)
    names, expect = [], []
    for k in range(40):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, (N, M)[g], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b))
    for op in ref.OPS:
        got = gmeta_amd.link_propagated_features({0: pf, 1: other}, names, op=op)
        expect = np.stack([(pf, other)[int(nm.split('_')[0])].pair_features([[int(v) for v in nm.split('_')[1:]]], op=op)[0] for nm in names])
        assert got.shape == (40, 4, 100) and got.dtype == f32 and np.array_equal(bits(got), bits(expect))
        flipped = ['%s_%s_%s' % (nm.split('_')[0], nm.split('_')[2], nm.split('_')[1]) for nm in names]
        assert np.array_equal(bits(gmeta_amd.link_propagated_features([pf, other], flipped, op=op)), bits(got))
    assert len({nm[0] for nm in names}) == 2
    short = store.propagated_features(1, hops=2)
    with pytest.raises(ValueError, match='different hops'):
        gmeta_amd.link_propagated_features({0: pf, 1: short}, names)
    short.close(); other.close()
    pf.close(); pf.close()
    with pytest.raises(ValueError, match='closed'):
        pf.rows([0], 0)
