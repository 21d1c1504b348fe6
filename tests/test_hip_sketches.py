"""GPU (-m gpu): gm_store_sketch_build, gm_sketch_registers, gm_sketch_pair_counts and the Python layers above them against the restatement of the definition
(tests/sketch_ref.py; the definition itself is in include/gmeta_hip.h) and against the device's own exact calls.  The sketches and the pair counts are
integers: everything is EQUAL, there is no tolerance.  Only the last test of the accuracy section holds float estimates, to the theoretical deviations of
the CPU test (sketch_ref.ball_bound / intersection_bound).  The references are computed once per (case, H, p, K) and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import distance_profile_ref
import pair_score_ref
import path_walk_ref
import sketch_ref as ref
from test_hip_pair_distance import _store, _stream, case_a, case_c, case_w, tuning

pytestmark = pytest.mark.gpu
SEED = 222
POISON8, POISON32, POISON64 = 0xAB, -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
SHAPES = [(1, 4, 32), (2, 8, 128), (3, 10, 512), (2, 6, 96)]                  # record dwords 36 (narrower than a wave), 192 (three chunks), 768, 112 (no power of two)


class built:
    """gm_store_sketch_build through the C ABI itself, destroyed at the end of the block."""

    def __init__(self, store, g, H, p, K, seed=SEED, stream=None):
        from gmeta_amd import _lib
        self.h = C.c_void_p()
        _lib.check(_lib.lib().gm_store_sketch_build(store.handle, g, H, p, K, seed, _stream(stream), C.byref(self.h)), 'gm_store_sketch_build')
        self.H, self.p, self.K = H, p, K

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from gmeta_amd import _lib
        _lib.lib().gm_sketch_destroy(self.h)
        self.h = None
        return False

    def registers(self, level, nodes, stream=None):
        """(uint8 [m, 2^p], uint32 [m, K]); 64 elements behind each output are poisoned beforehand and must stay so."""
        from gmeta_amd import _lib
        a = np.ascontiguousarray(np.asarray(nodes, np.int64).reshape(-1), np.int32)
        m, mreg = len(a), 1 << self.p
        d_a = torch.from_numpy(a).cuda() if m else None
        hll = torch.full((m * mreg + 64,), POISON8, dtype=torch.uint8, device='cuda')
        mh = torch.full((m * self.K + 64,), POISON32, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        _lib.check(_lib.lib().gm_sketch_registers(self.h, level, _lib.ptr(d_a), m, _lib.ptr(hll), _lib.ptr(mh), _stream(stream)), 'gm_sketch_registers')
        torch.cuda.synchronize()
        hll, mh = hll.cpu().numpy(), mh.cpu().numpy()
        assert (hll[m * mreg:] == POISON8).all() and (mh[m * self.K:] == POISON32).all()
        return hll[:m * mreg].reshape(m, mreg), mh[:m * self.K].reshape(m, self.K).view(np.uint32)

    def all_levels(self, N):
        got = [self.registers(d, np.arange(N)) for d in range(self.H + 1)]
        return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])

    def counts(self, pairs, stream=None):
        """(int64 [n, H + 1, H + 1, 3], int64 [n, 2, H + 1, 2]); 64 poisoned elements behind each."""
        from gmeta_amd import _lib
        p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
        n, L = len(p), self.H + 1
        E, EB = L * L * 3, 2 * L * 2
        d_p = torch.from_numpy(p).cuda() if n else None
        out = torch.full((n * E + 64,), POISON64, dtype=torch.int64, device='cuda')
        balls = torch.full((n * EB + 64,), POISON64, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        _lib.check(_lib.lib().gm_sketch_pair_counts(self.h, _lib.ptr(d_p), n, _lib.ptr(out), _lib.ptr(balls), _stream(stream)), 'gm_sketch_pair_counts')
        torch.cuda.synchronize()
        out, balls = out.cpu().numpy(), balls.cpu().numpy()
        assert (out[n * E:] == POISON64).all() and (balls[n * EB:] == POISON64).all()
        return out[:n * E].reshape(n, L, L, 3), balls[:n * EB].reshape(n, 2, L, 2)


# ---------------------------------------------------------------------------------------------------- shared references, computed once
@functools.lru_cache(maxsize=None)
def want_small(which, H, p, K):
    """The multigraph ('a') or the chain ('c') by the DEFINITION: registers of every node at every level, and the counts of every pair of nodes."""
    c = case_a() if which == 'a' else case_c()
    R, M = ref.by_definition(c.N, c.nb, H, p, K, SEED)
    counts, balls = ref.pair_counts_all(R, M)
    for w in (R, M, counts, balls):
        w.setflags(write=False)
    return R, M, counts, balls


@functools.lru_cache(maxsize=None)
def wide():
    """-> store, N, nb, the restated registers at (3, 8, 128) (its levels 0 .. 2 are those of H = 2), 40 random + 10 adjacent pairs, duplicates and one pair
    with a node outside the graph"""
    N, src, dst = distance_profile_ref.wide_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    rng = np.random.default_rng(8)
    some = rng.integers(0, N, (40, 2))
    ends = [u for u in rng.permutation(N).tolist() if nb[u]][:10]
    edges = np.array([(u, sorted(nb[u])[0]) if k % 2 else (sorted(nb[u])[0], u) for k, u in enumerate(ends)], np.int64)
    pairs = np.concatenate([some, edges, some[:3], edges[:2, ::-1], [[5, N]]])
    R, M = ref.by_recurrence(N, nb, 3, 8, 128, SEED)
    return _store([(N, src, dst)]), N, nb, R, M, pairs


@functools.lru_cache(maxsize=None)
def random_graph():
    N, src, dst, pairs = ref.random_case()
    return _store([(N, src, dst)]), N, pairs


def check_pairs_of_every_node(sk, N, counts, balls):
    """every ordered pair (x, y), in that order, against the all-pairs reference"""
    x, y = np.divmod(np.arange(N * N), N)
    got, got_b = sk.counts(np.stack([x, y], 1))
    assert np.array_equal(got, counts.reshape(N * N, *counts.shape[2:]))
    assert np.array_equal(got_b[:, 0], balls[np.minimum(x, y)]) and np.array_equal(got_b[:, 1], balls[np.maximum(x, y)])
    return got.reshape(N, N, *counts.shape[2:])


# ---------------------------------------------------------------------------------------------------- the multigraph and the chain: every node, every ordered pair
@pytest.mark.parametrize('H,p,K', SHAPES)
@pytest.mark.parametrize('which', ['a', 'c'])
def test_registers_of_every_node_and_counts_of_every_ordered_pair(which, H, p, K):
    c = case_a() if which == 'a' else case_c()
    R, M, counts, balls = want_small(which, H, p, K)
    assert max(len(r) for r in c.nb) == (211 if which == 'a' else 3) and not c.nb[c.N - 1] and c.N % 64 != 0
    with built(c.store, 0, H, p, K) as sk:
        gR, gM = sk.all_levels(c.N)
        assert gR.dtype == np.uint8 and gM.dtype == np.uint32
        assert np.array_equal(gR, R) and np.array_equal(gM, M)
        got = check_pairs_of_every_node(sk, c.N, counts, balls)
    assert np.array_equal(got, got.transpose(1, 0, 2, 3, 4))                                        # (x, y) and (y, x): the same bits
    d = np.arange(c.N)
    assert (got[d, d][:, np.arange(H + 1), np.arange(H + 1), 0] == K).all()                          # u == v on the diagonal
    assert (got[c.N - 1, c.N - 1, :, :, 0] == K).all() and (got[c.N - 1, c.N - 2, :, :, 0] == 0).all()      # isolated nodes: themselves at every level
    assert (np.diff(got[..., 1:], axis=2) <= 0).all() and (np.diff(got[..., 1:], axis=3) <= 0).all()


# ---------------------------------------------------------------------------------------------------- planted hubs: where a row is cut cannot change a bit
def test_planted_hubs_under_every_cut():
    store, N, nodes, sample, vec, pairs, dist = case_w()
    _, src, dst, _ = path_walk_ref.walk_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    H, p, K = 2, 8, 128
    R, M = ref.by_recurrence(N, nb, H, p, K, SEED)
    assert len(nb[0]) == len(nb[1]) == path_walk_ref.HUB_ROW and 1 in nb[0]
    for hub in (0, 1):                                                                             # level 1 of a hub: the sketch of its restated neighbourhood
        ball = np.array(sorted(nb[hub] | {hub}))
        assert np.array_equal(R[1, hub], R[0][ball].max(0)) and np.array_equal(M[1, hub], M[0][ball].min(0))
    want_c, want_b = ref.pair_counts(R, M, pairs)
    first = None
    for chunk in (1, 7, 64, 0):                                                                    # 1: every row of two or more entries is cut; 0: the library's choice
        with tuning(sketch_chunk=chunk):
            with built(store, 0, H, p, K) as sk:
                gR, gM = sk.all_levels(N)
                got = sk.counts(pairs)
        assert np.array_equal(gR, R) and np.array_equal(gM, M), chunk
        assert np.array_equal(got[0], want_c) and np.array_equal(got[1], want_b), chunk
        first = (gR, gM) if first is None else first
        assert np.array_equal(gR, first[0]) and np.array_equal(gM, first[1])


# ---------------------------------------------------------------------------------------------------- the wide case: N no multiple of 64, duplicates, outside, a stream
@pytest.mark.parametrize('H', [2, 3])
def test_wide_case_pairs_duplicates_outside_and_a_stream(H):
    store, N, nb, R, M, pairs = wide()
    assert N % 64 == 17 and len(pairs) == 56
    want_c, want_b = ref.pair_counts(R[:H + 1], M[:H + 1], pairs)
    assert not want_c[-1].any() and not want_b[-1].any() and want_c[:-1, ..., 2].all()
    side = torch.cuda.Stream()
    with built(store, 0, H, 8, 128, stream=side) as sk:
        for d in range(H + 1):
            gR, gM = sk.registers(d, np.arange(N), stream=side)
            assert np.array_equal(gR, R[d]) and np.array_equal(gM, M[d]), d
        got_c, got_b = sk.counts(pairs, stream=side)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_b, want_b)
        again = sk.counts(pairs[::-1])                                                             # the default stream, the other order: each entry on its own
        assert np.array_equal(again[0], want_c[::-1]) and np.array_equal(again[1], want_b[::-1])
        gR, gM = sk.registers(1, [N, 3, -1, 3])                                                    # outside the graph: zeros; duplicates
        assert not gR[0].any() and not gM[0].any() and not gR[2].any() and not gM[2].any()
        assert np.array_equal(gR[1], R[1, 3]) and np.array_equal(gR[3], R[1, 3]) and np.array_equal(gM[1], M[1, 3]) and np.array_equal(gM[3], M[1, 3])
        diag = np.stack([np.arange(0, N, 449)] * 2, 1)                                             # u == v: equal balls on the diagonal
        got_c = np.concatenate([got_c[:-1], sk.counts(diag)[0]])
    # against the device's own exact call: equal balls match in every word, disjoint balls in none
    inside = np.concatenate([pairs[:-1], diag])
    nodes, inv = np.unique(inside, return_inverse=True)
    inv = inv.reshape(-1, 2)
    dist = store.node_distances(0, nodes, max_dist=H)
    n_equal = n_disjoint = 0
    for i, (ix, iy) in enumerate(inv.tolist()):
        iu, iv = (ix, iy) if inside[i, 0] <= inside[i, 1] else (iy, ix)
        for a in range(H + 1):
            for b in range(H + 1):
                Bu, Bv = dist[iu] <= a, dist[iv] <= b
                if np.array_equal(Bu, Bv):
                    assert got_c[i, a, b, 0] == 128
                    n_equal += 1
                elif not (Bu & Bv).any():
                    assert got_c[i, a, b, 0] == 0
                    n_disjoint += 1
    assert n_equal >= 10 * (H + 1) and n_disjoint >= 100


# ---------------------------------------------------------------------------------------------------- the estimates against the device's exact profile
@pytest.mark.parametrize('H,p,K', [(2, 8, 128), (3, 8, 128)])
def test_estimated_profile_within_the_theoretical_deviation_of_the_exact_profile(H, p, K):
    import gmeta_amd
    store, N, pairs = random_graph()
    exact = store.pair_distance_profile(0, pairs, max_dist=H)
    I, su, sv = ref.cumulate(exact.astype(np.int64))
    U = su[:, :, None] + sv[:, None, :] - I
    with store.sketches(0, hops=H, p=p, k=K, seed=SEED) as sk:
        counts, balls = sk.pair_counts(pairs)
    P = gmeta_amd.sketch_distance_profile(counts, balls, N, p, K)
    assert P.shape == exact.shape and np.allclose(P.sum((1, 2)), N, rtol=1e-9, atol=0)
    est_I, est_su, est_sv = ref.cumulate(P)
    assert (np.abs(est_su - su) <= ref.ball_bound(su, p)).all() and (np.abs(est_sv - sv) <= ref.ball_bound(sv, p)).all()
    assert (np.abs(est_I - I) <= ref.intersection_bound(I, U, p, K)).all()


# ---------------------------------------------------------------------------------------------------- other graphs of a store, tiny stores
def test_second_graph_of_a_store_a_two_node_store_and_an_edgeless_graph():
    a = case_a()
    rng = np.random.default_rng(12)
    N2 = 150
    src, dst = rng.integers(0, N2, 400).astype(np.int64), rng.integers(0, N2, 400).astype(np.int64)
    store = _store([(a.N, a.src, a.dst), (N2, src, dst), (70, np.zeros(0, np.int64), np.zeros(0, np.int64))])
    nb = pair_score_ref.neighbourhoods(N2, src, dst)
    R, M = ref.by_recurrence(N2, nb, 2, 6, 96, SEED, g=1)
    assert not np.array_equal(M[0], ref.level0(N2, 6, 96, SEED, g=0)[1])                            # s_h, s_m differ by g
    pairs = rng.integers(0, N2, (200, 2))
    with built(store, 1, 2, 6, 96) as sk:
        gR, gM = sk.all_levels(N2)
        assert np.array_equal(gR, R) and np.array_equal(gM, M)
        want = ref.pair_counts(R, M, pairs)
        got = sk.counts(pairs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    R0, M0 = ref.level0(70, 8, 128, SEED, g=2)                                                      # no edge: every level is level 0
    with built(store, 2, 3, 8, 128) as sk:
        gR, gM = sk.all_levels(70)
        assert all(np.array_equal(gR[d], R0) and np.array_equal(gM[d], M0) for d in range(4))
        c, b = sk.counts([(4, 4), (4, 5)])
        assert (c[0, :, :, 0] == 128).all() and (c[1, :, :, 0] == 0).all() and (c[0, :, :, 1] == 255).all()
    two = _store([(2, np.array([0]), np.array([1]))])
    R, M = ref.by_definition(2, [{1}, {0}], 1, 4, 32, SEED)
    with built(two, 0, 1, 4, 32) as sk:
        gR, gM = sk.all_levels(2)
        assert np.array_equal(gR, R) and np.array_equal(gM, M) and np.array_equal(gR[1, 0], gR[1, 1])
        want = ref.pair_counts(R, M, [(0, 1), (1, 0), (1, 1)])
        got = sk.counts([(0, 1), (1, 0), (1, 1)])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0][0, 1, 1, 0] == 32


# ---------------------------------------------------------------------------------------------------- lifetimes
def test_two_sketches_alive_together_and_the_store_destroyed_first():
    from gmeta_amd import _lib
    c = case_c()
    store = _store([(c.N, c.src, c.dst)])
    R, M = want_small('c', 2, 8, 128)[:2]
    with built(store, 0, 2, 8, 128) as one, built(store, 0, 2, 8, 128, seed=SEED + 1) as other:
        R1, M1 = one.all_levels(c.N)
        R2, M2 = other.all_levels(c.N)
        assert np.array_equal(R1, R) and np.array_equal(M1, M)
        want2 = ref.by_recurrence(c.N, c.nb, 2, 8, 128, SEED + 1)
        assert np.array_equal(R2, want2[0]) and np.array_equal(M2, want2[1]) and not np.array_equal(M1, M2) and not np.array_equal(R1, R2)
        n, h, p, k, nbytes = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        assert _lib.lib().gm_sketch_dims(one.h, C.byref(n), C.byref(h), C.byref(p), C.byref(k), C.byref(nbytes)) == 0
        assert (n.value, h.value, p.value, k.value, nbytes.value) == (c.N, 2, 8, 128, c.N * 3 * (256 + 512))
        assert _lib.lib().gm_sketch_dims(one.h, None, None, None, None, None) == 0
        store.close()                                                                               # the store goes first: the sketch still answers
        assert store.handle is None
        R1b, M1b = one.all_levels(c.N)
        assert np.array_equal(R1b, R) and np.array_equal(M1b, M)
        pairs = np.array([(0, 5), (100, 260), (329, 330), (7, 7)])
        want = ref.pair_counts(R, M, pairs)
        got = one.counts(pairs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------------- errors
def test_bad_arguments_the_budget_and_n_zero():
    from gmeta_amd import _lib
    lib = _lib.lib()
    store, N, _ = random_graph()
    st = _lib.stream_ptr()
    out = C.c_void_p()

    def build(g=0, H=2, p=8, K=128, o=C.byref(out), s=store.handle):
        return lib.gm_store_sketch_build(s, g, H, p, K, SEED, st, o)

    def fails(rc, text, code=-1):
        assert rc == code, rc
        msg = lib.gm_last_error().decode()
        assert text in msg, msg

    fails(build(g=-1), 'graph -1'); fails(build(g=1), 'graph 1'); fails(build(s=None), 'store is NULL'); fails(build(o=None), 'out is NULL')
    fails(build(H=0), 'hops = 0'); fails(build(H=5), 'hops = 5'); fails(build(p=3), 'p = 3'); fails(build(p=11), 'p = 11')
    fails(build(K=0), 'k = 0'); fails(build(K=48), 'k = 48'); fails(build(K=544), 'k = 544'); fails(build(K=-32), 'k = -32')
    with tuning(sketch_chunk=-1):
        fails(build(), 'sketch_chunk = -1')
    with tuning(sketch_mib=-2):
        fails(build(), 'sketch_mib = -2')
    with tuning(sketch_mib=1):                                                                      # 2,000 x 4 x 3,072 = 24.6 MB
        rc = build(H=3, p=10, K=512)
        assert rc == -4 and out.value is None
        msg = lib.gm_last_error().decode()
        assert all(t in msg for t in ('24576000 bytes', 'N = 2000', 'hops = 3', 'p = 10', 'k = 512', 'sketch_mib = 1', '1048576')), msg
        with pytest.raises(RuntimeError, match=r'code -4.*N = 2000, hops = 3, p = 10, k = 512; sketch_mib = 1'):
            store.sketches(0, hops=3, p=10, k=512)
    assert lib.gm_get_tuning(b'sketch_mib') == 0 and lib.gm_get_tuning(b'sketch_chunk') == 0
    with built(store, 0, 2, 8, 128) as sk:                                                          # after the errors: a good call is unaffected
        d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')
        o64 = torch.zeros(4 * 27 + 4 * 12, dtype=torch.int64, device='cuda')
        o8 = torch.zeros(4 * 256, dtype=torch.uint8, device='cuda')
        o32 = torch.zeros(4 * 128, dtype=torch.int32, device='cuda')
        P, O = _lib.ptr(d_p), _lib.ptr(o64)
        fails(lib.gm_sketch_pair_counts(None, P, 4, O, O, st), 'sketch is NULL')
        fails(lib.gm_sketch_pair_counts(sk.h, P, -1, O, O, st), 'n = -1')
        fails(lib.gm_sketch_pair_counts(sk.h, P, 2 ** 31, O, O, st), 'n = 2147483648')
        fails(lib.gm_sketch_pair_counts(sk.h, None, 4, O, O, st), 'NULL argument')
        fails(lib.gm_sketch_pair_counts(sk.h, P, 4, None, O, st), 'NULL argument')
        fails(lib.gm_sketch_pair_counts(sk.h, P, 4, O, None, st), 'NULL argument')
        fails(lib.gm_sketch_registers(None, 0, P, 4, _lib.ptr(o8), _lib.ptr(o32), st), 'sketch is NULL')
        fails(lib.gm_sketch_registers(sk.h, -1, P, 4, _lib.ptr(o8), _lib.ptr(o32), st), 'level = -1')
        fails(lib.gm_sketch_registers(sk.h, 3, P, 4, _lib.ptr(o8), _lib.ptr(o32), st), 'level = 3')
        fails(lib.gm_sketch_registers(sk.h, 0, P, -5, _lib.ptr(o8), _lib.ptr(o32), st), 'm = -5')
        fails(lib.gm_sketch_registers(sk.h, 0, P, 2 ** 31, _lib.ptr(o8), _lib.ptr(o32), st), 'm = 2147483648')
        fails(lib.gm_sketch_registers(sk.h, 0, None, 4, _lib.ptr(o8), _lib.ptr(o32), st), 'NULL argument')
        fails(lib.gm_sketch_registers(sk.h, 0, P, 4, None, _lib.ptr(o32), st), 'NULL argument')
        fails(lib.gm_sketch_registers(sk.h, 0, P, 4, _lib.ptr(o8), None, st), 'NULL argument')
        fails(lib.gm_sketch_dims(None, None, None, None, None, None), 'sketch is NULL')
        assert lib.gm_sketch_pair_counts(sk.h, None, 0, None, None, st) == 0                        # n == 0 / m == 0: a no-op, with NULL pointers too
        assert lib.gm_sketch_registers(sk.h, 2, None, 0, None, None, st) == 0
        torch.cuda.synchronize()
        assert not o64.any() and not o8.any() and not o32.any()                                     # nothing was written by a refused call
        N_, src, dst, pairs = ref.random_case()
        R, M = ref.by_recurrence(N_, pair_score_ref.neighbourhoods(N_, src, dst), 2, 8, 128, SEED)
        want = ref.pair_counts(R, M, pairs[:20])
        got = sk.counts(pairs[:20])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    lib.gm_sketch_destroy(None)                                                                     # NULL: nothing to do


# ---------------------------------------------------------------------------------------------------- the Python layers
def test_node_sketches_methods_equal_the_raw_calls():
    import gmeta_amd
    store, N, nb, R, M, pairs = wide()
    inside = pairs[:-1]
    with built(store, 0, 2, 8, 128) as raw:
        want_c, want_b = raw.counts(inside)
        want_r = raw.registers(2, np.arange(0, N, 7))
    sk = store.sketches(0)
    assert isinstance(sk, gmeta_amd.NodeSketches)
    assert (sk.n_nodes, sk.hops, sk.p, sk.k, sk.seed, sk.nbytes) == (N, 2, 8, 128, 222, N * 3 * 768)
    c, b = sk.pair_counts(inside)
    assert c.dtype == np.int64 and c.shape == (55, 3, 3, 3) and b.dtype == np.int64 and b.shape == (55, 2, 3, 2)
    assert np.array_equal(c, want_c) and np.array_equal(b, want_b)
    hll, mh = sk.registers(np.arange(0, N, 7), 2)
    assert hll.dtype == np.uint8 and mh.dtype == np.uint32 and np.array_equal(hll, want_r[0]) and np.array_equal(mh, want_r[1])
    e = sk.pair_counts(np.zeros((0, 2), np.int64))
    assert e[0].shape == (0, 3, 3, 3) and e[1].shape == (0, 2, 3, 2) and sk.registers([], 0)[1].shape == (0, 128)
    with pytest.raises(ValueError, match='outside'):
        sk.pair_counts([[0, N]])
    sk.close(); sk.close()
    with pytest.raises(ValueError, match='closed'):
        sk.registers([0], 0)
    with store.sketches(0, hops=1, p=4, k=32, seed=5) as small:
        assert (small.hops, small.p, small.k, small.seed, small.nbytes) == (1, 4, 32, 5, N * 2 * 144)
        Rs, Ms = ref.by_recurrence(N, nb, 1, 4, 32, 5)
        hll, mh = small.registers(np.arange(N), 1)
        assert np.array_equal(hll, Rs[1]) and np.array_equal(mh, Ms[1])
    assert small.handle is None


def test_link_sketch_profiles_orient_by_name_and_the_features_have_the_exact_shape():
    import gmeta_amd
    store, N, nb, R, M, pairs = wide()
    inside = pairs[:-1]
    names = ['0_%d_%d' % (a, b) for a, b in inside.tolist()]
    with store.sketches(0, hops=3) as sk:
        counts, balls = sk.pair_counts(inside)
        want = gmeta_amd.sketch_distance_profile(counts, balls, N, 8, 128)
        got = gmeta_amd.link_sketch_profiles({0: sk}, names)
    swap = inside[:, 0] > inside[:, 1]
    assert swap.any() and (~swap).any() and got.shape == (55, 5, 5)
    assert np.array_equal(got[~swap], want[~swap]) and np.array_equal(got[swap], want[swap].transpose(0, 2, 1))
    assert any(not np.array_equal(t, t.T) for t in got[swap])
    exact = gmeta_amd.link_distance_profiles(store, names, max_dist=3)
    f, f_exact = gmeta_amd.sketch_profile_features(got), gmeta_amd.distance_profile_features(exact)
    assert f.shape == f_exact.shape == (55, 25) and f.dtype == f_exact.dtype == np.float64
    assert np.array_equal(f, gmeta_amd.sketch_profile_features(got.transpose(0, 2, 1)))             # symmetric: the orientation drops out
    raw = gmeta_amd.sketch_profile_features(got, symmetric=False)
    assert np.array_equal(raw.reshape(55, 5, 5)[swap], gmeta_amd.sketch_profile_features(want, symmetric=False).reshape(55, 5, 5)[swap].transpose(0, 2, 1))
