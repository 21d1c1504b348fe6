"""GPU (-m gpu): gm_sketch_pair_features and the Python layers above it (NodeSketches.pair_features, link_sketch_features, PairPredictor(..., sketches=),
train.py --buddy_columns) against the float64 restatement tests/sketch_feature_ref.py (the definition is in include/gmeta_hip.h) evaluated on the DEVICE'S OWN
pair_counts integers (test_hip_sketches.py holds those to the sketch restatement, bit for bit).  The bar is sketch_feature_ref's, derived there:
|dev - ref| <= 2^-23 |ref| + 2^-39 M per cell, none left out.  Which branch of the estimator an entry takes is asserted on the reference alone."""
import functools

import numpy as np
import pytest
import torch

import sketch_feature_ref as fref
from test_hip_pair_distance import _stream, case_a, case_c, case_w
from test_hip_sketches import SEED, built, random_graph

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = -7.25                                                                   # no column is negative


def raw_features(sk, pairs, symmetric=True, ld=None, stream=None, tail=64):
    """gm_sketch_pair_features through the C ABI itself -> float32 [n, S].  The spare columns S .. ld - 1 of every row and `tail` floats behind row n - 1 are
    poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
    n, S = len(p), (sk.H + 2) ** 2
    ld = S if ld is None else ld
    d_p = torch.from_numpy(p).cuda() if n else None
    out = torch.full((n * ld + tail,), POISON, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_sketch_pair_features(sk.h, _lib.ptr(d_p), n, 1 if symmetric else 0, _lib.ptr(out), ld, _stream(stream)), 'gm_sketch_pair_features')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n * ld:] == POISON).all()
    rows = out[:n * ld].reshape(n, ld)
    assert (rows[:, S:] == POISON).all()
    return rows[:, :S].copy()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def hold(got, counts, balls, pairs, N, p, K, symmetric, label):
    """got against the restatement on (counts, balls), per cell -> (the reference's unclipped tables, its branch record)"""
    want, M, P, met = fref.features_many(counts, balls, pairs, N, p, K, symmetric)
    assert fref.branch_margin(counts, balls, p) >= fref.BRANCH_MARGIN, label       # a condition on the inputs: both sides take the same branch
    assert got.dtype == f32 and got.shape == want.shape, label
    ok, worst = fref.within_bar(got, want, M)
    print('%s: %d pairs, worst |dev - ref| / bar %.3f' % (label, len(pairs), worst))
    assert ok, (label, worst)
    return P, met


def all_ordered(N):
    x, y = np.divmod(np.arange(N * N), N)
    return np.stack([x, y], 1)


# ---------------------------------------------------------------------------------------------------- every template instance, every record shape of the chunk walk
@pytest.mark.parametrize('H', [1, 2, 3, 4])
def test_every_ordered_pair_of_the_chain_at_every_hops(H):
    """(p 8, K 128): three chunks, registers and words in chunks of their own.  The chain case: u == v, isolated nodes (329, 330), pairs across components."""
    c = case_c()
    pairs = all_ordered(c.N)
    with built(c.store, 0, H, 8, 128) as sk:
        counts, balls = sk.counts(pairs)
        got = {s: raw_features(sk, pairs, s) for s in (True, False)}
    for s in (True, False):
        P, met = hold(got[s], counts, balls, pairs, c.N, 8, 128, s, 'chain H %d symmetric %d' % (H, s))
    assert met['linear'] and not met['zero']
    W = H + 2
    grid = got[True].reshape(c.N, c.N, W * W)
    assert np.array_equal(bits(grid), bits(grid.transpose(1, 0, 2)))                               # symmetric: (x, y) and (y, x) the same bits
    raw = got[False].reshape(c.N, c.N, W, W)
    assert np.array_equal(bits(raw), bits(raw.transpose(1, 0, 3, 2)))                              # oriented: exact transposes of each other
    assert any(not np.array_equal(t, t.T) for t in raw[0, 1:40])
    # the inputs hold: u == v, an isolated node, two components -- and what the definition makes of them
    assert not c.nb[329] and not c.nb[330] and 260 not in c.nb[329]
    iso = raw[329, 330]                                                                            # two isolated nodes: one node each at distance 0, the rest far from both
    assert abs(iso[0, W - 1] - np.log1p(1.0)) < 1e-2 and abs(iso[W - 1, 0] - np.log1p(1.0)) < 1e-2 and iso[0, 0] == 0.0
    assert abs(raw[329, 329][0, 0] - np.log1p(1.0)) < 1e-2                                         # u == v: the node itself at (0, 0)
    assert (raw[329, 5][:W - 1, :W - 1] == 0.0).all()                                              # different components: no node near both


@functools.lru_cache(maxsize=None)
def multigraph_pairs():
    """every ordered pair among 60 nodes of the multigraph (the two hubs, sinks and isolated nodes among them): 3,600 = 4 * 900 pairs, and three more"""
    c = case_a()
    nodes = np.concatenate([np.arange(0, 40), np.arange(270, 300, 2), [101, 150, 199, 250, 263]])
    assert len(nodes) == 60
    pairs = np.stack(np.meshgrid(nodes, nodes, indexing='ij'), -1).reshape(-1, 2)
    pairs = np.concatenate([pairs, [[7, 7], [299, 0], [0, 299]]])
    pairs.setflags(write=False)
    return pairs


@pytest.mark.parametrize('H,p,K', [(2, 4, 32), (1, 4, 32), (3, 10, 512), (4, 6, 96)])
def test_record_shapes_of_the_chunk_walk_and_both_estimator_branches(H, p, K):
    """(p 4, K 32): 36 dwords, registers and MinHash words share the one chunk; (p 10, K 512): 768 dwords, 12 chunks; (p 6, K 96): 112 dwords, no power of two.
    On the multigraph (a 400-entry row): at p 4 balls of hundreds of nodes saturate 16 registers, small ones leave most of them zero."""
    c = case_a()
    pairs = multigraph_pairs()
    assert len(pairs) % 4 == 3
    with built(c.store, 0, H, p, K) as sk:
        counts, balls = sk.counts(pairs)
        got = {s: raw_features(sk, pairs, s) for s in (True, False)}
    for s in (True, False):
        P, met = hold(got[s], counts, balls, pairs, c.N, p, K, s, 'multigraph (%d, %d, %d) symmetric %d' % (H, p, K, s))
    if p == 4:
        assert met['linear'] and met['raw'] and met['raw_no_zero_register']                        # a linear count, a raw estimate, a zeros == 0 entry
        assert (P < 0).any()                                                                       # a cell that is negative before the clip ...
        assert (got[False] >= 0).all() and (got[False][(P < 0).reshape(len(pairs), -1) & (pairs[:, :1] <= pairs[:, 1:])] == 0.0).all()      # ... and 0 after it
    if p == 10:
        assert met['linear']
    assert np.array_equal(bits(got[True][-2]), bits(got[True][-1]))                                # (299, 0) and (0, 299)


@pytest.mark.parametrize('H', [3, 4])
def test_random_graph_reaches_the_raw_estimate_at_p_8(H):
    """N = 2,000, mean degree 6: balls of three and four hops pass 2.5 m = 640 nodes, so the raw estimate is taken at p 8 too.  Duplicates: the 300 pairs twice."""
    store, N, pairs = random_graph()
    pairs = np.concatenate([pairs, pairs[::-1], [[11, 11]]])
    with built(store, 0, H, 8, 128) as sk:
        counts, balls = sk.counts(pairs)
        got = raw_features(sk, pairs)
        again = raw_features(sk, pairs, False)
    P, met = hold(got, counts, balls, pairs, N, 8, 128, True, 'random H %d' % H)
    hold(again, counts, balls, pairs, N, 8, 128, False, 'random H %d oriented' % H)
    assert met['linear'] and met['raw'] and (P < 0).any()
    assert np.array_equal(bits(got[:300]), bits(got[300:600][::-1]))                               # duplicates: each written on its own, the same bits


# ---------------------------------------------------------------------------------------------------- call behaviour
def test_rows_depend_on_their_own_pair_alone_and_nothing_else_is_written():
    store, N, nodes, sample, vec, hub_pairs, dist = case_w()                                       # the planted hubs: rows of 3,000 entries behind the records
    rng = np.random.default_rng(3)
    pairs = np.concatenate([hub_pairs[:40], rng.integers(0, N, (27, 2)), hub_pairs[:4]])           # 71 = 4 * 17 + 3
    assert len(pairs) % 4 == 3
    side = torch.cuda.Stream()
    with built(store, 0, 2, 8, 128) as sk:
        before = sk.counts(pairs)
        whole = raw_features(sk, pairs)
        hold(whole, before[0], before[1], pairs, N, 8, 128, True, 'hubs')
        for n in (1, 5):                                                                           # n = 1, 5, 4 k + 3: partial workgroups
            assert np.array_equal(bits(raw_features(sk, pairs[:n])), bits(whole[:n]))
        for i in (0, 33, 70):                                                                      # alone, and alone on a side stream
            assert np.array_equal(bits(raw_features(sk, pairs[i:i + 1])), bits(whole[i:i + 1]))
            assert np.array_equal(bits(raw_features(sk, pairs[i:i + 1], stream=side)), bits(whole[i:i + 1]))
        assert np.array_equal(bits(raw_features(sk, pairs[::-1], stream=side)), bits(whole[::-1]))  # another order, another stream
        assert np.array_equal(bits(raw_features(sk, pairs[:, ::-1])), bits(whole))                 # both orientations: bit-equal when symmetric
        assert np.array_equal(bits(whole[-4:]), bits(whole[:4]))                                   # duplicates
        fwd, back = raw_features(sk, pairs, False), raw_features(sk, pairs[:, ::-1], False)
        assert np.array_equal(bits(fwd.reshape(-1, 4, 4)), bits(back.reshape(-1, 4, 4).transpose(0, 2, 1)))
        for ld in (17, 24, 256):                                                                   # ld > S: the spare columns and what lies behind row n - 1 stay
            assert np.array_equal(bits(raw_features(sk, pairs, ld=ld)), bits(whole))
            assert np.array_equal(bits(raw_features(sk, pairs[:5], False, ld=ld, stream=side)), bits(fwd[:5]))
        # a node outside the graph, through the raw call: the chain's value on all-zero integers
        out = raw_features(sk, [[5, N], [-1, 3], [N, 5], [5, 6]], False)
        zero = fref.features(np.zeros((1, 3, 3, 3), np.int64), np.zeros((1, 2, 3, 2), np.int64), [[0, 1]], N, 8, 128, False)[0][0]
        assert not zero[:-1].any() and zero[-1] == np.log1p(float(N))                               # an empty table, every node in the corner
        assert fref.within_bar(out[:3], np.stack([zero] * 3), [float(N)] * 3)[0] and not out[:3, :-1].any()
        assert np.array_equal(bits(out[0]), bits(out[1])) and np.array_equal(bits(out[0]), bits(out[2]))
        assert np.array_equal(bits(out[3]), bits(raw_features(sk, [[5, 6]], False)[0])) and out[3, :-1].any()
        sym = raw_features(sk, [[5, N]])
        assert abs(float(sym[0, -1]) - np.log1p(2.0 * N)) <= 2.0 ** -23 * np.log1p(2.0 * N) + 2.0 ** -39 * N and not sym[0, :-1].any()
        after = sk.counts(pairs)                                                                   # pair_counts on the same sketch: the same bits before and after
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_bad_arguments_and_n_zero():
    from gmeta_amd import _lib
    lib = _lib.lib()
    c = case_c()
    st = _lib.stream_ptr()

    def fails(rc, text):
        assert rc == -1, rc
        msg = lib.gm_last_error().decode()
        assert text in msg and 'gm_sketch_pair_features' in msg, msg

    with built(c.store, 0, 3, 8, 128) as sk:
        d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')
        o = torch.full((4 * 25 + 8,), POISON, dtype=torch.float32, device='cuda')
        P, O = _lib.ptr(d_p), _lib.ptr(o)
        fails(lib.gm_sketch_pair_features(None, P, 4, 1, O, 25, st), 'sketch is NULL')
        fails(lib.gm_sketch_pair_features(sk.h, P, 4, 1, O, 24, st), 'ld = 24')
        fails(lib.gm_sketch_pair_features(sk.h, P, 4, 1, O, 16, st), 'ld = 16')
        fails(lib.gm_sketch_pair_features(sk.h, P, 4, 1, O, -1, st), 'ld = -1')
        fails(lib.gm_sketch_pair_features(sk.h, P, -1, 1, O, 25, st), 'n = -1')
        fails(lib.gm_sketch_pair_features(sk.h, P, 2 ** 31, 1, O, 25, st), 'n = 2147483648')
        fails(lib.gm_sketch_pair_features(sk.h, None, 4, 1, O, 25, st), 'NULL argument')
        fails(lib.gm_sketch_pair_features(sk.h, P, 4, 1, None, 25, st), 'NULL argument')
        assert lib.gm_sketch_pair_features(sk.h, None, 0, 1, None, 25, st) == 0                     # n == 0: a no-op, with NULL pointers too
        assert lib.gm_sketch_pair_features(sk.h, None, 0, 0, None, 4096, st) == 0
        torch.cuda.synchronize()
        assert (o == POISON).all()                                                                 # nothing was written by a refused call
        assert lib.gm_sketch_pair_features(sk.h, P, 4, 1, O, 25, st) == 0                           # after the errors: a good call is unaffected
        torch.cuda.synchronize()
        got = o.cpu().numpy()
        assert (got[100:] == POISON).all() and np.array_equal(bits(got[:100].reshape(4, 25)), bits(raw_features(sk, np.zeros((4, 2), np.int64))))


# ---------------------------------------------------------------------------------------------------- the Python layers
def test_node_sketches_pair_features_equals_the_raw_call():
    c = case_c()
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, c.N, (37, 2))
    with built(c.store, 0, 2, 8, 128) as raw:
        want = {s: raw_features(raw, pairs, s) for s in (True, False)}
    sk = c.store.sketches(0)
    assert sk.n_columns == 16 and (sk.hops, sk.p, sk.k, sk.seed) == (2, 8, 128, SEED)
    for s in (True, False):
        got = sk.pair_features(pairs, symmetric=s)
        assert isinstance(got, np.ndarray) and got.dtype == f32 and got.shape == (37, 16) and np.array_equal(bits(got), bits(want[s]))
    t = sk.pair_features(pairs, as_torch=True)
    assert t.is_cuda and t.dtype == torch.float32 and np.array_equal(bits(t.cpu().numpy()), bits(want[True]))
    wide = torch.full((37, 21), POISON, dtype=torch.float32, device='cuda')
    back = sk.pair_features(pairs, symmetric=False, as_torch=True, out=wide)
    assert back is wide and np.array_equal(bits(wide[:, :16].cpu().numpy()), bits(want[False])) and (wide[:, 16:] == POISON).all()
    assert np.array_equal(bits(sk.pair_features(pairs, out=wide)), bits(want[True]))               # numpy: the filled columns alone
    assert sk.pair_features(np.zeros((0, 2), np.int64)).shape == (0, 16)
    with pytest.raises(ValueError, match=r'out of shape \(37, 15\); \[37, at least 16\]'):
        sk.pair_features(pairs, out=torch.zeros((37, 15), device='cuda'))
    with pytest.raises(ValueError, match='contiguous rows'):
        sk.pair_features(pairs, out=torch.zeros((37, 40), device='cuda')[:, ::2])
    with pytest.raises(ValueError, match='CUDA float32'):
        sk.pair_features(pairs, out=torch.zeros((37, 16), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match=r'outside the graph \(331 nodes\)'):
        sk.pair_features([[0, c.N]])
    sk.close()
    with pytest.raises(ValueError, match='closed'):
        sk.pair_features(pairs)


@functools.lru_cache(maxsize=None)
def two_graphs():
    """a store of two graphs with features: the chain and a random graph of 150 nodes; 90 names over both, both orientations, and 0 / 1 labels"""
    import gmeta_amd
    c = case_c()
    rng = np.random.default_rng(12)
    N2, F = 150, 16
    src, dst = rng.integers(0, N2, 400).astype(np.int64), rng.integers(0, N2, 400).astype(np.int64)
    feats = [rng.standard_normal((c.N, F)).astype(f32), rng.standard_normal((N2, F)).astype(f32)]
    store = gmeta_amd.GraphStore([(c.N, c.src, c.dst), (N2, src, dst)], feats)
    names = []
    for _ in range(90):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, (c.N, N2)[g], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b))
    return store, F, names, (rng.random(90) < 0.5).astype(np.float64)


def test_link_sketch_features_is_the_host_twin_in_name_order():
    import gmeta_amd
    store, F, names, labels = two_graphs()
    trip = np.array([[int(x) for x in nm.split('_')] for nm in names])
    assert set(trip[:, 0]) == {0, 1} and (trip[:, 1] > trip[:, 2]).any() and (trip[:, 1] < trip[:, 2]).any()
    sks = [store.sketches(g, hops=2) for g in (0, 1)]
    try:
        for s in (True, False):
            got = gmeta_amd.link_sketch_features(sks, names, symmetric=s)
            twin = gmeta_amd.sketch_profile_features(gmeta_amd.link_sketch_profiles(sks, names), symmetric=s)
            assert got.dtype == f32 and got.shape == twin.shape == (90, 16)
            M = np.zeros(90)
            for g in (0, 1):
                at = np.nonzero(trip[:, 0] == g)[0]
                counts, balls = sks[g].pair_counts(trip[at, 1:])
                want, M[at], _, _ = fref.features_many(counts, balls, trip[at, 1:], store.n_nodes[g], 8, 128, s)
                assert fref.branch_margin(counts, balls, 8) >= fref.BRANCH_MARGIN
                assert fref.within_bar(got[at], want, M[at])[0]
            ok, worst = fref.within_bar(got, twin, M)                                              # the host chain: the same bar (it is within 1e-12 of the restatement)
            print('link_sketch_features symmetric %d: worst |dev - host twin| / bar %.3f' % (s, worst))
            assert ok
            assert np.array_equal(bits(gmeta_amd.link_sketch_features({0: sks[0], 1: sks[1]}, names, symmetric=s)), bits(got))
        assert gmeta_amd.link_sketch_features(sks, []).shape == (0, 4)
    finally:
        for o in sks:
            o.close()


def test_predictor_with_sketches_equals_the_predictor_fed_their_columns():
    import gmeta_amd
    store, F, names, labels = two_graphs()
    rng = np.random.default_rng(2)
    pairs = rng.integers(0, store.n_nodes[0], (133, 2))
    y = (rng.random(133) < 0.5).astype(f32)
    user = rng.standard_normal((133, 3)).astype(f32)
    with store.propagated_features(0, hops=2) as props, store.sketches(0, hops=2) as sk, store.sketches(1, hops=2) as other, store.sketches(0, hops=3) as deep:
        cols = sk.pair_features(pairs, as_torch=True)
        for extra_dim, tail in ((16, None), (19, user)):
            model = gmeta_amd.PairPredictor(F, 2, hidden=16, extra_dim=extra_dim, seed=4)
            fed = cols if tail is None else torch.cat([cols, torch.from_numpy(tail).cuda()], 1)
            want = model.scores(props, pairs, extra=fed)
            got = model.scores(props, pairs, extra=tail, sketches=sk)
            assert np.array_equal(bits(got), bits(want)) and np.isfinite(got).all()
            if tail is not None:                                                                   # extra as a CUDA tensor behind the sketch columns
                assert np.array_equal(bits(model.scores(props, pairs, extra=torch.from_numpy(tail).cuda(), sketches=sk)), bits(want))
            loss_want = model.step(props, pairs, y, extra=fed)
            grad_want = model.params.grad.cpu().numpy().copy()
            loss_got = model.step(props, pairs, y, extra=tail, sketches=sk)
            assert np.float64(loss_got).view(np.uint64) == np.float64(loss_want).view(np.uint64)
            assert np.array_equal(bits(model.params.grad.cpu().numpy()), bits(grad_want)) and np.abs(grad_want).max() > 0
            assert model.scores(props, np.zeros((0, 2), np.int64), extra=None if tail is None else tail[:0], sketches=sk).shape == (0,)
        # mismatches name their numbers
        model = gmeta_amd.PairPredictor(F, 2, hidden=16, extra_dim=19)
        with pytest.raises(ValueError, match=r'sketches give 16 columns and extra none; the predictor has extra_dim = 19'):
            model.scores(props, pairs, sketches=sk)
        with pytest.raises(ValueError, match=r'sketches give 16 columns and extra shape \(133, 4\); the predictor has extra_dim = 19'):
            model.scores(props, pairs, extra=np.zeros((133, 4), f32), sketches=sk)
        with pytest.raises(ValueError, match=r'sketches give 25 columns and extra none; the predictor has extra_dim = 19'):
            model.step(props, pairs, y, sketches=deep)
        with pytest.raises(ValueError, match=r'extra of shape \(5, 3\); \[133, 3\]'):
            model.scores(props, pairs, extra=np.zeros((5, 3), f32), sketches=sk)
        with pytest.raises(ValueError, match=r'sketches of a graph with 150 nodes; the propagated features have 331'):
            model.scores(props, pairs, extra=user, sketches=other)
        closed = store.sketches(0, hops=2)
        closed.close()
        with pytest.raises(ValueError, match='the sketches are closed'):
            model.scores(props, pairs, extra=user, sketches=closed)
        assert model.params.grad is None


def test_fit_with_sketches_gives_the_loss_curve_of_fit_on_their_columns():
    import gmeta_amd
    store, F, names, labels = two_graphs()
    props = [store.propagated_features(g, hops=2) for g in (0, 1)]
    sks = {g: store.sketches(g, hops=2) for g in (0, 1)}
    try:
        cols = gmeta_amd.link_sketch_features(sks, names)
        curves, aucs = [], []
        for kw in (dict(extra=cols), dict(sketches=sks)):
            model = gmeta_amd.PairPredictor(F, 2, hidden=16, extra_dim=16, seed=7)
            curves.append(model.fit(props, names, labels, epochs=3, batch=32, lr=0.01, **kw))
            aucs.append(model.auc(props, names, labels, **kw))
            scores = model.link_scores(props, names, **kw)
            assert scores.shape == (90,) and np.isfinite(scores).all()
        assert len(curves[0]) == 3 and np.array_equal(np.asarray(curves[0]).view(np.uint64), np.asarray(curves[1]).view(np.uint64))
        assert aucs[0] == aucs[1] and 0.0 <= aucs[0] <= 1.0
    finally:
        for o in props + list(sks.values()):
            o.close()


# ---------------------------------------------------------------------------------------------------- the driver
def test_train_driver_forms_the_buddy_columns_on_the_device(tmp_path, capsys):
    from gmeta_amd import datadir, synth
    from test_hip_pair_scores import DRIVER, _positives_only, _splits
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)                           # the tiny link data set of test_hip_pair_mlp.py
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric']
    dev = drv.main(drv.parse(base + ['--buddy', '3', '--buddy_columns', 'device']))
    text = capsys.readouterr().out
    assert 0.0 <= dev['buddy_auc'] <= 1.0 and 'BUDDY test AUC: %.4f' % dev['buddy_auc'] in text
    host = drv.main(drv.parse(base + ['--buddy', '3', '--buddy_columns', 'host']))
    plain = drv.main(drv.parse(base + ['--buddy', '3']))
    capsys.readouterr()
    assert host == plain and 0.0 <= host['buddy_auc'] <= 1.0                                       # 'host' is the default: the same result dict
    assert {k: v for k, v in dev.items() if k != 'buddy_auc'} == {k: v for k, v in plain.items() if k != 'buddy_auc'}
