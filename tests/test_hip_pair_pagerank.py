"""GPU (-m gpu): gm_store_rooted_pagerank, gm_store_pair_pagerank and the Python layers above them against the float64 restatement of the definition
(tests/pagerank_ref.py; the definition itself is in include/gmeta_hip.h).

Tolerance, derived and not measured (pagerank_ref.bound): every quantity of the iteration is non-negative, so rounding errors do not cancel and relative
errors do not grow beyond their count.  Per iteration an entry passes through at most d_max + 8 roundings of 2^-24 each -- the rounded 1 / deg, the scale,
d_max - 1 adds in any order, a, b, the product, the final add, slack -- hence |got - want| <= 1.01 iters (d_max + 8) 2^-24 want + 2^-100; the absolute term
covers underflow.  A wrong neighbour, degree or mask moves entries by percents.  The exactness clause is checked on bit patterns."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import negative_ref
import pagerank_ref as ref
import pair_score_ref
import path_walk_ref
from test_hip_pair_scores import DRIVER, _positives_only, _splits, _store

pytestmark = pytest.mark.gpu
ALPHA, ITERS = 0.15, 20
POISON = -7.0
CHUNKS = (0, 1, 7, 2 ** 30)                   # 0: the library's choice; 1: every row of two or more entries is cut; 2^30: none is
COLS = (0, 64, 128)


class tuning:
    def __init__(self, **knobs):
        from gmeta_amd import _lib
        self.lib, self.knobs = _lib.lib(), {k.encode(): v for k, v in knobs.items()}

    def __enter__(self):
        self.was = {k: self.lib.gm_get_tuning(k) for k in self.knobs}
        for k, v in self.knobs.items():
            assert self.lib.gm_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        for k, v in self.was.items():
            self.lib.gm_set_tuning(k, v)
        return False


def _stream(stream):
    from gmeta_amd import _lib
    return _lib.stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)


def _raw_vec(store, g, sources, alpha=ALPHA, iters=ITERS, stream=None):
    """The C ABI itself: float32 [m, N].  The row behind m is poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    a = np.ascontiguousarray(np.asarray(sources, np.int64).reshape(-1), np.int32)
    m, N = len(a), store.n_nodes[g]
    d_a = torch.from_numpy(a).cuda() if m else None
    out = torch.full((m + 1, N), POISON, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_store_rooted_pagerank(store.handle, g, _lib.ptr(d_a), m, alpha, iters, _lib.ptr(out), _stream(stream)), 'gm_store_rooted_pagerank')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.dtype == np.float32 and (out[m:] == POISON).all()
    return out[:m]


def _raw(store, g, pairs, flags=0, alpha=ALPHA, iters=ITERS, stream=None):
    """The C ABI itself: float32 [n, 2], the row behind n poisoned."""
    from gmeta_amd import _lib
    p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
    n = len(p)
    d_p = torch.from_numpy(p).cuda() if n else None
    out = torch.full((n + 1, 2), POISON, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_store_pair_pagerank(store.handle, g, _lib.ptr(d_p), n, flags, alpha, iters, _lib.ptr(out), _stream(stream)), 'gm_store_pair_pagerank')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.dtype == np.float32 and (out[n:] == POISON).all()
    return out[:n]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def within(got, want, iters, d_max):
    err, lim = np.abs(got.astype(np.float64) - want), ref.bound(want, iters, d_max)
    worst = float((err / lim).max()) if err.size else 0.0
    print('iters %d d_max %d: largest error / bound %.3g, largest relative error %.3g' % (iters, d_max, worst, float((err / np.maximum(want, 1e-300)).max()) if err.size else 0.0))
    return bool((err <= lim).all())


# ---------------------------------------------------------------------------------------------------- shared references, computed once
@functools.lru_cache(maxsize=None)
def case_a():
    N, src, dst = negative_ref.multigraph_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    return N, src, dst, nb, max(len(r) for r in nb)


@functools.lru_cache(maxsize=None)
def vectors_a(iters):
    N, src, dst, nb, _ = case_a()
    w = ref.rooted_pagerank(N, src, dst, np.arange(N), ALPHA, iters, nb)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def all_pairs_a():
    N = case_a()[0]
    return np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing='ij'), -1).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def want_a(flags):
    N, src, dst, nb, _ = case_a()
    w = ref.pair_pagerank(N, src, dst, all_pairs_a(), flags, ALPHA, ITERS, nb)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def store_a():
    return _store([case_a()[:3]])


@functools.lru_cache(maxsize=None)
def case_w():
    N, src, dst, nodes = path_walk_ref.walk_case()
    pairs = np.array([(a, b) for a in nodes for b in nodes], np.int64)
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    want = {f: ref.pair_pagerank(N, src, dst, pairs, f, ALPHA, ITERS, nb) for f in (0, 1)}
    for w in want.values():
        w.setflags(write=False)
    return _store([(N, src, dst)]), pairs, want, nodes, max(len(r) for r in nb)


# ---------------------------------------------------------------------------------------------------- the vector call
@pytest.mark.parametrize('iters', [1, 2, 20])
def test_multigraph_every_source_vector(iters):
    N, _, _, nb, d_max = case_a()
    want = vectors_a(iters)
    assert d_max > 200 and (want[:290] == 0).any() and (want > 0).sum() > 2000
    for chunk in CHUNKS:
        for cols in COLS:
            with tuning(ppr_chunk=chunk, ppr_cols=cols):
                got = _raw_vec(store_a(), 0, np.arange(N), ALPHA, iters)
            assert within(got, want, iters, d_max), (chunk, cols)
            assert np.array_equal(got == 0, want == 0), (chunk, cols)                      # zero entries: exactly those of the restatement
            lim = ref.bound(want, iters, d_max).sum(1)
            assert (np.abs(got.astype(np.float64).sum(1) - 1.0) <= lim).all(), (chunk, cols)      # the mass, within the row's summed bounds
            assert np.array_equal(got[290:], np.eye(N, dtype=np.float32)[290:])            # an isolated source: exactly e_s (a + b rounds to 1.0f)


def test_duplicate_unordered_and_outside_sources():
    N, _, _, _, d_max = case_a()
    rng = np.random.default_rng(9)
    sources = np.concatenate([rng.integers(0, N, 150), [0, 0, 1, 299, 299], rng.integers(0, N, 40)])
    with tuning(ppr_chunk=7):
        whole = _raw_vec(store_a(), 0, np.arange(N))
        got = _raw_vec(store_a(), 0, sources)
        odd = _raw_vec(store_a(), 0, [5, N, -1, 5, 2 ** 31 - 1])
        none = _raw_vec(store_a(), 0, [N, -3])
    assert np.array_equal(bits(got), bits(whole[sources]))                                 # every row on its own, whatever the list
    assert not odd[[1, 2, 4]].any() and np.array_equal(bits(odd[0]), bits(whole[5])) and np.array_equal(bits(odd[3]), bits(whole[5]))
    assert none.shape == (2, N) and not none.any()
    assert _raw_vec(store_a(), 0, []).shape == (0, N)


# ---------------------------------------------------------------------------------------------------- the pair call
def test_multigraph_every_ordered_pair():
    N, _, _, nb, d_max = case_a()
    with tuning(ppr_chunk=7):
        plain, masked = _raw(store_a(), 0, all_pairs_a(), 0), _raw(store_a(), 0, all_pairs_a(), 1)
        whole = _raw_vec(store_a(), 0, np.arange(N))
    for flags, got in ((0, plain), (1, masked)):
        assert within(got, want_a(flags), ITERS, d_max), flags
        sq = bits(got).reshape(N, N, 2)
        assert np.array_equal(sq, sq.transpose(1, 0, 2))                                   # (a, b) against (b, a)
    u, v = all_pairs_a().min(1), all_pairs_a().max(1)
    assert np.array_equal(bits(plain[:, 0]), bits(whole[u, v])) and np.array_equal(bits(plain[:, 1]), bits(whole[v, u]))      # the entries of the vector call
    adj = np.array([b in nb[a] for a, b in all_pairs_a().tolist()])
    differs = (bits(plain) != bits(masked)).any(1)
    assert (differs & adj).sum() > 1000 and not differs[~adj].any()                        # a non-adjacent pair: the bits of the unflagged call
    with tuning(ppr_chunk=0):
        assert within(_raw(store_a(), 0, all_pairs_a()[::3], 1), want_a(1)[::3], ITERS, d_max)


@pytest.mark.parametrize('chunk', [0, 5])
def test_exactness_clause(chunk):
    """For one ppr_chunk: a row depends on its own pair, the flags, alpha and iters alone."""
    N = case_a()[0]
    rng = np.random.default_rng(12)
    pairs = np.concatenate([rng.integers(0, N, (700, 2)), np.stack([rng.integers(0, 2, 60), rng.integers(0, N, 60)], 1)])
    for flags in (0, 1):
        with tuning(ppr_chunk=chunk):
            base = _raw(store_a(), 0, pairs, flags)
            perm = rng.permutation(len(pairs))
            assert np.array_equal(bits(_raw(store_a(), 0, pairs[perm], flags)), bits(base[perm]))          # shuffled
            dup = rng.integers(0, len(pairs), 2000)
            assert np.array_equal(bits(_raw(store_a(), 0, pairs[dup], flags)), bits(base[dup]))            # with duplicates
            cut = np.concatenate([_raw(store_a(), 0, part, flags) for part in (pairs[:100], pairs[100:101], pairs[101:])])
            assert np.array_equal(bits(cut), bits(base))                                                   # three calls
            for cols in (64, 128, 0):
                with tuning(ppr_cols=cols):
                    assert np.array_equal(bits(_raw(store_a(), 0, pairs, flags)), bits(base)), cols        # columns per round
            assert np.array_equal(bits(_raw(store_a(), 0, pairs, flags, stream=torch.cuda.Stream())), bits(base))      # a second stream
            assert np.array_equal(bits(_raw(store_a(), 0, pairs, flags)), bits(base))                      # two runs
    with tuning(ppr_chunk=chunk):
        other = _raw(store_a(), 0, pairs, 0, 0.5, 3)
    assert not np.array_equal(bits(other), bits(base)) and within(other, ref.pair_pagerank(*case_a()[:3], pairs, 0, 0.5, 3, case_a()[3]), 3, case_a()[4])


@pytest.mark.parametrize('chunk', [0, 63, 64, 65, 2 ** 30])
def test_planted_hubs_and_boundary_rows(chunk):
    """The cut at 63, 64 and 65 lands below, on and above the planted row lengths; the 3,000-entry rows take many segments."""
    store, pairs, want, nodes, d_max = case_w()
    assert d_max == path_walk_ref.HUB_ROW
    with tuning(ppr_chunk=chunk):
        got = {flags: _raw(store, 0, pairs, flags) for flags in (0, 1)}
    for flags in (0, 1):
        assert within(got[flags], want[flags], ITERS, d_max), (chunk, flags)
    assert pairs[1].tolist() == [0, 1] and (want[1][1] > 0).all() and (want[1][1] != want[0][1]).all()      # the masked hub pair: other walks remain
    leaf, stem = nodes[3], nodes[-11]                                          # the 1-entry endpoint and the 300-row middle node it hangs off
    k = nodes.index(leaf) * len(nodes) + nodes.index(stem)
    assert pairs[k].tolist() == [leaf, stem] and (want[0][k] > 0).all() and not want[1][k].any()
    assert not got[1][k].any() and (got[0][k] > 0).all()                       # the leaf whose only edge is masked: (0, 0)


# ---------------------------------------------------------------------------------------------------- stores, streams, arguments
def test_third_graph_of_a_store_and_a_weighted_store():
    rng = np.random.default_rng(2)
    g0 = (50, rng.integers(0, 50, 333).astype(np.int64), rng.integers(0, 50, 333).astype(np.int64))
    g1 = (7, np.array([0, 1, 5], np.int64), np.array([1, 2, 5], np.int64))
    N, src, dst, nb, d_max = case_a()
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(src))).astype(np.float32)
    weights = [np.ones(len(g0[1]), np.float32), np.ones(3, np.float32), w]
    pairs = np.concatenate([rng.integers(0, N, (600, 2)), np.stack([rng.integers(0, 2, 100), rng.integers(0, N, 100)], 1)])
    every1 = np.array([(a, b) for a in range(7) for b in range(7)])
    at = pairs[:, 0] * N + pairs[:, 1]
    with tuning(ppr_chunk=5):
        alone = {flags: _raw(store_a(), 0, pairs, flags) for flags in (0, 1)}
        for wts in (None, weights):
            store = _store([g0, g1, (N, src, dst)], weights=wts)
            assert store.weighted == (wts is not None)
            for flags in (0, 1):
                got = _raw(store, 2, pairs, flags)
                assert np.array_equal(bits(got), bits(alone[flags])) and within(got, want_a(flags)[at], ITERS, d_max)      # offsets and weights change nothing
            assert within(_raw(store, 1, every1, 1), ref.pair_pagerank(*g1, every1, 1), ITERS, int(pair_score_ref.degrees(*g1).max()))
            assert within(_raw_vec(store, 0, np.arange(50)), ref.rooted_pagerank(*g0, np.arange(50)), ITERS, int(pair_score_ref.degrees(*g0).max()))


def test_two_streams_on_a_fresh_store():
    """The index is built by the first call (here on s1); the second stream reads it with no event between them."""
    N, src, dst, _, d_max = case_a()
    store = _store([(N, src, dst)])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pairs = all_pairs_a()[::7]
    with tuning(ppr_chunk=3):
        a = _raw(store, 0, pairs, stream=s1)
        b = _raw(store, 0, pairs, stream=s2)
        c = _raw(store, 0, pairs)
        with torch.cuda.stream(s2):
            d = store.pair_pagerank(0, pairs)
    assert within(a, want_a(0)[::7], ITERS, d_max)
    for x in (b, c, d):
        assert np.array_equal(bits(x), bits(a))


def test_bad_arguments_and_n_zero():
    from gmeta_amd import _lib
    store, lib = store_a(), _lib.lib()
    N = case_a()[0]
    got = _raw(store, 0, [(0, N), (-1, 5), (N, N), (2 ** 31 - 1, 0), (0, 1)])
    assert not got[:4].any() and (got[4] > 0).all()
    assert _raw(store, 0, np.zeros((0, 2))).shape == (0, 2)                   # n == 0: the poisoned row stays
    null, st = C.c_void_p(0), _lib.stream_ptr()
    assert lib.gm_store_pair_pagerank(store.handle, 0, null, 0, 0, ALPHA, ITERS, null, st) == 0      # n == 0 with NULL pointers
    assert lib.gm_store_rooted_pagerank(store.handle, 0, null, 0, ALPHA, ITERS, null, st) == 0
    out = torch.zeros((4, N), dtype=torch.float32, device='cuda')
    d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')

    def pair(g=0, n=4, flags=0, alpha=ALPHA, iters=ITERS, p=_lib.ptr(d_p), o=_lib.ptr(out), s=store.handle):
        return lib.gm_store_pair_pagerank(s, g, p, n, flags, alpha, iters, o, st)

    def vec(g=0, n=4, flags=0, alpha=ALPHA, iters=ITERS, p=_lib.ptr(d_p), o=_lib.ptr(out), s=store.handle):
        return lib.gm_store_rooted_pagerank(s, g, p, n, alpha, iters, o, st)
    for call, name in ((pair, 'gm_store_pair_pagerank'), (vec, 'gm_store_rooted_pagerank')):
        cnt = 'n' if call is pair else 'm'
        bad = [(dict(g=1), 'graph 1'), (dict(g=-1), 'graph -1'), (dict(n=-1), '%s = -1' % cnt), (dict(n=2 ** 31), '%s = 2147483648' % cnt),
               (dict(alpha=0.0), 'alpha = 0'), (dict(alpha=1.0), 'alpha = 1'), (dict(alpha=float('nan')), 'alpha = nan'), (dict(alpha=-0.5), 'alpha = -0.5'),
               (dict(iters=0), 'iters = 0'), (dict(iters=256), 'iters = 256'), (dict(p=null), 'NULL argument'), (dict(o=null), 'NULL argument'),
               (dict(s=null), 'store is NULL')]
        if call is pair:
            bad += [(dict(flags=2), 'flag bits 0x2'), (dict(flags=5), 'flag bits 0x5')]
        for kw, word in bad:
            with pytest.raises(ValueError, match=word):
                _lib.check(call(**kw), name)
        for knob, value, word in (('ppr_cols', 48, 'ppr_cols = 48'), ('ppr_cols', -64, 'ppr_cols = -64'), ('ppr_cols', 8192, 'ppr_cols = 8192'), ('ppr_chunk', -1, 'ppr_chunk = -1')):
            with tuning(**{knob: value}):
                with pytest.raises(ValueError, match=word):
                    _lib.check(call(), name)
        assert call(n=0) == 0 and call() == 0 and call(iters=1) == 0 and call(iters=255) == 0
    assert pair(flags=1) == 0
    assert store.pair_pagerank(0, np.zeros((0, 2))).shape == (0, 2) and store.pair_pagerank(0, []).dtype == np.float32
    assert store.rooted_pagerank(0, []).shape == (0, N)
    with pytest.raises(ValueError, match='graph'):
        store.pair_pagerank(1, [[0, 1]])
    with pytest.raises(ValueError, match='outside'):
        store.pair_pagerank(0, [[0, N]])
    torch.cuda.synchronize()


def test_graphstore_methods_equal_the_raw_calls():
    store, pairs, want, nodes, d_max = case_w()
    for mask in (False, True):
        got = store.pair_pagerank(0, pairs, mask_target=mask)
        assert got.dtype == np.float32 and got.shape == (len(pairs), 2)
        assert np.array_equal(bits(got), bits(_raw(store, 0, pairs, 1 if mask else 0)))
    vec = store.rooted_pagerank(0, nodes[:5])
    assert vec.dtype == np.float32 and np.array_equal(bits(vec), bits(_raw_vec(store, 0, nodes[:5])))
    other = store_a().pair_pagerank(0, all_pairs_a()[:3000], mask_target=True, alpha=0.3, iters=5)
    assert np.array_equal(bits(other), bits(_raw(store_a(), 0, all_pairs_a()[:3000], 1, 0.3, 5)))
    assert np.array_equal(bits(store_a().rooted_pagerank(0, [3, 3], alpha=0.3, iters=5)), bits(_raw_vec(store_a(), 0, [3, 3], 0.3, 5)))


# ---------------------------------------------------------------------------------------------------- AUC over completed tables, driver
@pytest.mark.parametrize('mask', [False, True])
def test_link_pagerank_auc_equals_the_auc_of_the_restated_scores(mask):
    import gmeta_amd
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, pos, info1)
    names, labels = tables['train']
    got = gmeta_amd.link_pagerank_auc(store, names, labels, mask_target=mask)
    assert tuple(got) == gmeta_amd.PAGERANK_SCORES
    want = np.zeros((len(names), 2), np.float64)
    for k, nm in enumerate(names):
        g, a, b = (int(x) for x in nm.split('_'))
        want[k] = ref.pair_pagerank(*d['graphs'][g], [(a, b)], 1 if mask else 0)[0]
    y = np.asarray(labels).astype(np.int64)
    assert y.sum() * 2 == len(y) > 100
    cols = gmeta_amd.link_pagerank_scores(store, names, mask_target=mask)
    assert cols.dtype == np.float32 and within(cols, want, ITERS, max(int(pair_score_ref.degrees(*g).max()) for g in d['graphs']))
    assert got['rooted_pagerank'] == gmeta_amd.link_auc(gmeta_amd.rooted_pagerank_index(cols), labels)
    assert got['rooted_pagerank'] == pytest.approx(gmeta_amd.link_auc(want.sum(1), labels), abs=1e-3)
    print('mask %s: AUC rooted_pagerank %.6f' % (mask, got['rooted_pagerank']))


def test_train_driver_reports_the_pagerank_auc(tmp_path, capsys):
    import gmeta_amd
    from gmeta_amd import datadir, synth
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric']
    res = drv.main(drv.parse(base + ['--pagerank', '1']))
    text = capsys.readouterr().out
    auc = res['pagerank_auc']
    assert tuple(auc) == gmeta_amd.PAGERANK_SCORES and np.isfinite(auc['rooted_pagerank']) and 0.0 <= auc['rooted_pagerank'] <= 1.0, auc
    assert 'PageRank test AUC: rooted_pagerank %.4f' % auc['rooted_pagerank'] in text and 'Heuristic test AUC' not in text and 'heuristic_auc' not in res
    # over the completed test table, with the mask: the same call by hand
    from gmeta_amd.negatives import read_link_tables
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root + '/'), info1, mode='uniform')
    assert auc == gmeta_amd.link_pagerank_auc(store, *tables['test'], mask_target=True)
    both = drv.main(drv.parse(base + ['--pagerank', '1', '--heuristics', '2']))
    text = capsys.readouterr().out
    assert text.index('Heuristic test AUC:') < text.index('Path test AUC:') < text.index('PageRank test AUC:')
    assert both['pagerank_auc'] == auc and {k: v for k, v in both.items() if k not in ('heuristic_auc', 'path_auc')} == res
    plain = drv.main(drv.parse(base + ['--heuristics', '2']))
    text = capsys.readouterr().out
    assert 'PageRank test AUC' not in text and 'pagerank_auc' not in plain
    assert plain == {k: v for k, v in both.items() if k != 'pagerank_auc'}      # the flag changes nothing else
