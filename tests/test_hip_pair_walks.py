"""GPU (-m gpu): gm_store_pair_walks and the Python layers above it against the restatement of the definition (tests/path_walk_ref.py; the definition itself
is in include/gmeta_hip.h), under every forced lanes-per-item value, the library's own choice, and work-item sizes that make every pair heavy, none, and
that put the cut at, one below and one above a row length.  Integer work: every comparison is np.array_equal on int64."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import negative_ref
import pair_score_ref
import path_walk_ref as ref
from test_hip_pair_scores import DRIVER, _positives_only, _splits, _store

pytestmark = pytest.mark.gpu
LANES = (0, 32, 64)                          # 0: the library's choice; the others: every width that is built
POISON = -7


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


def _raw(store, g, pairs, flags=0, stream=None):
    """The C ABI itself: int64 [n, 3].  The row behind n is poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
    n = len(p)
    d_p = torch.from_numpy(p).cuda() if n else None
    out = torch.full((n + 1, 3), POISON, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    st = _lib.stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_lib.lib().gm_store_pair_walks(store.handle, g, _lib.ptr(d_p), n, flags, _lib.ptr(out), st), 'gm_store_pair_walks')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.dtype == np.int64 and (out[n:] == POISON).all()
    return out[:n]


# ---------------------------------------------------------------------------------------------------- shared references, computed once
@functools.lru_cache(maxsize=None)
def case_a():
    N, src, dst = negative_ref.multigraph_case()
    return N, src, dst, pair_score_ref.neighbourhoods(N, src, dst)


@functools.lru_cache(maxsize=None)
def all_pairs_a():
    N = case_a()[0]
    return np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing='ij'), -1).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def want_a(flags):
    N, src, dst, nb = case_a()
    w = ref.pair_walks(N, src, dst, all_pairs_a(), flags, nb)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def store_a():
    return _store([case_a()[:3]])


@functools.lru_cache(maxsize=None)
def case_w():
    N, src, dst, nodes = ref.walk_case()
    pairs = np.array([(a, b) for a in nodes for b in nodes], np.int64)
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    want = {f: ref.pair_walks(N, src, dst, pairs, f, nb) for f in (0, 1)}
    for w in want.values():
        w.setflags(write=False)
    return _store([(N, src, dst)]), pairs, want, nodes


# ---------------------------------------------------------------------------------------------------- the cases, under every instantiation and cut
@pytest.mark.parametrize('lanes', LANES)
def test_multigraph_every_ordered_pair(lanes):
    """walk_chunk 1: every pair with a non-empty outer row of two or more entries is heavy (seed, items, atomics); 2^30: none is; 7 and the library's: a mix."""
    N = case_a()[0]
    for chunk in (0, 1, 7, 2 ** 30):
        with tuning(walk_lanes=lanes, walk_chunk=chunk):
            for flags in (0, 1):
                got = _raw(store_a(), 0, all_pairs_a(), flags)
                assert np.array_equal(got, want_a(flags)), (lanes, chunk, flags)
    sq = got.reshape(N, N, 3)
    assert np.array_equal(sq, sq.transpose(1, 0, 2))                          # (a, b) against (b, a)
    assert (want_a(0)[:, 0] != want_a(1)[:, 0]).sum() > 1000 and want_a(0)[:, 2].max() > 1000


@pytest.mark.parametrize('lanes', LANES)
def test_planted_hubs_boundary_rows_and_long_inner_rows(lanes):
    """Both hubs against each other, against the middle hubs (inner rows of 64, 65, 129 and 300) and against every boundary degree; the cut at 63, 64 and 65
    lands one below, on and one above the rows of those lengths."""
    store, pairs, want, nodes = case_w()
    for chunk in (0, 1, 63, 64, 65, 2 ** 30):
        with tuning(walk_lanes=lanes, walk_chunk=chunk):
            for flags in (0, 1):
                assert np.array_equal(_raw(store, 0, pairs, flags), want[flags]), (lanes, chunk, flags)
    hub = want[0][1]                                                          # the pair (0, 1)
    assert pairs[1].tolist() == [0, 1] and hub[0] == 1 and hub[1] > 2000 and hub[2] > 10000
    assert want[1][1].tolist() == [0, int(hub[1]), int(hub[2]) - (2 * ref.HUB_ROW - 1)]


def test_a_heavy_pair_repeated_among_light_pairs():
    """Fifty copies of the hub pair, in both orientations, between light pairs: every copy's row is seeded and summed on its own."""
    store, pairs, want, nodes = case_w()
    rng = np.random.default_rng(4)
    at = rng.integers(0, len(pairs), 400)
    hub_at = rng.choice(400, 50, replace=False)
    at[hub_at[:25]] = 1                                                       # (0, 1)
    at[hub_at[25:]] = len(nodes)                                              # (1, 0)
    assert pairs[len(nodes)].tolist() == [1, 0]
    for chunk in (0, 7):
        for flags in (0, 1):
            with tuning(walk_chunk=chunk):
                got = _raw(store, 0, pairs[at], flags)
            assert np.array_equal(got, want[flags][at]), (chunk, flags)
            assert (got[hub_at] == got[hub_at[0]]).all() and got[hub_at[0], 2] > 10000


@pytest.mark.parametrize('lanes', LANES)
def test_third_graph_of_a_store_and_a_weighted_store(lanes):
    rng = np.random.default_rng(2)
    g0 = (50, rng.integers(0, 50, 333).astype(np.int64), rng.integers(0, 50, 333).astype(np.int64))
    g1 = (7, np.array([0, 1, 5], np.int64), np.array([1, 2, 5], np.int64))
    N, src, dst, nb = case_a()
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(src))).astype(np.float32)
    weights = [np.ones(len(g0[1]), np.float32), np.ones(3, np.float32), w]
    pairs = np.concatenate([rng.integers(0, N, (3000, 2)), np.stack([rng.integers(0, 2, 500), rng.integers(0, N, 500)], 1)])      # hubs 0 and 1 among them
    every1 = np.array([(a, b) for a in range(7) for b in range(7)])
    every0 = np.array([(a, b) for a in range(50) for b in range(50)])
    at = pairs[:, 0] * N + pairs[:, 1]
    with tuning(walk_lanes=lanes, walk_chunk=5):
        for wts in (None, weights):
            store = _store([g0, g1, (N, src, dst)], weights=wts)
            assert store.weighted == (wts is not None)
            for flags in (0, 1):
                assert np.array_equal(_raw(store, 2, pairs, flags), want_a(flags)[at])      # offsets and weights change nothing
            assert np.array_equal(_raw(store, 1, every1), ref.pair_walks(*g1, every1))
            assert np.array_equal(_raw(store, 0, every0, 1), ref.pair_walks(*g0, every0, 1))


def test_two_streams_on_a_fresh_store_against_one_and_two_runs():
    """The index is built by the first call (here on s1); the second stream reads it with no event between them."""
    N, src, dst, _ = case_a()
    store = _store([(N, src, dst)])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pairs = all_pairs_a()[::7]
    with tuning(walk_chunk=3):
        a = _raw(store, 0, pairs, stream=s1)
        b = _raw(store, 0, pairs, stream=s2)
        c = _raw(store, 0, pairs)
        with torch.cuda.stream(s2):
            d = store.pair_walks(0, pairs)
        again = _raw(store, 0, pairs)
    for x in (a, b, c, d, again):
        assert np.array_equal(x, want_a(0)[::7])


def test_ids_outside_the_graph_n_zero_and_bad_arguments():
    from gmeta_amd import _lib
    store, lib = store_a(), _lib.lib()
    N = case_a()[0]
    got = _raw(store, 0, [(0, N), (-1, 5), (N, N), (2 ** 31 - 1, 0), (0, 1)])
    assert not got[:4].any() and np.array_equal(got[4], want_a(0)[1]) and got[4, 2] > 0
    assert _raw(store, 0, np.zeros((0, 2))).shape == (0, 3)                   # n == 0: the poisoned row stays
    null = C.c_void_p(0)
    assert lib.gm_store_pair_walks(store.handle, 0, null, 0, 0, null, _lib.stream_ptr()) == 0      # n == 0 with NULL pointers
    out = torch.zeros((4, 3), dtype=torch.int64, device='cuda')
    d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')
    call = lambda g, n, flags, p=_lib.ptr(d_p), o=_lib.ptr(out): lib.gm_store_pair_walks(store.handle, g, p, n, flags, o, _lib.stream_ptr())      # noqa: E731
    for g, n, flags, word in ((1, 4, 0, 'graph 1'), (-1, 4, 0, 'graph -1'), (0, -1, 0, 'n = -1'), (0, 2 ** 31, 0, 'n = 2147483648'), (0, 4, 2, 'flag bits 0x2'),
                              (0, 4, 5, 'flag bits 0x5')):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(g, n, flags), 'gm_store_pair_walks')
    for p, o in ((null, _lib.ptr(out)), (_lib.ptr(d_p), null)):
        with pytest.raises(ValueError, match='NULL argument'):
            _lib.check(call(0, 4, 0, p, o), 'gm_store_pair_walks')
    with pytest.raises(ValueError, match='store is NULL'):
        _lib.check(lib.gm_store_pair_walks(null, 0, _lib.ptr(d_p), 4, 0, _lib.ptr(out), _lib.stream_ptr()), 'gm_store_pair_walks')
    for knob, value, word in (('walk_chunk', -1, 'walk_chunk = -1'), ('walk_lanes', 16, 'walk_lanes = 16'), ('walk_lanes', 48, 'walk_lanes = 48')):
        with tuning(**{knob: value}):
            with pytest.raises(ValueError, match=word):
                _lib.check(call(0, 4, 0), 'gm_store_pair_walks')
    assert call(0, 0, 0) == 0 and call(0, 4, 1) == 0
    assert store.pair_walks(0, np.zeros((0, 2))).shape == (0, 3) and store.pair_walks(0, []).dtype == np.int64
    with pytest.raises(ValueError, match='graph'):
        store.pair_walks(1, [[0, 1]])
    with pytest.raises(ValueError, match='outside'):
        store.pair_walks(0, [[0, N]])
    torch.cuda.synchronize()


def test_graphstore_pair_walks_equals_the_raw_call():
    store, pairs, want, _ = case_w()
    for mask in (False, True):
        got = store.pair_walks(0, pairs, mask_target=mask)
        assert got.dtype == np.int64 and got.shape == (len(pairs), 3)
        assert np.array_equal(got, _raw(store, 0, pairs, 1 if mask else 0)) and np.array_equal(got, want[1 if mask else 0])
    assert np.array_equal(store_a().pair_walks(0, all_pairs_a()[:5000], mask_target=True), want_a(1)[:5000])


# ---------------------------------------------------------------------------------------------------- AUC over completed tables, driver
@pytest.mark.parametrize('mask', [False, True])
def test_link_path_auc_equals_the_auc_of_the_restated_scores(mask):
    """The walk counts are equal integers and the scores are formed from them by the same float64 expression: the AUCs are EQUAL."""
    import gmeta_amd
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, pos, info1)
    names, labels = tables['train']
    got = gmeta_amd.link_path_auc(store, names, labels, mask_target=mask)
    assert tuple(got) == gmeta_amd.PATH_SCORES
    want = np.zeros((len(names), 3), np.int64)
    for k, nm in enumerate(names):
        g, a, b = (int(x) for x in nm.split('_'))
        want[k] = ref.pair_walks(*d['graphs'][g], [(a, b)], 1 if mask else 0)[0]
    assert np.array_equal(gmeta_amd.link_path_scores(store, names, mask_target=mask), want)
    y = np.asarray(labels).astype(np.int64)
    assert y.sum() * 2 == len(y) > 100
    lp, kz = want[:, 1] + 0.01 * want[:, 2], 0.005 * want[:, 0] + 0.005 ** 2 * want[:, 1] + 0.005 ** 3 * want[:, 2]
    assert got['local_path'] == gmeta_amd.link_auc(lp, labels) == pytest.approx(pair_score_ref.auc_by_pair_count(lp, labels), abs=1e-12)
    assert got['katz'] == gmeta_amd.link_auc(kz, labels) == pytest.approx(pair_score_ref.auc_by_pair_count(kz, labels), abs=1e-12)
    print('mask %s: AUC local_path %.6f  katz %.6f' % (mask, got['local_path'], got['katz']))


def test_train_driver_reports_the_path_aucs(tmp_path, capsys):
    import gmeta_amd
    from gmeta_amd import datadir, synth
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric']
    res = drv.main(drv.parse(base + ['--heuristics', '2']))
    auc = res['path_auc']
    assert tuple(auc) == gmeta_amd.PATH_SCORES and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in auc.values()), auc
    assert tuple(res['heuristic_auc']) == gmeta_amd.PAIR_SCORES
    text = capsys.readouterr().out
    assert 'Heuristic test AUC:' in text and 'Path test AUC:' in text and all(k in text for k in gmeta_amd.PAIR_SCORES + gmeta_amd.PATH_SCORES)
    assert text.index('Heuristic test AUC:') < text.index('Path test AUC:')
    # over the completed test table, with the mask: the same calls by hand
    from gmeta_amd.negatives import read_link_tables
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root + '/'), info1, mode='uniform')
    assert auc == gmeta_amd.link_path_auc(store, *tables['test'], mask_target=True)
    assert res['heuristic_auc'] == gmeta_amd.link_heuristic_auc(store, *tables['test'], mask_target=True)
    one = drv.main(drv.parse(base + ['--heuristics', '1']))
    text = capsys.readouterr().out
    assert 'path_auc' not in one and 'Path test AUC' not in text and 'Heuristic test AUC:' in text
    assert one == {k: v for k, v in res.items() if k != 'path_auc'}
