"""GPU (-m gpu): gm_store_negative_pairs / gm_store_has_edges and the Python layers above them, bit for bit against the restatement of the definition
(tests/negative_ref.py; the definition itself is in include/gmeta_hip.h), in both modes: a multigraph with everything the adjacency search can meet, a
dense graph that the budget exhausts, many small rounds against one, exclusion lists, a multi-graph store, keys above 2^32, weights, streams; then the
table builder through Subgraphs and the driver."""
import argparse
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

import negative_ref as ref

pytestmark = pytest.mark.gpu
MODES = ('uniform', 'two_hop')
f32 = np.float32


def _store(graphs, weights=None, F=3):
    import gmeta_amd
    return gmeta_amd.GraphStore(graphs, [np.zeros((g[0], F), f32) for g in graphs], edge_weights=weights)


def _raw(store, g, n, seed, mode, exclude=None, stream=None):
    """The C ABI itself: (pairs int32 [found, 2], found).  The rows behind `found` are poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    N = store.n_nodes[g]
    ex = np.asarray([] if exclude is None else exclude, np.int64).reshape(-1, 2)
    keys = np.unique(np.minimum(ex[:, 0], ex[:, 1]) * N + np.maximum(ex[:, 0], ex[:, 1]))
    d_keys = torch.from_numpy(keys).cuda() if len(keys) else None
    out = torch.full((n + 1, 2), -7, dtype=torch.int32, device='cuda')
    found = C.c_int64(-1)
    torch.cuda.synchronize()
    st = _lib.stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_lib.lib().gm_store_negative_pairs(store.handle, g, n, seed, ref.MODES[mode], _lib.ptr(d_keys), len(keys), _lib.ptr(out), C.byref(found), st),
               'gm_store_negative_pairs')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert 0 <= found.value <= n and (out[found.value:] == -7).all()
    return out[:found.value], found.value


class neg_round:
    def __init__(self, R):
        from gmeta_amd import _lib
        self.lib, self.R = _lib.lib(), R

    def __enter__(self):
        self.was = self.lib.gm_get_tuning(b'neg_round')
        assert self.lib.gm_set_tuning(b'neg_round', self.R) == 0

    def __exit__(self, *exc):
        self.lib.gm_set_tuning(b'neg_round', self.was)
        return False


@functools.lru_cache(maxsize=None)
def case_a():
    return ref.multigraph_case()


@functools.lru_cache(maxsize=None)
def want_a(n, mode, seed=222):
    N, src, dst = case_a()
    return ref.negative_pairs(N, src, dst, 0, n, seed, mode)


@functools.lru_cache(maxsize=None)
def store_a():
    return _store([case_a()])


def assert_same(got, want):
    (p, found), (wp, wfound) = got, want
    assert found == wfound, (found, wfound)
    assert np.array_equal(p.astype(np.int64), wp)


# ---------------------------------------------------------------------------------------------------- (a), (c)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n', [1, 2, 257, 3000])
def test_multigraph_bit_for_bit(n, mode):
    want = want_a(n, mode)
    assert want[1] > 0
    assert_same(_raw(store_a(), 0, n, 222, mode), want)
    if want[1] == n:
        assert np.array_equal(store_a().negative_pairs(0, n, mode=mode), want[0])


@pytest.mark.parametrize('mode', MODES)
def test_many_small_rounds_equal_one(mode):
    """neg_round = 64: a pair met again in a later round must lose to its first occurrence -- the table lives through the call."""
    for n in (1, 2, 257, 3000):
        with neg_round(64):
            small = _raw(store_a(), 0, n, 222, mode)
        assert_same(small, want_a(n, mode))
    with neg_round(1000):
        mid = _raw(store_a(), 0, 3000, 222, mode)
    dflt = _raw(store_a(), 0, 3000, 222, mode)
    assert_same(mid, want_a(3000, mode)); assert_same(dflt, want_a(3000, mode))
    assert np.array_equal(small[0], dflt[0]) and np.array_equal(mid[0], dflt[0])


def test_repeats_exist_across_rounds_of_64():
    """Of the restated n = 3000 draw: some k beyond the first 64 candidates repeats an earlier pair (so distinctness ACROSS rounds is exercised)."""
    import gmeta_oracle as orc
    N, src, dst = case_a()
    salt = int(orc.sample_salt(222, 0, ref.TAG, 0))
    w = ref.words(salt, 0, 20000)
    seen, repeats = {}, 0
    for k, r in enumerate(w):
        a, b = ref.pick(r[0], N), ref.pick(r[1], N)
        key = (min(a, b), max(a, b))
        if key in seen and k // 64 != seen[key] // 64:
            repeats += 1
        seen.setdefault(key, k)
    assert repeats > 100


# ---------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize('mode', MODES)
def test_dense_graph_every_free_pair_then_the_budget_runs_out(mode):
    N, src, dst = ref.dense_case()
    free = ref.free_pairs(N, src, dst)
    assert free == {(u, v) for u in range(N) for v in range(u + 1, N) if (u + v) % 7 == 0}
    n = len(free)
    store = _store([(N, src, dst)])
    want = ref.negative_pairs(N, src, dst, 0, n, 222, mode)
    got = _raw(store, 0, n, 222, mode)
    assert_same(got, want)
    want1 = ref.negative_pairs(N, src, dst, 0, n + 1, 222, mode)
    got1 = _raw(store, 0, n + 1, 222, mode)
    assert_same(got1, want1)
    if mode == 'uniform':
        assert got[1] == n and {tuple(x) for x in got[0].tolist()} == free and got1[1] == n
    with pytest.raises(ValueError, match=r'only %d distinct' % got1[1]):
        store.negative_pairs(0, n + 1, mode=mode)


def test_five_node_graph():
    src, dst = np.array([0, 1, 1, 2, 3]), np.array([1, 0, 2, 1, 3])
    store = _store([(5, src, dst)])
    for n in (8, 9):
        got = _raw(store, 0, n, 222, 'uniform')
        assert_same(got, ref.negative_pairs(5, src, dst, 0, n))
        assert got[1] == 8
    with pytest.raises(ValueError, match='only 8 distinct'):
        store.negative_pairs(0, 9)


# ---------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize('mode', MODES)
def test_exclusion_list(mode):
    N, src, dst = case_a()
    n = 257
    plain = want_a(n, mode)[0]
    ex = np.array([plain[0][::-1], plain[6], plain[-1]])                 # the first (given as v, u), the seventh, the last
    want = ref.negative_pairs(N, src, dst, 0, n, 222, mode, exclude=ex)
    got = store_a().negative_pairs(0, n, mode=mode, exclude=np.concatenate([ex, ex[:1]]))      # (a duplicate in the list)
    assert np.array_equal(got, want[0]) and want[1] == n
    gone = {tuple(sorted(x)) for x in ex.tolist()}
    assert not {tuple(x) for x in got.tolist()} & gone
    keep = [x for x in plain.tolist() if tuple(x) not in gone]
    assert got[:len(keep)].tolist() == keep and len(keep) == n - 3
    with neg_round(64):
        assert_same(_raw(store_a(), 0, n, 222, mode, exclude=ex), want)


# ---------------------------------------------------------------------------------------------------- (e), (f), (g)
@pytest.mark.parametrize('mode', MODES)
def test_third_graph_of_a_store(mode):
    rng = np.random.default_rng(2)
    g0 = (50, rng.integers(0, 50, 333).astype(np.int64), rng.integers(0, 50, 333).astype(np.int64))
    g1 = (7, np.array([0, 1], np.int64), np.array([1, 2], np.int64))
    store = _store([g0, g1, case_a()])
    N, src, dst = case_a()
    want = ref.negative_pairs(N, src, dst, 2, 500, 222, mode)
    assert_same(_raw(store, 2, 500, 222, mode), want)
    assert not np.array_equal(want[0], want_a(500, mode)[0])             # the graph index is part of the salt
    assert_same(_raw(store, 0, 100, 222, mode), ref.negative_pairs(*g0, 0, 100, 222, mode))
    h = store.has_edges(2, want[0])
    assert not h.any()


@functools.lru_cache(maxsize=None)
def case_f():
    return ref.big_case()


@pytest.mark.parametrize('mode', MODES)
def test_keys_above_2_to_32(mode):
    N, src, dst = case_f()
    store = _store([(N, src, dst)], F=1)
    want = ref.negative_pairs(N, src, dst, 0, 1000, 222, mode)
    big = np.nonzero(want[0][:, 0] * N + want[0][:, 1] >= 2 ** 32)[0]      # (u >= 61,357: about 1.5 % of uniform pairs)
    assert want[1] == 1000 and len(big) >= 5
    assert_same(_raw(store, 0, 1000, 222, mode), want)
    ex = want[0][[0, int(big[0]), int(big[-1]), 999]]                    # exclusion keys on both sides of 2^32
    assert (ex[:, 0] * N + ex[:, 1]).min() < 2 ** 32
    assert_same(_raw(store, 0, 1000, 222, mode, exclude=ex), ref.negative_pairs(N, src, dst, 0, 1000, 222, mode, exclude=ex))


@pytest.mark.parametrize('mode', MODES)
def test_weighted_store_gives_the_same_pairs(mode):
    N, src, dst = case_a()
    w = np.exp(np.random.default_rng(4).uniform(np.log(0.25), np.log(4.0), len(src))).astype(f32)
    store = _store([(N, src, dst)], weights=[w])
    assert store.weighted
    assert_same(_raw(store, 0, 257, 222, mode), want_a(257, mode))


# ---------------------------------------------------------------------------------------------------- repeatability, streams, errors
@pytest.mark.parametrize('mode', MODES)
def test_two_streams_and_another_seed(mode):
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = _raw(store_a(), 0, 3000, 222, mode, stream=s1)
    b = _raw(store_a(), 0, 3000, 222, mode, stream=s2)
    assert_same(a, want_a(3000, mode)); assert_same(b, want_a(3000, mode))
    with torch.cuda.stream(s1):
        c = store_a().negative_pairs(0, 257, mode=mode)
    assert np.array_equal(c, want_a(257, mode)[0])
    other = _raw(store_a(), 0, 257, 223, mode)
    assert_same(other, want_a(257, mode, 223))
    assert not np.array_equal(other[0], c)
    big = (1 << 40) + 5                                                  # the high word of the seed counts
    N, src, dst = case_a()
    assert_same(_raw(store_a(), 0, 50, big, mode), ref.negative_pairs(N, src, dst, 0, 50, big, mode))
    assert not np.array_equal(_raw(store_a(), 0, 50, big, mode)[0], _raw(store_a(), 0, 50, 5, mode)[0])


def test_bad_arguments():
    from gmeta_amd import _lib
    store = store_a()
    lib = _lib.lib()
    found = C.c_int64(0)
    out = torch.empty((4, 2), dtype=torch.int32, device='cuda')
    call = lambda g, n, mode: lib.gm_store_negative_pairs(store.handle, g, n, 222, mode, None, 0, _lib.ptr(out), C.byref(found), _lib.stream_ptr())      # noqa: E731
    assert call(1, 2, 0) == -1 and call(-1, 2, 0) == -1 and call(0, -1, 0) == -1 and call(0, 2, 2) == -1
    assert call(0, (2 ** 31 - 1 - 4096) // 64 + 1, 0) == -1 and b'budget' in lib.gm_last_error()
    assert call(0, 0, 0) == 0 and found.value == 0
    one = _store([(1, np.zeros(0, np.int64), np.zeros(0, np.int64))])
    assert lib.gm_store_negative_pairs(one.handle, 0, 1, 222, 0, None, 0, _lib.ptr(out), C.byref(found), _lib.stream_ptr()) == -1
    assert lib.gm_store_has_edges(store.handle, 3, _lib.ptr(out), 4, _lib.ptr(out), _lib.stream_ptr()) == -1
    with pytest.raises(ValueError, match='mode'):
        store.negative_pairs(0, 3, mode='three_hop')
    with pytest.raises(ValueError, match='graph'):
        store.negative_pairs(1, 3)
    with pytest.raises(ValueError, match='outside'):
        store.has_edges(0, [[0, 300]])
    assert store.negative_pairs(0, 0).shape == (0, 2) and store.has_edges(0, np.zeros((0, 2))).shape == (0,)


# ---------------------------------------------------------------------------------------------------- has_edges
def test_has_edges_against_brute_force():
    N, src, dst = case_a()
    A = np.zeros((N, N), bool)
    A[src, dst] = True
    A |= A.T
    rng = np.random.default_rng(8)
    pairs = rng.integers(0, N, (5000, 2))
    hubs = np.concatenate([np.stack([np.zeros(125, np.int64), rng.integers(0, N, 125)], 1), np.stack([rng.integers(0, N, 125), np.zeros(125, np.int64)], 1),
                           np.stack([np.ones(125, np.int64), rng.integers(0, N, 125)], 1), np.stack([rng.integers(0, N, 125), np.ones(125, np.int64)], 1)])
    for p in (pairs, hubs, np.array([[5, 5], [17, 17], [6, 6], [0, 0], [295, 296], [285, 285]])):
        got = store_a().has_edges(0, p)
        assert got.dtype == bool and np.array_equal(got, A[p[:, 0], p[:, 1]])
    assert 0 < store_a().has_edges(0, hubs).sum() < len(hubs)


# ---------------------------------------------------------------------------------------------------- through Subgraphs
def _positives_only(d):
    tables = {k: ([nm for nm, l in zip(*v) if l == '1'], ['1'] * sum(l == '1' for l in v[1])) for k, v in d['tables'].items()}
    info = {nm: 1 for nm in tables['train'][0]}
    return tables, info


@pytest.mark.parametrize('mode', MODES)
def test_completed_tables_through_subgraphs_and_a_meta_step(mode):
    import gmeta_amd
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, info = gmeta_amd.link_tables_with_negatives(store, pos, info1, mode=mode)
    for key in ('train_spt', 'train_qry'):
        assert len(tables[key][0]) == 2 * len(pos[key][0])
    assert tables['train'] == (tables['train_spt'][0] + tables['train_qry'][0], tables['train_spt'][1] + tables['train_qry'][1])
    by = {}
    for nm, l in zip(*tables['train']):
        g, a, b = (int(x) for x in nm.split('_'))
        by.setdefault((g, l), []).append((a, b))
        assert info[nm] == int(l)
    for g in (0, 1):
        assert not store.has_edges(g, by[(g, '0')]).any() and store.has_edges(g, by[(g, '1')]).all()
        assert len(set(by[(g, '0')])) == len(by[(g, '0')]) == len(by[(g, '1')])
        N, src, dst = d['graphs'][g]
        want, found = ref.negative_pairs(N, src, dst, g, len(by[(g, '1')]), 222, mode, exclude=by[(g, '1')])
        assert found == len(want) and by[(g, '0')] == [tuple(x) for x in want.tolist()]
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    K = 3
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=2, k_spt=2, k_qry=3, task_num=3, update_step=K, update_step_test=K, method='G-Meta',
                              sample_nodes=20, link_pred_mode='True', task_setup='Shared', h=2)
    db = gmeta_amd.Subgraphs(None, 'train', info, n_way=2, k_shot=2, k_query=3, batchsz=3, args=args, adjs=store, h=2, tables=tables, verbose=False,
                             mask_target=True, link_hops='symmetric', hop_labels=2)
    batch = db.get_batch([0, 1, 2])
    assert batch[0][0].view_of.mask_target
    config = synth.make_config(5 + gmeta_amd.hop_label_width(2, True), 16, 2, 2, link=True)
    m = gmeta_amd.Meta(args, config).to('cuda')
    out, P, T = m._run(batch[0], batch[1], batch[2], batch[3], K, True)
    out = out.cpu().numpy()
    losses = out[P:P + K + 1] / T
    assert np.isfinite(losses).all() and np.isfinite(out[:P]).all(), losses
    accs = m.forward_deferred(*batch[:4]).accs()
    assert np.isfinite(accs).all()


# ---------------------------------------------------------------------------------------------------- driver
def _splits(d):
    """The train tables of a two-graph link data set dealt out to train / val / test (3 : 1 : 1 by position, per graph, part and label), every split with its
    _spt / _qry parts and its plain table = the two parts; each name lands in exactly one split."""
    splits = {}
    for part in ('_spt', '_qry'):
        seen = {}
        for nm, lab in zip(*d['tables']['train' + part]):
            k = seen[(nm.split('_')[0], lab)] = seen.get((nm.split('_')[0], lab), -1) + 1
            split = ('train', 'train', 'train', 'val', 'test')[k % 5]
            for key in (split + part, split):
                names, labels = splits.setdefault(key, ([], []))
                names.append(nm); labels.append(lab)
    return splits


# test_acc of the commit before --negatives existed, its own train.py on the injected-negatives data set below with the DRIVER flags (measured on an MI355X, twice)
PARENT_TEST_ACC = 0.4583333432674408
DRIVER = ['--epoch', '1', '--k_spt', '2', '--k_qry', '3', '--task_num', '2', '--update_step', '2', '--update_step_test', '2', '--update_lr', '0.05', '--meta_lr', '0.01',
          '--hidden_dim', '16', '--batchsz', '8', '--h', '2', '--eval_tasks', '4', '--task_setup', 'Shared', '--link_pred_mode', 'True', '--n_way', '2',
          '--sample_nodes', '20']


def test_train_driver_draws_its_negatives(tmp_path, capsys):
    from gmeta_amd import datadir, synth
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER
    res = drv.main(drv.parse(base + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric', '--hop_labels', '2']))
    assert np.isfinite(res['test_acc']) and 0.0 <= res['test_acc'] <= 1.0, res
    text = capsys.readouterr().out
    assert 'There are 2 classes' in text and 'visible to the model' not in text
    res = drv.main(drv.parse(base + ['--negatives', 'two_hop']))
    assert np.isfinite(res['test_acc'])
    assert 'target edges of the positive pairs are visible to the model' in capsys.readouterr().out
    with pytest.raises(SystemExit, match='link_pred_mode'):
        drv.main(drv.parse(['--data_dir', root + '/', '--task_setup', 'Shared', '--negatives', 'uniform']))


def test_train_driver_file_mode_is_the_unchanged_path(tmp_path):
    """--negatives file (the default) on the injected-negatives variant: the driver of the commit before the flag existed, same seed, same test_acc.
    Its code path reads no table through the new code; the run with the flag spelled out, the run without it and the recorded figure agree."""
    from gmeta_amd import datadir, synth
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11)
    root = str(tmp_path / 'inj')
    datadir.write_datadir(root, d['graphs'], d['feats'], d['info'], _splits(d))
    base = ['--data_dir', root + '/'] + DRIVER
    a = drv.main(drv.parse(base + ['--negatives', 'file']))
    b = drv.main(drv.parse(base))
    print('file mode:', a)
    assert a == b and np.isfinite(a['test_acc'])
    assert a['test_acc'] == PARENT_TEST_ACC, a
