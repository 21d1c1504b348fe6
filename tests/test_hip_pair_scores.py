"""GPU (-m gpu): gm_store_pair_scores / gm_store_neighbour_degrees and the Python layers above them against the restatement of the definition
(tests/pair_score_ref.py; the definition itself is in include/gmeta_hip.h), under every forced lanes-per-pair value and the library's own choice.

Tolerances (set by the definition, not measured):
    cn, pref_attachment            EQUAL (the integer rounded once to fp32)
    jaccard                        relative 2^-22 (an fp32 quotient of two integers, each below 2^32)
    adamic_adar, resource_alloc.   relative (min(deg a, deg b) + 8) 2^-24 to the fp64 restatement, per pair: at most min(deg a, deg b) positive fp32 terms,
                                   each rounded once, added in fp32 in some order -- (terms - 1) roundings of a growing positive sum -- whatever the order."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import negative_ref
import pair_score_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
CN, JAC, AA, RA, PA = range(5)
LANES = (0, 16, 32, 64)                      # 0: the library's choice


def _store(graphs, weights=None, F=3):
    import gmeta_amd
    return gmeta_amd.GraphStore(graphs, [np.zeros((g[0], F), f32) for g in graphs], edge_weights=weights)


class pair_lanes:
    def __init__(self, L):
        from gmeta_amd import _lib
        self.lib, self.L = _lib.lib(), L

    def __enter__(self):
        self.was = self.lib.gm_get_tuning(b'pair_lanes')
        assert self.lib.gm_set_tuning(b'pair_lanes', self.L) == 0

    def __exit__(self, *exc):
        self.lib.gm_set_tuning(b'pair_lanes', self.was)
        return False


def _raw(store, g, pairs, flags=0, stream=None):
    """The C ABI itself: float32 [n, 5].  The row behind n is poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
    n = len(p)
    d_p = torch.from_numpy(p).cuda() if n else None
    out = torch.full((n + 1, 5), -7.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    st = _lib.stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_lib.lib().gm_store_pair_scores(store.handle, g, _lib.ptr(d_p), n, flags, _lib.ptr(out), st), 'gm_store_pair_scores')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n:] == -7.0).all()
    return out[:n]


def assert_scores(got, want, deg, pairs, what=''):
    """got: device float32 [n, 5]; want: restatement float64 [n, 5]; deg: the restatement's degrees; pairs inside the graph."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    assert got.dtype == f32 and got.shape == want.shape == (len(pairs), 5)
    assert np.array_equal(got[:, CN], want[:, CN].astype(f32)), what
    assert np.array_equal(got[:, PA], want[:, PA].astype(f32)), what
    g64 = got.astype(np.float64)
    terms = np.minimum(deg[pairs[:, 0]], deg[pairs[:, 1]]).astype(np.float64)
    err = np.abs(g64 - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(want > 0, err / want, np.where(err > 0, np.inf, 0.0))
    print('%s: max relative error  jaccard %.3g x 2^-22   adamic_adar %.3g, resource_allocation %.3g of its (min deg + 8) 2^-24'
          % (what, rel[:, JAC].max(initial=0) * 2.0 ** 22, (rel[:, AA] / ((terms + 8) * 2.0 ** -24)).max(initial=0), (rel[:, RA] / ((terms + 8) * 2.0 ** -24)).max(initial=0)))
    assert (rel[:, JAC] <= 2.0 ** -22).all(), what
    assert (rel[:, AA] <= (terms + 8) * 2.0 ** -24).all(), what
    assert (rel[:, RA] <= (terms + 8) * 2.0 ** -24).all(), what


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- shared references, computed once
@functools.lru_cache(maxsize=None)
def case_a():
    N, src, dst = negative_ref.multigraph_case()
    return N, src, dst, ref.neighbourhoods(N, src, dst), ref.degrees(N, src, dst)


@functools.lru_cache(maxsize=None)
def all_pairs_a():
    N = case_a()[0]
    return np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing='ij'), -1).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def want_a(flags):
    N, src, dst, nb, _ = case_a()
    w = ref.pair_scores(N, src, dst, all_pairs_a(), flags, nb)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def store_a():
    return _store([case_a()[:3]])


@functools.lru_cache(maxsize=None)
def case_p():
    N, src, dst, nodes = ref.planted_case()
    pairs = np.array([(a, b) for a in nodes for b in nodes], np.int64)
    nb = ref.neighbourhoods(N, src, dst)
    want = {f: ref.pair_scores(N, src, dst, pairs, f, nb) for f in (0, 1)}
    return _store([(N, src, dst)]), pairs, want, ref.degrees(N, src, dst)


# ---------------------------------------------------------------------------------------------------- the cases, under every instantiation
@pytest.mark.parametrize('lanes', LANES)
def test_multigraph_every_ordered_pair(lanes):
    N, _, _, _, deg = case_a()
    with pair_lanes(lanes):
        got = _raw(store_a(), 0, all_pairs_a())
        again = _raw(store_a(), 0, all_pairs_a())
    assert_scores(got, want_a(0), deg, all_pairs_a(), 'multigraph, lanes %d' % lanes)
    assert np.array_equal(bits(got), bits(again))                              # two runs, bit for bit
    sq = bits(got).reshape(N, N, 5)
    assert np.array_equal(sq, sq.transpose(1, 0, 2))                           # (a, b) against (b, a), bit for bit
    diag = got.reshape(N, N, 5)[np.arange(N), np.arange(N)]                    # a == b: I = Gamma(a)
    assert np.array_equal(diag[:, CN], deg.astype(f32)) and np.array_equal(diag[:, JAC], (deg > 0).astype(f32))
    assert np.array_equal(diag[:, PA], (deg.astype(np.int64) ** 2).astype(f32))
    if lanes == 0:
        assert np.array_equal(store_a().pair_scores(0, all_pairs_a()[:5000]), got[:5000])


@pytest.mark.parametrize('flags', [0, 1])
@pytest.mark.parametrize('lanes', LANES)
def test_planted_rows_every_length_meets_every_length(lanes, flags):
    store, pairs, want, deg = case_p()
    assert tuple(deg[:len(ref.PLANTED_ROWS)].tolist()) == ref.PLANTED_ROWS
    with pair_lanes(lanes):
        got = _raw(store, 0, pairs, flags)
    assert_scores(got, want[flags], deg, pairs, 'planted, lanes %d, flags %d' % (lanes, flags))
    P = len(ref.PLANTED_ROWS)
    sq = bits(got).reshape(P, P, 5)
    assert np.array_equal(sq, sq.transpose(1, 0, 2))
    assert want[0][:, CN].max() >= 129 and (want[0][:, CN] > 0).sum() > 50


@pytest.mark.parametrize('lanes', LANES)
def test_mask_flag_on_adjacent_non_adjacent_and_self_pairs(lanes):
    N, _, _, nb, deg = case_a()
    with pair_lanes(lanes):
        got = _raw(store_a(), 0, all_pairs_a(), ref.MASK_TARGET)
        plain = _raw(store_a(), 0, all_pairs_a())
    assert_scores(got, want_a(1), deg, all_pairs_a(), 'multigraph masked, lanes %d' % lanes)
    adj = np.array([a != b and b in nb[a] for a, b in all_pairs_a().tolist()])
    assert adj.sum() > 1000 and (~adj).sum() > 1000
    assert np.array_equal(bits(got[~adj]), bits(plain[~adj]))                 # non-adjacent and self pairs: untouched
    da, db = deg[all_pairs_a()[:, 0]].astype(np.int64), deg[all_pairs_a()[:, 1]].astype(np.int64)
    assert np.array_equal(got[adj][:, PA], ((da - 1) * (db - 1))[adj].astype(f32))
    assert np.array_equal(bits(got[:, [CN, AA, RA]]), bits(plain[:, [CN, AA, RA]]))      # the intersection never held a or b
    if lanes == 0:
        assert np.array_equal(store_a().pair_scores(0, all_pairs_a()[:3000], mask_target=True), got[:3000])


@pytest.mark.parametrize('lanes', LANES)
def test_third_graph_of_a_store_and_a_weighted_store(lanes):
    rng = np.random.default_rng(2)
    g0 = (50, rng.integers(0, 50, 333).astype(np.int64), rng.integers(0, 50, 333).astype(np.int64))
    g1 = (7, np.array([0, 1, 5], np.int64), np.array([1, 2, 5], np.int64))
    N, src, dst, nb, deg = case_a()
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(src))).astype(f32)
    weights = [np.ones(len(g0[1]), f32), np.ones(3, f32), w]
    pairs = np.concatenate([rng.integers(0, N, (3000, 2)), np.stack([rng.integers(0, 2, 500), rng.integers(0, N, 500)], 1)])      # hubs 0 and 1 among them
    every1 = np.array([(a, b) for a in range(7) for b in range(7)])
    every0 = np.array([(a, b) for a in range(50) for b in range(50)])
    at = pairs[:, 0] * N + pairs[:, 1]
    with pair_lanes(lanes):
        one = _raw(store_a(), 0, pairs)
        for wts in (None, weights):
            store = _store([g0, g1, (N, src, dst)], weights=wts)
            assert store.weighted == (wts is not None)
            got = _raw(store, 2, pairs)
            assert_scores(got, want_a(0)[at], deg, pairs, 'graph 2 of 3, lanes %d%s' % (lanes, ', weighted' if wts else ''))
            assert np.array_equal(bits(got), bits(one))                        # offsets and weights change nothing
            assert_scores(_raw(store, 1, every1), ref.pair_scores(*g1, every1), ref.degrees(*g1), every1, 'graph 1 of 3')
            assert_scores(_raw(store, 0, every0, 1), ref.pair_scores(*g0, every0, 1), ref.degrees(*g0), every0, 'graph 0 of 3, masked')
            for g, gr in enumerate((g0, g1, (N, src, dst))):
                d = store.neighbour_degrees(g)
                assert d.dtype == np.int32 and np.array_equal(d, ref.degrees(*gr))


def test_the_library_moves_to_wider_groups_on_dense_graphs():
    """Mean distinct degrees of about 33 (16 lanes), 260 (32) and 390 (64): the library's own choice is the forced width's result bit for bit, and the
    neighbouring width's sums come in another order."""
    rng = np.random.default_rng(6)
    N0, src0, dst0 = negative_ref.dense_case()
    cases = [((N0, src0, dst0), 16, 32)]
    for N, lanes, other in ((300, 32, 16), (450, 64, 32)):
        e = np.array([(u, v) for u in range(N) for v in range(u + 1, N) if (u * 7 + v * 3) % 8 != 0], np.int64)
        cases.append(((N, e[:, 1].copy(), e[:, 0].copy()), lanes, other))
    for gr, lanes, other in cases:
        deg = ref.degrees(*gr)
        assert {16: 16 < deg.mean() <= 192, 32: 192 < deg.mean() <= 384, 64: 384 < deg.mean()}[lanes], deg.mean()
        pairs = np.concatenate([rng.integers(0, gr[0], (500, 2)), np.stack([np.arange(0, gr[0], 5)] * 2, 1)])      # self pairs among them
        store = _store([gr])
        nb = ref.neighbourhoods(*gr)
        for flags in (0, 1):
            got = _raw(store, 0, pairs, flags)
            assert_scores(got, ref.pair_scores(*gr, pairs, flags, nb), deg, pairs, 'dense %d, flags %d' % (gr[0], flags))
            with pair_lanes(lanes):
                assert np.array_equal(bits(got), bits(_raw(store, 0, pairs, flags)))
            with pair_lanes(other):
                assert not np.array_equal(bits(got), bits(_raw(store, 0, pairs, flags)))


# ---------------------------------------------------------------------------------------------------- streams, edges of the interface
def test_two_streams_on_a_fresh_store_against_one():
    """The index is built by the first call (here on s1); the second stream reads it with no event between them."""
    N, src, dst, _, _ = case_a()
    store = _store([(N, src, dst)])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pairs = all_pairs_a()[::7]
    a = _raw(store, 0, pairs, stream=s1)
    b = _raw(store, 0, pairs, stream=s2)
    c = _raw(store, 0, pairs)
    with torch.cuda.stream(s2):
        d = store.pair_scores(0, pairs)
    want = _raw(store_a(), 0, pairs)
    for x in (a, b, c, d):
        assert np.array_equal(bits(x), bits(want))


def test_ids_outside_the_graph_n_zero_and_bad_arguments():
    from gmeta_amd import _lib
    store, lib = store_a(), _lib.lib()
    N = case_a()[0]
    got = _raw(store, 0, [(0, N), (-1, 5), (N, N), (2 ** 31 - 1, 0), (0, 1)])
    assert (got[:4] == 0).all() and np.array_equal(bits(got[4]), bits(_raw(store, 0, [(1, 0)])[0])) and got[4, PA] > 0
    assert _raw(store, 0, np.zeros((0, 2))).shape == (0, 5)                   # n == 0: the poisoned row stays
    assert store.pair_scores(0, np.zeros((0, 2))).shape == (0, 5) and store.pair_scores(0, []).dtype == f32
    out = torch.zeros((4, 5), dtype=torch.float32, device='cuda')
    d_p = torch.zeros((4, 2), dtype=torch.int32, device='cuda')
    call = lambda g, n, flags: lib.gm_store_pair_scores(store.handle, g, _lib.ptr(d_p), n, flags, _lib.ptr(out), _lib.stream_ptr())      # noqa: E731
    for g, n, flags, word in ((1, 4, 0, 'graph 1'), (-1, 4, 0, 'graph -1'), (0, -1, 0, 'n = -1'), (0, 4, 2, 'flag'), (0, 4, 5, 'flag')):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(g, n, flags), 'gm_store_pair_scores')
    assert call(0, 0, 0) == 0 and call(0, 4, 1) == 0
    with pytest.raises(ValueError, match='graph 3'):
        _lib.check(lib.gm_store_neighbour_degrees(store.handle, 3, _lib.ptr(out), _lib.stream_ptr()), 'gm_store_neighbour_degrees')
    with pair_lanes(8):
        with pytest.raises(ValueError, match='pair_lanes = 8'):
            _lib.check(call(0, 4, 0), 'gm_store_pair_scores')
    with pytest.raises(ValueError, match='graph'):
        store.pair_scores(1, [[0, 1]])
    with pytest.raises(ValueError, match='outside'):
        store.pair_scores(0, [[0, N]])
    with pytest.raises(ValueError, match='graph'):
        store.neighbour_degrees(-1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- AUC over completed tables, driver
def _positives_only(d):
    tables = {k: ([nm for nm, l in zip(*v) if l == '1'], ['1'] * sum(l == '1' for l in v[1])) for k, v in d['tables'].items()}
    info = {nm: 1 for nm in tables['train'][0]}
    return tables, info


@pytest.mark.parametrize('mask', [False, True])
def test_link_heuristic_auc_equals_the_auc_of_the_restated_scores(mask):
    """The exact columns rank identically, so their AUC is EQUAL.  An fp32 sum or quotient may order two pairs differently from the fp64 restatement only
    where their restated scores lie within the columns' tolerance of each other; each such (positive, negative) pair moves the AUC by at most
    1 / (positives x negatives)."""
    import gmeta_amd
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, pos, info1)
    names, labels = tables['train']
    got = gmeta_amd.link_heuristic_auc(store, names, labels, mask_target=mask)
    assert tuple(got) == gmeta_amd.PAIR_SCORES
    want = np.zeros((len(names), 5))
    tol = np.zeros(len(names))
    for k, nm in enumerate(names):
        g, a, b = (int(x) for x in nm.split('_'))
        want[k] = ref.pair_scores(*d['graphs'][g], [(a, b)], 1 if mask else 0)[0]
        deg = ref.degrees(*d['graphs'][g])
        tol[k] = (min(deg[a], deg[b]) + 8) * 2.0 ** -24
    y = np.asarray(labels).astype(np.int64)
    assert y.sum() * 2 == len(y) > 100
    for k, nm in enumerate(gmeta_amd.PAIR_SCORES):
        auc = gmeta_amd.link_auc(want[:, k], labels)
        assert auc == pytest.approx(ref.auc_by_pair_count(want[:, k], labels), abs=1e-12)
        p, q = want[y == 1, k], want[y == 0, k]
        t = np.maximum(tol[y == 1][:, None], tol[y == 0][None, :]) * 2 * np.maximum(p[:, None], q[None, :])
        near = 0 if k in (CN, PA) else int(((np.abs(p[:, None] - q[None, :]) <= t) & (p[:, None] != q[None, :])).sum())
        print('%s: AUC %.6f device, %.6f restated; %d near-tied (positive, negative) pairs' % (nm, got[nm], auc, near))
        assert abs(got[nm] - auc) <= near / (len(p) * len(q)) + 1e-12, nm


def _splits(d):
    """The train tables of a two-graph link data set dealt out to train / val / test (3 : 1 : 1 by position, per graph, part and label), every split with its
    _spt / _qry parts and its plain table = the two parts."""
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


DRIVER = ['--epoch', '1', '--k_spt', '2', '--k_qry', '3', '--task_num', '2', '--update_step', '2', '--update_step_test', '2', '--update_lr', '0.05', '--meta_lr', '0.01',
          '--hidden_dim', '16', '--batchsz', '8', '--h', '2', '--eval_tasks', '4', '--task_setup', 'Shared', '--link_pred_mode', 'True', '--n_way', '2',
          '--sample_nodes', '20']


def test_train_driver_reports_the_heuristic_aucs(tmp_path, capsys):
    import gmeta_amd
    from gmeta_amd import datadir, synth
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric']
    res = drv.main(drv.parse(base + ['--heuristics', '1']))
    auc = res['heuristic_auc']
    assert tuple(auc) == gmeta_amd.PAIR_SCORES and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in auc.values()), auc
    text = capsys.readouterr().out
    assert 'Heuristic test AUC:' in text and all(k in text for k in gmeta_amd.PAIR_SCORES)
    # over the completed test table, with the mask: the same call by hand
    from gmeta_amd.negatives import read_link_tables
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root + '/'), info1, mode='uniform')
    assert auc == gmeta_amd.link_heuristic_auc(store, *tables['test'], mask_target=True)
    plain = drv.main(drv.parse(base))
    assert sorted(plain) == ['early_stopped_test_acc', 'test_acc', 'val_best'] and 'Heuristic' not in capsys.readouterr().out
    assert {k: v for k, v in res.items() if k != 'heuristic_auc'} == plain
    with pytest.raises(SystemExit, match='link_pred_mode'):
        drv.main(drv.parse(['--data_dir', root + '/', '--task_setup', 'Shared', '--heuristics', '1']))
