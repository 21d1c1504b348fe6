"""GPU (-m gpu): rank counts and ranking metrics (gm_rank_counts, gm_rank_summary, gmeta_amd.rank_counts / rank_metrics / link_ranking, PairPredictor.ranking,
train.py --rank_k) against the restatement of the definition (tests/ranking_ref.py; the definition itself is in include/gmeta_hip.h).  Every integer must be
equal, none left out; the output is poisoned around [P, 2] and the poison must stay.  The one float, rr_sum, is held to P * 2^-52 * fsum: the bound of a sum of P
positive correctly rounded terms (each term carries at most 2^-53 relative error, each of the fewer than P additions another 2^-53 of a partial sum that never
exceeds the total)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ranking_ref as ref
from test_hip_pair_pagerank import _stream, tuning

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = -0x0123456789ABCDE
INT32_MAX = 2 ** 31 - 1
PATHS = {'sorted': 1, 'brute': INT32_MAX}          # rank_sort_min: always sort / never sort
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097, 70001]      # the last spans several workgroups of any tile
KINDS = ['ties', 'special', 'normal', 'equal', 'ascending', 'descending', 'above', 'below']
P_MAX = 1000


def make(kind, P, N, seed=0):
    """float32 positives [P], negatives [N] of a score kind"""
    if kind in ('ties', 'special', 'normal', 'equal'):
        return ref.scores(kind, P, 2 * seed + 1), ref.scores(kind, N, 2 * seed + 2)
    pos, neg = ref.scores('normal', P, 2 * seed + 1), ref.scores('normal', N, 2 * seed + 2)
    if kind == 'ascending':
        return pos, np.sort(neg)
    if kind == 'descending':
        return pos, np.sort(neg)[::-1].copy()
    return pos, (neg + f32(100.0) if kind == 'above' else neg - f32(100.0))      # every negative above / below every positive


def _dev(a, dtype):
    a = np.array(a, dtype, order='C')                 # a copy: the cached cases are read-only
    return torch.from_numpy(a).cuda() if a.size else None


def raw_counts(pos, neg, ranges=None, stream=None):
    """The C ABI itself: int64 [P, 2]; the rows in front of it and behind it are poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    P, N = len(pos), len(neg)
    d_p, d_n, d_r = _dev(pos, f32), _dev(neg, f32), None if ranges is None else _dev(ranges, np.int64)
    out = torch.full((P + 2, 2), POISON, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_rank_counts(_lib.ptr(d_p), P, _lib.ptr(d_n), N, _lib.ptr(d_r), C.c_void_p(out.data_ptr() + 16), _stream(stream)), 'gm_rank_counts')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[0] == POISON).all() and (out[P + 1] == POISON).all()
    return out[1:P + 1]


def raw_summary(pos, neg, ks, ranges=None, with_counts=True, stream=None):
    """The C ABI itself: ({'n_pos', ...} as ranking_ref.summary gives it, the counts or None)"""
    from gmeta_amd import _lib
    P, N = len(pos), len(neg)
    d_p, d_n, d_r = _dev(pos, f32), _dev(neg, f32), None if ranges is None else _dev(ranges, np.int64)
    out = torch.full((P + 2, 2), POISON, dtype=torch.int64, device='cuda')
    h_ks = (C.c_int64 * max(len(ks), 1))(*ks)
    s = _lib.RankSummary()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_rank_summary(_lib.ptr(d_p), P, _lib.ptr(d_n), N, _lib.ptr(d_r), h_ks, len(ks), C.c_void_p(out.data_ptr() + 16) if with_counts else None,
                                          C.byref(s), _stream(stream)), 'gm_rank_summary')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[0] == POISON).all() and (out[P + 1] == POISON).all() and (with_counts or (out == POISON).all())
    got = {'n_pos': int(s.n_pos), 'n_pairs': int(s.n_pairs), 'auc2': int(s.auc2), 'rr_sum': float(s.rr_sum), 'hits': [int(s.hits[j]) for j in range(len(ks))]}
    assert all(s.hits[j] == 0 for j in range(len(ks), ref.MAX_K))
    return got, (out[1:P + 1] if with_counts else None)


@functools.lru_cache(maxsize=None)
def shared_case(kind, N):
    """the inputs of a shared-mode case and their counts by the restatement, computed once for the P_MAX positives (a positive's counts do not depend on the
    others: the smaller P of the tests are prefixes) and left unchanged"""
    pos, neg = make(kind, P_MAX, N, seed=N % 97)
    want = ref.counts(pos, neg)
    for a in (pos, neg, want):
        a.setflags(write=False)
    return pos, neg, want


def check_summary(got, want, P, what):
    assert {k: got[k] for k in ('n_pos', 'n_pairs', 'auc2', 'hits')} == {k: want[k] for k in ('n_pos', 'n_pairs', 'auc2', 'hits')}, what
    err, tol = abs(got['rr_sum'] - want['rr_sum']), P * 2.0 ** -52 * want['rr_sum']
    print('%s: rr_sum %.17g, |error| %.3g, bound %.3g' % (what, got['rr_sum'], err, tol))
    assert err <= tol, what


# ---------------------------------------------------------------------------------------------------- shared mode
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_shared_mode_both_paths_equal_the_restatement(kind, N):
    pos, neg, want = shared_case(kind, N)
    for P in (1, 65, P_MAX):
        got = {}
        for path, v in PATHS.items():
            with tuning(rank_sort_min=v):
                got[path] = raw_counts(pos[:P], neg)
            assert got[path].dtype == np.int64 and np.array_equal(got[path], want[:P]), (kind, N, P, path)
        assert np.array_equal(got['sorted'], got['brute'])
    with tuning(rank_sort_min=0):                                                       # the library's own choice: the same integers
        assert np.array_equal(raw_counts(pos, neg), want)


def test_knob_cut_is_the_n_at_or_above_which_the_call_sorts_and_a_negative_one_is_refused():
    from gmeta_amd import _lib
    pos, neg, want = shared_case('ties', 257)
    for v in (256, 257, 258):                                                           # either side of the cut: the same integers
        with tuning(rank_sort_min=v):
            assert np.array_equal(raw_counts(pos, neg), want)
    with tuning(GM_RANK_SORT_MIN=5):
        assert _lib.lib().gm_get_tuning(b'rank_sort_min') == 5
    with tuning(rank_sort_min=-1):
        with pytest.raises(ValueError, match='rank_sort_min = -1'):
            raw_counts(pos, neg)
    assert _lib.lib().gm_get_tuning(b'rank_sort_min') == 0


# ---------------------------------------------------------------------------------------------------- ranged mode
@functools.lru_cache(maxsize=None)
def ranged_case(kind):
    """range lengths 0, 1, 64, 65 and 5,000 (past the split cut), overlapping and repeated ranges"""
    N = 12000
    neg = ref.scores(kind, N, 71)
    rng = np.random.default_rng(72)
    lens = [0, 1, 64, 65, 5000, 5000, 4096, 4097, 63, 200, 0, 12000]
    r = [[b, b + n] for n in lens for b in (0, int(rng.integers(0, N - n + 1)), N - n)]
    r += [[100, 5100], [100, 5100], [100, 5100], [3000, 8000], [4999, 5001], [N, N]]      # repeated, overlapping, empty at the end
    r += [[int(b), int(b) + int(n)] for b, n in zip(rng.integers(0, N - 300, 150), rng.integers(0, 300, 150))]
    r = np.asarray(r, np.int64)
    pos = ref.scores(kind, len(r), 73)
    want = ref.counts(pos, neg, r)
    for a in (pos, neg, r, want):
        a.setflags(write=False)
    return pos, neg, r, want


@pytest.mark.parametrize('kind', ['ties', 'special', 'normal'])
def test_ranged_mode_equals_the_restatement(kind):
    pos, neg, r, want = ranged_case(kind)
    got = raw_counts(pos, neg, r)
    assert np.array_equal(got, want)
    for at in ([4], [0, 1, 2], [13, 14]):                                              # alone and in small batches: the same integers (a long range alone too)
        assert np.array_equal(raw_counts(pos[at], neg, r[at]), want[at])


@pytest.mark.parametrize('N', [0, 1, 257, 4097, 70001])
def test_full_ranges_give_the_shared_modes_integers(N):
    pos, neg, want = shared_case('ties', N)
    P = 65
    full = np.tile(np.array([[0, N]], np.int64), (P, 1))
    assert np.array_equal(raw_counts(pos[:P], neg, full), want[:P])
    ks = (1, 20, 50)
    a, _ = raw_summary(pos[:P], neg, ks, full)
    b, _ = raw_summary(pos[:P], neg, ks)
    assert a == b


# ---------------------------------------------------------------------------------------------------- invariance
@pytest.mark.parametrize('path', sorted(PATHS))
def test_counts_do_not_depend_on_the_batch_the_order_of_the_negatives_or_the_stream(path):
    pos, neg, want = shared_case('special', 4097)
    rng = np.random.default_rng(3)
    with tuning(rank_sort_min=PATHS[path]):
        for i in (0, 64, 999):
            assert np.array_equal(raw_counts(pos[i:i + 1], neg), want[i:i + 1])          # alone
        assert np.array_equal(raw_counts(pos, neg[rng.permutation(len(neg))]), want)     # a permutation of the negatives
        side = torch.cuda.Stream()
        assert np.array_equal(raw_counts(pos, neg, stream=side), want)                   # a non-default stream
        got, cnt = raw_summary(pos, neg, (1, 100), stream=side)
    assert np.array_equal(cnt, want)
    check_summary(got, ref.summary(want, len(neg), (1, 100)), len(pos), 'side stream, ' + path)
    pos_r, neg_r, r, want_r = ranged_case('ties')
    assert np.array_equal(raw_counts(pos_r, neg_r, r, stream=side), want_r)


# ---------------------------------------------------------------------------------------------------- summary
@pytest.mark.parametrize('kind,N', [('ties', 257), ('special', 4097), ('normal', 70001), ('equal', 64), ('below', 65), ('above', 255), ('ties', 0)])
def test_summary_integers_are_exact_and_rr_sum_is_within_the_bound_and_reproducible(kind, N):
    pos, neg, want = shared_case(kind, N)
    ks = (1, 2, 3, 20, 50, 100, 1000, 100000)                                           # n_k = 8
    for P in (1, 65, P_MAX):
        for path, v in PATHS.items():
            with tuning(rank_sort_min=v):
                got, cnt = raw_summary(pos[:P], neg, ks)
                again, none = raw_summary(pos[:P], neg, ks, with_counts=False)           # d_counts == NULL is allowed
            assert np.array_equal(cnt, want[:P]) and none is None
            check_summary(got, ref.summary(want[:P], N, ks), P, '%s N %d P %d %s' % (kind, N, P, path))
            assert np.float64(got['rr_sum']).view(np.uint64) == np.float64(again['rr_sum']).view(np.uint64) and got == again      # the same bits
    got, _ = raw_summary(pos, neg, ())                                                  # n_k = 0
    check_summary(got, ref.summary(want, N, ()), P_MAX, '%s N %d, no K' % (kind, N))


def test_summary_of_ranges_and_of_no_positive():
    pos, neg, r, want = ranged_case('ties')
    ks = (1, 5, 100)
    got, cnt = raw_summary(pos, neg, ks, r)
    assert np.array_equal(cnt, want)
    check_summary(got, ref.summary(want, len(neg), ks, r), len(pos), 'ranged')
    got, _ = raw_summary(pos[:0], neg, ks)                                              # P == 0: a zero summary
    assert got == {'n_pos': 0, 'n_pairs': 0, 'auc2': 0, 'rr_sum': 0.0, 'hits': [0, 0, 0]}
    assert raw_counts(pos[:0], neg).shape == (0, 2)


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_name_the_value_and_leave_later_calls_alone():
    from gmeta_amd import _lib
    lib, P_ = _lib.lib(), _lib.ptr
    st = _lib.stream_ptr()
    pos, neg, want = shared_case('normal', 257)
    P, N = 65, len(neg)
    d_p, d_n = _dev(pos[:P], f32), _dev(neg, f32)
    full = np.tile(np.array([[0, N]], np.int64), (P, 1))
    out = torch.full((P, 2), POISON, dtype=torch.int64, device='cuda')
    s = _lib.RankSummary()
    s.n_pos = -77
    ks3 = (C.c_int64 * 3)(1, 20, 50)

    def counts(p=d_p, n_p=P, n=d_n, n_n=N, r=None, o=out):
        return lib.gm_rank_counts(P_(p), n_p, P_(n), n_n, P_(r), P_(o), st)

    def summ(p=d_p, n_p=P, n=d_n, n_n=N, r=None, ks=ks3, n_k=3, o=out, h=s):
        return lib.gm_rank_summary(P_(p), n_p, P_(n), n_n, P_(r), ks, n_k, P_(o), C.byref(h) if h is not None else None, st)

    def fails(rc, text):
        msg = lib.gm_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg)

    for call in (counts, summ):
        bad = pos[:P].copy(); bad[40] = np.nan
        fails(call(p=_dev(bad, f32)), 'd_pos[40] is a NaN')
        bad = neg.copy(); bad[[200, 17]] = np.nan
        fails(call(n=_dev(bad, f32)), 'd_neg[17] is a NaN')
        for path in PATHS.values():
            with tuning(rank_sort_min=path):
                fails(call(n=_dev(bad, f32)), 'd_neg[17] is a NaN')
        r = full.copy(); r[7] = (3, N + 1)
        fails(call(r=_dev(r, np.int64)), 'range 7 = (3, %d) with N = %d' % (N + 1, N))
        r = full.copy(); r[9] = (30, 29)
        fails(call(r=_dev(r, np.int64)), 'range 9 = (30, 29)')
        r = full.copy(); r[64] = (-1, 5)
        fails(call(r=_dev(r, np.int64)), 'range 64 = (-1, 5)')
        fails(call(n_p=-1), 'P = -1'); fails(call(n_p=2 ** 31), 'P = 2147483648'); fails(call(n_n=-2), 'N = -2'); fails(call(n_n=2 ** 31), 'N = 2147483648')
        fails(call(p=None), 'd_pos is NULL'); fails(call(n=None), 'd_neg is NULL')
    fails(counts(o=None), 'd_counts is NULL')
    fails(summ(n_k=9), 'n_k = 9'); fails(summ(n_k=-1), 'n_k = -1')
    fails(summ(ks=(C.c_int64 * 3)(1, 0, 50)), 'h_ks[1] = 0')                            # K = 0
    fails(summ(ks=None), 'h_ks is NULL'); fails(summ(h=None), 'h_out is NULL')
    assert s.n_pos == -77                                                               # *h_out untouched by every failure
    assert lib.gm_rank_counts(None, 2 ** 31 - 1, None, 2 ** 31 - 1, None, None, st) == -1
    assert summ(n_p=0, p=None, n=None, o=None) == 0 and s.n_pos == 0                    # P == 0: nothing else is looked at
    assert counts(n=None, n_n=0) == 0                                                   # d_neg may be NULL where N == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()
    assert counts() == 0 and summ(o=None) == 0                                          # after the errors: good calls are unaffected
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[:P])
    check_summary({'n_pos': s.n_pos, 'n_pairs': s.n_pairs, 'auc2': s.auc2, 'rr_sum': s.rr_sum, 'hits': list(s.hits[:3])}, ref.summary(want[:P], N, (1, 20, 50)), P, 'after errors')


# ---------------------------------------------------------------------------------------------------- the Python layers
def _same(got, want):
    assert set(got) == set(want)
    for k in want:
        if k == 'mrr':
            assert abs(got[k] - want[k]) <= want['n_pos'] * 2.0 ** -52 * want[k] + 2.0 ** -53 * want[k], k      # rr_sum's bound, and the one division by P
        else:
            assert got[k] == want[k], k


@pytest.mark.parametrize('kind', ['ties', 'normal'])
def test_rank_metrics_and_rank_counts_from_numpy_and_from_cuda_tensors(kind):
    import gmeta_amd
    pos, neg, want = shared_case(kind, 4097)
    pos = pos[:333]
    ks = (1, 20, 50)
    m = ref.metrics(pos, neg, ks)
    auc = gmeta_amd.link_auc(np.concatenate([pos, neg]), np.concatenate([np.ones(len(pos)), np.zeros(len(neg))]))
    d_pos, d_neg = torch.from_numpy(pos.copy()).cuda(), torch.from_numpy(neg.copy()).cuda()
    for a, b in ((pos, neg), (pos.astype(np.float64), neg.astype(np.float64)), (d_pos, d_neg), (pos, d_neg)):
        got = gmeta_amd.rank_metrics(a, b, ks)
        _same(got, m)
        assert np.float64(got['auc']).view(np.uint64) == np.float64(auc).view(np.uint64)             # link_auc's number, bit for bit
        assert np.array_equal(gmeta_amd.rank_counts(a, b), want[:333])
    t = gmeta_amd.rank_counts(d_pos, d_neg, as_torch=True)
    assert t.is_cuda and t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), want[:333])
    r = np.stack([np.arange(333), np.arange(333) + 700], 1)
    _same(gmeta_amd.rank_metrics(pos, neg, ks, ranges=r), ref.metrics(pos, neg, ks, r))
    _same(gmeta_amd.rank_metrics(d_pos, d_neg, ks, ranges=torch.from_numpy(r).cuda()), ref.metrics(pos, neg, ks, r))
    assert np.array_equal(gmeta_amd.rank_counts(pos, neg, r), ref.counts(pos, neg, r))
    assert list(gmeta_amd.rank_metrics(pos, neg)) == ['hits@20', 'hits@50', 'hits@100', 'mrr', 'auc', 'n_pos', 'n_pairs']


def test_rank_metrics_refuses_what_it_cannot_rank():
    import gmeta_amd
    pos, neg = np.array([1.0, 2.0], f32), np.array([0.5, 1.0, 3.0], f32)
    with pytest.raises(ValueError, match=r'0 positive\(s\), 3 negative\(s\)'):
        gmeta_amd.rank_metrics(pos[:0], neg)
    with pytest.raises(ValueError, match=r'2 positive\(s\), 0 negative\(s\)'):
        gmeta_amd.rank_metrics(pos, neg[:0])
    with pytest.raises(ValueError, match='every one of the 2 range'):
        gmeta_amd.rank_metrics(pos, neg, ranges=[[1, 1], [3, 3]])
    with pytest.raises(ValueError, match='9 values of K; at most 8'):
        gmeta_amd.rank_metrics(pos, neg, ks=range(1, 10))
    with pytest.raises(ValueError, match='K = 0'):
        gmeta_amd.rank_metrics(pos, neg, ks=(5, 0))
    with pytest.raises(ValueError, match=r'd_neg\[1\] is a NaN'):
        gmeta_amd.rank_metrics(pos, np.array([0.0, np.nan], f32))
    with pytest.raises(ValueError, match=r'range 1 = \(2, 4\)'):
        gmeta_amd.rank_counts(pos, neg, [[0, 3], [2, 4]])
    with pytest.raises(ValueError, match='ranges of shape'):
        gmeta_amd.rank_counts(pos, neg, [[0, 3]])
    with pytest.raises(ValueError, match='dtype int64'):
        gmeta_amd.rank_counts(np.array([1, 2]), neg)
    with pytest.raises(ValueError, match='torch.float64'):
        gmeta_amd.rank_counts(torch.zeros(2, dtype=torch.float64, device='cuda'), neg)
    assert gmeta_amd.rank_metrics(pos, neg, ks=(1,))['n_pairs'] == 6                     # and a good call afterwards


def test_link_ranking_with_and_without_groups_from_numpy_and_from_a_cuda_tensor():
    import gmeta_amd
    rng = np.random.default_rng(17)
    n = 3000
    y = (rng.random(n) < 0.3).astype(np.int64)
    g = rng.integers(0, 40, n)
    g[np.nonzero(y == 1)[0][:3]] = 77                                                    # three positives whose group has no negative
    ks = (1, 10, 20)
    for kind in ('ties', 'normal'):
        s = ref.scores(kind, n, 19)
        d_s = torch.from_numpy(s.copy()).cuda()
        want = ref.metrics(s[y == 1], s[y == 0], ks)
        auc = gmeta_amd.link_auc(s, y)
        for a, lab in ((s, y), (s.astype(np.float64), [str(v) for v in y]), (d_s, y)):
            got = gmeta_amd.link_ranking(a, lab, ks)
            _same(got, want)
            assert np.float64(got['auc']).view(np.uint64) == np.float64(auc).view(np.uint64)
        at_pos, at_neg, r = ref.group_ranges(g, y)
        want_g = ref.metrics(s[at_pos], s[at_neg], ks, r)
        assert want_g['n_pairs'] == int(np.diff(r, axis=1).sum()) < want['n_pairs']
        for a in (s, d_s):
            _same(gmeta_amd.link_ranking(a, y, ks, groups=g), want_g)
    with pytest.raises(ValueError, match=r'link_ranking needs both labels: 0 positive\(s\), 5 negative\(s\)'):
        gmeta_amd.link_ranking(np.zeros(5, f32), np.zeros(5))
    with pytest.raises(ValueError, match='labels must be 0 or 1'):
        gmeta_amd.link_ranking(np.zeros(3, f32), [0, 1, 2])
    with pytest.raises(ValueError, match='3 scores, 2 labels'):
        gmeta_amd.link_ranking(np.zeros(3, f32), [0, 1])
    with pytest.raises(ValueError, match='groups of 2'):
        gmeta_amd.link_ranking(np.zeros(3, f32), [0, 1, 1], groups=[1, 2])


def test_pair_predictor_ranking_on_a_two_graph_store_equals_link_ranking_of_its_scores():
    import gmeta_amd
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11)
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    names, labels = d['tables']['train']
    props = [store.propagated_features(g, hops=2) for g in range(2)]
    try:
        model = gmeta_amd.PairPredictor(store.feat_dim, 2, hidden=16, seed=3)
        sc = model.link_scores(props, names)
        dev = model.link_scores(props, names, as_torch=True)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), sc.view(np.uint32))      # the same bits, in the order of the names
        ks = (1, 5, 20)
        got = model.ranking(props, names, labels, ks=ks)
        assert got == gmeta_amd.link_ranking(sc, labels, ks)
        y = np.asarray(labels).astype(np.int64)
        _same(got, ref.metrics(sc[y == 1], sc[y == 0], ks))
        assert got['auc'] == model.auc(props, names, labels)
        src = [int(nm.split('_')[0]) * 1000 + int(nm.split('_')[1]) for nm in names]                  # groups: the pair's graph and source node
        assert model.ranking(props, names, labels, ks=ks, groups=src) == gmeta_amd.link_ranking(sc, labels, ks, groups=src)
    finally:
        for p in props:
            p.close()


def test_train_driver_prints_the_ranking_lines_and_changes_nothing_else(tmp_path, capsys):
    import gmeta_amd
    from gmeta_amd import datadir, synth
    from test_hip_pair_scores import DRIVER, _positives_only, _splits
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric', '--buddy', '3', '--heuristics', '2',
                                                  '--pagerank', '1', '--distance', '4']
    plain = drv.main(drv.parse(base))
    text0 = capsys.readouterr().out
    res = drv.main(drv.parse(base + ['--rank_k', '5,20']))
    text = capsys.readouterr().out
    keep = lambda t: [l for l in t.splitlines() if 'Hits@' not in l and 'time' not in l.lower()]      # noqa: E731  (the timing lines differ from run to run)
    new = [l for l in text.splitlines() if 'Hits@' in l]
    assert keep(text) == keep(text0) and 'Hits@' not in text0 and len(new) == 5
    assert {k: v for k, v in res.items() if not k.endswith('_ranking')} == plain
    assert sorted(k for k in res if k.endswith('_ranking')) == ['buddy_ranking', 'distance_ranking', 'heuristic_ranking', 'pagerank_ranking', 'path_ranking']
    lines = text.splitlines()
    for title, family in (('Heuristic', 'heuristic'), ('Path', 'path'), ('PageRank', 'pagerank'), ('Distance', 'distance'), ('BUDDY', 'buddy')):
        at = [i for i, l in enumerate(lines) if l.startswith(title + ' test AUC')]
        assert len(at) == 1 and lines[at[0] + 1].startswith(title + ' test') and 'Hits@5 ' in lines[at[0] + 1] and 'Hits@20 ' in lines[at[0] + 1] \
            and 'MRR ' in lines[at[0] + 1]                                                # one more line after the AUC line
        for nm, m in res[family + '_ranking'].items():
            assert 0.0 <= m['hits@5'] <= m['hits@20'] <= 1.0 and 0.0 < m['mrr'] <= 1.0
            assert 'Hits@5 %.4f Hits@20 %.4f MRR %.4f' % (m['hits@5'], m['hits@20'], m['mrr']) in lines[at[0] + 1]
    b = res['buddy_ranking']['buddy']
    assert lines[[i for i, l in enumerate(lines) if l.startswith('BUDDY test AUC')][0] + 1] == 'BUDDY test Hits@5 %.4f Hits@20 %.4f MRR %.4f' % (b['hits@5'], b['hits@20'], b['mrr'])
    # shared negatives, all graphs pooled, as the AUC lines: the heuristics' numbers by hand, and the family's AUC from the same counts
    from gmeta_amd.negatives import read_link_tables
    from gmeta_amd.heuristics import link_heuristic_scores
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root + '/'), info1, mode='uniform')
    names, labels = tables['test']
    sc = link_heuristic_scores(store, names, True)
    y = np.asarray(labels).astype(np.int64)
    for k, nm in enumerate(gmeta_amd.PAIR_SCORES):
        _same(res['heuristic_ranking'][nm], ref.metrics(sc[y == 1, k], sc[y == 0, k], (5, 20)))
        assert res['heuristic_ranking'][nm]['auc'] == res['heuristic_auc'][nm]
    assert res['buddy_ranking']['buddy']['auc'] == res['buddy_auc']
