"""CPU: the restatement of the ranking definition (tests/ranking_ref.py; the definition is in include/gmeta_hip.h) against what it claims to equal -- link_auc bit
for bit, OGB's Hits@K (pos > the K-th largest negative), a hand-worked MRR, ranges (0, N) against the shared mode -- and the key map against numpy's own order
of the floats.  Plus the surface that needs no GPU: the ABI text, the binding, the knob and the driver flag."""
import os

import numpy as np
import pytest

import ranking_ref as ref

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _auc(pos, neg):
    return ref.metrics(pos, neg, ks=())['auc']


@pytest.mark.parametrize('kind', ['ties', 'normal', 'equal'])
def test_auc_equals_link_auc_bit_for_bit(kind):
    import gmeta_amd
    for seed, (P, N) in enumerate([(1, 1), (7, 3), (50, 200), (333, 129), (200, 1000)]):
        pos, neg = ref.scores(kind, P, 10 + seed), ref.scores(kind, N, 20 + seed)
        want = gmeta_amd.link_auc(np.concatenate([pos, neg]), np.concatenate([np.ones(P), np.zeros(N)]))
        assert np.float64(_auc(pos, neg)).view(np.uint64) == np.float64(want).view(np.uint64), (kind, P, N)
    assert _auc([3, 2], [1, 0]) == 1.0 and _auc([0, 1], [2, 3]) == 0.0 and _auc([1, 1], [1, 1]) == 0.5 and _auc([2, 1], [1, 0]) == (2 + 1 + 0.5) / 4


@pytest.mark.parametrize('kind', ['ties', 'special', 'normal', 'equal'])
def test_hits_equal_ogb_pos_above_the_kth_largest_negative(kind):
    for seed, (P, N) in enumerate([(40, 1), (40, 19), (64, 20), (100, 257)]):
        pos, neg = ref.scores(kind, P, 30 + seed), ref.scores(kind, N, 40 + seed)
        ks = (1, 5, 20, 50, 300)
        got = ref.summary(ref.counts(pos, neg), N, ks)['hits']
        for k, h in zip(ks, got):
            want = P if N < k else int((pos > np.sort(neg)[-k]).sum())          # OGB: fewer than K negatives -> every positive is a hit
            assert h == want, (kind, P, N, k)


def test_mrr_of_a_hand_worked_case():
    # negatives 5 4 4 2 1; positives 6 (rank 1), 4 (one above, two tied: 1 + 1 + 2/2 = 3), 3 (three above: 4), 0 (five above: 6), 2 (three above, one tied: 4.5)
    pos, neg = np.array([6, 4, 3, 0, 2], f32), np.array([5, 4, 4, 2, 1], f32)
    cnt = ref.counts(pos, neg)
    assert cnt.tolist() == [[0, 0], [1, 2], [3, 0], [5, 0], [3, 1]]
    s = ref.summary(cnt, 5, (1, 2, 4))
    assert s['rr_sum'] == pytest.approx(1 + 1 / 3 + 1 / 4 + 1 / 6 + 1 / 4.5, rel=1e-15) and s['hits'] == [1, 1, 3] and s['n_pairs'] == 25
    assert s['auc2'] == 2 * (5 + 2 + 2 + 0 + 1) + (0 + 2 + 0 + 0 + 1)
    assert ref.metrics(pos, neg, (1,))['mrr'] == s['rr_sum'] / 5


@pytest.mark.parametrize('kind', ['ties', 'special'])
def test_full_ranges_equal_the_shared_mode_and_ranges_see_only_their_own(kind):
    P, N = 37, 150
    pos, neg = ref.scores(kind, P, 5), ref.scores(kind, N, 6)
    full = np.tile(np.array([[0, N]], np.int64), (P, 1))
    assert np.array_equal(ref.counts(pos, neg, full), ref.counts(pos, neg))
    assert ref.summary(ref.counts(pos, neg, full), N, (3, 20), full) == ref.summary(ref.counts(pos, neg), N, (3, 20))
    rng = np.random.default_rng(7)
    b = rng.integers(0, N + 1, P); e = np.minimum(N, b + rng.integers(0, 40, P))
    r = np.stack([b, e], 1)
    cnt = ref.counts(pos, neg, r)
    for i in range(P):
        assert np.array_equal(cnt[i], ref.counts(pos[i:i + 1], neg[b[i]:e[i]])[0])
    s = ref.summary(cnt, N, (1,), r)
    assert s['n_pairs'] == int((e - b).sum()) and s['hits'][0] == int((cnt.sum(1) < 1).sum())      # an empty range: a hit, rank 1


def test_key_map_orders_the_special_pool_as_numpy_orders_the_floats():
    x = np.concatenate([ref.SPECIAL, ref.scores('normal', 200, 1), ref.scores('ties', 50, 2)])
    k = ref.key(x)
    assert k.dtype == np.uint32
    a, b = x[:, None], x[None, :]
    assert np.array_equal(k[:, None] < k[None, :], a < b) and np.array_equal(k[:, None] == k[None, :], a == b)      # the two zeros equal, denormals distinct
    assert np.array_equal(np.sort(x), x[np.argsort(k, kind='stable')]) and np.array_equal(ref.key(np.sort(x)), np.sort(k))      # sorted by key = np.sort
    assert ref.key([0.0])[0] == ref.key([-0.0])[0] == 0x80000000 and ref.key([ref.DENORM])[0] == 0x80000001 and ref.key([-ref.DENORM])[0] == 0x7FFFFFFE
    assert ref.key([np.inf])[0] == 0xFF800000 and ref.key([-np.inf])[0] == 0x007FFFFF
    # the definition, the binding and the knob say the same
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    sec = txt[txt.index('RANK COUNTS AND RANKING METRICS'):txt.index('gm_rank_summary_t* h_out, void* stream);')]
    assert 'key = u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000)' in sec and 'tests/ranking_ref.py' in sec and 'rank_sort_min' in sec and 'GM_RANK_SORT_MIN' in sec
    assert '#define GM_RANK_MAX_K 8' in sec and _lib.RANK_MAX_K == ref.MAX_K == 8
    assert 'gm_rank_counts' in _lib.PROTOTYPES and 'gm_rank_summary' in _lib.PROTOTYPES
    import ctypes as C
    assert C.sizeof(_lib.RankSummary) == 8 * (4 + ref.MAX_K)


def test_group_ranges_are_a_stable_grouping_of_the_negatives():
    y = np.array([1, 0, 0, 1, 0, 1, 0, 0, 1])
    g = np.array([5, 5, 2, 2, 5, 9, 2, 7, 7])
    at_pos, at_neg, r = ref.group_ranges(g, y)
    assert at_pos.tolist() == [0, 3, 5, 8] and at_neg.tolist() == [2, 6, 1, 4, 7]      # groups ascending, rows of a group in their own order
    assert r.tolist() == [[2, 4], [0, 2], [5, 5], [4, 5]]                             # group 9 has no negative: an empty range


def test_driver_flag_parses_and_refuses_what_it_cannot_rank():
    import train as drv
    base = ['--data_dir', 'x/', '--task_setup', 'Shared', '--link_pred_mode', 'True']
    assert drv.parse(base).rank_ks == [] and drv.parse(base).rank_k == ''
    assert drv.parse(base + ['--heuristics', '1', '--rank_k', '20,50,100']).rank_ks == [20, 50, 100]
    assert drv.parse(base + ['--buddy', '2', '--rank_k', '7']).rank_ks == [7]
    with pytest.raises(SystemExit, match='--rank_k 20 ranks the scores of a family'):
        drv.parse(base + ['--rank_k', '20'])                                           # no family selected: nothing to rank
    for bad in ('0', '20,x', '1,2,3,4,5,6,7,8,9', '-3'):
        with pytest.raises(SystemExit, match='--rank_k'):
            drv.parse(base + ['--heuristics', '1', '--rank_k', bad])
