"""GPU (-m gpu): gm_store_pagerank_candidates and GraphStore.pagerank_candidates against the restatement of the definition (tests/pagerank_candidate_ref.py;
the definition itself is in include/gmeta_hip.h).  The definition makes the scores the bits of gm_store_rooted_pagerank's rows, so the restatement is fed the
device's own rows (test_hip_pair_pagerank.py holds those against float64) and everything is EQUAL: partner ids, score bits, totals.

The one tolerance, derived and not measured (test_against_float64): a returned score is a device entry, within pagerank_ref.bound of its float64 value.
If the device leaves out a member w of the float64 candidate set while it returns x, then got[w] <= got[x] (it ranked x first, or w's entry is +0), hence
want[w] - bound(want[w]) <= got[w] <= got[x] <= want[x] + bound(want[x]): no omitted member lies above the smallest returned float64 score plus the two
bounds.  An entry can be zero on one side only by underflow, which 2^-100 keeps away from."""
import argparse
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

import negative_ref
import pagerank_candidate_ref as ref
import pagerank_ref
import pair_score_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
ALPHA, ITERS = 0.15, 20
POISON = -7


def _store(graphs):
    import gmeta_amd
    return gmeta_amd.GraphStore(graphs, [np.zeros((g[0], 1), f32) for g in graphs])


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


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _stream(stream):
    from gmeta_amd import _lib
    return _lib.stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)


def _raw(store, g, nodes, k, alpha=ALPHA, iters=ITERS, stream=None):
    """The C ABI itself -> (nodes int32 [m, k], scores float32 [m, k], totals int32 [m]).  The row behind m is poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    a = np.ascontiguousarray(np.asarray(nodes, np.int64).reshape(-1), np.int32)
    m = len(a)
    d_a = torch.from_numpy(a).cuda() if m else None
    on = torch.full((m + 1, k), POISON, dtype=torch.int32, device='cuda')
    os_ = torch.full((m + 1, k), float(POISON), dtype=torch.float32, device='cuda')
    ot = torch.full((m + 1,), POISON, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    _lib.check(_lib.lib().gm_store_pagerank_candidates(store.handle, g, _lib.ptr(d_a), m, k, alpha, iters, _lib.ptr(on), _lib.ptr(os_), _lib.ptr(ot), _stream(stream)),
               'gm_store_pagerank_candidates')
    torch.cuda.synchronize()
    on, os_, ot = on.cpu().numpy(), os_.cpu().numpy(), ot.cpu().numpy()
    assert (on[m:] == POISON).all() and (os_[m:] == POISON).all() and (ot[m:] == POISON).all()      # nothing beyond row m - 1 is written
    return on[:m], os_[:m], ot[:m]


def _rows(store, g, sources, alpha=ALPHA, iters=ITERS):
    """The device's own gm_store_rooted_pagerank rows, float32 [m, N] (through the C ABI, so that sources outside the graph give their rows of zeros)."""
    from gmeta_amd import _lib
    a = np.ascontiguousarray(np.asarray(sources, np.int64).reshape(-1), np.int32)
    out = torch.empty((len(a), store.n_nodes[g]), dtype=torch.float32, device='cuda')
    _lib.check(_lib.lib().gm_store_rooted_pagerank(store.handle, g, _lib.ptr(torch.from_numpy(a).cuda()), len(a), alpha, iters, _lib.ptr(out), _lib.stream_ptr()),
               'gm_store_rooted_pagerank')
    return out.cpu().numpy()


def assert_equal(got, want, what=''):
    gn, gs, gt = got
    wn, ws, wt = want
    assert gn.shape == wn.shape and gs.shape == ws.shape and gs.dtype == f32, what
    assert np.array_equal(gt.astype(np.int64), wt), what
    assert np.array_equal(gn.astype(np.int64), wn), what
    assert np.array_equal(bits(gs), bits(ws)), what
    pad = wn < 0
    assert (gn[pad] == -1).all() and (bits(gs)[pad] == 0).all(), what           # padding: -1 and +0.0f
    assert ((gn >= 0).sum(1) == np.minimum(wt, gn.shape[1])).all(), what


# ---------------------------------------------------------------------------------------------------- shared cases, computed once
@functools.lru_cache(maxsize=None)
def case_a():
    N, src, dst = negative_ref.multigraph_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    return N, src, dst, nb, max(len(r) for r in nb), _store([(N, src, dst)])


@functools.lru_cache(maxsize=None)
def rows_a(iters, chunk=0):
    N, *_, store = case_a()
    with tuning(ppr_chunk=chunk):
        w = _rows(store, 0, np.arange(N), ALPHA, iters)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def case_star():
    N, src, dst = ref.star_case()
    return N, pair_score_ref.neighbourhoods(N, src, dst), _store([(N, src, dst)])


@functools.lru_cache(maxsize=None)
def case_big():
    N, src, dst = ref.random_connected_case()
    return N, pair_score_ref.neighbourhoods(N, src, dst), _store([(N, src, dst)])


# ---------------------------------------------------------------------------------------------------- the selection
@pytest.mark.parametrize('iters', [1, 2, 20])
def test_selection_is_exact_on_the_multigraph(iters):
    N, _, _, nb, _, store = case_a()
    rows = rows_a(iters)
    tot = None
    for k in (1, 3, N, 1024):
        want = ref.top_k(N, nb, np.arange(N), rows, k)
        assert_equal(_raw(store, 0, np.arange(N), k, ALPHA, iters), want, (iters, k))
        tot = want[2]
    if iters == 1:
        assert (tot == 0).all()                                                 # one step leaves the mass on the source and its neighbours: nobody is a candidate
    else:
        assert (tot[290:] == 0).all() and tot.max() > 100                       # isolated sources: nothing


def test_ties_cut_by_k_take_the_lowest_ids():
    N, nb, store = case_star()
    a = 5                                                                       # a leaf; leaf 1 carries the tail
    tied = np.array([w for w in range(2, 71) if w != a])
    row = _rows(store, 0, [a])[0]
    assert len(np.unique(bits(row[tied]))) == 1 and row[tied[0]] > 0            # the same expression for each: bitwise equal mass
    above = int((row[ref.candidates(N, nb, a, row)] > row[tied[0]]).sum())      # whatever comes above (leaf 1 and its tail, if they do)
    for k in (10, 3, 40, 70):
        gn, gs, gt = _raw(store, 0, [a], k)
        assert_equal((gn, gs, gt), ref.top_k(N, nb, [a], row[None], k), k)
        mine = [w for w in gn[0].tolist() if w in set(tied.tolist())]
        assert mine == tied[:len(mine)].tolist() and len(mine) == max(0, min(k - above, len(tied)))
    assert 0 < 10 - above < len(tied)                                           # k = 10 cuts the tie group


@pytest.mark.parametrize('cols', [64, 128])
def test_rounds_duplicates_and_sources_outside(cols):
    N, _, _, nb, _, store = case_a()
    rng = np.random.default_rng(5)
    sources = np.concatenate([rng.choice(290, 100, replace=False), [3, 3, 17], rng.integers(0, N, 25), [-1, N]])
    sources = sources[rng.permutation(len(sources))]
    assert len(sources) == 130 and 64 < len(np.unique(sources)) < 130           # duplicates; more than one round of 64 columns
    k = 9
    with tuning(ppr_cols=cols):
        got = _raw(store, 0, sources, k)
    for r, a in enumerate(sources.tolist()):
        one = _raw(store, 0, [a], k)                                            # the row of a one-source call
        assert np.array_equal(got[0][r], one[0][0]) and np.array_equal(bits(got[1][r]), bits(one[1][0])) and got[2][r] == one[2][0], (r, a)
        if not 0 <= a < N:
            assert got[2][r] == 0 and (got[0][r] == -1).all() and (bits(got[1][r]) == 0).all()
    inside = (sources >= 0) & (sources < N)
    assert_equal(tuple(x[inside] for x in got), ref.top_k(N, nb, sources[inside], rows_a(ITERS)[sources[inside]], k))


@pytest.mark.parametrize('chunk', [0, 1, 7, 2 ** 30])
def test_hub_cut_scores_carry_the_vector_calls_bits(chunk):
    N, _, _, nb, d_max, store = case_a()
    assert d_max > 200                                                          # a hub row: cut by 1 and by 7, whole at 2^30
    rows = rows_a(ITERS, chunk)
    with tuning(ppr_chunk=chunk):
        got = _raw(store, 0, np.arange(N), 12)
    assert_equal(got, ref.top_k(N, nb, np.arange(N), rows, 12), chunk)
    if chunk == 2 ** 30:
        assert not np.array_equal(bits(rows), bits(rows_a(ITERS, 7)))           # the cut does move low bits: the equality above is not vacuous


@pytest.mark.parametrize('k', [1, 1023, 1024])
def test_more_than_1024_survivors_and_ragged_n(k):
    N, nb, store = case_big()
    sources = [0, 1500, N - 1]
    rows = _rows(store, 0, sources)
    want = ref.top_k(N, nb, sources, rows, k)
    assert (want[2] > 1024).all() and N % 64 != 0
    assert_equal(_raw(store, 0, sources, k), want, k)


def test_against_float64():
    N, src, dst, nb, d_max, store = case_a()
    k = 25
    want = pagerank_ref.rooted_pagerank(N, src, dst, np.arange(N), ALPHA, ITERS, nb)
    gn, gs, gt = _raw(store, 0, np.arange(N), k)
    lim = pagerank_ref.bound(want, ITERS, d_max)
    clean = 0
    for a in range(N):
        cand = ref.candidates(N, nb, a, want[a])                               # the float64 candidate set
        ret = gn[a][gn[a] >= 0].astype(np.int64)
        assert (np.abs(gs[a][:len(ret)].astype(np.float64) - want[a][ret]) <= lim[a][ret]).all(), a
        assert set(ret.tolist()) <= set(cand.tolist()), a
        left = np.setdiff1d(cand, ret)
        if len(left) and len(ret):
            x = ret[np.argmin(want[a][ret])]
            assert (want[a][left] - lim[a][left] <= want[a][x] + lim[a][x]).all(), a
        elif len(left):
            assert (want[a][left] < 2.0 ** -100).all(), a
        if not ((want[a] > 0) & (want[a] < 2.0 ** -100)).any():
            clean += 1
            assert gt[a] == len(cand), a
    assert clean > 100                                                          # the case has rows without an entry near underflow


def test_isolated_source():
    N, *_, store = case_a()
    gn, gs, gt = _raw(store, 0, [295, 290, 299], 4)
    assert (gt == 0).all() and (gn == -1).all() and (bits(gs) == 0).all()


def test_two_streams_agree():
    N, src, dst, _, _, _ = case_a()
    store = _store([(N, src, dst)])                                             # fresh: the first call builds the index
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    sources = np.arange(0, N, 2)
    a = _raw(store, 0, sources, 16, stream=s1)
    b = _raw(store, 0, sources, 16, stream=s2)
    c = _raw(store, 0, sources, 16)
    for x in (b, c):
        assert np.array_equal(x[0], a[0]) and np.array_equal(bits(x[1]), bits(a[1])) and np.array_equal(x[2], a[2])
    assert_equal(a, ref.top_k(N, case_a()[3], sources, rows_a(ITERS)[sources], 16))


def test_bad_arguments_and_m_zero():
    from gmeta_amd import _lib
    N, *_, store = case_a()
    lib = _lib.lib()
    null, st = C.c_void_p(0), _lib.stream_ptr()
    assert lib.gm_store_pagerank_candidates(store.handle, 0, null, 0, 5, ALPHA, ITERS, null, null, null, st) == 0      # m == 0 with NULL pointers
    on, os_, ot = _raw(store, 0, [], 5)
    assert on.shape == (0, 5) and ot.shape == (0,)
    d_a = torch.zeros(4, dtype=torch.int32, device='cuda')
    o_n = torch.zeros((4, 1024), dtype=torch.int32, device='cuda')
    o_s = torch.zeros((4, 1024), dtype=torch.float32, device='cuda')
    o_t = torch.zeros(4, dtype=torch.int32, device='cuda')

    def call(g=0, m=4, k=5, alpha=ALPHA, iters=ITERS, a=_lib.ptr(d_a), n=_lib.ptr(o_n), s=_lib.ptr(o_s), t=_lib.ptr(o_t), h=store.handle):
        return lib.gm_store_pagerank_candidates(h, g, a, m, k, alpha, iters, n, s, t, st)
    bad = [(dict(g=1), 'graph 1'), (dict(g=-1), 'graph -1'), (dict(m=-1), 'm = -1'), (dict(m=2 ** 31), 'm = 2147483648'), (dict(k=0), 'k = 0'), (dict(k=1025), 'k = 1025'),
           (dict(k=-2), 'k = -2'), (dict(alpha=0.0), 'alpha = 0'), (dict(alpha=1.0), 'alpha = 1'), (dict(alpha=float('nan')), 'alpha = nan'), (dict(iters=0), 'iters = 0'),
           (dict(iters=256), 'iters = 256'), (dict(a=null), 'NULL argument'), (dict(n=null), 'NULL argument'), (dict(s=null), 'NULL argument'), (dict(t=null), 'NULL argument'),
           (dict(h=null), 'store is NULL')]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**kw), 'gm_store_pagerank_candidates')
    for knob, value, word in (('ppr_cols', 48, 'ppr_cols = 48'), ('ppr_chunk', -1, 'ppr_chunk = -1')):
        with tuning(**{knob: value}):
            with pytest.raises(ValueError, match=word):
                _lib.check(call(), 'gm_store_pagerank_candidates')
    assert call() == 0 and call(m=0) == 0 and call(k=1) == 0 and call(k=1024) == 0 and call(iters=255) == 0
    torch.cuda.synchronize()


def test_graphstore_method_and_candidate_names():
    import gmeta_amd
    from gmeta_amd import synth
    N, *_, store = case_a()
    nodes = [0, 17, 17, 295, 120]
    part, sc, tot = store.pagerank_candidates(0, nodes, k=7)
    raw = _raw(store, 0, nodes, 7)
    assert part.dtype == np.int64 and sc.dtype == f32 and tot.dtype == np.int64 and part.shape == sc.shape == (5, 7) and tot.shape == (5,)
    assert np.array_equal(part, raw[0]) and np.array_equal(bits(sc), bits(raw[1])) and np.array_equal(tot, raw[2])
    other = store.pagerank_candidates(0, nodes, k=7, alpha=0.3, iters=5)
    assert np.array_equal(bits(other[1]), bits(_raw(store, 0, nodes, 7, 0.3, 5)[1])) and not np.array_equal(bits(other[1]), bits(sc))
    empty = store.pagerank_candidates(0, [], k=3)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)
    assert not store.has_edges(0, [(a, w) for a, row in zip(nodes, part) for w in row if w >= 0]).any()      # candidates are never adjacent
    # partners further than two steps away do come back: link_candidates cannot propose them
    nb = case_a()[3]
    full = store.pagerank_candidates(0, nodes, k=1024)[0]
    assert any(set(row[row >= 0].tolist()) - set().union(*[nb[x] for x in nb[a]]) for a, row in zip(nodes, full))
    # candidate_names -> Subgraphs.query_batch
    G, n, F0, T, k = 2, 120, 5, 2, 6
    d = synth.link_dataset(G, n, 2, F0, seed=11, inject_negatives=False)
    st2 = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    np.random.seed(222); random.seed(222)
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=2, k_spt=2, k_qry=3, task_num=T, update_step=2, update_step_test=2, method='G-Meta', sample_nodes=20,
                              link_pred_mode='True', task_setup='Shared', h=2)
    db = gmeta_amd.Subgraphs(None, 'train', d['info'], n_way=2, k_shot=2, k_query=3, batchsz=T, args=args, adjs=st2, h=2, tables=d['tables'], verbose=False,
                             link_hops='symmetric', mask_target=True)
    names = []
    for g in range(G):
        src_nodes = [3, 40, 77]
        p, _, t = st2.pagerank_candidates(g, src_nodes, k=k)
        got = gmeta_amd.candidate_names(g, src_nodes, p)
        assert [len(nm) for nm in got] == np.minimum(t, k).tolist() and (t > 0).all()
        assert got[0] == ['%d_%d_%d' % (g, 3, w) for w in p[0] if w >= 0]
        names += got
    batch = db.query_batch(names)
    assert batch.sets == len(names) and batch.subs == sum(len(nm) for nm in names) and batch.centres == 2
