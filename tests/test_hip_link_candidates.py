"""GPU (-m gpu): gm_store_pair_candidates and the Python layers above it against the restatement of the definition (tests/candidate_ref.py; the definition
itself is in include/gmeta_hip.h).  The restatement is fed with the device's own GraphStore.pair_scores under the same pair_lanes, as the definition makes the
scores the bits of gm_store_pair_scores.  Everything is EQUAL: partner ids, score bits, totals.  No tolerance anywhere."""
import argparse
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

import candidate_ref as ref
import negative_ref
import pair_score_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
LANES = (0, 16, 32, 64)                      # 0: the library's choice
LDS_NODES = 262144                           # the largest graph whose membership bitmap lives in LDS (csrc/candidates.hip: GM_CAND_LDS_WORDS x 32)


def _store(graphs, weights=None, F=1):
    import gmeta_amd
    return gmeta_amd.GraphStore(graphs, [np.zeros((g[0], F), f32) for g in graphs], edge_weights=weights)


class tuning:
    """gm_set_tuning(name, value) for the length of the block."""

    def __init__(self, name, value):
        from gmeta_amd import _lib
        self.lib, self.name, self.value = _lib.lib(), name.encode(), value

    def __enter__(self):
        self.was = self.lib.gm_get_tuning(self.name)
        assert self.lib.gm_set_tuning(self.name, self.value) == 0

    def __exit__(self, *exc):
        self.lib.gm_set_tuning(self.name, self.was)
        return False


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _raw(store, g, nodes, k, col, stream=None):
    """The C ABI itself -> (nodes int32 [m, k], scores float32 [m, k], totals int32 [m]).  The row behind m is poisoned beforehand and must stay so."""
    from gmeta_amd import _lib
    a = np.ascontiguousarray(np.asarray(nodes, np.int64).reshape(-1), np.int32)
    m = len(a)
    d_a = torch.from_numpy(a).cuda() if m else None
    on = torch.full((m + 1, k), -7, dtype=torch.int32, device='cuda')
    os_ = torch.full((m + 1, k), -7.0, dtype=torch.float32, device='cuda')
    ot = torch.full((m + 1,), -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    st = _lib.stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_lib.lib().gm_store_pair_candidates(store.handle, g, _lib.ptr(d_a), m, k, col, _lib.ptr(on), _lib.ptr(os_), _lib.ptr(ot), st), 'gm_store_pair_candidates')
    torch.cuda.synchronize()
    on, os_, ot = on.cpu().numpy(), os_.cpu().numpy(), ot.cpu().numpy()
    assert (on[m:] == -7).all() and (os_[m:] == -7.0).all() and (ot[m:] == -7).all()      # nothing beyond row m - 1 is written
    return on[:m], os_[:m], ot[:m]


def assert_equal(got, want, what=''):
    gn, gs, gt = got
    wn, ws, wt = want
    assert gn.shape == wn.shape and gs.shape == ws.shape and gs.dtype == f32, what
    assert np.array_equal(gt.astype(np.int64), wt), what
    assert np.array_equal(gn.astype(np.int64), wn), what
    assert np.array_equal(bits(gs), bits(ws)), what
    pad = wn < 0
    assert (gn[pad] == -1).all() and (bits(gs)[pad] == 0).all(), what           # padding: -1 and +0.0f


class Case:
    """A graph, its store, sources, their candidate sets (restated) and the device's pair scores of all their pairs per pair_lanes value, computed once."""

    def __init__(self, graph, sources, store=None, g=0):
        self.N, self.src, self.dst = graph
        self.store = _store([graph]) if store is None else store
        self.g = g
        self.nb = pair_score_ref.neighbourhoods(self.N, self.src, self.dst)
        self.sources = [int(a) for a in sources]
        self.sets = [ref.candidates(self.N, self.src, self.dst, a, self.nb) for a in self.sources]
        self.pairs = ref.pairs_of(self.sources, self.sets)
        self._scores = {}

    def scores(self, lanes):
        if lanes not in self._scores:
            with tuning('pair_lanes', lanes):
                s = self.store.pair_scores(self.g, self.pairs)
            assert (s[:, 0] >= 1).all() and (s > 0).all() and np.isfinite(s).all()      # every candidate: cn >= 1, every score a positive finite fp32
            s.setflags(write=False)
            self._scores[lanes] = s
        return self._scores[lanes]

    def want(self, k, col, lanes=0):
        return ref.top_k(self.sources, self.sets, self.scores(lanes)[:, col], k)

    def got(self, k, col, lanes=0, **kw):
        with tuning('pair_lanes', lanes):
            return _raw(self.store, self.g, self.sources, k, col, **kw)


@functools.lru_cache(maxsize=None)
def case_multi():
    N, src, dst = negative_ref.multigraph_case()
    sources = list(range(N)) + [0, 0, 17, 299, -1, N, 1, 2 ** 31 - 1]           # duplicates, ids outside the graph
    c = Case((N, src, dst), sources)
    assert sum(len(s) for s in c.sets[:N]) == 65896 and sum(1 for s in c.sets[:N] if not s) == 10
    return c


@functools.lru_cache(maxsize=None)
def case_planted():
    N, src, dst, planted = pair_score_ref.planted_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    P = len(planted)
    near = [x for x in range(P, N) if 12 in nb[x]][::70][:40]                   # pool nodes next to the 3,000-entry hub (node 12) ...
    far = [x for x in range(P, N) if 12 not in nb[x] and nb[x]][:8]             # ... and pool nodes that are not
    assert len(near) == 40 and len(far) == 8
    c = Case((N, src, dst), list(planted) + near + far)
    sizes = [len(s) for s in c.sets]
    assert 2900 < max(sizes) <= 3014
    assert sum(1 for s in sizes if s > 1024) >= 40                              # the select sees more than 1,024 keys
    return c


# ---------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize('lanes', LANES)
def test_multigraph_every_source_every_column(lanes):
    c = case_multi()
    cn = c.scores(lanes)[:, 0]
    at = np.cumsum([0] + [len(s) for s in c.sets])
    assert all(len(np.unique(cn[at[r]:at[r + 1]])) < len(s) for r, s in enumerate(c.sets) if len(s) > 1)      # cn ties in every set
    for k in (1, 7, 300, 1024):
        for col in range(5):
            got = c.got(k, col, lanes)
            assert_equal(got, c.want(k, col, lanes), 'multigraph lanes %d k %d col %d' % (lanes, k, col))
            if k in (7, 1024):
                again = c.got(k, col, lanes)
                assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, again))      # two runs, bit for bit
    n, s, t = c.got(7, 2, lanes)
    N = c.N
    assert np.array_equal(n[0], n[N]) and np.array_equal(n[0], n[N + 1]) and np.array_equal(bits(s[17]), bits(s[N + 2]))      # duplicate sources: independent, equal rows
    assert t[N + 4] == t[N + 5] == t[N + 7] == 0 and (n[[N + 4, N + 5, N + 7]] == -1).all()                                  # ids -1, N, 2^31 - 1: C is empty


@pytest.mark.parametrize('k', [1, 64, 1024])
def test_planted_rows_across_the_hub(k):
    c = case_planted()
    for col, lanes in ((0, 0), (2, 0), (1, 16), (3, 64), (4, 32)):
        assert_equal(c.got(k, col, lanes), c.want(k, col, lanes), 'planted k %d col %d lanes %d' % (k, col, lanes))
    cn = c.scores(0)[:, 0]
    assert np.bincount(cn.astype(np.int64)).max() > 2000                        # thousands of equal cn scores behind one select


def test_dense_case_pads():
    N, src, dst = negative_ref.dense_case()
    c = Case((N, src, dst), range(N))
    assert sorted({len(s) for s in c.sets}) == [5, 6]
    for col in range(5):
        got = c.got(8, col)
        assert_equal(got, c.want(8, col), 'dense col %d' % col)
        assert (got[0][:, 6:] == -1).all() and (got[1][:, 6:] == 0).all()


def test_word_boundaries():
    N, src, dst = ref.word_boundary_case()
    c = Case((N, src, dst), range(N))
    assert N % 32 and c.sets[5] == [0, 32, 63, 69]
    for k in (1, 4, 70):
        for col in (0, 2):
            assert_equal(c.got(k, col), c.want(k, col), 'words k %d col %d' % (k, col))
    for home in (1, 2):
        with tuning('cand_bitmap', home):
            assert_equal(c.got(70, 0), c.want(70, 0), 'words, bitmap home %d' % home)


def test_rounds_change_nothing():
    """cand_round 1: every source with candidates is a round of its own; 2998: each pool node next to the hub exceeds the budget alone, the short rows share
    rounds; 4096: several sources a round (no set of this 3,213-node graph reaches 4,096 keys); 0: one round."""
    c = case_planted()
    sizes = [len(s) for s in c.sets]
    assert sum(1 for s in sizes if s > 2998) >= 40 and sum(sizes[:9]) < 2998 and max(sizes) < 4096
    base = c.got(64, 2)
    assert_equal(base, c.want(64, 2), 'planted, default round')
    for budget in (1, 2998, 4096):
        with tuning('cand_round', budget):
            got = c.got(64, 2)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, base)), budget
    with tuning('cand_round', 1):
        m = case_multi()
        assert_equal(m.got(7, 1), m.want(7, 1), 'multigraph, one source a round')


def test_bitmap_home_changes_nothing():
    c = case_multi()
    base = c.got(300, 3)
    for home in (1, 2):
        with tuning('cand_bitmap', home):
            got = c.got(300, 3)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, base)), home
    with tuning('cand_bitmap', 2):
        p = case_planted()
        assert_equal(p.got(64, 0), p.want(64, 0), 'planted, HBM slab')


def test_graph_just_above_the_lds_bound():
    """N = bound + 40: a few hundred edges among the 48 highest ids (the last bitmap words, the last one partial) and two long-range edges to node 0."""
    from gmeta_amd import _lib
    rng = np.random.default_rng(8)
    N = LDS_NODES + 40
    assert N % 32 != 0
    top = np.arange(N - 48, N)
    src = np.concatenate([rng.choice(top, 300), [0, N - 1]]).astype(np.int64)
    dst = np.concatenate([rng.choice(top, 300), [N - 3, 0]]).astype(np.int64)
    c = Case((N, src, dst), list(top) + [0, 1, N // 2, N])
    assert sum(len(s) for s in c.sets) > 500 and c.sets[-4] and not c.sets[-3] and not c.sets[-1]
    for k, col in ((8, 2), (64, 0)):
        assert_equal(c.got(k, col), c.want(k, col), 'above the LDS bound, auto')
    with tuning('cand_bitmap', 2):
        assert_equal(c.got(8, 2), c.want(8, 2), 'above the LDS bound, HBM forced')
    with tuning('cand_bitmap', 1):
        with pytest.raises(ValueError, match=r'cand_bitmap = 1 \(LDS\).*%d nodes' % N):
            c.got(8, 2)
    # at the bound itself the graph still fits
    Nb = LDS_NODES
    cb = Case((Nb, np.minimum(src, Nb - 1), np.minimum(dst, Nb - 1)), [Nb - 1, Nb - 2, 0])
    with tuning('cand_bitmap', 1):
        assert_equal(cb.got(8, 2), cb.want(8, 2), 'at the LDS bound, LDS forced')
    assert _lib.lib().gm_get_tuning(b'cand_bitmap') == 0


def test_third_graph_of_a_store_and_a_weighted_store():
    rng = np.random.default_rng(2)
    g0 = (50, rng.integers(0, 50, 333).astype(np.int64), rng.integers(0, 50, 333).astype(np.int64))
    g1 = (7, np.array([0, 1, 5], np.int64), np.array([1, 2, 5], np.int64))
    m = case_multi()
    g2 = (m.N, m.src, m.dst)
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(m.src))).astype(f32)
    base = m.got(7, 2)
    for wts in (None, [np.ones(len(g0[1]), f32), np.ones(3, f32), w]):
        store = _store([g0, g1, g2], weights=wts)
        assert store.weighted == (wts is not None)
        got = _raw(store, 2, m.sources, 7, 2)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, base))      # offsets and weights change nothing
        c1 = Case(g1, range(-1, 8), store=store, g=1)
        assert c1.sets[1] == [2] and c1.sets[3] == [0]                        # sources -1, 0, 1, 2, ...: 0 - 1 - 2 is a path
        assert_equal(c1.got(3, 0), c1.want(3, 0), 'graph 1 of 3')
        c0 = Case(g0, range(50), store=store, g=0)
        assert_equal(c0.got(5, 3), c0.want(5, 3), 'graph 0 of 3')


def test_two_streams_on_a_fresh_store_against_one():
    """The neighbour index is built by the first call (here on s1); the second stream reads it with no event between them."""
    m = case_multi()
    store = _store([(m.N, m.src, m.dst)])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = _raw(store, 0, m.sources, 7, 2, stream=s1)
    b = _raw(store, 0, m.sources, 7, 2, stream=s2)
    with torch.cuda.stream(s2):
        d = store.link_candidates(0, m.sources[:m.N], k=7)
    want = m.got(7, 2)
    for x in (a, b):
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(x, want))
    assert np.array_equal(d[0], want[0][:m.N]) and np.array_equal(bits(d[1]), bits(want[1][:m.N])) and np.array_equal(d[2], want[2][:m.N])


def test_bad_arguments_and_m_zero():
    from gmeta_amd import _lib
    c = case_multi()
    store, lib = c.store, _lib.lib()
    d_a = torch.zeros(4, dtype=torch.int32, device='cuda')
    on = torch.zeros((4, 1024), dtype=torch.int32, device='cuda')
    os_ = torch.zeros((4, 1024), dtype=torch.float32, device='cuda')
    ot = torch.zeros(4, dtype=torch.int32, device='cuda')

    def call(g=0, m=4, k=5, col=2, a=d_a, n=on, s=os_, t=ot):
        return lib.gm_store_pair_candidates(store.handle, g, _lib.ptr(a), m, k, col, _lib.ptr(n), _lib.ptr(s), _lib.ptr(t), _lib.stream_ptr())

    bad = [(dict(g=1), 'graph 1'), (dict(g=-1), 'graph -1'), (dict(m=-1), 'm = -1'), (dict(m=2 ** 31), 'm = 2147483648'), (dict(k=0), 'k = 0'), (dict(k=1025), 'k = 1025'),
           (dict(col=-1), 'col = -1'), (dict(col=5), 'col = 5'), (dict(a=None), 'NULL'), (dict(n=None), 'NULL'), (dict(s=None), 'NULL'), (dict(t=None), 'NULL')]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**kw), 'gm_store_pair_candidates')
    for name, value, word in (('pair_lanes', 8, 'pair_lanes = 8'), ('cand_bitmap', 3, 'cand_bitmap = 3'), ('cand_round', -1, 'cand_round = -1')):
        with tuning(name, value):
            with pytest.raises(ValueError, match=word):
                _lib.check(call(), 'gm_store_pair_candidates')
    assert call(m=0) == 0 and call(m=0, a=None, n=None, s=None, t=None) == 0     # m == 0: a no-op
    assert call() == 0 and call(k=1024, col=4) == 0
    assert _raw(store, 0, [], 5, 2)[0].shape == (0, 5)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- Python, and the path through the model
def test_link_candidates_equals_the_c_abi():
    import gmeta_amd
    c = case_multi()
    nodes = c.sources[:c.N]
    for k, score in ((10, 'adamic_adar'), (3, 'cn'), (40, 'jaccard'), (1024, 'pref_attachment'), (5, 'resource_allocation')):
        part, sc, tot = c.store.link_candidates(0, nodes, k=k, score=score)
        n, s, t = _raw(c.store, 0, nodes, k, gmeta_amd.PAIR_SCORES.index(score))
        assert part.dtype == np.int64 and sc.dtype == f32 and tot.dtype == np.int64 and part.shape == sc.shape == (c.N, k) and tot.shape == (c.N,)
        assert np.array_equal(part, n) and np.array_equal(bits(sc), bits(s)) and np.array_equal(tot, t)
    part, sc, tot = c.store.link_candidates(0, nodes)                           # the defaults: k = 10, Adamic-Adar
    assert_equal((part, sc, tot), ref.top_k(nodes, c.sets[:c.N], c.scores(0)[:len(ref.pairs_of(nodes, c.sets[:c.N])), 2], 10), 'defaults')
    e = c.store.link_candidates(0, [], k=4)
    assert e[0].shape == (0, 4) and e[1].shape == (0, 4) and e[2].shape == (0,)
    with pytest.raises(ValueError, match='outside'):
        c.store.link_candidates(0, [c.N])
    with pytest.raises(ValueError, match='score'):
        c.store.link_candidates(0, [1], score='katz')
    with pytest.raises(ValueError, match='k = 0'):
        c.store.link_candidates(0, [1], k=0)


def test_candidates_through_query_batch_and_predict():
    """link_candidates -> candidate_names -> Subgraphs.query_batch -> Adapted.predict: finite log-probabilities of the right shapes, equal to predict on the
    same names written out by hand."""
    import gmeta_amd
    from gmeta_amd import synth
    G, n, F0, T, k = 3, 120, 5, 3, 6
    d = synth.link_dataset(G, n, 2, F0, seed=11, inject_negatives=False)
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    np.random.seed(222); random.seed(222)
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=2, k_spt=2, k_qry=3, task_num=T, update_step=2, update_step_test=2, method='G-Meta', sample_nodes=20,
                              link_pred_mode='True', task_setup='Shared', h=2)
    db = gmeta_amd.Subgraphs(None, 'train', d['info'], n_way=2, k_shot=2, k_query=3, batchsz=T, args=args, adjs=store, h=2, tables=d['tables'], verbose=False,
                             link_hops='symmetric', mask_target=True)
    batch = db.get_batch(list(range(T)))
    torch.manual_seed(3)
    maml = gmeta_amd.Meta(args, synth.make_config(F0, 16, 2, 2, link=True)).to('cuda')
    ad = maml.adapt(batch[0], batch[1])
    names, tasks, hand = [], [], []
    for g in range(G):
        nodes = [3, 40, 77]
        part, sc, tot = store.link_candidates(g, nodes, k=k)
        assert (tot > 0).all() and ((part >= 0).sum(1) == np.minimum(tot, k)).all()
        got = gmeta_amd.candidate_names(g, nodes, part)
        for a, row, nm in zip(nodes, part, got):
            assert nm == ['%d_%d_%d' % (g, a, w) for w in row if w >= 0] and len(nm) == min(k, tot[nodes.index(a)])
            assert not store.has_edges(g, [(a, w) for w in row if w >= 0]).any()      # candidates are never adjacent
        names += got; tasks += [g % T] * len(got)
        hand += [['%d_%d_%d' % (g, a, int(w)) for w in row.tolist() if w >= 0] for a, row in zip(nodes, part)]
    pr = ad.predict(db.query_batch(names), tasks=tasks)
    assert [lp.shape for lp in pr.log_probs] == [(len(nm), 2) for nm in names] and [len(p) for p in pr.pred] == [len(nm) for nm in names]
    assert all(np.isfinite(lp).all() and (lp <= 0).all() for lp in pr.log_probs)
    by_hand = ad.predict(db.query_batch(hand), tasks=tasks)
    for x, y in zip(pr.log_probs, by_hand.log_probs):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert all(np.array_equal(x, y) for x, y in zip(pr.pred, by_hand.pred))
