"""GPU (-m gpu): target-link masking in the pair-subgraph extraction (link_pred | GM_LINK_MASK_TARGET) against its restatement out of the oracle's pieces
(tests/link_mask_ref.py): node lists, both CSR orientations, centres and norms bit for bit through the C ABI -- random multigraphs with planted pairs,
the boundaries of the two adjacency walkers, every launch shape, weighted stores, hop labels, concatenation -- the whole meta-step on every schedule
within the project's 1e-4, and the Python surface.  Every extraction case checks that the mask had work to do, so an unmasked build fails."""
import argparse
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, ROOT)
import gmeta_oracle as orc      # noqa: E402
import edge_weight_ref as ewr   # noqa: E402
import hop_label_ref as hop     # noqa: E402
import link_mask_ref as ref     # noqa: E402
import link_sym_ref as sym      # noqa: E402
import readout_ref as ro        # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4                       # the project's tolerance on losses / meta-gradients (README; tests/test_hip_fuzz.py)
M = ref.MASK
f32 = np.float32
# (field, dtype): every GM_F_* field an unlabelled, unweighted batch has -- floats compared as bit patterns
FIELDS = ((0, np.int32), (1, np.int32), (2, np.int32), (3, np.int32), (4, np.int32), (5, np.int32), (6, np.int32), (7, np.int32), (8, np.int32),
          (9, np.uint32), (10, np.int32), (11, np.uint32), (12, np.uint32), (16, np.uint32), (17, np.int32))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _count(B, field):
    return {0: B.subs + 1, 1: B.sets + 1, 2: B.rows, 3: B.subs, 4: B.rows + 1, 5: B.edges, 6: B.rows + 1, 7: B.edges, 8: B.subs * B.centres, 9: B.rows,
            10: B.rows, 11: B.rows, 12: B.rows, 13: B.edges, 14: B.edges, 16: B.rows, 17: B.edges}[field]


def _field(B, field, dt):
    from gmeta_amd import _lib
    x = np.empty(_count(B, field), dt)
    assert _lib.lib().gm_batch_read(B.handle, field, _lib.ptr(x), x.nbytes) == 0, field
    return x


def assert_bitwise_equal(one, two, weighted=False):
    assert (one.rows, one.edges, one.subs, one.sets, one.centres, one.mask_target) == (two.rows, two.edges, two.subs, two.sets, two.centres, two.mask_target)
    for field, dt in FIELDS + (((13, np.uint32), (14, np.uint32)) if weighted else ()):
        assert np.array_equal(_field(one, field, dt), _field(two, field, dt)), field


def _store(graphs, weights=None, F=3):
    import gmeta_amd
    return gmeta_amd.GraphStore(graphs, [np.zeros((g[0], F), f32) for g in graphs], edge_weights=weights)


def _extract(store, seeds, h, sample_n, mode, off=None):
    from gmeta_amd.subgraphs import SubgraphBatch
    seeds = np.asarray(seeds, np.int32)
    return SubgraphBatch.extract(store, seeds, [0, len(seeds)] if off is None else off, h, sample_n, ref.RNG_SEED, mode)


def assert_matches(B, ob):
    """A device batch against ONE restated batch over the same subgraphs, bit for bit: parent, both CSR orientations, centres, norm; indptr[-1] == edges;
    every index inside its own subgraph's row range.  Weighted restatements: both weight arrays too."""
    assert B.mask_target and B.centres == 2
    assert np.array_equal(B.parent(), ob.parent)
    sub = B.sub_off
    assert np.array_equal(sub, ob.sub_off)
    tp, td = orc._by_source(ob)
    for (ip, ix), (wp, wx) in ((B.csr(), (ob.indptr, ob.indices)), (B.csr(True), (tp, td))):
        assert ip[0] == 0 and ip[-1] == B.edges == len(wx)
        assert np.array_equal(ip, wp) and np.array_equal(ix, wx)
        row = np.repeat(np.arange(B.rows), np.diff(ip))
        s = np.searchsorted(sub, row, 'right') - 1
        assert ((ix >= sub[s]) & (ix < sub[s + 1])).all()
    assert np.array_equal(_field(B, 8, np.int32), (ob.centre_rows - ob.sub_off[:-1, None]).reshape(-1))
    assert np.array_equal(_field(B, 9, np.uint32), _bits(ref.header_norm(ob)))      # (the header's two IEEE operations on the restated degrees: link_mask_ref.header_norm)
    if hasattr(ob, 'ew'):
        assert B.weighted
        assert np.array_equal(_field(B, 13, np.uint32), _bits(ob.ew)) and np.array_equal(_field(B, 14, np.uint32), _bits(ob.by_source()[2]))


def rows_of(B, transposed=False):
    """Per row: its neighbour list as local indices of its subgraph."""
    ip, ix = B.csr(transposed)
    sub = B.sub_off
    s = np.searchsorted(sub, np.arange(B.rows), 'right') - 1
    return [tuple((ix[ip[r]:ip[r + 1]] - sub[s[r]]).tolist()) for r in range(B.rows)]


def assert_only_the_target_changed(Bm, Bu, og, seeds):
    """Against the unmasked batch of the same seeds: parent identical; every non-centre row identical in both orientations; the subgraphs of the
    non-adjacent pairs bitwise the unmasked ones; the adjacent ones lose exactly their target edges."""
    assert Bm.mask_target and not Bu.mask_target
    assert np.array_equal(Bm.parent(), Bu.parent()) and np.array_equal(Bm.sub_off, Bu.sub_off)
    sub = Bm.sub_off
    cen = _field(Bm, 8, np.int32).reshape(-1, 2) + sub[:-1, None]
    assert np.array_equal(_field(Bu, 8, np.int32).reshape(-1, 2) + sub[:-1, None], cen)
    centre = np.zeros(Bm.rows, bool); centre[cen.reshape(-1)] = True
    for t in (False, True):
        rm, ru = rows_of(Bm, t), rows_of(Bu, t)
        assert all(a == b for a, b, c in zip(rm, ru, centre) if not c)
        ipm, ipu = Bm.csr(t)[0], Bu.csr(t)[0]
        for k, (g, i, j) in enumerate(np.asarray(seeds).tolist()):
            lost = (ipu[sub[k + 1]] - ipu[sub[k]]) - (ipm[sub[k + 1]] - ipm[sub[k]])
            assert lost == ref.adjacent(og[g], i, j), (k, g, i, j)
            if lost == 0:
                assert rm[sub[k]:sub[k + 1]] == ru[sub[k]:sub[k + 1]]
    nm, nu = _field(Bm, 9, np.uint32), _field(Bu, 9, np.uint32)
    assert np.array_equal(nm[~centre], nu[~centre])


# ---------------------------------------------------------------------------------------------------- 1. integer work, random multigraphs
@functools.lru_cache(maxsize=None)
def fuzz(seed):
    return ref.fuzz_case(seed)


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('seed', sym.FUZZ_SEEDS)
def test_random_multigraphs_with_planted_pairs(seed, mode):
    c = fuzz(seed)                                       # (fuzz_case asserts every planted property on the generated parent)
    store = _store(c['graphs'])
    B = _extract(store, c['seeds'], c['h'], c['sample_n'], mode | M)
    assert_matches(B, ref.extract_batch(c['og'], c['seeds'], c['h'], c['sample_n'], mode))
    assert_only_the_target_changed(B, _extract(store, c['seeds'], c['h'], c['sample_n'], mode), c['og'], c['seeds'])


# ---------------------------------------------------------------------------------------------------- 2. walker boundaries, hand-built graphs
# (deg, positions of J in I's list, side, further in-edges of J); the group walker takes 32 ids per iteration, the wave walker (degree > 256) 256
GROUP = [(40, (31, 32), 'in', 0), (40, (0,), 'in', 0), (40, (39,), 'in', 0)]
WAVE = [(300, (10,), 'in', 0), (300, (255, 256), 'in', 0), (300, (299,), 'in', 0), (300, (10,), 'in', 280)]          # (the last: both centres hubs)
SPREAD = [(40, (0, 31, 32, 39), 'in', 0), (300, (10, 255, 256, 299), 'in', 0), (300, (10, 255, 256, 299), 'out', 0)]  # parallel copies apart: directed stores only


# (a symmetric store keeps its rows ascending: parallel copies are adjacent and there is no separate out-list, so SPREAD runs on directed stores only)
BOUNDARIES = [c + (sym_,) for c in GROUP + WAVE for sym_ in (True, False)] + [c + (False,) for c in SPREAD]


@pytest.mark.parametrize('deg,positions,side,j_extra,symmetric', BOUNDARIES)
def test_walker_boundaries(deg, positions, side, j_extra, symmetric):
    from gmeta_amd.subgraphs import SubgraphBatch
    g, I, J = ref.boundary_graph(deg, positions, symmetric, side, j_extra)
    assert ref.list_positions(g, I, J, side) == list(positions)
    G = orc.Graph(*g)
    store = _store([g])
    assert store.symmetric() == symmetric
    hub = lambda v: max(len(G.preds(v)), int((np.asarray(g[1]) == v).sum())) > ref.EX_BIG_DEG      # noqa: E731
    assert hub(I) == (deg > ref.EX_BIG_DEG) and hub(J) == (j_extra > ref.EX_BIG_DEG)
    seeds = np.array([(0, I, J), (0, J, I), (0, I, I), (0, J, J), (0, I, 5 if 5 not in (I, J) else 6)], np.int32)      # a hub j with a non-hub i: (J, I)
    for mode in ref.MODES:
        B = _extract(store, seeds, 1, 10000, mode | M)
        assert_matches(B, ref.extract_batch([G], seeds, 1, 10000, mode))
        assert_only_the_target_changed(B, _extract(store, seeds, 1, 10000, mode), [G], seeds)
    # every node inside: each of the walked list's entries is a hit but the target's (gm_batch_from_nodes, the masked count and fill of given lists)
    lists = [np.arange(g[0], dtype=np.int32)] * 2
    B = SubgraphBatch.from_nodes(store, seeds[:2], [0, 2], lists, True, mask_target=True)
    ob = ref.batch_from_lists([G], seeds[:2], lists)
    assert_matches(B, ob)
    assert B.edges == 2 * (len(g[1]) - len(positions) * (2 if symmetric else 1))


def test_centre_rows_left_without_an_edge_have_norm_one():
    """a -> b is b's only in-edge and a has none: under the mask both centre rows end with degree 0 and the norm clamps to 1."""
    g = (6, np.array([0, 2, 3], np.int64), np.array([1, 3, 2], np.int64))
    G = orc.Graph(*g)
    store = _store([g])
    seeds = np.array([(0, 0, 1), (0, 1, 0), (0, 2, 3)], np.int32)
    for mode in ref.MODES:
        B = _extract(store, seeds, 2, 100, mode | M)
        assert_matches(B, ref.extract_batch([G], seeds, 2, 100, mode))
        assert B.edges == 0 and B.rows == 6
        assert np.array_equal(_field(B, 9, np.uint32), _bits(np.ones(6, f32)))
        assert _extract(store, seeds, 2, 100, mode).edges == 4


# ---------------------------------------------------------------------------------------------------- 3. launch shapes
def test_32_bit_prefix_words_on_a_70k_node_graph():
    """sample_nodes = 70,000: a subgraph may hold 65,536 nodes or more, so the prefix words are 32-bit (the LDS kernels' other shape)."""
    rng = np.random.default_rng(17)
    n = 70_000
    src, dst = rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)
    g = (n, src.astype(np.int64), dst.astype(np.int64))
    G = orc.Graph(*g)
    pick = rng.choice(2 * n, 6, replace=False)
    seeds = np.array([(0, int(src[k]), int(dst[k])) for k in pick] + [(0, int(dst[pick[0]]), int(src[pick[0]])), (0, 11, 12)], np.int32)
    assert sum(ref.adjacent(G, i, j) > 0 for _, i, j in seeds.tolist()) >= 7
    store = _store([g])
    for mode in ref.MODES:
        B = _extract(store, seeds, 3, 70_000, mode | M)
        assert_matches(B, ref.extract_batch([G], seeds, 3, 70_000, mode))


def test_global_bitmap_path_on_a_800k_node_graph():
    c = sym.large_case()
    n, src, dst = c['graphs'][0]
    G = orc.Graph(n, src, dst)
    rng = np.random.default_rng(5)
    pick = rng.choice(len(src), 8, replace=False)
    seeds = np.array([(0, int(src[k]), int(dst[k])) for k in pick], np.int32)          # eight existing edges (the graph stores both directions)
    seeds[6] = (0, int(src[pick[6]]), 1) if ref.adjacent(G, int(src[pick[6]]), 1) else seeds[6]
    assert all(ref.adjacent(G, i, j) >= 2 for _, i, j in seeds.tolist())
    store = _store(c['graphs'], F=4)
    for mode in ref.MODES:
        B = _extract(store, seeds, c['h'], c['sample_n'], mode | M)
        assert_matches(B, ref.extract_batch([G], seeds, c['h'], c['sample_n'], mode))


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('seed', [1, 5])
def test_joint_build_equals_two_builds(seed, mode):
    from gmeta_amd.subgraphs import SubgraphBatch
    c = fuzz(seed)
    store = _store(c['graphs'])
    sa, sb = c['seeds'][:9], c['seeds'][9:]
    oa, ob = [0, 1, 9], [0, 4, len(sb)]
    A1, B1 = _extract(store, sa, c['h'], c['sample_n'], mode | M, oa), _extract(store, sb, c['h'], c['sample_n'], mode | M, ob)
    A2, B2 = SubgraphBatch.extract_pair(store, sa, oa, sb, ob, c['h'], c['sample_n'], ref.RNG_SEED, mode | M)
    assert_matches(B2, ref.extract_batch(c['og'], sb, c['h'], c['sample_n'], mode))
    assert_bitwise_equal(A1, A2)
    assert_bitwise_equal(B1, B2)


@pytest.mark.parametrize('seed', [6, 7, 8])
def test_given_node_lists_with_the_mask_bit_equal_the_extraction(seed):
    """gm_batch_from_nodes reads bit 2 as the mask (any other non-zero bit: pairs), on the unsampled cases: bitwise gm_extract's batch."""
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    import ctypes as C
    c = fuzz(seed)
    assert c['sample_n'] == 10000
    store = _store(c['graphs'])
    for mode in ref.MODES:
        E = _extract(store, c['seeds'], c['h'], c['sample_n'], mode | M)
        lists = ref.node_lists(c['og'], c['seeds'], c['h'], c['sample_n'], mode)
        assert_bitwise_equal(E, SubgraphBatch.from_nodes(store, c['seeds'], [0, len(c['seeds'])], lists, True, mask_target=True))
        # the C ABI itself, with the mode's own value beside the bit
        flat = np.ascontiguousarray(np.concatenate(lists), np.int32)
        off = np.ascontiguousarray(np.cumsum([0] + [len(x) for x in lists]), np.int64)
        so = np.array([0, len(lists)], np.int32)
        arr = np.ascontiguousarray(c['seeds'], np.int32)
        out = C.c_void_p()
        _lib.check(_lib.lib().gm_batch_from_nodes(store.handle, _lib.ptr(arr), len(arr), _lib.ptr(so), 1, _lib.ptr(flat), _lib.ptr(off), mode | M, _lib.stream_ptr(),
                                                  C.byref(out)), 'gm_batch_from_nodes')
        assert_bitwise_equal(E, SubgraphBatch(out, store))
    assert not SubgraphBatch.from_nodes(store, c['seeds'], [0, len(c['seeds'])], lists, True).mask_target


# ---------------------------------------------------------------------------------------------------- 4. weights
@pytest.mark.parametrize('mode,seed', [(1, 4), (2, 5)])
def test_weighted_random_multigraphs(mode, seed):
    c = fuzz(seed)
    wg, wog = ref.weighted(c)
    store = _store(wg)
    assert store.weighted
    B = _extract(store, c['seeds'], c['h'], c['sample_n'], mode | M)
    assert_matches(B, ref.extract_batch(wog, c['seeds'], c['h'], c['sample_n'], mode))
    # all weights 1: the unweighted masked floats, bit for bit
    unit = _store(c['graphs'], weights=[np.ones(len(g[1]), f32) for g in c['graphs']])
    U, P = _extract(unit, c['seeds'], c['h'], c['sample_n'], mode | M), _extract(_store(c['graphs']), c['seeds'], c['h'], c['sample_n'], mode | M)
    assert U.weighted and not P.weighted
    assert_bitwise_equal(U, P)
    assert np.array_equal(_field(U, 13, np.uint32), _bits(np.ones(U.edges, f32))) and np.array_equal(_field(U, 14, np.uint32), _bits(np.ones(U.edges, f32)))


@pytest.mark.parametrize('symmetric', [True, False], ids=['symmetric_store', 'directed_store'])
def test_weighted_hub_row(symmetric):
    """The 300-degree centre on a weighted store: the wave walker moves the surviving weights to their new slots (a symmetric store: both orientations
    from the one walk)."""
    from gmeta_amd import synth
    g, I, J = ref.boundary_graph(300, (255, 256), symmetric)
    if symmetric:
        gw = synth.with_edge_weights([g], seed=3, symmetric=True)[0]
    else:
        gw = (g[0], g[1], g[2], np.exp(np.random.default_rng(2).uniform(np.log(0.25), np.log(4.0), len(g[1]))).astype(f32))
    store = _store([gw])
    assert store.weighted and store.symmetric() == symmetric
    G = ewr.Graph(*gw)
    seeds = np.array([(0, I, J), (0, J, I), (0, I, 7)], np.int32)
    for mode in ref.MODES:
        B = _extract(store, seeds, 1, 10000, mode | M)
        assert_matches(B, ref.extract_batch([G], seeds, 1, 10000, mode))


# ---------------------------------------------------------------------------------------------------- 5. composition
def _hop_extract(store, seeds, h, sample_n, mode, D, off=None):
    import gmeta_amd
    with gmeta_amd.hop_labels_switch(D):
        return _extract(store, seeds, h, sample_n, mode, off)


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('seed', [0, 4, 8])
def test_hop_labels_come_from_the_masked_csr(seed, mode):
    c = fuzz(seed)
    store = _store(c['graphs'])
    B = _hop_extract(store, c['seeds'], c['h'], c['sample_n'], mode | M, 3)
    ob = ref.extract_batch(c['og'], c['seeds'], c['h'], c['sample_n'], mode)
    assert_matches(B, ob)
    assert B.hop_labels_cap == 3 and np.array_equal(B.hop_labels, hop.labels(ob, 3))


@pytest.mark.parametrize('mode', ref.MODES)
def test_hop_labels_leak_the_link_only_without_the_mask(mode):
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    names, labels = d['tables']['train']
    seeds = np.array([[int(x) for x in nm.split('_')] for nm in names], np.int32)
    y = np.array([int(l) for l in labels])
    assert (seeds[:, 1] != seeds[:, 2]).all() and 0 < y.sum() < len(y)
    store = _store(d['graphs'])
    for sample_n in (8, 10000):
        Bu, Bm = _hop_extract(store, seeds, 2, sample_n, mode, 3), _hop_extract(store, seeds, 2, sample_n, mode | M, 3)
        cen = _field(Bm, 8, np.int32).reshape(-1, 2) + Bm.sub_off[:-1, None]
        lu, lm = Bu.hop_labels, Bm.hop_labels
        assert np.array_equal((lu[cen[:, 0], 1] == 1) | (lu[cen[:, 1], 0] == 1), y == 1)
        assert (lm[cen[:, 0], 1] != 1).all() and (lm[cen[:, 1], 0] != 1).all()


def test_concat_carries_the_flag_and_refuses_a_mix():
    from gmeta_amd.subgraphs import SubgraphBatch
    c = fuzz(3)
    store = _store(c['graphs'])
    k = 9
    for mode in ref.MODES:
        one = _extract(store, c['seeds'], c['h'], c['sample_n'], mode | M, [0, k, len(c['seeds'])])
        a, b = _extract(store, c['seeds'][:k], c['h'], c['sample_n'], mode | M), _extract(store, c['seeds'][k:], c['h'], c['sample_n'], mode | M)
        cat = SubgraphBatch.concat([a, b])
        assert cat.mask_target
        assert_bitwise_equal(cat, one)
        plain = _extract(store, c['seeds'][k:], c['h'], c['sample_n'], mode)
        with pytest.raises(ValueError, match='GM_LINK_MASK_TARGET'):
            SubgraphBatch.concat([a, plain])
        with pytest.raises(ValueError, match='GM_LINK_MASK_TARGET'):
            SubgraphBatch.concat([plain, b])
        assert not SubgraphBatch.concat([plain, _extract(store, c['seeds'][:k], c['h'], c['sample_n'], mode)]).mask_target


def test_the_flag_alone_is_refused_with_its_reason():
    from gmeta_amd.subgraphs import SubgraphBatch
    c = fuzz(4)
    store = _store(c['graphs'])
    nodes = np.array([(0, 3, -1), (0, 4, -1)], np.int32)
    with pytest.raises(ValueError, match='node seeds have no target link'):
        _extract(store, nodes, 2, 40, M)
    with pytest.raises(ValueError, match='node seeds have no target link'):
        _extract(store, c['seeds'], 2, 40, M)
    with pytest.raises(ValueError, match='node seeds have no target link'):
        SubgraphBatch.extract_pair(store, nodes, [0, 2], nodes, [0, 2], 2, 40, ref.RNG_SEED, M)
    with pytest.raises(ValueError, match='no target link'):
        SubgraphBatch.from_nodes(store, nodes, [0, 2], [np.arange(5)] * 2, False, mask_target=True)
    for bad in (3 | M, 8, 8 | M, -1):
        with pytest.raises(ValueError, match='mode'):
            _extract(store, c['seeds'], 2, 40, bad)
    with pytest.raises(ValueError, match='symmetric'):
        _extract(store, c['seeds'], 4, 40, 2 | M)
    assert _extract(store, c['seeds'], 9, 40, 1 | M).mask_target          # reference pairs ignore h, masked or not


# ---------------------------------------------------------------------------------------------------- 6. whole path
SCHEDULES = (('dense', {}), ('hoist_z1', dict(hoist_z1=1)), ('sparse_bwd', dict(sparse_bwd=1)), ('cone', dict(cone=1)), ('cone+hoist', dict(cone=1, hoist_z1=1)))
K, LR = 3, 0.02


def _adjacent_pairs(c, rng, count):
    """`count` pairs (g, u, v) with an edge u -> v in the parent, u != v, either direction seeded."""
    out = []
    while len(out) < count:
        g = int(rng.integers(0, len(c['graphs'])))
        n, src, dst = c['graphs'][g]
        k = int(rng.integers(0, len(src)))
        u, v = int(src[k]), int(dst[k])
        if u != v:
            out.append((g, u, v) if rng.integers(0, 2) else (g, v, u))
    return np.array(out, np.int32)


class Path:
    """One whole-path case: link_sym_ref.whole_path_case's shapes; for the even seeds every pair is replaced by an adjacent one (the odd seeds keep the
    random pairs: mostly no-ops, the unmasked floats).  Biases off the relu kink, as tests/test_hip_fuzz.py."""

    def __init__(self, seed, mode=2, F0=None):
        c = sym.whole_path_case(seed)
        self.c, self.seed, self.mode = c, seed, mode
        rng = c['rng']
        if seed % 2 == 0:
            c['spt_seeds'] = [_adjacent_pairs(c, rng, len(s)) for s in c['spt_seeds']]
            c['qry_seeds'] = [_adjacent_pairs(c, rng, len(s)) for s in c['qry_seeds']]
            assert all(ref.adjacent(c['og'][g], i, j) > 0 for s in c['spt_seeds'] + c['qry_seeds'] for g, i, j in s.tolist())
        self.T, self.C, self.k_spt, self.k_qry, self.h, self.sample_n = (c[k] for k in ('T', 'C', 'k_spt', 'k_qry', 'h', 'sample_n'))
        self.ys = [np.repeat(np.arange(self.C), self.k_spt).astype(np.int32) for _ in range(self.T)]
        self.yq = [np.repeat(np.arange(self.C), self.k_qry).astype(np.int32) for _ in range(self.T)]
        self.feats = c['feats']

    def config(self, f_in=None, extra=()):
        d = [f_in or self.c['dims'][0]] + self.c['dims'][1:]
        return [('GraphConv', [d[l], d[l + 1]]) for l in range(self.h)] + [('Linear', [d[-1], self.C])] + list(extra) + [('LinkPred', [True])]

    def theta(self, config, link_width=2):
        rng = np.random.default_rng(100 + self.seed)
        gcn, lin, _ = orc.parse_config(config)
        th = []
        for fi, fo in gcn:
            th += [(rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(f32), (rng.uniform(0.15, 0.4, fo) * rng.choice([-1.0, 1.0], fo)).astype(f32)]
        hc = lin[0] * link_width
        th += [(0.5 * rng.standard_normal((lin[1], hc)) / np.sqrt(hc)).astype(f32), (rng.uniform(0.15, 0.4, lin[1]) * rng.choice([-1.0, 1.0], lin[1])).astype(f32)]
        return th

    def args(self):
        return argparse.Namespace(update_lr=LR, meta_lr=1e-3, n_way=self.C, k_spt=self.k_spt, k_qry=self.k_qry, task_num=self.T, update_step=K,
                                  update_step_test=K, method='G-Meta', sample_nodes=self.sample_n, link_pred_mode='True', task_setup='Shared', h=self.h)

    def batches(self, store, D=0, mode=None):
        mode = (self.mode | M) if mode is None else mode
        S = _hop_extract(store, np.concatenate(self.c['spt_seeds']), self.h, self.sample_n, mode, D, np.arange(self.T + 1) * self.C * self.k_spt)
        Q = _hop_extract(store, np.concatenate(self.c['qry_seeds']), self.h, self.sample_n, mode, D, np.arange(self.T + 1) * self.C * self.k_qry)
        return S, Q

    def restated(self, og=None):
        og = og or self.c['og']
        return ([ref.extract_batch(og, s, self.h, self.sample_n, self.mode) for s in self.c['spt_seeds']],
                [ref.extract_batch(og, s, self.h, self.sample_n, self.mode) for s in self.c['qry_seeds']])

    def meta(self, config, theta, **flags):
        import gmeta_amd
        m = gmeta_amd.Meta(self.args(), config).to('cuda')
        with torch.no_grad():
            for p, v in zip(m.net.parameters(), theta):
                p.copy_(torch.from_numpy(v))
        for k, v in flags.items():
            setattr(m, k, v)
        return m

    def labels(self):
        return [torch.from_numpy(y.astype(np.int64)) for y in self.ys], [torch.from_numpy(y.astype(np.int64)) for y in self.yq]

    def step(self, S, Q, config, theta, **flags):
        ys, yq = self.labels()
        out, P, _ = self.meta(config, theta, **flags)._run(S.views(), ys, Q.views(), yq, K, True)
        return out.cpu().numpy().copy(), P

    def close(self, out, P, accs, grad, lq, what):
        """The comparison of tests/test_hip_link_symmetric.py's whole-path test: 1e-4 on losses and (scaled) gradients, one tie on the accuracies."""
        g, l, a = out[:P] / self.T, out[P:P + K + 1] / self.T, out[P + K + 1:P + 2 * K + 2] / self.T
        grad = np.concatenate([x.reshape(-1) for x in grad])
        assert out[-1] == 0, what
        np.testing.assert_allclose(l, lq, atol=TOL, rtol=1e-4, err_msg=what)
        np.testing.assert_allclose(g, grad, atol=TOL * max(1.0, float(np.abs(grad).max())), rtol=1e-3, err_msg=what)
        assert np.abs(a - np.asarray(accs)).max() <= 1.0 / (self.C * self.k_qry) + 1e-6, what


@pytest.mark.parametrize('seed', sym.WHOLE_PATH_SEEDS)
def test_meta_step_on_every_schedule_matches_oracle(seed):
    import gmeta_amd
    p = Path(seed, mode=(2, 2, 1, 2)[seed])
    if p.mode == 1:
        p.h = 2                                                                     # (reference pairs ignore h; a two-layer model)
        p.c['dims'] = p.c['dims'][:1] + [16, 32]
    store = gmeta_amd.GraphStore(p.c['graphs'], p.feats)
    S, Q = p.batches(store)
    ospt, oqry = p.restated()
    for B, obs in ((S, ospt), (Q, oqry)):
        assert B.mask_target and np.array_equal(B.parent(), np.concatenate([b.parent for b in obs]))
        assert np.array_equal(B.csr()[1], np.concatenate([b.indices + r0 for b, r0 in zip(obs, np.cumsum([0] + [b.n for b in obs]))]))
    config = p.config()
    theta = p.theta(config)
    accs, grad, _, lq = orc.meta_step(p.c['og'], p.feats, ospt, oqry, p.ys, p.yq, theta, config, p.k_spt, LR, 1e-3, K, adam_state={})
    first = None
    for name, flags in SCHEDULES:
        out, P = p.step(S, Q, config, theta, **flags)
        p.close(out, P, accs, grad, lq, '%d %s' % (seed, name))
        if name == 'dense':
            first = out
            again, _ = p.step(S, Q, config, theta)
            assert np.array_equal(_bits(first), _bits(again))                       # two runs from identical state


def test_meta_step_with_the_mean_readout():
    import gmeta_amd
    p = Path(0)
    store = gmeta_amd.GraphStore(p.c['graphs'], p.feats)
    S, Q = p.batches(store)
    ospt, oqry = p.restated()
    config = p.config(extra=[('Readout', ['mean'])])
    theta = p.theta(config, link_width=1)                                          # one pooled vector per pair (tests/readout_ref.py)
    with ro.patched():
        accs, grad, _, lq = orc.meta_step(p.c['og'], p.feats, ospt, oqry, p.ys, p.yq, theta, ro.mean_config(config), p.k_spt, LR, 1e-3, K, adam_state={})
    for name, flags in SCHEDULES[:2] + SCHEDULES[3:4]:
        out, P = p.step(S, Q, config, theta, **flags)
        p.close(out, P, accs, grad, lq, 'mean %s' % name)


def test_meta_step_with_hop_labels():
    import gmeta_amd
    D = 3
    p = Path(0)
    store = gmeta_amd.GraphStore(p.c['graphs'], p.feats)
    S, Q = p.batches(store, D)
    ospt, oqry = p.restated()
    assert S.hop_labels_cap == D and np.array_equal(S.hop_labels, np.concatenate([hop.labels(b, D) for b in ospt]))
    config = p.config(f_in=p.c['dims'][0] + hop.width(D, True))
    theta = p.theta(config)
    accs, grad, lq = hop.meta_step(p.feats, ospt, oqry, p.ys, p.yq, theta, config, p.k_spt, LR, K, D)
    for name, flags in SCHEDULES:
        out, P = p.step(S, Q, config, theta, **flags)
        p.close(out, P, accs, grad, lq, 'hop %s' % name)


def test_meta_step_with_unit_edge_weights():
    """A weighted store with all weights 1 under the mask: the restated weighted batches (edge_weight_ref) within the bar, and bitwise the unweighted
    masked step."""
    import gmeta_amd
    p = Path(2)
    plain = gmeta_amd.GraphStore(p.c['graphs'], p.feats)
    unit = gmeta_amd.GraphStore(p.c['graphs'], p.feats, edge_weights=[np.ones(len(g[1]), f32) for g in p.c['graphs']])
    wog = ewr.unit_graphs(p.c['graphs'])
    ospt, oqry = p.restated(wog)
    config = p.config()
    theta = p.theta(config)
    accs, grad, lq = ewr.meta_step(p.feats, ospt, oqry, p.ys, p.yq, theta, config, p.k_spt, LR, 1e-3, K)
    S, Q = p.batches(unit)
    assert S.weighted and S.mask_target
    out, P = p.step(S, Q, config, theta)
    p.close(out, P, accs, grad, lq, 'unit weights')
    Sp, Qp = p.batches(plain)
    assert np.array_equal(_bits(out), _bits(p.step(Sp, Qp, config, theta)[0]))


# ---------------------------------------------------------------------------------------------------- 7. surface
def _surface_db(d, store, h, **kw):
    import gmeta_amd
    s = sym.SURFACE
    np.random.seed(222); random.seed(222)
    over = kw.pop('args', {})
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=s['n_way'], k_spt=s['k_spt'], k_qry=s['k_qry'], task_num=s['tasks'], update_step=2,
                              update_step_test=2, method='G-Meta', sample_nodes=s['sample_nodes'], link_pred_mode='True', task_setup='Shared', h=h)
    for k, v in over.items():
        setattr(args, k, v)
    db = gmeta_amd.Subgraphs(None, 'train', d['info'], n_way=s['n_way'], k_shot=s['k_spt'], k_query=s['k_qry'], batchsz=s['tasks'], args=args,
                             adjs=store, h=h, tables=d['tables'], verbose=False, **kw)
    return args, db


def _mask_dataset():
    from gmeta_amd import synth
    s = sym.SURFACE
    return synth.link_dataset(s['n_graphs'], s['n'], s['m'], s['F0'], seed=11, inject_negatives=False)


def assert_views_match(batch, obs):
    assert batch.mask_target
    r0 = e0 = 0
    assert np.array_equal(batch.parent(), np.concatenate([b.parent for b in obs]))
    ip, ix = batch.csr()
    for b in obs:
        assert np.array_equal(ip[r0:r0 + b.n + 1] - e0, b.indptr) and np.array_equal(ix[e0:e0 + len(b.indices)] - r0, b.indices)
        r0 += b.n; e0 += len(b.indices)


@pytest.mark.parametrize('link_hops,h', [('symmetric', 2), ('reference', 2)])
def test_subgraphs_mask_target(link_hops, h):
    import gmeta_amd
    from gmeta_amd import synth
    s = sym.SURFACE
    mode = 2 if link_hops == 'symmetric' else 1
    d = _mask_dataset()
    og = [orc.Graph(*g) for g in d['graphs']]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    args, db = _surface_db(d, store, h, link_hops=link_hops, mask_target=True)
    assert db.mask_target and db.link_mode == mode | M
    idx = list(range(s['tasks']))
    arrs = [db._task_arrays(i) for i in idx]
    assert sum(ref.adjacent(og[g], i, j) > 0 for a in arrs for g, i, j in np.concatenate([a[0], a[1]]).tolist()) >= 3
    ospt = [ref.extract_batch(og, a[0], h, s['sample_nodes'], mode) for a in arrs]
    oqry = [ref.extract_batch(og, a[1], h, s['sample_nodes'], mode) for a in arrs]
    batch = db.get_batch(idx)
    assert_views_match(batch[0][0].view_of, ospt)
    assert_views_match(batch[2][0].view_of, oqry)
    one = db[1]
    assert_views_match(one[0], ospt[1:2])
    assert_views_match(one[2], oqry[1:2])
    for b3 in db.batches([idx[:2], idx[2:], idx[:1]], prefetch=1, workers=2):
        assert b3[0][0].view_of.mask_target and b3[2][0].view_of.mask_target
    assert_views_match(b3[0][0].view_of, ospt[:1])
    names = sym.surface_query_names(d)
    seeds = [np.array([[int(x) for x in nm.split('_')] for nm in task], np.int32) for task in names]
    QB = db.query_batch(names)
    assert_views_match(QB, [ref.extract_batch(og, sd, h, s['sample_nodes'], mode) for sd in seeds])
    # Meta.adapt / predict on the masked batches against the oracle's support chain (tests/test_hip_predict.py: K steps of classifier_forward ->
    # proto_loss_spt -> classifier_backward -> SGD) on the RESTATED support batches, scored on the restated query batches: fast weights, prototypes
    # and log-probabilities within the project's 1e-4, predictions equal wherever the two best classes are more than 2e-4 apart
    config = synth.make_config(s['F0'], 16, h, 2, link=True)
    gcn, lin, _ = orc.parse_config(config)
    rng = np.random.default_rng(5)
    theta = []
    for fi, fo in gcn:                                                             # (biases off the relu kink, as tests/test_hip_fuzz.py)
        theta += [(rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(f32), (rng.uniform(0.15, 0.4, fo) * rng.choice([-1.0, 1.0], fo)).astype(f32)]
    theta += [(0.5 * rng.standard_normal((lin[1], 2 * lin[0])) / np.sqrt(2 * lin[0])).astype(f32), (rng.uniform(0.15, 0.4, lin[1]) * rng.choice([-1.0, 1.0], lin[1])).astype(f32)]
    m = gmeta_amd.Meta(args, config).to('cuda')
    with torch.no_grad():
        for p_, v_ in zip(m.net.parameters(), theta):
            p_.copy_(torch.from_numpy(v_))
    oq = [ref.extract_batch(og, sd, h, s['sample_nodes'], mode) for sd in seeds]
    for K_ in (0, args.update_step_test):
        ad = m.adapt(batch[0], batch[1], K=K_)
        pr = ad.predict(QB)
        assert [len(p) for p in pr.pred] == [len(t) for t in names]
        fw_h, pt_h = ad.fast_weights.cpu().numpy(), ad.prototypes.cpu().numpy()
        for t in range(s['tasks']):
            ys_t = np.asarray(batch[1][t]).astype(np.int32)
            fw, protos = [v.copy() for v in theta], None
            xs = ospt[t].features(d['feats'])
            for _ in range(max(K_, 1)):
                logit_s, cs = orc.classifier_forward(ospt[t], xs, fw, config)
                _, _, protos, dls = orc.proto_loss_spt(logit_s, ys_t, s['k_spt'], need_grad=K_ > 0)
                if K_ > 0:
                    fw = [w - f32(args.update_lr) * g for w, g in zip(fw, orc.classifier_backward(ospt[t], fw, config, cs, dls))]
            np.testing.assert_allclose(fw_h[t], np.concatenate([w.reshape(-1) for w in fw]), atol=TOL, rtol=0)
            np.testing.assert_allclose(pt_h[t, :len(protos)], protos, atol=TOL, rtol=0)
            z, _ = orc.classifier_forward(oq[t], oq[t].features(d['feats']), fw, config)
            lp = orc._log_softmax(-((z[:, None, :] - protos[None, :, :]) ** 2).sum(2))
            np.testing.assert_allclose(pr.log_probs[t], lp, atol=TOL, rtol=0)
            top = np.sort(lp, axis=1)
            clear = top[:, -1] - top[:, -2] > 2 * TOL
            assert np.array_equal(pr.pred[t][clear], lp.argmax(1)[clear]) and np.array_equal(pr.labels[t], ad.classes[t][pr.pred[t]])
    # args.mask_target is the keyword's fallback; the default is off
    _, db2 = _surface_db(d, store, h, link_hops=link_hops, args=dict(mask_target=1))
    assert db2.mask_target and db2.query_batch(names).mask_target
    _, db3 = _surface_db(d, store, h, link_hops=link_hops)
    assert not db3.mask_target and db3.link_mode == mode and not db3.get_batch(idx)[0][0].view_of.mask_target


def test_subgraphs_mask_target_with_reference_sampling():
    """sample_mode='reference' (reference pairs only): the node sets are the reference's RNG draws, the induced subgraphs are masked."""
    import gmeta_amd
    s = sym.SURFACE
    d = _mask_dataset()
    og = [orc.Graph(*g) for g in d['graphs']]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    _, db = _surface_db(d, store, 2, sample_mode='reference', mask_target=True)
    idx = list(range(s['tasks']))
    arrs = [db._task_arrays(i) for i in idx]
    batch = db.get_batch(idx)
    for part, a_k in ((0, 0), (2, 1)):
        B = batch[part][0].view_of
        assert B.mask_target
        seeds = np.concatenate([a[a_k] for a in arrs])
        sub, par = B.sub_off, B.parent()
        lists = [par[sub[k]:sub[k + 1]] for k in range(B.subs)]
        assert max(len(l) for l in lists) <= s['sample_nodes'] + 2
        ob = ref.batch_from_lists(og, seeds, lists)
        assert np.array_equal(B.csr()[0], ob.indptr) and np.array_equal(B.csr()[1], ob.indices)
        assert sum(ref.adjacent(og[g], i, j) > 0 for g, i, j in seeds.tolist()) >= 1


def test_subgraphs_mask_target_errors():
    import gmeta_amd
    d = _mask_dataset()
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    with pytest.raises(ValueError, match='link_pred_mode'):
        _surface_db(d, store, 2, mask_target=True, args=dict(link_pred_mode='False'))


def test_train_driver_with_mask_target(tmp_path):
    """A few epochs of the SEAL configuration on graphs that hold the positive pairs only; it runs and finishes (no accuracy bar)."""
    from gmeta_amd import datadir, synth
    d = synth.link_dataset(6, 120, 2, 8, seed=3, inject_negatives=False)
    splits = {}
    for key in ('train', 'train_spt', 'train_qry'):
        for nm, lab in zip(*d['tables'][key]):
            mode = ('train', 'train', 'train', 'train', 'val', 'test')[int(nm.split('_')[0])]
            names, labels = splits.setdefault(key.replace('train', mode), ([], []))
            names.append(nm); labels.append(lab)
    datadir.write_datadir(str(tmp_path), d['graphs'], d['feats'], d['info'], splits)
    import train as drv
    args = drv.parse(['--data_dir', str(tmp_path) + '/', '--epoch', '2', '--k_spt', '2', '--k_qry', '6', '--task_num', '4', '--update_step', '3',
                      '--update_step_test', '4', '--update_lr', '0.05', '--meta_lr', '0.01', '--hidden_dim', '32', '--batchsz', '40', '--h', '2',
                      '--eval_tasks', '10', '--train_result_report_steps', '5', '--task_setup', 'Shared', '--link_pred_mode', 'True', '--n_way', '2',
                      '--link_hops', 'symmetric', '--hop_labels', '3', '--mask_target', '1'])
    assert args.mask_target == 1 and drv.parse(['--data_dir', 'x', '--task_setup', 'Shared']).mask_target == 0
    res = drv.main(args)
    assert np.isfinite(res['test_acc']) and 0.0 <= res['test_acc'] <= 1.0, res
