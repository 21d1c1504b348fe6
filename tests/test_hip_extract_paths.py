"""GPU (-m gpu): the extraction kernels' two bitmap homes build the same batches.  Store A holds a small graph G, store B the same G followed by a
700,000-node ring: B's largest graph is beyond what the LDS bitmap pair takes (~643k nodes), so every build on B runs the global-bitmap instantiations
of k_nodes / k_fill and every build on A the LDS ones.  All seeds lie in graph 0: the two builds must agree in the dimensions and in every GM_F_* field,
floats compared as bit patterns -- for node seeds, pairs, symmetric pairs, given node lists, the two-part build, hop labels, weighted stores and masked
pairs on them (the *_pref32 cases: the LDS side with GM_EXTRACT_PREF16 = 0, the 32-bit-prefix instantiations of symmetric pairs and of the weighted fill).  The
32-bit-prefix LDS kernels (GM_EXTRACT_PREF16=0, read once per process) are held against the default build from a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, RING, SAMPLE = 3000, 700_000, 60
I32, U32 = np.int32, np.uint32


def _graphs(weighted):
    from gmeta_amd import synth
    rng = np.random.default_rng(11)
    e = synth.pa_edges(N, 3, rng)
    g = [N, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])]
    a = np.arange(RING)
    r = [RING, np.concatenate([a, (a + 1) % RING]), np.concatenate([(a + 1) % RING, a])]
    if weighted:
        g.append(rng.uniform(0.25, 4.0, len(g[1])).astype(np.float32))
        r.append(np.full(2 * RING, 0.5, np.float32))
    feats = [rng.standard_normal((N, 4)).astype(np.float32), np.zeros((RING, 4), np.float32)]
    return [tuple(g), tuple(r)], feats


def _store(weighted, with_ring):
    import gmeta_amd
    graphs, feats = _graphs(weighted)
    return gmeta_amd.GraphStore(graphs if with_ring else graphs[:1], feats if with_ring else feats[:1])


def _seeds(pairs):
    rng = np.random.default_rng(5)
    i = np.concatenate([np.arange(4), rng.integers(4, N, 8)])          # the four oldest nodes of a preferential-attachment graph are hubs
    j = rng.integers(0, N, 12) if pairs else -np.ones(12, np.int64)
    return np.stack([np.zeros(12, np.int64), i, j], 1)


def _adjacent_seeds():
    """_seeds(True) with the first eight pairs (the hubs among them) moved onto edges of G: a target-link mask has work to do"""
    from gmeta_amd import synth
    e = synth.pa_edges(N, 3, np.random.default_rng(11))                # G's edges, as _graphs draws them
    s = _seeds(True)
    for k in range(8):
        s[k, 2] = np.concatenate([e[e[:, 0] == s[k, 1], 1], e[e[:, 1] == s[k, 1], 0]])[0]
    return s


def _fields(b):
    """dims and every GM_F_* field the batch carries, floats as their bit patterns"""
    from gmeta_amd import _lib as L
    r, e, s, c = b.rows, b.edges, b.subs, b.centres
    spec = {L.F_SUB_OFF: (s + 1, I32), L.F_SET_SUB_OFF: (b.sets + 1, I32), L.F_PARENT: (r, I32), L.F_GRAPH: (s, I32), L.F_INDPTR: (r + 1, I32),
            L.F_INDICES: (e, I32), L.F_INDPTR_T: (r + 1, I32), L.F_INDICES_T: (e, I32), L.F_CENTRE: (s * c, I32), L.F_NORM: (r, U32),
            L.F_FEAT_ROW: (r, I32), L.F_NORM_SRC: (r, U32), L.F_NORM_CENTRE: (r, U32), L.F_NORM_E1: (r, U32), L.F_EDGE_CENTRE_T: (e, I32)}
    if b.weighted:
        spec.update({L.F_EDGE_W: (e, U32), L.F_EDGE_W_T: (e, U32)})
    if b.hop_labels_cap:
        spec[L.F_HOP] = (r * c, np.int8)
    out = {'dims': np.array([r, e, s, b.sets, c], np.int64)}
    for f, (n, dt) in spec.items():
        a = np.empty(n, dt)
        L.check(L.lib().gm_batch_read(b.handle, f, L.ptr(a), a.nbytes), 'gm_batch_read')      # (no host-side cache in the way)
        out['f%d' % f] = a
    return out


def _node_case(store, h=2):
    from gmeta_amd.subgraphs import SubgraphBatch
    return [SubgraphBatch.extract(store, _seeds(False), [0, 5, 12], h, SAMPLE, 222, False)]


def _build(case, store):
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch, hop_labels_switch
    if case in ('nodes_h2', 'weighted'):
        return _node_case(store)
    if case.endswith('_pref32'):
        lib = _lib.lib()
        prev = lib.gm_get_tuning(b'GM_EXTRACT_PREF16')
        _lib.check(lib.gm_set_tuning(b'GM_EXTRACT_PREF16', 0), 'gm_set_tuning')
        try:
            return _build(case[:-len('_pref32')], store)
        finally:
            lib.gm_set_tuning(b'GM_EXTRACT_PREF16', prev)
    if case == 'weighted_pairs':
        return [SubgraphBatch.extract(store, _adjacent_seeds(), [0, 12], 2, SAMPLE, 222, True)]
    if case == 'masked_weighted':
        return [SubgraphBatch.extract(store, _adjacent_seeds(), [0, 12], 2, SAMPLE, 222, 1 | _lib.LINK_MASK_TARGET)]
    if case == 'symmetric_h3':
        return [SubgraphBatch.extract(store, _seeds(True), [0, 12], 3, SAMPLE, 222, _lib.LINK_SYMMETRIC)]
    if case == 'nodes_h3':
        return _node_case(store, 3)
    if case == 'pairs':
        return [SubgraphBatch.extract(store, _seeds(True), [0, 12], 2, SAMPLE, 222, True)]
    if case == 'symmetric_h2':
        return [SubgraphBatch.extract(store, _seeds(True), [0, 12], 2, SAMPLE, 222, _lib.LINK_SYMMETRIC)]
    if case == 'from_nodes':
        b = _node_case(store)[0]
        par, off = b.parent(), b.sub_off
        return [b, SubgraphBatch.from_nodes(store, _seeds(False), [0, 5, 12], [par[off[k]:off[k + 1]] for k in range(12)], False)]
    if case == 'extract_pair':
        s = _seeds(False)
        return list(SubgraphBatch.extract_pair(store, s[:4], [0, 4], s[4:], [0, 3, 8], 2, SAMPLE, 222, False))
    if case == 'hop_labels':
        with hop_labels_switch(2):
            return _node_case(store)
    raise KeyError(case)


@pytest.fixture(scope='module')
def stores():
    made = {}

    def get(weighted, with_ring):
        if (weighted, with_ring) not in made:
            made[(weighted, with_ring)] = _store(weighted, with_ring)
        return made[(weighted, with_ring)]
    return get


@pytest.mark.parametrize('case', ['nodes_h2', 'nodes_h3', 'pairs', 'symmetric_h2', 'symmetric_h3', 'from_nodes', 'extract_pair', 'hop_labels', 'weighted',
                                  'symmetric_h2_pref32', 'weighted_pairs_pref32', 'masked_weighted', 'masked_weighted_pref32'])
def test_global_bitmap_build_equals_lds_build(stores, case):
    w = 'weighted' in case
    got = [[_fields(b) for b in _build(case, stores(w, ring))] for ring in (False, True)]
    assert len(got[0]) == len(got[1])
    for x, y in zip(*got):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), (case, k)
    if case in ('nodes_h2', 'nodes_h3', 'weighted'):
        sizes = np.diff(got[0][0]['f0'])                               # a thinned neighbourhood keeps sample_nodes nodes, and its centre
        assert (sizes >= SAMPLE).any() and (case == 'nodes_h3' or (sizes < SAMPLE).any()), sizes      # h = 2: two of the seeds reach 21 nodes, the others 100 and more
    if case.startswith('masked_weighted'):                             # the same node sets, and the mask took edges away
        from gmeta_amd import _lib
        plain, par = _fields(_build('weighted_pairs', stores(True, False))[0]), 'f%d' % _lib.F_PARENT
        assert np.array_equal(plain[par], got[0][0][par]) and got[0][0]['dims'][1] < plain['dims'][1]


def _dump(path):
    np.savez(path, **_fields(_node_case(_store(False, False))[0]))


def test_32_bit_prefix_words_build_the_same_batch(stores, tmp_path):
    out = str(tmp_path / 'pref32.npz')
    here = os.path.dirname(os.path.abspath(__file__))
    code = 'import sys; sys.path[:0] = %r; import test_hip_extract_paths as t; t._dump(%r)' % ([os.path.dirname(here), here], out)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, GM_EXTRACT_PREF16='0'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want, got = _fields(_node_case(stores(False, False))[0]), np.load(out)
    assert set(want) == set(got.files)
    for k in want:
        assert np.array_equal(want[k], got[k]), k
