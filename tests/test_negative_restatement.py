"""CPU (-m "not gpu"): the restatement of the negative-pair definition (tests/negative_ref.py) against brute force and an independently written
enumeration; the host logic of link_tables_with_negatives on a store whose negative_pairs IS the restatement; the out-CSR row order the device
searches rest on; the C ABI surface and the driver flag."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import gmeta_oracle as orc
import negative_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('uniform', 'two_hop')


def small_graphs():
    rng = np.random.default_rng(3)
    out = []
    for N, E in ((12, 20), (30, 90), (50, 400), (64, 64)):
        out.append((N, rng.integers(0, N, E).astype(np.int64), rng.integers(0, N, E).astype(np.int64)))
    out.append(ref.multigraph_case())
    return out


def enumerate_first_valid(N, src, dst, g, n, seed, mode, exclude=()):
    """Independent of negative_ref.negative_pairs: every candidate of the budget at once in numpy, validity by key membership, first occurrences by
    np.unique, then the n smallest k."""
    m = ref.MODES[mode]
    B = ref.budget(n)
    salt = np.uint32(orc.sample_salt(seed, g, ref.TAG, m))
    with np.errstate(over='ignore'):
        k4 = (np.arange(B, dtype=np.uint32) * np.uint32(4) + salt)
        r = [orc.lowbias32(k4 + np.uint32(c)).astype(np.uint64) for c in range(3)]
    a = ((r[0] * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    ok = np.ones(B, bool)
    if m == 0:
        b = ((r[1] * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    else:
        order = np.lexsort((dst, src))                                  # by source, destinations ascending
        od = dst[order]
        ptr = np.searchsorted(src[order], np.arange(N + 1))
        deg = np.diff(ptr)
        ok &= deg[a] > 0
        w = od[np.minimum(ptr[a] + ((r[1] * deg[a].astype(np.uint64)) >> np.uint64(32)).astype(np.int64), len(od) - 1)]
        ok &= deg[w] > 0
        b = od[np.minimum(ptr[w] + ((r[2] * deg[w].astype(np.uint64)) >> np.uint64(32)).astype(np.int64), len(od) - 1)]
    u, v = np.minimum(a, b), np.maximum(a, b)
    key = u * N + v
    edge_keys = np.unique(np.minimum(src, dst) * N + np.maximum(src, dst))
    ex = np.asarray(exclude, np.int64).reshape(-1, 2)
    ok &= (u != v) & ~np.isin(key, edge_keys) & ~np.isin(key, np.minimum(ex[:, 0], ex[:, 1]) * N + np.maximum(ex[:, 0], ex[:, 1]))
    ks = np.nonzero(ok)[0]
    _, first = np.unique(key[ks], return_index=True)
    ks = np.sort(ks[first])[:n]
    return np.stack([u[ks], v[ks]], 1)


@pytest.mark.parametrize('mode', MODES)
def test_restatement_against_brute_force_and_enumeration(mode):
    for g, (N, src, dst) in enumerate(small_graphs()):
        free = ref.free_pairs(N, src, dst)
        for n in (0, 1, 7, 40):
            p, found = ref.negative_pairs(N, src, dst, g, n, 222, mode)
            want = enumerate_first_valid(N, src, dst, g, n, 222, mode)
            assert found == len(p) == len(want) and np.array_equal(p, want), (g, n)
            assert (p[:, 0] < p[:, 1]).all()
            assert len({tuple(x) for x in p.tolist()}) == len(p)
            assert all(tuple(x) in free for x in p.tolist())
            if n and mode == 'uniform':
                assert found == n                                       # (these graphs are sparse)
        # exclusion: the first, a middle and the last pair of the unexcluded draw, given in either orientation
        p, _ = ref.negative_pairs(N, src, dst, g, 20, 5, mode)
        if len(p) >= 3:
            ex = np.array([p[0][::-1], p[len(p) // 2], p[-1]])
            q, _ = ref.negative_pairs(N, src, dst, g, 20, 5, mode, exclude=ex)
            assert not {tuple(x) for x in q.tolist()} & {tuple(sorted(x)) for x in ex.tolist()}
            assert np.array_equal(q, enumerate_first_valid(N, src, dst, g, 20, 5, mode, ex))
            keep = [x for x in p.tolist() if tuple(x) not in {tuple(sorted(y)) for y in ex.tolist()}]
            assert q[:len(keep)].tolist() == keep                       # the rest shifts up, the tail is new
        # a prefix property: n pairs are the first n of n + 5 whenever both are found
        a, fa = ref.negative_pairs(N, src, dst, g, 9, 222, mode)
        b, fb = ref.negative_pairs(N, src, dst, g, 14, 222, mode)
        if fa == 9:
            assert np.array_equal(a, b[:9])
        assert not np.array_equal(ref.negative_pairs(N, src, dst, g, 9, 223, mode)[0], a) or fa == 0


def test_five_node_graph_has_exactly_eight_free_pairs():
    src, dst = np.array([0, 1, 1, 2, 3]), np.array([1, 0, 2, 1, 3])
    free = ref.free_pairs(5, src, dst)
    assert len(free) == 8
    p, found = ref.negative_pairs(5, src, dst, 0, 8)
    assert found == 8 and {tuple(x) for x in p.tolist()} == free
    p, found = ref.negative_pairs(5, src, dst, 0, 9)
    assert found == 8 and {tuple(x) for x in p.tolist()} == free


def test_two_hop_pairs_have_a_directed_path_and_never_start_at_a_sink():
    for g, (N, src, dst) in enumerate(small_graphs()):
        adj = set(zip(src.tolist(), dst.tolist()))
        outdeg = np.bincount(src, minlength=N)
        trace = []
        p, found = ref.negative_pairs(N, src, dst, g, 60, 11, 'two_hop', trace=trace)
        assert len(trace) == found
        for (u, v), (k, a, w, b) in zip(p.tolist(), trace):
            assert (u, v) == (min(a, b), max(a, b)) and (a, w) in adj and (w, b) in adj
            assert outdeg[a] > 0 and outdeg[w] > 0
    N, src, dst = ref.multigraph_case()
    assert found > 0 and not {a for _, a, _, _ in trace} & set(range(280, 300))


class Data:
    """Two undirected graphs of 60 nodes stored in both directions; positives = pairs u < v with an edge; some validation / test positives are NOT edges of
    the graph (taken out for evaluation)."""

    def __init__(self):
        rng = np.random.default_rng(9)
        self.graphs, self.tables, self.info, self.held_out = [], {}, {}, {}
        for g in range(2):
            N = 60
            e = np.unique(np.sort(rng.integers(0, N, (90, 2)), 1), axis=0)
            e = e[e[:, 0] != e[:, 1]]
            held = e[-12:]                                              # listed in val / test, absent from the graph
            kept = e[:-12]
            self.graphs.append((N, np.concatenate([kept[:, 0], kept[:, 1]]), np.concatenate([kept[:, 1], kept[:, 0]])))
            self.held_out[g] = {tuple(x) for x in held.tolist()}
            cut = [0, 10, 30, 36, len(kept)]
            parts = {'train_spt': kept[cut[0]:cut[1]], 'train_qry': kept[cut[1]:cut[2]], 'val_spt': kept[cut[2]:cut[3]], 'val_qry': held[:5],
                     'test_spt': kept[cut[3]:cut[4]], 'test_qry': held[5:]}
            for key, arr in parts.items():
                names, labels = self.tables.setdefault(key, ([], []))
                for a, b in arr.tolist():
                    nm = '%d_%d_%d' % (g, a, b)
                    names.append(nm); labels.append('1'); self.info[nm] = 1
        for s in ('train', 'val', 'test'):
            self.tables[s] = (self.tables[s + '_spt'][0] + self.tables[s + '_qry'][0], self.tables[s + '_spt'][1] + self.tables[s + '_qry'][1])


def _by_graph(names):
    out = {}
    for nm in names:
        g, a, b = (int(x) for x in nm.split('_'))
        out.setdefault(g, []).append((a, b))
    return out


@pytest.mark.parametrize('mode', MODES)
def test_link_tables_with_negatives_host_logic(mode):
    from gmeta_amd.negatives import link_tables_with_negatives
    d = Data()
    store = ref.HostStore(d.graphs)
    t0, i0 = copy.deepcopy(d.tables), dict(d.info)
    tables, info = link_tables_with_negatives(store, d.tables, d.info, mode=mode, seed=5)
    assert d.tables == t0 and d.info == i0                              # inputs untouched
    assert [c[0] for c in store.calls] == [0, 1] and all(c[2] == 5 and c[3] == mode for c in store.calls)      # one call per graph
    parts = [s + p for s in ('train', 'val', 'test') for p in ('_spt', '_qry')]
    seen = {0: [], 1: []}
    for key in parts:
        names, labels = tables[key]
        n_pos = len(t0[key][0])
        assert names[:n_pos] == t0[key][0] and labels[:n_pos] == ['1'] * n_pos and labels[n_pos:] == ['0'] * (len(names) - n_pos)
        pos, neg = _by_graph(names[:n_pos]), _by_graph(names[n_pos:])
        assert {g: len(v) for g, v in pos.items()} == {g: len(v) for g, v in neg.items()}      # counts per table and graph
        for g, v in neg.items():
            seen[g] += v
        assert all(info[nm] == 0 for nm in names[n_pos:]) and all(info[nm] == 1 for nm in names[:n_pos])
    for g in (0, 1):
        N, src, dst = store.graphs[g]
        assert len(set(seen[g])) == len(seen[g])                        # disjoint across the six tables
        assert all(u < v for u, v in seen[g]) and not store.has_edges(g, seen[g]).any()
        assert not set(seen[g]) & d.held_out[g]                         # positives passed in exclude but absent from the graph
        total = sum(len(_by_graph(t0[key][0]).get(g, [])) for key in parts)
        # dealt out in order: the concatenation over the six tables IS the one draw of `total` pairs
        every = {tuple(sorted(x)) for key in t0 for x in _by_graph(t0[key][0]).get(g, [])}
        want, found = ref.negative_pairs(N, src, dst, g, total, 5, mode, exclude=sorted(every))
        assert found == total and seen[g] == [tuple(x) for x in want.tolist()]
        # ... and without the exclusion a held-out positive WOULD have come back in uniform mode on some graph (checked below over both graphs)
    for s in ('train', 'val', 'test'):
        assert tables[s] == (tables[s + '_spt'][0] + tables[s + '_qry'][0], tables[s + '_spt'][1] + tables[s + '_qry'][1])
    assert len(info) == len(i0) + sum(len(v) for v in seen.values())
    # absent tables are skipped
    some = {k: v for k, v in d.tables.items() if k.startswith('train')}
    t2, _ = link_tables_with_negatives(ref.HostStore(d.graphs), some, d.info, mode=mode, seed=5)
    assert sorted(t2) == ['train', 'train_qry', 'train_spt'] and len(t2['train'][0]) == 2 * len(some['train'][0])
    # a table that already holds negatives
    bad = copy.deepcopy(d.tables)
    bad['val_qry'][1][0] = '0'
    with pytest.raises(ValueError, match='val_qry'):
        link_tables_with_negatives(ref.HostStore(d.graphs), bad, d.info, mode=mode)


def test_the_exclusion_list_is_what_keeps_held_out_positives_away():
    """On a graph where most free pairs are held-out positives, the unexcluded draw returns some of them; the completed tables never do."""
    from gmeta_amd.negatives import link_tables_with_negatives
    N = 12
    held = [(u, v) for u in range(N) for v in range(u + 1, N) if (u + v) % 3 == 0]
    graph = (N, np.array([0, 1, 2]), np.array([1, 2, 4]))
    names = ['0_%d_%d' % p for p in held[:4]]
    tables = {'test_qry': (names, ['1'] * 4), 'test_spt': (['0_0_1'], ['1']), 'test': (['0_0_1'] + names + ['0_%d_%d' % p for p in held[4:]], ['1'] * (1 + len(held)))}
    plain, _ = ref.negative_pairs(N, graph[1], graph[2], 0, 5)
    assert {tuple(x) for x in plain.tolist()} & set(held)
    out, _ = link_tables_with_negatives(ref.HostStore([graph]), tables, {})
    neg = [nm for key in ('test_spt', 'test_qry') for nm, l in zip(*out[key]) if l == '0']
    assert len(neg) == 5 and not {tuple(int(x) for x in nm.split('_')[1:]) for nm in neg} & set(held)      # (pairs only the plain table lists are excluded too)


def test_out_csr_rows_ascend_on_the_host_arrays():
    """The invariant the device's binary searches rest on (csrc/negatives.hip: row_has): the by-source regrouping of the in-CSR that edges_to_in_csr
    builds -- the store's stable counting sort, restated with numpy's stable argsort as GraphStore.symmetric does -- has ascending destinations in every
    row, parallel copies included, for every graph of a multi-graph store."""
    from gmeta_amd.graphstore import edges_to_in_csr
    rng = np.random.default_rng(1)
    graphs = [ref.multigraph_case(), (17, rng.integers(0, 17, 200), rng.integers(0, 17, 200)), (5, np.array([4, 4, 4, 0]), np.array([3, 3, 0, 4])), (3, np.array([], np.int64), np.array([], np.int64))]
    for N, src, dst in graphs:
        ptr, ix = edges_to_in_csr(N, src, dst)
        in_dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(ptr))
        # the store's sort (csrc/store.hip): walk the in-CSR rows in ascending destination, append to the source's out-row
        rows = [[] for _ in range(N)]
        for v, u in zip(in_dst.tolist(), ix.tolist()):
            rows[u].append(v)
        assert all(r == sorted(r) for r in rows)
        order = np.argsort(ix, kind='stable')
        assert np.array_equal(np.concatenate([np.asarray(r, np.int64) for r in rows]) if len(ix) else np.zeros(0, np.int64), in_dst[order])
        assert rows == ref.out_rows(N, src, dst)
        assert sorted(zip(np.asarray(src).tolist(), np.asarray(dst).tolist())) == sorted((u, v) for u, r in enumerate(rows) for v in r)      # multiplicities kept
    N, src, dst = graphs[0]
    assert any(len(r) != len(set(r)) for r in ref.out_rows(N, src, dst))      # parallel copies were there


def test_exports_are_declared_and_bound():
    import gmeta_amd  # noqa: F401
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gm_store_negative_pairs', 'gm_store_has_edges'):
        assert re.search(r'\b%s\s*\(' % name, code) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES['gm_store_negative_pairs'][1]) == 10 and len(_lib.PROTOTYPES['gm_store_has_edges'][1]) == 6
    assert re.search(r'#define GM_NEG_UNIFORM 0\b', code) and re.search(r'#define GM_NEG_TWO_HOP 1\b', code)
    assert _lib.NEG_MODES == {'uniform': 0, 'two_hop': 1} == ref.MODES
    assert '0x6E454721' in txt and ref.TAG == 0x6E454721
    assert hasattr(gmeta_amd, 'link_tables_with_negatives') and hasattr(gmeta_amd.GraphStore, 'negative_pairs') and hasattr(gmeta_amd.GraphStore, 'has_edges')
    assert 'negatives.hip' in open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert _lib.lib().gm_set_tuning(b'neg_round', 64) == 0 and _lib.lib().gm_get_tuning(b'neg_round') == 64
    assert _lib.lib().gm_set_tuning(b'neg_round', 0) == 0


def test_train_flag_parses_and_defaults_to_file():
    import train as drv
    base = ['--data_dir', 'x', '--task_setup', 'Shared']
    assert drv.parse(base).negatives == 'file'
    assert drv.parse(base + ['--negatives', 'uniform']).negatives == 'uniform' and drv.parse(base + ['--negatives', 'two_hop']).negatives == 'two_hop'
    with pytest.raises(SystemExit):
        drv.parse(base + ['--negatives', 'three_hop'])
