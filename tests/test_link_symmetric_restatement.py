"""CPU: the restatement of the symmetric pair mode (tests/link_sym_ref.py) against an independent multi-source reachability, the inputs of the GPU
tests of that mode (tests/test_hip_link_symmetric.py), and the driver's option."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, ROOT)
import gmeta_oracle as orc      # noqa: E402
import link_sym_ref as ref      # noqa: E402


def _reach(n, src, dst, roots, h):
    """Nodes within h in-hops of any root, by boolean reachability on the dense adjacency matrix (no CSR, no per-root BFS)."""
    into = np.zeros((n, n), bool)
    into[dst, src] = True                       # into[v, u]: an edge u -> v (parallel edges collapse: reachability does not count them)
    seen = np.zeros(n, bool); seen[list(roots)] = True
    for _ in range(h):
        seen = seen | into[seen].any(0)
    return np.nonzero(seen)[0].astype(np.int32)


@pytest.mark.parametrize('seed', range(6))
def test_restatement_is_the_multi_source_neighbourhood(seed):
    from test_hip_fuzz import _graph
    rng = np.random.default_rng(300 + seed)
    n, src, dst = _graph(rng, int(rng.integers(25, 160)))
    G = orc.Graph(n, src, dst)
    pairs = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(12)] + [(3, 3)]
    n_strict = 0
    for i, j in pairs:
        for h in (1, 2, 3):
            got = ref.nodes(G, i, j, h)
            assert np.array_equal(got, _reach(n, src, dst, (i, j), h)), (i, j, h)
            assert np.array_equal(got, ref.nodes(G, j, i, h)), (i, j, h)                      # no preferred endpoint
            assert i in got and j in got
        quirk, sym2 = orc.linkpred_nodes(G, i, j), ref.nodes(G, i, j, 2)
        assert np.isin(quirk, sym2).all(), (i, j)                                             # the reference's set lacks j's second hop, nothing else
        n_strict += len(sym2) > len(quirk)
    assert n_strict >= 1
    # sampling: the oracle's own key, both centres kept, the strict threshold
    i, j = pairs[0]
    full = ref.nodes(G, i, j, 3)
    for k in (len(full), len(full) - 1, 4):
        lst = ref.node_lists([G], [(0, i, j)], 3, k)[0]
        if len(full) > k:
            assert np.array_equal(lst, orc.sample_nodes(full, k, ref.RNG_SEED, 0, i, j)) and i in lst and j in lst and k <= len(lst) <= k + 2
        else:
            assert np.array_equal(lst, full)


@pytest.mark.parametrize('seed', ref.FUZZ_SEEDS)
def test_fuzz_cases_tell_the_modes_apart_and_hold_the_planted_pairs(seed):
    c = ref.fuzz_case(seed)
    G, sp, seeds, h = c['og'][0], c['special'], c['seeds'], c['h']
    assert ref.differs_from_reference_mode(c['og'], seeds, h, c['sample_n']) >= 1
    _, i, j = seeds[sp['isolated_j']]
    assert len(G.preds(j)) == 0 and j not in G.indices and len(G.preds(i)) > 0
    _, i, j = seeds[sp['j_inside']]
    assert j != i and j in orc.khop_nodes(G, i, 1)
    _, i, j = seeds[sp['disjoint']]
    assert len(np.intersect1d(orc.khop_nodes(G, i, h), orc.khop_nodes(G, j, h))) == 0
    assert ('self_pair' in sp) == (seed == 0)
    if 'self_pair' in sp:
        assert seeds[sp['self_pair']][1] == seeds[sp['self_pair']][2]
    assert all(s[1] != s[2] for k, s in enumerate(seeds) if k != sp.get('self_pair'))


def test_fuzz_cases_cover_the_grid_and_a_real_disjoint_pair():
    cases = [ref.fuzz_case(s) for s in ref.FUZZ_SEEDS]
    assert {(c['h'], c['sample_n']) for c in cases} == {(h, k) for h in (1, 2, 3) for k in (6, 40, 10000)}
    assert sum(c['disjoint_nontrivial'] for c in cases) >= 3                 # both sides with predecessors of their own
    # sampling happens in some cases and not in others
    sampled = [sum(len(ref.nodes(c['og'][g], i, j, c['h'])) > c['sample_n'] for g, i, j in c['seeds'].tolist()) for c in cases]
    assert sum(s > 0 for s in sampled) >= 3 and sum(s == 0 for s in sampled) >= 3


@pytest.mark.parametrize('h,sample_n', ref.HUB_CASES)
def test_hub_case_reaches_each_hub_from_its_own_side_only(h, sample_n):
    c = ref.hub_case()
    G = c['og'][0]
    (A, B), (i, j, i2) = c['hubs'], c['centres']
    deg = np.diff(G.indptr)
    assert deg[A] > 256 and deg[B] > 256 and (np.delete(deg, [A, B]) <= 256).all()
    assert A in G.preds(i) and B in G.preds(j) and A in G.preds(i2)
    assert B not in orc.khop_nodes(G, i, 3) and A not in orc.khop_nodes(G, j, 3)             # each hub is walked from one root only
    assert ref.differs_from_reference_mode(c['og'], c['seeds'], h, sample_n) >= 1
    full = ref.nodes(G, i, j, h)
    assert np.isin(G.preds(A), full).all() and np.isin(G.preds(B), full).all()
    assert (len(full) > sample_n) == (sample_n < 10000)


def test_large_case_tells_the_modes_apart():
    c = ref.large_case()
    og = [orc.Graph(*g) for g in c['graphs']]
    assert len(c['seeds']) == 8 and c['graphs'][0][0] > 650_000
    assert ref.differs_from_reference_mode(og, c['seeds'], c['h'], c['sample_n']) >= 1
    assert sum(len(ref.nodes(og[0], i, j, c['h'])) > c['sample_n'] for _, i, j in c['seeds'].tolist()) >= 2


@pytest.mark.parametrize('seed', ref.WHOLE_PATH_SEEDS)
def test_whole_path_cases_tell_the_modes_apart(seed):
    c = ref.whole_path_case(seed)
    assert len(c['dims']) == c['h'] + 1
    for seeds in c['spt_seeds'] + c['qry_seeds']:
        assert (seeds[:, 1] != seeds[:, 2]).all()
    assert ref.differs_from_reference_mode(c['og'], np.concatenate(c['spt_seeds'] + c['qry_seeds']), c['h'], c['sample_n']) >= 1


def test_whole_path_cases_cover_every_hop_count():
    assert {ref.whole_path_case(s)['h'] for s in ref.WHOLE_PATH_SEEDS} == {1, 2, 3}


@pytest.mark.parametrize('h', ref.SURFACE_HOPS)
def test_surface_queries_tell_the_modes_apart(h):
    d = ref.surface_dataset()
    og = [orc.Graph(*g) for g in d['graphs']]
    names = ref.surface_query_names(d)
    assert len(names) == ref.SURFACE['tasks']
    seeds = np.array([[int(x) for x in nm.split('_')] for task in names for nm in task], np.int32)
    assert ref.differs_from_reference_mode(og, seeds, h, ref.SURFACE['sample_nodes']) >= 1


def test_train_parse_link_hops():
    sys.path.insert(0, ROOT)
    import train
    base = ['--data_dir', 'x', '--task_setup', 'Shared']
    assert train.parse(base).link_hops == 'reference'
    assert train.parse(base + ['--link_hops', 'symmetric']).link_hops == 'symmetric'
    with pytest.raises(SystemExit):
        train.parse(base + ['--link_hops', 'both'])
