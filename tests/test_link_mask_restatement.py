"""CPU: the restatement of target-link masking (tests/link_mask_ref.py, GM_LINK_MASK_TARGET) against a brute-force filter of the edge list, against the
unmasked oracle on the pairs the mask has nothing to do for, the header's remark on the node sets, what the mask does to the hop labels, and the
declaration of the flag and its getter in the header and the binding (the one test here that loads the library)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, ROOT)
import gmeta_oracle as orc      # noqa: E402
import hop_label_ref as hop     # noqa: E402
import link_mask_ref as ref     # noqa: E402
import link_sym_ref as sym      # noqa: E402

SEEDS = sym.FUZZ_SEEDS


@pytest.fixture(scope='module')
def cases():
    return {s: ref.fuzz_case(s) for s in SEEDS}


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('seed', SEEDS)
def test_restated_csr_is_the_brute_force_filter_of_the_edge_list(cases, seed, mode):
    c = cases[seed]
    lists = ref.node_lists(c['og'], c['seeds'], c['h'], c['sample_n'], mode)
    b = ref.batch_from_lists(c['og'], c['seeds'], lists)
    worked = 0
    for s, ((g, i, j), nodes) in enumerate(zip(c['seeds'].tolist(), lists)):
        r0, r1 = int(b.sub_off[s]), int(b.sub_off[s + 1])
        assert np.array_equal(b.parent[r0:r1], nodes)
        ip, ix = ref.brute_force_csr(c['graphs'][g], nodes, i, j)
        assert np.array_equal(b.indptr[r0:r1 + 1] - b.indptr[r0], ip), (s, g, i, j)
        assert np.array_equal(b.indices[b.indptr[r0]:b.indptr[r1]] - r0, ix), (s, g, i, j)
        uip, _ = orc.induce(c['og'][g], nodes)
        worked += int(uip[-1] != ip[-1])
        assert uip[-1] - ip[-1] == ref.adjacent(c['og'][g], i, j)                  # both centres are always inside: every target edge goes
        # masked_from edits two rows of the built CSR; masked_graph filters the edge list and builds the graph again
        M, F = ref.masked_from(c['og'][g], i, j), ref.masked_graph(*c['graphs'][g], i, j)
        assert np.array_equal(M.indptr, F.indptr) and np.array_equal(M.indices, F.indices)
    assert worked >= 5


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('seed', SEEDS)
def test_non_adjacent_pairs_reproduce_the_unmasked_oracle(cases, seed, mode):
    c = cases[seed]
    keep = np.array([ref.adjacent(c['og'][g], i, j) == 0 for g, i, j in c['seeds'].tolist()])
    assert keep[c['planted']['non_adjacent']] and keep[c['planted']['isolated_j']] and keep[c['planted']['via_third']] and keep.sum() >= 3
    seeds = c['seeds'][keep]
    m, u = ref.extract_batch(c['og'], seeds, c['h'], c['sample_n'], mode), ref.unmasked_batch(c['og'], seeds, c['h'], c['sample_n'], mode)
    for f in ('parent', 'indptr', 'indices', 'centre_rows', 'sub_off', 'graph_id'):
        assert np.array_equal(getattr(m, f), getattr(u, f)), f
    assert np.array_equal(m.norm.view(np.uint32), u.norm.view(np.uint32))


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('seed', SEEDS)
def test_node_lists_do_not_depend_on_the_mask(cases, seed, h):
    """The header's remark: the expansion on the masked graph gives the unmasked node set, in both pair modes (checked with the expansion actually run
    on every pair's masked graph, before and after sampling)."""
    c = cases[seed]
    for mode in ref.MODES:
        for sample_n in (10000, c['sample_n']):
            a = ref.node_lists(c['og'], c['seeds'], h, sample_n, mode)
            b = ref.masked_node_lists(c['og'], c['seeds'], h, sample_n, mode)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (mode, sample_n)


def _dataset_pairs(inject):
    from gmeta_amd import synth
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=inject)
    names, labels = d['tables']['train']
    seeds = np.array([[int(x) for x in nm.split('_')] for nm in names], np.int32)
    return d, seeds, np.array([int(l) for l in labels])


def test_inject_negatives_false_keeps_everything_but_the_negative_edges():
    a, sa, la = _dataset_pairs(True)
    b, sb, lb = _dataset_pairs(False)
    assert np.array_equal(sa, sb) and np.array_equal(la, lb) and a['info'] == b['info'] and a['tables'] == b['tables']
    assert all(np.array_equal(x, y) for x, y in zip(a['feats'], b['feats']))
    for g, ((n, s, d), (n2, s2, d2)) in enumerate(zip(a['graphs'], b['graphs'])):
        pos = sa[(sa[:, 0] == g) & (la == 1)]
        assert n == n2 and len(s) == 2 * len(s2) and np.array_equal(s[:len(s2)], s2) and np.array_equal(d[:len(d2)], d2)
        assert sorted(map(tuple, pos[:, 1:].tolist())) == sorted(zip(s2.tolist(), d2.tolist()))


@pytest.mark.parametrize('mode', ref.MODES)
def test_hop_labels_leak_the_link_only_without_the_mask(mode):
    """On graphs that hold the positives only: unmasked, label_j(i) or label_i(j) is 1 for exactly the positive pairs -- the label is the answer; masked,
    neither is ever 1."""
    d, seeds, y = _dataset_pairs(False)
    assert (seeds[:, 1] != seeds[:, 2]).all() and 0 < y.sum() < len(y)
    og = [orc.Graph(*g) for g in d['graphs']]
    for sample_n in (8, 10000):
        u, m = ref.unmasked_batch(og, seeds, 2, sample_n, mode), ref.extract_batch(og, seeds, 2, sample_n, mode)
        assert np.array_equal(u.parent, m.parent)
        lu, lm = hop.labels(u, 3), hop.labels(m, 3)
        ci, cj = m.centre_rows[:, 0], m.centre_rows[:, 1]
        leak = (lu[ci, 1] == 1) | (lu[cj, 0] == 1)
        assert np.array_equal(leak, y == 1)
        assert (lm[ci, 1] != 1).all() and (lm[cj, 0] != 1).all()
        assert (lm[ci, 0] == 0).all() and (lm[cj, 1] == 0).all()


def test_header_and_binding_declare_the_flag_and_the_getter():
    from gmeta_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    assert re.search(r'^#define\s+GM_LINK_MASK_TARGET\s+4\s*$', text, re.M)
    assert re.search(r'^int32_t\s+gm_batch_mask_target\s*\(\s*const\s+gm_batch_t\s*\*\s*b\s*\)\s*;', text, re.M)
    assert _lib.LINK_MASK_TARGET == 4 and _lib.LINK_MASK_TARGET & (_lib.LINK_SYMMETRIC | 1) == 0
    assert 'gm_batch_mask_target' in _lib.PROTOTYPES
    fn = _lib.lib().gm_batch_mask_target
    assert fn.restype is _lib.i32 and fn(None) == 0           # (a NULL batch is not masked)
