"""CPU: the restatement of the hop-distance node labels (tests/hop_label_ref.py) is validated on hand-checked graphs before the GPU tests trust
it -- a directed path, a star, a pair with a common neighbour, the D cap, an unreachable row, i == j -- the label widths, a labelled model with
zero label rows in W1 against the unlabelled oracle, and the library's three new symbols (exported, declared, the per-thread switch)."""
import ctypes
import threading

import numpy as np
import pytest

import gmeta_oracle as orc
import hop_label_ref as hl

f32 = np.float32


def _batch(n, edges, seeds, lists=None):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    g = [orc.Graph(n, e[:, 0], e[:, 1])]
    seeds = np.asarray(seeds, np.int32).reshape(-1, 3)
    return g, orc.Batch(g, seeds, lists if lists is not None else [np.arange(n)] * len(seeds))


def test_directed_path_counts_edges_towards_the_centre():
    # 0 -> 1 -> 2 -> 3 -> 4: d_4(v) = 4 - v along the edges; from centre 0 nothing else is reachable AGAINST the edges
    _, b = _batch(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [(0, 4, -1), (0, 0, -1)])
    lab = hl.labels(b, 7)
    assert lab.shape == (10, 1) and lab.dtype == np.int8
    assert lab[:5, 0].tolist() == [4, 3, 2, 1, 0]
    assert lab[5:, 0].tolist() == [0, 8, 8, 8, 8]


def test_the_cap_folds_farther_rows_into_the_last_bucket():
    _, b = _batch(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [(0, 4, -1)])
    assert hl.labels(b, 2)[:, 0].tolist() == [3, 3, 2, 1, 0]
    assert hl.labels(b, 1)[:, 0].tolist() == [2, 2, 2, 1, 0]
    assert hl.labels(b, 4)[:, 0].tolist() == [4, 3, 2, 1, 0]


def test_star_leaves_are_one_hop_from_the_hub_and_unreachable_from_each_other():
    # leaves 1..5 -> hub 0
    _, b = _batch(6, [(k, 0) for k in range(1, 6)], [(0, 0, -1), (0, 3, -1)])
    lab = hl.labels(b, 3)
    assert lab[:6, 0].tolist() == [0, 1, 1, 1, 1, 1]
    assert lab[6:, 0].tolist() == [4, 4, 4, 0, 4, 4]          # no path v -> ... -> 3 for any other v: the far / unreachable bucket D + 1


def test_pair_with_a_common_neighbour_is_told_from_a_one_sided_node():
    # 2 -> 0, 2 -> 1 (common in-neighbour of i = 0 and j = 1); 3 -> 0 only; 4 -> 3 (two hops from i, none to j)
    _, b = _batch(5, [(2, 0), (2, 1), (3, 0), (4, 3)], [(0, 0, 1)])
    lab = hl.labels(b, 3)
    assert lab.shape == (5, 2)
    assert lab.tolist() == [[0, 4], [4, 0], [1, 1], [1, 4], [2, 4]]
    x = hl.features(b, [np.zeros((5, 3), f32)], 3)
    assert x.shape == (5, 3 + 10)
    assert x[2].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0] and x[3].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]


def test_a_row_cut_off_by_sampling_is_unreachable():
    # 0 -> 1 -> 2, the subgraph keeps {0, 2}: the path through 1 is gone
    _, b = _batch(3, [(0, 1), (1, 2)], [(0, 2, -1)], [np.array([0, 2])])
    assert hl.labels(b, 3)[:, 0].tolist() == [4, 0]


def test_i_equal_j_gives_two_identical_blocks_and_self_loops_and_parallel_edges_change_nothing():
    edges = [(1, 0), (2, 1)]
    _, b = _batch(3, edges, [(0, 0, 0)])
    lab = hl.labels(b, 2)
    assert np.array_equal(lab[:, 0], lab[:, 1]) and lab[:, 0].tolist() == [0, 1, 2]
    x = hl.features(b, [np.ones((3, 2), f32)], 2)
    assert np.array_equal(x[:, 2:6], x[:, 6:10])
    _, b2 = _batch(3, edges + [(0, 0), (1, 1), (1, 0), (1, 0), (2, 1)], [(0, 0, 0)])
    assert np.array_equal(hl.labels(b2, 2), lab)


def test_label_widths():
    import gmeta_amd
    for D in range(1, 8):
        assert gmeta_amd.hop_label_width(D, False) == D + 2 == hl.width(D, False)
        assert gmeta_amd.hop_label_width(D, True) == 2 * (D + 2) == hl.width(D, True)
    assert gmeta_amd.hop_label_width(0, True) == 0 and gmeta_amd.hop_label_width(None, False) == 0
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            gmeta_amd.hop_label_width(bad, False)


@pytest.mark.parametrize('link', [False, True])
def test_zero_label_rows_in_w1_give_the_unlabelled_oracles_logits(link):
    rng = np.random.default_rng(5)
    n, F0, H, D = 40, 6, 16, 3
    e = rng.integers(0, n, size=(160, 2))
    g = [orc.Graph(n, e[:, 0], e[:, 1])]
    seeds = np.array([(0, int(rng.integers(0, n)), int(rng.integers(0, n)) if link else -1) for _ in range(5)], np.int32)
    b = orc.extract_batch(g, seeds, 2, 1000, 222, link)
    feats = [rng.standard_normal((n, F0)).astype(f32)]
    Lw = hl.width(D, link)
    config = lambda f: [('GraphConv', [f, H]), ('GraphConv', [H, H]), ('Linear', [H, 3])] + ([('LinkPred', [True])] if link else [])      # noqa: E731
    th = [rng.standard_normal((F0, H)).astype(f32), rng.standard_normal(H).astype(f32), rng.standard_normal((H, H)).astype(f32), rng.standard_normal(H).astype(f32),
          rng.standard_normal((3, H * (2 if link else 1))).astype(f32), rng.standard_normal(3).astype(f32)]
    thl = [np.vstack([th[0], np.zeros((Lw, H), f32)])] + th[1:]
    x = hl.features(b, feats, D)
    assert x.shape == (b.n, F0 + Lw) and np.array_equal(x[:, :F0], b.features(feats)) and (x[:, F0:].sum(axis=1) == (2 if link else 1)).all()
    plain, _ = orc.classifier_forward(b, b.features(feats), th, config(F0))
    lab, _ = orc.classifier_forward(b, x, thl, config(F0 + Lw))
    np.testing.assert_allclose(lab, plain, atol=1e-6, rtol=0)


def test_the_library_exports_the_hop_label_symbols_and_the_binding_declares_them():
    import gmeta_amd  # noqa: F401
    from gmeta_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gm_set_hop_labels', 'gm_get_hop_labels', 'gm_batch_hop_labels'):
        assert hasattr(raw, name), 'libgmeta_hip.so does not export %s' % name
        assert name in _lib.PROTOTYPES
    assert _lib.F_HOP == _lib.F_EDGE_W_T + 1                  # appended at the end of enum gm_field
    lib = _lib.lib()
    assert lib.gm_get_hop_labels() == 0                       # off by default
    try:
        lib.gm_set_hop_labels(3)
        assert lib.gm_get_hop_labels() == 3
        for bad in (8, -1):                                   # ignored, with an error string
            lib.gm_set_hop_labels(bad)
            assert lib.gm_get_hop_labels() == 3 and b'gm_set_hop_labels' in lib.gm_last_error()
        seen = []
        t = threading.Thread(target=lambda: seen.append(lib.gm_get_hop_labels()))      # per calling thread
        t.start(); t.join()
        assert seen == [0]
        with gmeta_amd.hop_labels_switch(5):
            assert lib.gm_get_hop_labels() == 5
        assert lib.gm_get_hop_labels() == 3                   # the block restores what it found
    finally:
        lib.gm_set_hop_labels(0)
    assert lib.gm_batch_hop_labels(None) == 0
