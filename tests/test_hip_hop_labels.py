"""GPU (-m gpu): opt-in hop-distance node labels (include/gmeta_hip.h, gm_set_hop_labels) from the BFS kernel to the meta-step, against the CPU
restatement tests/hop_label_ref.py (validated by tests/test_hop_label_restatement.py) and the oracle run on the labelled rows x'.

One directed multigraph of 300 nodes (random edges of in-degree ~3, self loops, parallel edges, an isolated node, a node with 40 in-neighbours: above the
batch's heavy-degree threshold) serves every small case; the label exactness cases add graphs made by hand.  The model cases run hidden 128 at
dims[0] = 64 (nodes: 59 features + 5 label columns, pairs: 54 + 10) with the split GEMM / weight-gradient kernels forced onto the small batches, so
that the fused feeders and the table-formed weight gradient read the batch's own feature table; 2 tasks, 2-way, k_spt 2, k_qry 3, K = 2."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, ROOT)
import gmeta_oracle as orc       # noqa: E402
import hop_label_ref as hl       # noqa: E402
import link_sym_ref as lsr       # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4                       # the project's parity tolerance (tests/test_hip_fuzz.py)
f32 = np.float32
N, HID, T, C_WAY, K_SPT, K_QRY, K, LR, D = 300, 128, 2, 2, 2, 3, 2, 0.005, 3
FORCE = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
SCHEDULES = (('dense', {}), ('hoist_z1', dict(hoist_z1=1)), ('sparse_bwd', dict(sparse_bwd=1)), ('cone', dict(cone=1)), ('cone+hoist', dict(cone=1, hoist_z1=1)))
LINK = {'node': False, 'link': True, 'link_sym': 2}
F0_OF = {'node': 59, 'link': 54, 'link_sym': 54}      # dims[0] = 64 with D = 3 either way


class tuning:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from gmeta_amd import _lib
        self.lib = _lib.lib()
        self.prev = {k: self.lib.gm_get_tuning(k.encode()) for k in self.kv}
        for k, v in self.kv.items():
            _lib.check(self.lib.gm_set_tuning(k.encode(), v), 'set_tuning')
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.lib.gm_set_tuning(k.encode(), v)
        return False


def switch(d):
    import gmeta_amd
    return gmeta_amd.hop_labels_switch(d)


def graph_a():
    rng = np.random.default_rng(11)
    e = [(int(u), int(v)) for u, v in rng.integers(1, N - 1, size=(3 * N, 2))]      # node 0 and node N - 1 get no random edge
    e += [(u, 0) for u in range(1, 41)] + [(0, 50), (0, 60)]                        # node 0: 40 in-neighbours
    e += [(5, 5), (6, 6), (5, 6), (5, 6), (5, 6), (7, 6)]                           # self loops, parallel edges
    e = np.array(e, np.int64)                                                       # N - 1: isolated
    assert not (e == N - 1).any()
    return N, e[:, 0], e[:, 1]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def extract(store, seeds, off, h, sample_n, link, d):
    from gmeta_amd.subgraphs import SubgraphBatch
    with switch(d):
        return SubgraphBatch.extract(store, np.asarray(seeds, np.int32), off, h, sample_n, 222, link)


def ref_batch(graphs, seeds, h, sample_n, link):
    seeds = np.asarray(seeds, np.int32)
    if link == 2:
        return orc.Batch(graphs, seeds, lsr.node_lists(graphs, seeds, h, sample_n))
    return orc.extract_batch(graphs, seeds, h, sample_n, 222, bool(link))


def check_labels(B, ob, d):
    """GM_F_HOP of a labelled batch against the restatement on the oracle's batch (same node sets first), exactly."""
    assert np.array_equal(B.parent(), ob.parent)
    assert B.hop_labels_cap == d
    want = hl.labels(ob, d)
    got = B.hop_labels
    assert got.dtype == np.int8 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    return want


# ---------------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize('mode,h', [('node', 1), ('node', 2), ('node', 3), ('link', 2), ('link_sym', 2)])
def test_hop_field_is_the_restatement(mode, h):
    import gmeta_amd
    n, src, dst = graph_a()
    store = gmeta_amd.GraphStore([(n, src, dst)], [np.zeros((n, 4), f32)])
    g = [orc.Graph(n, src, dst)]
    centres = [0, 5, 6, 7, 50, 60, N - 1, 123, 222]
    seeds = [(0, i, -1 if mode == 'node' else centres[(k + 3) % len(centres)]) for k, i in enumerate(centres)]
    ob = ref_batch(g, seeds, h, 1000, LINK[mode])
    for d in (1, 3, 7):
        B = extract(store, seeds, [0, 4, len(seeds)], h, 1000, LINK[mode], d)
        lab = check_labels(B, ob, d)
        assert lab.shape[1] == (1 if mode == 'node' else 2)
        assert B.feat_dim == 4 + gmeta_amd.hop_label_width(d, mode != 'node')
    assert (lab[:, 0] == 0).sum() == len(seeds)                                    # one centre row per subgraph


def test_sampling_that_disconnects_rows_fills_the_far_bucket():
    import gmeta_amd
    n, src, dst = graph_a()
    store = gmeta_amd.GraphStore([(n, src, dst)], [np.zeros((n, 4), f32)])
    g = [orc.Graph(n, src, dst)]
    seeds = [(0, i, -1) for i in (0, 50, 60, 100, 150, 200)]
    ob = orc.extract_batch(g, np.asarray(seeds, np.int32), 2, 6, 222, False)
    lab = check_labels(extract(store, seeds, [0, len(seeds)], 2, 6, False, 7), ob, 7)
    # every node of a 2-hop neighbourhood is within two hops of its centre: only a path cut by the sampling puts a row into bucket D + 1 = 8
    assert (lab == 8).any() and not ((lab > 2) & (lab < 8)).any()
    pairs = [(0, 0, 50), (0, 60, 0), (0, 100, 150)]
    obp = orc.extract_batch(g, np.asarray(pairs, np.int32), 2, 6, 222, True)
    labp = check_labels(extract(store, pairs, [0, len(pairs)], 2, 6, True, 7), obp, 7)
    assert (labp == 8).any()


def test_given_node_lists_a_weighted_store_one_row_and_i_equal_j():
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    n, src, dst = graph_a()
    rng = np.random.default_rng(3)
    wt = np.exp(rng.uniform(-1, 1, size=len(src))).astype(f32)
    g = [orc.Graph(n, src, dst)]
    plain = gmeta_amd.GraphStore([(n, src, dst)], [np.zeros((n, 4), f32)])
    weighted = gmeta_amd.GraphStore([(n, src, dst)], [np.zeros((n, 4), f32)], edge_weights=[wt])
    # gm_batch_from_nodes: arbitrary node sets (what sample_mode='reference' replays), nodes and pairs
    seeds = np.array([(0, 0, -1), (0, 6, -1), (0, 77, -1)], np.int32)
    lists = [np.unique(np.concatenate([[int(s[1])], rng.choice(n, 60, replace=False)])) for s in seeds]
    with switch(4):
        B = SubgraphBatch.from_nodes(plain, seeds, [0, 3], lists, False)
    check_labels(B, orc.Batch(g, seeds, lists), 4)
    pseeds = np.array([(0, 0, 6), (0, 77, 5)], np.int32)
    plists = [np.unique(np.concatenate([[int(s[1]), int(s[2])], rng.choice(n, 80, replace=False)])) for s in pseeds]
    with switch(2):
        B = SubgraphBatch.from_nodes(plain, pseeds, [0, 2], plists, True)
    check_labels(B, orc.Batch(g, pseeds, plists), 2)
    # a weighted store: distances are topological
    seeds = [(0, i, -1) for i in (0, 6, 50)]
    Bw, Bp = extract(weighted, seeds, [0, 3], 2, 1000, False, 3), extract(plain, seeds, [0, 3], 2, 1000, False, 3)
    assert Bw.weighted and not Bp.weighted
    check_labels(Bw, orc.extract_batch(g, np.asarray(seeds, np.int32), 2, 1000, 222, False), 3)
    assert np.array_equal(Bw.hop_labels, Bp.hop_labels)
    # a one-row subgraph (the isolated node), alone and among others
    for sd in ([(0, N - 1, -1)], [(0, 5, -1), (0, N - 1, -1), (0, 0, -1)]):
        B = extract(plain, sd, [0, len(sd)], 2, 1000, False, 3)
        lab = check_labels(B, orc.extract_batch(g, np.asarray(sd, np.int32), 2, 1000, 222, False), 3)
        k = [s[1] for s in sd].index(N - 1)
        assert B.sub_off[k + 1] - B.sub_off[k] == 1 and lab[B.sub_off[k], 0] == 0
    # pairs with i == j: two identical blocks (both pair modes)
    for link in (True, 2):
        sd = [(0, 6, 6), (0, 0, 0), (0, 50, 60)]
        B = extract(plain, sd, [0, 3], 2, 1000, link, 3)
        lab = check_labels(B, ref_batch(g, sd, 2, 1000, link), 3)
        r = B.sub_off
        assert np.array_equal(lab[:r[2], 0], lab[:r[2], 1]) and not np.array_equal(lab[r[2]:, 0], lab[r[2]:, 1])


def test_a_subgraph_above_the_lds_limit_takes_the_global_memory_path():
    """k_hop_labels keeps the distance bytes in LDS up to 2,048 rows per subgraph (GM_HOP_LDS_ROWS) and in the output array above: one subgraph of 2,601 rows
    from an extraction with sample_nodes above the limit, and one of 2,500 given nodes whose distances use all seven levels."""
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    rng = np.random.default_rng(8)
    n = 2601
    e = [(k, 0) for k in range(1, 1301)] + [(1300 + k, k) for k in range(1, 1301)]          # 1,300 in-neighbours of node 0, each with one of its own
    e += [(int(u), int(v)) for u, v in rng.integers(1, n, size=(2000, 2))]                  # shortcuts, parallel edges, self loops among them
    e = np.array(e, np.int64)
    store = gmeta_amd.GraphStore([(n, e[:, 0], e[:, 1])], [np.zeros((n, 4), f32)])
    g = [orc.Graph(n, e[:, 0], e[:, 1])]
    for sd, link in (([(0, 0, -1)], False), ([(0, 0, 1300)], True)):
        ob = orc.extract_batch(g, np.asarray(sd, np.int32), 2, 4000, 222, link)
        assert ob.n == n > 2048
        lab = check_labels(extract(store, sd, [0, 1], 2, 4000, link, 3), ob, 3)
        assert set(np.unique(lab[:, 0]).tolist()) == {0, 1, 2}
    # sparse random graph, every node given: breadth-first depth ~ log2(n), so that all of the levels 1..7 and the far bucket occur
    n2 = 2500
    e2 = rng.integers(0, n2, size=(2 * n2, 2)).astype(np.int64)
    store2 = gmeta_amd.GraphStore([(n2, e2[:, 0], e2[:, 1])], [np.zeros((n2, 4), f32)])
    g2 = [orc.Graph(n2, e2[:, 0], e2[:, 1])]
    seeds = np.array([(0, 17, 1234), (0, 3, 4)], np.int32)
    lists = [np.arange(n2), np.arange(40)]                                                  # (the second subgraph: the LDS path in the same launch)
    with switch(7):
        B = SubgraphBatch.from_nodes(store2, seeds, [0, 2], lists, True)
    lab = check_labels(B, orc.Batch(g2, seeds, lists), 7)
    assert set(np.unique(lab[:n2, 0]).tolist()) == set(range(9))


# ---------------------------------------------------------------------------------------------------- the labelled feature table
@pytest.mark.parametrize('mode,F0', [('node', 16), ('node', 59), ('link', 54), ('link', 7)])
def test_gather_features_returns_the_labelled_rows_bitwise(mode, F0):
    """Widths 21 (not a multiple of 4) and 64 for nodes; 64 and 17 for pairs."""
    import gmeta_amd
    from gmeta_amd import _lib
    n, src, dst = graph_a()
    rng = np.random.default_rng(F0)
    feats = [rng.standard_normal((n, F0)).astype(f32)]
    store = gmeta_amd.GraphStore([(n, src, dst)], feats)
    g = [orc.Graph(n, src, dst)]
    seeds = [(0, i, -1 if mode == 'node' else j) for i, j in ((0, 50), (6, 6), (N - 1, 7), (123, 60))]
    B = extract(store, seeds, [0, 2, 4], 2, 1000, LINK[mode], D)
    ob = ref_batch(g, seeds, 2, 1000, LINK[mode])
    want = hl.features(ob, feats, D)
    assert B.feat_dim == want.shape[1] == F0 + hl.width(D, mode != 'node')
    x = torch.full((B.rows, B.feat_dim), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(_lib.lib().gm_gather_features(B.handle, _lib.ptr(x), _lib.stream_ptr()), 'gm_gather_features')
    torch.cuda.synchronize()
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want))
    # GM_F_FEAT_ROW keeps its documented meaning: the row of the STORE's feature matrix
    assert np.array_equal(B._read(_lib.F_FEAT_ROW, B.rows, np.int32), ob.parent)


# ---------------------------------------------------------------------------------------------------- the model on labelled batches
class World:
    """The graph, one task layout per mode, labelled and unlabelled parameters with every bias off the relu kink (tests/test_hip_fuzz.py: why); small
    features, head weights and inner step as in tests/test_hip_edge_weights.py (node 0's row sums 40 sources)."""

    def __init__(self, mode):
        self.mode, self.link, self.F0 = mode, LINK[mode], F0_OF[mode]
        self.n, self.src, self.dst = graph_a()
        rng = np.random.default_rng(77)
        self.feats = [(0.2 * rng.standard_normal((N, self.F0))).astype(f32)]
        self.Lw = hl.width(D, bool(self.link))
        assert self.F0 + self.Lw == 64
        node = [[(0, 50, 6, N - 1), (123, 60, 5, 0, 222, 7)], [(60, 6, 200, 0), (7, N - 1, 250, 50, 101, 33)]]
        other = {0: 50, 50: 0, 6: 7, N - 1: 5, 123: 60, 60: 6, 5: 7, 222: 123, 7: 0, 200: 201, 250: 6, 101: 33, 33: 50}      # (no i == j: such a pair sends cone back to dense)
        self.seeds = [[np.array([(0, i, -1 if mode == 'node' else other[i]) for i in part], np.int32) for part in tq] for tq in node]
        self.ys = [np.repeat(np.arange(C_WAY), K_SPT).astype(np.int32) for _ in range(T)]
        self.yq = [np.repeat(np.arange(C_WAY), K_QRY).astype(np.int32) for _ in range(T)]
        self.config = self.config_for(self.F0 + self.Lw)
        gcn, lin, _ = orc.parse_config(self.config)
        th = []
        for fi, fo in gcn:
            th += [(rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(f32), (rng.uniform(0.15, 0.4, fo) * rng.choice([-1.0, 1.0], fo)).astype(f32)]
        hc = lin[0] * (2 if self.link else 1)
        th += [(0.3 * rng.standard_normal((lin[1], hc)) / np.sqrt(hc)).astype(f32), (rng.uniform(0.15, 0.4, lin[1]) * rng.choice([-1.0, 1.0], lin[1])).astype(f32)]
        self.theta = th
        self._ref = {}

    def config_for(self, f_in):
        return [('GraphConv', [f_in, HID]), ('GraphConv', [HID, HID]), ('Linear', [HID, C_WAY])] + ([('LinkPred', [True])] if self.link else [])

    def args(self):
        return argparse.Namespace(update_lr=LR, meta_lr=1e-3, n_way=C_WAY, k_spt=K_SPT, k_qry=K_QRY, task_num=T, update_step=K, update_step_test=K,
                                  method='G-Meta', sample_nodes=1000, link_pred_mode='True' if self.link else 'False', task_setup='Shared', h=2)

    def store(self):
        import gmeta_amd
        return gmeta_amd.GraphStore([(self.n, self.src, self.dst)], self.feats)

    def batches(self, store, d=D):
        out = []
        for part, per in ((0, C_WAY * K_SPT), (1, C_WAY * K_QRY)):
            out.append(extract(store, np.concatenate([s[part] for s in self.seeds]), np.arange(T + 1) * per, 2, 1000, self.link, d))
        return out

    def meta(self, theta=None, config=None, **flags):
        import gmeta_amd
        m = gmeta_amd.Meta(self.args(), config or self.config).to('cuda')
        with torch.no_grad():
            for p, v in zip(m.net.parameters(), theta or self.theta):
                p.copy_(torch.from_numpy(v))
        for k, v in flags.items():
            setattr(m, k, v)
        return m

    def labels(self):
        return [torch.from_numpy(y.astype(np.int64)) for y in self.ys], [torch.from_numpy(y.astype(np.int64)) for y in self.yq]

    def step(self, S, Q, need_grad=True, theta=None, config=None, **flags):
        """gm_meta_step's whole `out` (host copy) and P."""
        ys, yq = self.labels()
        out, P, _ = self.meta(theta, config, **flags)._run(S.views(), ys, Q.views(), yq, K, need_grad)
        return out.cpu().numpy().copy(), P

    def ref_batches(self):
        if 'b' not in self._ref:
            g = [orc.Graph(self.n, self.src, self.dst)]
            self._ref['b'] = tuple([ref_batch(g, self.seeds[t][part], 2, 1000, self.link) for t in range(T)] for part in (0, 1))
        return self._ref['b']

    def reference(self, need_grad):
        """(accs, flat grad or None, losses_q) of the oracle's inner loop on the labelled rows (computed once)."""
        if need_grad not in self._ref:
            spt, qry = self.ref_batches()
            accs, grad, lq = hl.meta_step(self.feats, spt, qry, self.ys, self.yq, self.theta, self.config, K_SPT, LR, K, D, need_grad)
            self._ref[need_grad] = (np.asarray(accs), np.concatenate([x.reshape(-1) for x in grad]) if need_grad else None, np.asarray(lq))
        return self._ref[need_grad]


_WORLDS = {}


def world(mode):
    if mode not in _WORLDS:
        _WORLDS[mode] = World(mode)
    return _WORLDS[mode]


def split_out(out, P):
    """mean meta-gradient, mean losses_q, mean accuracies, violation word of a gm_meta_step `out`."""
    return out[:P] / T, out[P:P + K + 1] / T, out[P + K + 1:P + 2 * K + 2] / T, out[-1]


def assert_step_close(out, P, accs, grad, lq, what):
    g, l, a, viol = split_out(out, P)
    assert viol == 0, what
    np.testing.assert_allclose(l, lq, atol=TOL, rtol=1e-4, err_msg=what)
    if grad is not None:
        np.testing.assert_allclose(g, grad, atol=TOL * max(1.0, float(np.abs(grad).max())), rtol=1e-3, err_msg=what)
    assert np.abs(a - accs).max() <= 1.0 / (C_WAY * K_QRY) + 1e-6, what      # argmax decisions: equal unless two distances tie within noise


@pytest.mark.parametrize('mode', ['node', 'link'])
def test_gcn_forward_and_backward_match_the_oracle_on_the_labelled_rows(mode):
    w = world(mode)
    rspt, _ = w.ref_batches()
    rng = np.random.default_rng(4)
    close = lambda got, want, what: np.testing.assert_allclose(got, want, atol=TOL * max(1.0, float(np.abs(want).max())), rtol=1e-4, err_msg=what)      # noqa: E731
    for force in (FORCE, {}):                                                       # the split kernels, and the library's own choice at this size
        with tuning(**force):
            store = w.store()
            B0 = extract(store, w.seeds[0][0], [0, C_WAY * K_SPT], 2, 1000, w.link, D)
            m = w.meta()
            logits, _ = m.net(B0, None, None)
            R = rng.standard_normal((B0.subs, C_WAY)).astype(f32)
            (logits * torch.from_numpy(R).cuda()).sum().backward()
            rl, cache = orc.classifier_forward(rspt[0], hl.features(rspt[0], w.feats, D), w.theta, w.config)
            rg = np.concatenate([g.reshape(-1) for g in orc.classifier_backward(rspt[0], w.theta, w.config, cache, R)])
            close(logits.detach().cpu().numpy(), rl, 'gcn_forward')
            close(torch.cat([p.grad.reshape(-1) for p in m.net.parameters()]).cpu().numpy(), rg, 'gcn_backward')


@pytest.mark.parametrize('mode', ['node', 'link', 'link_sym'])
def test_meta_step_matches_the_oracle_on_every_schedule(mode):
    """Training step and fine-tuning, the five schedules, the fused aggregate + GEMM on and off."""
    from gmeta_amd import _lib
    w = world(mode)
    lib = _lib.lib()
    with tuning(**FORCE):
        S, Q = w.batches(w.store())
        assert S.hop_labels_cap == D and Q.feat_dim == 64
        for need_grad in (True, False):
            accs, grad, lq = w.reference(need_grad)
            for name, flags in SCHEDULES:
                for fuse in (1, 0):
                    lib.gm_set_fuse_agg(fuse)
                    try:
                        out, P = w.step(S, Q, need_grad, **flags)
                    finally:
                        lib.gm_set_fuse_agg(-1)
                    assert_step_close(out, P, accs, grad, lq, '%s, %s, fuse_agg=%d, need_grad=%s' % (mode, name, fuse, need_grad))


@pytest.mark.parametrize('mode', ['node', 'link'])
def test_adapt_and_predict_on_a_labelled_query_batch(mode):
    w = world(mode)
    with tuning(**FORCE):
        S, Q = w.batches(w.store())
        ys, yq = w.labels()
        m = w.meta()
        fb = m.finetunning_batch(S.views(), ys, Q.views(), yq)
        accs, _, _ = w.reference(False)
        assert np.abs(fb.mean(axis=0) - accs).max() <= 1.0 / (C_WAY * K_QRY) + 1e-6
        for j in range(K + 1):
            pr = m.adapt(S.views(), ys, K=j).predict(Q.views())
            for t in range(T):
                y = yq[t].numpy()
                assert f32(np.count_nonzero(pr.labels[t] == y)) / f32(len(y)) == f32(fb[t, j]), (j, t)


@pytest.mark.parametrize('mode', ['node', 'link'])
def test_zero_label_rows_in_w1_give_the_unlabelled_model(mode):
    """theta' = theta with zero rows appended to W1: the labelled step returns the unlabelled step's numbers (W1's gradient: its first F0 rows).  The
    unlabelled model runs at dims[0] = F0 padded to 64 inside the library, the labelled one at 64: a wrong cut / shift of either padding shows here."""
    w = world(mode)
    rng = np.random.default_rng(12)
    th_u = [(rng.standard_normal((w.F0, HID)) / np.sqrt(w.F0)).astype(f32)] + w.theta[1:]
    th_l = [np.vstack([th_u[0], np.zeros((w.Lw, HID), f32)])] + w.theta[1:]
    with tuning(**FORCE):
        store = w.store()
        Su, Qu = w.batches(store, 0)
        Sl, Ql = w.batches(store, D)
        assert Su.hop_labels_cap == 0 and Su.feat_dim == w.F0 and Sl.feat_dim == 64
        for name, flags in SCHEDULES:
            for need_grad in (True, False):
                ou, Pu = w.step(Su, Qu, need_grad, th_u, w.config_for(w.F0), **flags)
                ol, Pl = w.step(Sl, Ql, need_grad, th_l, **flags)
                gu, lu, au, _ = split_out(ou, Pu)
                gl, ll, al, viol = split_out(ol, Pl)
                cut = w.F0 * HID
                assert viol == 0 and Pl - Pu == w.Lw * HID
                np.testing.assert_allclose(ll, lu, atol=TOL, rtol=1e-4, err_msg=name)
                assert np.abs(al - au).max() <= 1.0 / (C_WAY * K_QRY) + 1e-6, name      # argmax decisions: equal unless two distances tie within noise
                if need_grad:
                    glu = np.concatenate([gl[:cut], gl[cut + w.Lw * HID:]])
                    np.testing.assert_allclose(glu, gu, atol=TOL * max(1.0, float(np.abs(gu).max())), rtol=1e-3, err_msg=name)


# ---------------------------------------------------------------------------------------------------- errors, guards, the switch
def test_concat_and_the_model_check_name_their_cause():
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    w = world('node')
    store = w.store()
    Sl, Ql = w.batches(store, D)
    Su, Qu = w.batches(store, 0)
    S2, _ = w.batches(store, 2)
    cat = SubgraphBatch.concat([Sl, Ql])                                             # two labelled batches: the concatenation
    assert cat.hop_labels_cap == D and cat.feat_dim == 64 and cat.rows == Sl.rows + Ql.rows
    assert np.array_equal(cat.hop_labels, np.concatenate([Sl.hop_labels, Ql.hop_labels]))
    assert np.array_equal(cat._read(_lib.F_FEAT_ROW, cat.rows, np.int32), np.concatenate([Sl.parent(), Ql.parent()]))
    xs = []
    for B in (cat, Sl, Ql):
        x = torch.empty((B.rows, B.feat_dim), dtype=torch.float32, device='cuda')
        _lib.check(_lib.lib().gm_gather_features(B.handle, _lib.ptr(x), _lib.stream_ptr()), 'gm_gather_features')
        xs.append(x.cpu().numpy())
    assert np.array_equal(_bits(xs[0]), _bits(np.concatenate(xs[1:])))
    assert SubgraphBatch.concat([Su, Qu]).hop_labels_cap == 0
    for parts in ([Sl, Qu], [Su, Ql], [Sl, S2]):                                     # labelled + unlabelled, two different caps
        with pytest.raises(ValueError, match='all be labelled with the same D, or all unlabelled'):
            SubgraphBatch.concat(parts)
    with pytest.raises(ValueError, match='no hop labels'):                           # GM_F_HOP on an unlabelled batch
        Su.hop_labels
    ys, yq = w.labels()
    m = w.meta(theta=[w.theta[0][:w.F0]] + w.theta[1:], config=w.config_for(w.F0))   # the unlabelled dims[0] on labelled batches
    with pytest.raises(ValueError) as ei:
        m._run(Sl.views(), ys, Ql.views(), yq, K, True)
    assert 'dims[0]=59' in str(ei.value) and '64' in str(ei.value) and 'hop-label' in str(ei.value)
    with pytest.raises(ValueError) as ei:
        m.net(Sl, None, None)
    assert 'dims[0]=59' in str(ei.value) and '64' in str(ei.value)
    # ... and a wrong dims[0] on unlabelled ones, in the words used before (60: neither the store's 59 features nor its padded row of 64, which the
    # library has always taken as the same model with zero rows in W1)
    m60 = w.meta(theta=[np.vstack([w.theta[0][:w.F0], np.zeros((1, HID), f32)])] + w.theta[1:], config=w.config_for(w.F0 + 1))
    with pytest.raises(ValueError) as ei:
        m60._run(Su.views(), ys, Qu.views(), yq, K, True)
    assert 'dims[0]=60' in str(ei.value) and '59' in str(ei.value) and 'hop-label' not in str(ei.value)
    with pytest.raises(ValueError, match='hop labels D='):                           # a labelled support batch with an unlabelled query batch
        w.meta()._run(Sl.views(), ys, Qu.views(), yq, K, True)


def test_off_means_untouched_after_a_labelled_build_on_the_same_thread():
    from gmeta_amd import _lib
    w = world('link')
    fields = [(_lib.F_SUB_OFF, 'subs+1', np.int32), (_lib.F_SET_SUB_OFF, 'sets+1', np.int32), (_lib.F_PARENT, 'rows', np.int32), (_lib.F_GRAPH, 'subs', np.int32),
              (_lib.F_INDPTR, 'rows+1', np.int32), (_lib.F_INDICES, 'edges', np.int32), (_lib.F_INDPTR_T, 'rows+1', np.int32), (_lib.F_INDICES_T, 'edges', np.int32),
              (_lib.F_CENTRE, 'subs*centres', np.int32), (_lib.F_NORM, 'rows', np.uint32), (_lib.F_FEAT_ROW, 'rows', np.int32), (_lib.F_NORM_SRC, 'rows', np.uint32),
              (_lib.F_NORM_CENTRE, 'rows', np.uint32)]

    def snapshot(B):
        dims = dict(rows=B.rows, edges=B.edges, subs=B.subs, sets=B.sets, centres=B.centres)
        out = []
        for f, n, dt in fields:
            a = np.empty(eval(n, {}, dims), dt)
            _lib.check(_lib.lib().gm_batch_read(B.handle, f, _lib.ptr(a), a.nbytes), 'gm_batch_read')
            out.append(a)
        return out
    th = [w.theta[0][:w.F0]] + w.theta[1:]
    with tuning(**FORCE):
        store = w.store()
        assert _lib.lib().gm_get_hop_labels() == 0
        S0, Q0 = w.batches(store, 0)
        before = snapshot(S0) + snapshot(Q0) + [w.step(S0, Q0, True, th, w.config_for(w.F0))[0]]
        Sl, Ql = w.batches(store, D)                                                 # a labelled build (and step) on this thread in between
        w.step(Sl, Ql)
        assert _lib.lib().gm_get_hop_labels() == 0                                   # the block restored the switch
        S1, Q1 = w.batches(store, 0)
        after = snapshot(S1) + snapshot(Q1) + [w.step(S1, Q1, True, th, w.config_for(w.F0))[0]]
    assert S1.hop_labels_cap == 0 and S1.feat_dim == w.F0
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def test_two_piece_mode_is_ignored_on_labelled_batches():
    """gm_set_split_pieces(2) with the two-piece threshold at zero: a labelled step is the three-piece step bit for bit, violation word 0 -- and the
    knob does engage on the unlabelled twin (its result differs), so the guard is what kept the labelled step."""
    from gmeta_amd import _lib
    w = world('node')
    lib = _lib.lib()
    th_u, cfg_u = [w.theta[0][:w.F0]] + w.theta[1:], w.config_for(w.F0)
    with tuning(GM_SPLIT16_MIN_ROWS=0, **FORCE):
        store = w.store()
        (Sl, Ql), (Su, Qu) = w.batches(store, D), w.batches(store, 0)
        three_l, three_u = w.step(Sl, Ql)[0], w.step(Su, Qu, True, th_u, cfg_u)[0]
        lib.gm_set_split_pieces(2)
        try:
            assert lib.gm_get_split_pieces() == 2
            two_l, two_u = w.step(Sl, Ql)[0], w.step(Su, Qu, True, th_u, cfg_u)[0]
        finally:
            lib.gm_set_split_pieces(-1)
    assert np.array_equal(_bits(two_l), _bits(three_l)) and two_l[-1] == 0
    assert not np.array_equal(_bits(two_u), _bits(three_u))


# ---------------------------------------------------------------------------------------------------- end to end
def _db_args(**kv):
    a = dict(update_lr=0.05, meta_lr=0.01, n_way=3, k_spt=2, k_qry=6, task_num=4, update_step=3, update_step_test=4, method='G-Meta', sample_nodes=1000,
             link_pred_mode='False', task_setup='Disjoint', h=2)
    a.update(kv)
    return argparse.Namespace(**a)


def test_subgraphs_collate_meta_forward_with_hop_labels(tmp_path):
    """Subgraphs(hop_labels=2) -> collate -> Meta.forward on a synthetic data directory: the per-task batches (concatenated by Meta.forward), the joint
    build of get_batch and the builder threads of batches() all carry the labels; args.hop_labels works alike; the caller's switch stays off."""
    import random
    import gmeta_amd
    from gmeta_amd import _lib, datadir
    from test_train_driver import _dataset
    np.random.seed(1); random.seed(1); torch.manual_seed(1)
    _dataset(tmp_path)
    root = str(tmp_path) + '/'
    feat, graphs, info = datadir.load_features(root), datadir.load_graphs(root), datadir.load_labels(root)
    store = gmeta_amd.GraphStore(graphs, feat)
    args = _db_args()
    mk = lambda a, **kw: gmeta_amd.Subgraphs(root, 'train', info, n_way=3, k_shot=2, k_query=6, batchsz=8, args=a, adjs=store, h=2, verbose=False, **kw)      # noqa: E731
    db = mk(args, hop_labels=2)
    F1 = feat[0].shape[1] + gmeta_amd.hop_label_width(2, False)
    config = [('GraphConv', [F1, 32]), ('GraphConv', [32, 32]), ('Linear', [32, 3])]
    maml = gmeta_amd.Meta(args, config).to('cuda')
    batch = gmeta_amd.collate([db[i] for i in range(4)])
    assert all(b.hop_labels_cap == 2 and b.feat_dim == F1 for b in batch[0] + batch[2])
    g = [orc.Graph(*gr) for gr in graphs]
    seeds = db._task_arrays(0)[1]
    assert np.array_equal(batch[2][0].hop_labels, hl.labels(orc.extract_batch(g, seeds, 2, 1000, db.rng_seed, False), 2))
    accs = maml(*batch, feat)
    assert np.isfinite(accs).all() and len(accs) == 4
    joint = db.get_batch([0, 1, 2, 3])
    assert joint[0][0].view_of.hop_labels_cap == 2
    accs2 = maml(*joint, feat)
    assert np.isfinite(accs2).all()
    for b in db.batches([[0, 1], [2, 3], [4, 5]], prefetch=1):                       # builder threads
        assert b[0][0].view_of.hop_labels_cap == 2 and b[2][0].view_of.hop_labels_cap == 2
    assert db.query_batch([['0_1', '0_2']]).hop_labels_cap == 2
    assert _lib.lib().gm_get_hop_labels() == 0
    assert mk(_db_args(hop_labels=3)).get_batch([0])[0][0].view_of.hop_labels_cap == 3
    assert mk(args).get_batch([0])[0][0].view_of.hop_labels_cap == 0
    with pytest.raises(ValueError):
        mk(args, hop_labels=8)


def test_train_driver_with_hop_labels(tmp_path):
    sys.path.insert(0, ROOT)
    import train as drv
    from test_train_driver import _dataset
    _dataset(tmp_path)
    args = drv.parse(['--data_dir', str(tmp_path) + '/', '--task_setup', 'Disjoint', '--epoch', '1', '--n_way', '3', '--k_spt', '2',
                      '--k_qry', '6', '--task_num', '4', '--update_step', '3', '--update_step_test', '4', '--update_lr', '0.05',
                      '--meta_lr', '0.01', '--hidden_dim', '32', '--batchsz', '16', '--h', '2', '--eval_tasks', '6',
                      '--train_result_report_steps', '2', '--hop_labels', '2', '--num_workers', '1'])
    res = drv.main(args)
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in res.values()), res      # (a handful of steps: that it runs end to end, not that it has learnt)
