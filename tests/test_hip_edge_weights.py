"""GPU (-m gpu): edge-weighted parent graphs from GraphStore to the meta-step (include/gmeta_hip.h, gm_store_create_weighted), against the CPU
restatement tests/edge_weight_ref.py (validated by tests/test_edge_weight_restatement.py).

One hand-built directed multigraph of 400 nodes carries every shape the weighted paths branch on: an isolated node, a centre without in-edges,
a self loop, parallel edges with different weights, rows of in-degree 1 .. 10, a node with 300 in-neighbours (above EX_BIG_DEG = 256: the
extraction's whole-wave path; its row is also above the batch's heavy-degree threshold of 32 / 64: the aggregate's hub path).  Feature width
64, hidden 128, 2 tasks x 2-way, K = 3, the split GEMM / weight-gradient kernels forced onto it (GM_GEMM_SPLIT_MIN_TILES,
GM_WGRAD_SPLIT_MIN_CHUNKS), one case with the stream aggregate (GM_AGG_STREAM_MIN_ROWS).

1 unit weights: a store of all-ones weights against the plain store, bit for bit, every schedule; 2 integer weights against the store of the
expanded multigraph; 3 fractional weights against the restatement, every consumer; 4 refusals and the two-piece guard; 5 fuzz."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, ROOT)
import edge_weight_ref as ew     # noqa: E402
import gmeta_oracle as orc       # noqa: E402
import link_sym_ref as lsr       # noqa: E402
from golden_util import Fixture  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4                       # the project's parity tolerance (tests/test_hip_fuzz.py)
f32 = np.float32
N, F0, HID, T, C_WAY, K_SPT, K_QRY, K, LR = 400, 64, 128, 2, 2, 2, 3, 3, 0.005
FORCE = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
SCHEDULES = (('dense', {}), ('hoist_z1', dict(hoist_z1=1)), ('sparse_bwd', dict(sparse_bwd=1)), ('cone', dict(cone=1)), ('cone+hoist', dict(cone=1, hoist_z1=1)))


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


# ---------------------------------------------------------------------------------------------------- the hand-built graph
def hand_graph():
    rng = np.random.default_rng(2024)
    e = [(u, 0) for u in range(1, 301)]                                  # node 0: 300 in-neighbours
    e += [(0, 7), (0, 310), (0, 320)]                                    # ... and it is inside the 2-hop neighbourhoods of 7, 310, 320
    e += [(5, 5), (5, 6)]                                                # a self loop
    e += [(6, 7), (6, 7), (6, 7)]                                        # parallel edges (their weights differ wherever weights do)
    for v in range(301, 398):                                            # in-degrees 1 .. 10
        for u in rng.integers(1, 398, size=(v - 301) % 10 + 1):
            e.append((int(u), v))
    e += [(398, 301), (398, 302)]                                        # 398: out-edges only (a centre without in-edges); 399: isolated
    e = np.array(e, np.int64)
    e = e[rng.permutation(len(e))]                                       # edge-id order is not row order
    src, dst = e[:, 0], e[:, 1]
    deg = np.bincount(dst, minlength=N)
    assert deg[0] == 300 and deg[398] == 0 and deg[399] == 0 and not (src == 399).any() and set(range(1, 11)) <= set(deg[301:398].tolist())
    return N, src, dst


def make_weights(kind, m, seed=9):
    rng = np.random.default_rng(seed)
    if kind == 'unit':
        return np.ones(m, f32)
    if kind == 'int':
        return rng.integers(1, 4, size=m).astype(f32)
    return np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=m)).astype(f32)      # log-uniform in [0.25, 4], not symmetric


def seeds_for(mode):
    """[T][spt / qry] seed arrays: centres on the hub, the parallel edges, the self loop, the isolated node, the node without in-edges, ..."""
    node = [[(0, 7, 320, 399), (398, 310, 5, 0, 333, 361)], [(310, 6, 345, 0), (7, 399, 397, 320, 302, 398)]]
    other = {0: 7, 7: 0, 320: 310, 399: 5, 398: 301, 310: 0, 5: 6, 333: 320, 361: 398, 6: 7, 345: 399, 397: 396, 302: 398}
    out = []
    for spt, qry in node:
        out.append([np.array([(0, i, -1 if mode == 'node' else other[i]) for i in part], np.int32) for part in (spt, qry)])
    return out


LINK = {'node': False, 'link': True, 'link_sym': 2}


class World:
    """The graph, one task layout per mode, parameters with every bias off the relu kink (tests/test_hip_fuzz.py: why).  The hub's subgraphs make the
    support loss steep (300 weighted sources in one row), so the inner step is small (LR) and the head's weights start small: K = 3 inner steps
    then stay in the regime where fp32 rounding differences are not amplified (at update_lr = 0.05 the query loss grows 50-fold in three steps and
    two fp32 CPU evaluations of the same step already differ by 1e-2)."""

    def __init__(self, mode):
        self.mode, self.link = mode, LINK[mode]
        self.n, self.src, self.dst = hand_graph()
        rng = np.random.default_rng(77)
        self.feats = [(0.2 * rng.standard_normal((N, F0))).astype(f32)]
        self.seeds = seeds_for(mode)
        self.ys = [np.repeat(np.arange(C_WAY), K_SPT).astype(np.int32) for _ in range(T)]
        self.yq = [np.repeat(np.arange(C_WAY), K_QRY).astype(np.int32) for _ in range(T)]
        self.config = [('GraphConv', [F0, HID]), ('GraphConv', [HID, HID]), ('Linear', [HID, C_WAY])] + ([('LinkPred', [True])] if self.link else [])
        self.args = argparse.Namespace(update_lr=LR, meta_lr=1e-3, n_way=C_WAY, k_spt=K_SPT, k_qry=K_QRY, task_num=T, update_step=K, update_step_test=K,
                                       method='G-Meta', sample_nodes=1000, link_pred_mode='True' if self.link else 'False', task_setup='Shared', h=2)
        gcn, lin, _ = orc.parse_config(self.config)
        th = []
        for fi, fo in gcn:
            th += [(rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(f32), (rng.uniform(0.15, 0.4, fo) * rng.choice([-1.0, 1.0], fo)).astype(f32)]
        hc = lin[0] * (2 if self.link else 1)
        th += [(0.3 * rng.standard_normal((lin[1], hc)) / np.sqrt(hc)).astype(f32), (rng.uniform(0.15, 0.4, lin[1]) * rng.choice([-1.0, 1.0], lin[1])).astype(f32)]
        self.theta = th
        self._ref = {}

    def store(self, weights=None, graph=None):
        import gmeta_amd
        g = graph if graph is not None else (self.n, self.src, self.dst)
        return gmeta_amd.GraphStore([g], self.feats, edge_weights=None if weights is None else [weights])

    def batches(self, store):
        from gmeta_amd.subgraphs import SubgraphBatch
        out = []
        for part, per in ((0, C_WAY * K_SPT), (1, C_WAY * K_QRY)):
            out.append(SubgraphBatch.extract(store, np.concatenate([s[part] for s in self.seeds]), np.arange(T + 1) * per, 2, 1000, 222, self.link))
        return out

    def meta(self, **flags):
        import gmeta_amd
        m = gmeta_amd.Meta(self.args, self.config).to('cuda')
        with torch.no_grad():
            for p, v in zip(m.net.parameters(), self.theta):
                p.copy_(torch.from_numpy(v))
        for k, v in flags.items():
            setattr(m, k, v)
        return m

    def labels(self):
        return [torch.from_numpy(y.astype(np.int64)) for y in self.ys], [torch.from_numpy(y.astype(np.int64)) for y in self.yq]

    def step(self, S, Q, need_grad=True, **flags):
        """gm_meta_step's whole `out` (host copy) and P."""
        ys, yq = self.labels()
        out, P, _ = self.meta(**flags)._run(S.views(), ys, Q.views(), yq, K, need_grad)
        return out.cpu().numpy().copy(), P

    def ref_batches(self, graphs, cls):
        """Restatement batches [T] x (spt, qry) over `graphs` (ew.Graph -> weighted, cls = ew.Batch; orc.Graph -> cls = orc.Batch)."""
        spt, qry = [], []
        for t in range(T):
            for part, dstl in ((0, spt), (1, qry)):
                sd = self.seeds[t][part]
                if self.mode == 'link_sym':
                    lists = lsr.node_lists(graphs, sd, 2, 1000)
                else:
                    ob = orc.extract_batch(graphs, sd, 2, 1000, 222, bool(self.link))
                    lists = [ob.parent[ob.sub_off[s]:ob.sub_off[s + 1]] for s in range(ob.S)]
                dstl.append(cls(graphs, sd, lists))
        return spt, qry

    def reference(self, weights):
        """(spt, qry, accs, flat grad, losses_q) of the restatement for these weights (computed once per weight vector)."""
        key = weights.tobytes()
        if key not in self._ref:
            g = [ew.Graph(self.n, self.src, self.dst, weights)]
            spt, qry = self.ref_batches(g, ew.Batch)
            accs, grad, lq = ew.meta_step(self.feats, spt, qry, self.ys, self.yq, self.theta, self.config, K_SPT, LR, 1e-3, K)
            self._ref[key] = (spt, qry, np.asarray(accs), np.concatenate([x.reshape(-1) for x in grad]), np.asarray(lq))
        return self._ref[key]


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
    np.testing.assert_allclose(g, grad, atol=TOL * max(1.0, float(np.abs(grad).max())), rtol=1e-3, err_msg=what)
    assert np.abs(a - accs).max() <= 1.0 / (C_WAY * K_QRY) + 1e-6, what      # argmax decisions: equal unless two distances tie within noise


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def read_f(B, field, n):
    return B._read(field, n, np.float32).copy()


def aggregate(B, x, transposed=0, gather=0, s_in=None, s_out=None, width=None):
    """gm_aggregate through the C ABI; s_in / s_out: None, 'norm' (the batch's own device pointer) or a device tensor."""
    from gmeta_amd import _lib
    width = width if width is not None else x.shape[1]
    out = torch.empty(B.rows, width, dtype=torch.float32, device='cuda')
    pick = lambda s: B.device_ptr(_lib.F_NORM) if isinstance(s, str) else _lib.ptr(s)      # noqa: E731
    _lib.check(_lib.lib().gm_aggregate(B.handle, transposed, gather, _lib.ptr(x), width, pick(s_in), pick(s_out), _lib.ptr(out), _lib.stream_ptr()), 'gm_aggregate')
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 1. unit weights: bit for bit
def _unit_pair(make_plain, make_ones, batches, step):
    res = []
    for mk in (make_plain, make_ones):
        store = mk()
        S, Q = batches(store)
        res.append((store, S, Q))
    (sp, Sp, Qp), (so, So, Qo) = res
    from gmeta_amd import _lib
    assert not sp.weighted and so.weighted and not Sp.weighted and So.weighted
    assert (read_f(So, _lib.F_EDGE_W, So.edges) == 1).all() and (read_f(Qo, _lib.F_EDGE_W_T, Qo.edges) == 1).all()
    for a, b in ((Sp, So), (Qp, Qo)):
        assert np.array_equal(a.parent(), b.parent()) and all(np.array_equal(x, y) for x, y in zip(a.csr() + a.csr(True), b.csr() + b.csr(True)))
        assert np.array_equal(_bits(read_f(a, _lib.F_NORM, a.rows)), _bits(read_f(b, _lib.F_NORM, b.rows)))
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((a.rows, 64)).astype(f32)).cuda()
        for tr in (0, 1):
            for s_in, s_out in ((None, None), ('norm', None), (None, 'norm'), ('norm', 'norm')):
                assert np.array_equal(_bits(aggregate(a, x, tr, 0, s_in, s_out)), _bits(aggregate(b, x, tr, 0, s_in, s_out))), (tr, s_in, s_out)
        fd = a.store.feat_dim
        assert np.array_equal(_bits(aggregate(a, None, 0, 1, 'norm', None, fd)), _bits(aggregate(b, None, 0, 1, 'norm', None, fd)))
    for name, flags in SCHEDULES:
        for need_grad in (True, False):
            op, P = step(Sp, Qp, need_grad, flags)
            oo, _ = step(So, Qo, need_grad, flags)
            assert np.array_equal(_bits(op), _bits(oo)), (name, need_grad, int((_bits(op) != _bits(oo)).sum()))


def test_unit_weights_are_bitwise_the_unweighted_store_on_the_hand_graph():
    w = world('node')
    m = len(w.src)
    with tuning(**FORCE):
        _unit_pair(lambda: w.store(), lambda: w.store(np.ones(m, f32)), w.batches, lambda S, Q, ng, fl: w.step(S, Q, ng, **fl))


@pytest.mark.parametrize('case', ['g2_shared', 'g7_wide_h2', 'g3_linkpred'])
def test_unit_weights_are_bitwise_the_unweighted_store_on_golden_fixtures(case):
    """g2_shared (3 graphs, hidden below the split kernels' widths), g7_wide_h2 (hidden 128, split kernels forced, sampled subgraphs) and the
    link-prediction fixture, replayed node lists (gm_batch_from_nodes) -- every schedule, training step and fine-tuning."""
    import gmeta_amd
    import hip_util as hu
    fx = Fixture(case)
    ys = [torch.from_numpy(y.astype(np.int64)) for y in fx.z['y_spt']]; yq = [torch.from_numpy(y.astype(np.int64)) for y in fx.z['y_qry']]

    def step(S, Q, need_grad, flags):
        m = hu.fixture_meta(fx)
        for k, v in flags.items():
            setattr(m, k, v)
        out, P, _ = m._run(S.views(), ys, Q.views(), yq, fx.K, need_grad)
        return out.cpu().numpy().copy(), P
    with tuning(**(FORCE if case == 'g7_wide_h2' else {})):
        _unit_pair(lambda: hu.make_store(fx), lambda: gmeta_amd.GraphStore(fx.edges, fx.feats, edge_weights=[np.ones(len(s), f32) for n, s, d in fx.edges]),
                   lambda store: hu.fixture_batches(fx, store, True), step)


def test_unit_weights_through_the_stream_aggregate_and_concat():
    """GM_AGG_STREAM_MIN_ROWS lowered before the batches exist (the stream tables are built at a batch's first eligible launch), the fused
    aggregate + GEMM off so that the full launches are the stream kernel's; gm_batch_concat of the weighted task batches carries the weights."""
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    w = world('node')
    lib = _lib.lib()
    with tuning(GM_AGG_STREAM_MIN_ROWS=1, **FORCE):
        lib.gm_set_fuse_agg(0)
        try:
            outs = []
            for wt in (None, np.ones(len(w.src), f32)):
                store = w.store(wt)
                S, Q = w.batches(store)
                x = torch.from_numpy(np.random.default_rng(2).standard_normal((Q.rows, 128)).astype(f32)).cuda()
                outs.append([aggregate(Q, x, tr, 0, 'norm', None) for tr in (0, 1)] + [aggregate(Q, None, 0, 1, 'norm', None, F0), w.step(S, Q)[0]])
                if wt is not None:
                    parts = [SubgraphBatch.extract(store, w.seeds[t][1], [0, C_WAY * K_QRY], 2, 1000, 222, False) for t in range(T)]
                    cat = SubgraphBatch.concat(parts)
                    assert cat.weighted and np.array_equal(cat.csr()[1], Q.csr()[1])
                    for f in (_lib.F_EDGE_W, _lib.F_EDGE_W_T):
                        assert np.array_equal(read_f(cat, f, cat.edges), read_f(Q, f, Q.edges))
                    assert np.array_equal(_bits(read_f(cat, _lib.F_NORM, cat.rows)), _bits(read_f(Q, _lib.F_NORM, Q.rows)))
            for a, b in zip(*outs):
                assert np.array_equal(_bits(a), _bits(b))
        finally:
            lib.gm_set_fuse_agg(-1)


# ---------------------------------------------------------------------------------------------------- 2. integer weights: the expanded multigraph
@pytest.mark.parametrize('mode', ['node', 'link'])
def test_integer_weights_equal_the_store_of_the_expanded_multigraph(mode):
    from gmeta_amd import _lib
    w = world(mode)
    wt = make_weights('int', len(w.src))
    multi = ew.expand(w.n, w.src, w.dst, wt)
    og = [orc.Graph(*multi)]
    ospt, oqry = w.ref_batches(og, orc.Batch)
    oaccs, ograd, _, olq = orc.meta_step(og, w.feats, ospt, oqry, w.ys, w.yq, w.theta, w.config, K_SPT, LR, 1e-3, K, adam_state={})
    ograd = np.concatenate([g.reshape(-1) for g in ograd])
    with tuning(**FORCE):
        sw, sm = w.store(wt), w.store(None, multi)
        (Sw, Qw), (Sm, Qm) = w.batches(sw), w.batches(sm)
        for a, b in ((Sw, Sm), (Qw, Qm)):
            assert np.array_equal(a.parent(), b.parent()) and np.array_equal(a.sub_off, b.sub_off)
            assert np.array_equal(_bits(read_f(a, _lib.F_NORM, a.rows)), _bits(read_f(b, _lib.F_NORM, b.rows)))
            assert b.edges == int(read_f(a, _lib.F_EDGE_W, a.edges).sum()) and b.edges > a.edges
        for name, flags in SCHEDULES:
            ow, P = w.step(Sw, Qw, True, **flags)
            om, _ = w.step(Sm, Qm, True, **flags)
            gm_, lm, am, _ = split_out(om, P)
            assert_step_close(ow, P, am, gm_, lm, 'multigraph store, ' + name)
            assert_step_close(ow, P, np.asarray(oaccs), ograd, np.asarray(olq), 'oracle on the multigraph, ' + name)


# ---------------------------------------------------------------------------------------------------- 3. fractional weights: every consumer
@pytest.mark.parametrize('mode', ['node', 'link', 'link_sym'])
def test_fractional_weights_match_the_restatement(mode):
    from gmeta_amd import _lib
    w = world(mode)
    wt = make_weights('frac', len(w.src))
    rspt, rqry, raccs, rgrad, rlq = w.reference(wt)
    lib = _lib.lib()
    with tuning(**FORCE):
        store = w.store(wt)
        assert store.weighted and not store.symmetric()
        S, Q = w.batches(store)
        # ---- extraction: topology and the induced weights in both orientations, bit for bit; the weighted norm
        for B, obs in ((S, rspt), (Q, rqry)):
            assert np.array_equal(B.parent(), np.concatenate([b.parent for b in obs]))
            assert np.array_equal(B.csr()[1], np.concatenate([b.indices + o for b, o in zip(obs, np.cumsum([0] + [b.n for b in obs[:-1]]))]))
            assert np.array_equal(_bits(read_f(B, _lib.F_EDGE_W, B.edges)), _bits(np.concatenate([b.ew for b in obs])))
            assert np.array_equal(_bits(read_f(B, _lib.F_EDGE_W_T, B.edges)), _bits(np.concatenate([b.by_source()[2] for b in obs])))
            np.testing.assert_allclose(read_f(B, _lib.F_NORM, B.rows), np.concatenate([b.norm for b in obs]), rtol=2e-7, atol=0)
        # ---- gm_aggregate: plain, with the batch's norm, gather, transposed
        rng = np.random.default_rng(4)
        x = rng.standard_normal((Q.rows, 64)).astype(f32); xd = torch.from_numpy(x).cuda()
        off = np.cumsum([0] + [b.n for b in rqry])
        norm = np.concatenate([b.norm for b in rqry])
        agg, agg_t = ew.make(rqry)
        ref = lambda fn: np.concatenate([fn(b, slice(off[k], off[k + 1])) for k, b in enumerate(rqry)])      # noqa: E731
        close = lambda got, want, what: np.testing.assert_allclose(got, want, atol=TOL * max(1.0, float(np.abs(want).max())), rtol=1e-4, err_msg=what)      # noqa: E731
        close(aggregate(Q, xd), ref(lambda b, s: agg(b.indptr, b.indices, x[s])), 'plain')
        close(aggregate(Q, xd, 0, 0, 'norm', 'norm'), ref(lambda b, s: agg(b.indptr, b.indices, x[s] * norm[s, None]) * norm[s, None]), 'norm')
        close(aggregate(Q, xd, 1), ref(lambda b, s: agg_t(b, x[s])), 'transposed')
        close(aggregate(Q, xd, 1, 0, 'norm', None), ref(lambda b, s: agg_t(b, x[s] * norm[s, None])), 'transposed, norm')
        feat = w.feats[0]
        close(aggregate(Q, None, 0, 1, None, None, F0), ref(lambda b, s: agg(b.indptr, b.indices, feat[b.parent])), 'gather')
        close(aggregate(Q, None, 0, 1, 'norm', None, F0), ref(lambda b, s: agg(b.indptr, b.indices, feat[b.parent] * norm[s, None])), 'gather, norm')
        # ---- Classifier.forward / backward under autograd (gm_gcn_forward / gm_gcn_backward), one task's support batch
        from gmeta_amd.subgraphs import SubgraphBatch
        B0 = SubgraphBatch.extract(store, w.seeds[0][0], [0, C_WAY * K_SPT], 2, 1000, 222, w.link)
        m = w.meta()
        logits, _ = m.net(B0, None, None)
        R = rng.standard_normal((B0.subs, C_WAY)).astype(f32)
        (logits * torch.from_numpy(R).cuda()).sum().backward()
        with ew.patched([rspt[0]]):
            rl, cache = orc.classifier_forward(rspt[0], rspt[0].features(w.feats), w.theta, w.config)
            rg = np.concatenate([g.reshape(-1) for g in orc.classifier_backward(rspt[0], w.theta, w.config, cache, R)])
        close(logits.detach().cpu().numpy(), rl, 'gcn_forward')
        close(torch.cat([p.grad.reshape(-1) for p in m.net.parameters()]).cpu().numpy(), rg, 'gcn_backward')
        # ---- gm_meta_step: every schedule, fused aggregate + GEMM on and off
        for name, flags in SCHEDULES:
            for fuse in (1, 0):
                lib.gm_set_fuse_agg(fuse)
                try:
                    out, P = w.step(S, Q, True, **flags)
                finally:
                    lib.gm_set_fuse_agg(-1)
                assert_step_close(out, P, raccs, rgrad, rlq, '%s, %s, fuse_agg=%d' % (mode, name, fuse))
        # ---- finetunning (task 0), and adapt + predict against finetunning_batch
        ys, yq = w.labels()
        m = w.meta()
        one = lambda part: SubgraphBatch.extract(store, w.seeds[0][part], [0, len(w.seeds[0][part])], 2, 1000, 222, w.link)      # noqa: E731
        ft = m.finetunning([one(0)], ys[:1], [one(1)], yq[:1], None, None, None, None, None, None, w.feats)
        rft = ew.finetune(w.feats, rspt[0], rqry[0], w.ys[0], w.yq[0], w.theta, w.config, K_SPT, LR, K)
        assert np.abs(np.asarray(ft) - rft).max() <= 1.0 / (C_WAY * K_QRY) + 1e-6
        fb = m.finetunning_batch(S.views(), ys, Q.views(), yq)
        for j in range(K + 1):
            pr = m.adapt(S.views(), ys, K=j).predict(Q.views())
            for t in range(T):
                y = yq[t].numpy()
                assert f32(np.count_nonzero(pr.labels[t] == y)) / f32(len(y)) == f32(fb[t, j]), (j, t)


@pytest.mark.parametrize('symmetric', [True, False], ids=['symmetric_weights', 'asymmetric_weights'])
def test_symmetrically_stored_graph_with_and_without_symmetric_weights(symmetric):
    """An undirected graph stored in both directions: with w_uv == w_vu the store is symmetric and the fill walks every adjacency list once,
    copying the weight to both orientations; with asymmetric weights the single walk must be refused (it would copy w_uv where the by-source
    CSR holds w_vu).  Either way both weight arrays are the restatement's, bit for bit, and a meta-step agrees."""
    import gmeta_amd
    from gmeta_amd import _lib, synth
    from gmeta_amd.subgraphs import SubgraphBatch
    rng = np.random.default_rng(31)
    n = 300
    e = synth.pa_edges(n, 3, rng)
    g = (n, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))
    gw = synth.with_edge_weights([g], seed=3, symmetric=symmetric)[0]
    feats = [(0.5 * rng.standard_normal((n, F0))).astype(f32)]
    store = gmeta_amd.GraphStore([gw], feats)
    assert gmeta_amd.GraphStore([g], feats).symmetric() and store.symmetric() == symmetric
    w = world('node')
    seeds = [[rng.integers(0, n, size=k) for k in (C_WAY * K_SPT, C_WAY * K_QRY)] for _ in range(T)]
    sd = lambda t, p: np.array([(0, int(i), -1) for i in seeds[t][p]], np.int32)      # noqa: E731
    og = [ew.Graph(*gw)]
    with tuning(**FORCE):
        S = SubgraphBatch.extract(store, np.concatenate([sd(t, 0) for t in range(T)]), np.arange(T + 1) * C_WAY * K_SPT, 2, 40, 222, False)      # sampled: 40 of ~100+
        Q = SubgraphBatch.extract(store, np.concatenate([sd(t, 1) for t in range(T)]), np.arange(T + 1) * C_WAY * K_QRY, 2, 40, 222, False)
        rspt = [ew.extract_batch(og, sd(t, 0), 2, 40, 222, False) for t in range(T)]; rqry = [ew.extract_batch(og, sd(t, 1), 2, 40, 222, False) for t in range(T)]
        for B, obs in ((S, rspt), (Q, rqry)):
            assert np.array_equal(B.parent(), np.concatenate([b.parent for b in obs]))
            assert np.array_equal(_bits(read_f(B, _lib.F_EDGE_W, B.edges)), _bits(np.concatenate([b.ew for b in obs])))
            assert np.array_equal(_bits(read_f(B, _lib.F_EDGE_W_T, B.edges)), _bits(np.concatenate([b.by_source()[2] for b in obs])))
        accs, grad, lq = ew.meta_step(feats, rspt, rqry, w.ys, w.yq, w.theta, w.config, K_SPT, LR, 1e-3, K)
        out, P = w.step(S, Q)
        assert_step_close(out, P, np.asarray(accs), np.concatenate([x.reshape(-1) for x in grad]), np.asarray(lq), 'symmetric store')


# ---------------------------------------------------------------------------------------------------- 4. refusals and guards
@pytest.mark.parametrize('bad,word', [(0.0, 'finite and > 0'), (-1.5, 'finite and > 0'), (float('nan'), 'finite and > 0'), (float('inf'), 'finite and > 0')])
def test_a_bad_weight_is_refused_and_named(bad, word):
    w = world('node')
    wt = np.ones(len(w.src), f32)
    k = 17
    wt[k] = bad
    with pytest.raises(ValueError, match=word) as ei:
        w.store(wt)
    assert 'graph 0' in str(ei.value) and '(%d -> %d)' % (w.src[k], w.dst[k]) in str(ei.value)      # the graph and the edge


def test_refusals_name_their_cause():
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    w = world('node')
    lib = _lib.lib()
    sp, sw = w.store(), w.store(make_weights('frac', len(w.src)))
    Sp, Qp = w.batches(sp)
    Sw, Qw = w.batches(sw)
    assert lib.gm_store_weighted(sp.handle) == 0 and lib.gm_store_weighted(sw.handle) == 1 and lib.gm_batch_weighted(Sp.handle) == 0 and lib.gm_batch_weighted(Sw.handle) == 1
    for f in (_lib.F_EDGE_W, _lib.F_EDGE_W_T):                                    # GM_F_EDGE_W* on an unweighted batch
        with pytest.raises(ValueError, match='unweighted'):
            Sp._read(f, Sp.edges, np.float32)
        with pytest.raises(ValueError, match='unweighted'):
            Sp.device_ptr(f)
    x = torch.ones(Sw.rows, 64, device='cuda')
    foreign = torch.ones(Sw.rows, device='cuda')
    with pytest.raises(ValueError, match='edge-weight slot'):                     # gm_aggregate with a foreign s_in
        aggregate(Sw, x, 0, 0, foreign, None)
    aggregate(Sp, x, 0, 0, torch.ones(Sp.rows, device='cuda'), None)              # (fine on an unweighted batch, as before)
    with pytest.raises(ValueError, match='weighted batch'):
        aggregate(Sw, None, 1, 1, None, None, F0)
    with pytest.raises(ValueError, match='weighted and unweighted batches cannot be concatenated'):      # mixed concat
        SubgraphBatch.concat([Sw, Sp])
    with pytest.raises(ValueError, match='weighted and unweighted batches cannot be concatenated'):
        SubgraphBatch.concat([Qp, Qw])
    assert SubgraphBatch.concat([Sw, Qw]).weighted and not SubgraphBatch.concat([Sp, Qp]).weighted
    with pytest.raises(ValueError, match='one of the support and query batches is weighted|different stores'):
        w.step(Sw, Qp)


def test_two_piece_mode_is_ignored_on_weighted_batches():
    """gm_set_split_pieces(2) with the two-piece threshold at zero: a weighted step is the three-piece step bit for bit, violation word 0 -- and
    the knob does engage on the unweighted twin (its result differs), so the guard is what kept the weighted step."""
    from gmeta_amd import _lib
    w = world('node')
    lib = _lib.lib()
    with tuning(GM_SPLIT16_MIN_ROWS=0, **FORCE):
        sw, sp = w.store(make_weights('frac', len(w.src))), w.store()
        (Sw, Qw), (Sp, Qp) = w.batches(sw), w.batches(sp)
        three_w, three_p = w.step(Sw, Qw)[0], w.step(Sp, Qp)[0]
        lib.gm_set_split_pieces(2)
        try:
            assert lib.gm_get_split_pieces() == 2
            two_w, two_p = w.step(Sw, Qw)[0], w.step(Sp, Qp)[0]
        finally:
            lib.gm_set_split_pieces(-1)
    assert np.array_equal(_bits(two_w), _bits(three_w)) and two_w[-1] == 0
    assert not np.array_equal(_bits(two_p), _bits(three_p))


# ---------------------------------------------------------------------------------------------------- 5. fuzz
@pytest.mark.parametrize('seed', list(range(6)))
def test_random_weighted_multigraph_matches_the_restatement(seed):
    """tests/test_hip_fuzz.py's generator (self loops, parallel edges, isolated nodes, a hub, h = 1..3, pairs, sampling on and off, odd feature
    widths, 1-3 layers in both branch orders) with random weights: extraction bit-exact, one meta-step per schedule within the tolerance."""
    import gmeta_amd
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    from test_hip_fuzz import _graph
    rng = np.random.default_rng(3000 + seed)
    link = seed % 4 == 3
    h = int(rng.integers(1, 4))
    n_graphs = int(rng.integers(1, 4))
    Fin = int(rng.choice([1, 5, 12, 32, 50, 64]))
    graphs = [_graph(rng, int(rng.integers(25, 160))) for _ in range(n_graphs)]
    graphs = [g + (make_weights('frac', len(g[1]), seed=100 * seed + k),) for k, g in enumerate(graphs)]
    feats = [rng.standard_normal((g[0], Fin)).astype(f32) for g in graphs]
    sample_n = int(rng.choice([6, 15, 40, 10000]))
    Tn, Cn = int(rng.integers(1, 4)), int(rng.integers(2, 4))
    k_spt, k_qry = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    n_gcn = 2 if link else int(rng.integers(1, 4))
    dims = [Fin] + [int(rng.choice([8, 16, 20, 32, 64])) for _ in range(n_gcn)]
    if seed % 3 == 0 and Fin >= 32:
        dims[1] = 8                                                     # multiply-first first layer (in > out)

    def seeds_of(count):
        out = []
        for _ in range(count):
            g = int(rng.integers(0, n_graphs)); n = graphs[g][0]
            i = int(rng.integers(0, n)); j = int(rng.integers(0, n)) if link else -1
            if link and j == i:
                j = (i + 1) % n
            out.append((g, i, j))
        return np.array(out, np.int32)
    store = gmeta_amd.GraphStore(graphs, feats)
    og = [ew.Graph(*g) for g in graphs]
    spt_seeds = [seeds_of(Cn * k_spt) for _ in range(Tn)]; qry_seeds = [seeds_of(Cn * k_qry) for _ in range(Tn)]
    ys = [np.repeat(np.arange(Cn), k_spt).astype(np.int32) for _ in range(Tn)]; yq = [np.repeat(np.arange(Cn), k_qry).astype(np.int32) for _ in range(Tn)]
    S = SubgraphBatch.extract(store, np.concatenate(spt_seeds), np.arange(Tn + 1) * Cn * k_spt, h, sample_n, 222, link)
    Q = SubgraphBatch.extract(store, np.concatenate(qry_seeds), np.arange(Tn + 1) * Cn * k_qry, h, sample_n, 222, link)
    ospt = [ew.extract_batch(og, s, h, sample_n, 222, link) for s in spt_seeds]; oqry = [ew.extract_batch(og, s, h, sample_n, 222, link) for s in qry_seeds]
    for hb, obs in ((S, ospt), (Q, oqry)):                              # bit-exact: node lists, CSR, centres, both weight arrays
        assert np.array_equal(hb.parent(), np.concatenate([b.parent for b in obs]))
        ip, ix = hb.csr()
        r0 = e0 = 0
        for b in obs:
            assert np.array_equal(ip[r0:r0 + b.n + 1] - e0, b.indptr) and np.array_equal(ix[e0:e0 + len(b.indices)] - r0, b.indices)
            r0 += b.n; e0 += len(b.indices)
        cen = np.concatenate([(b.centre_rows - b.sub_off[:-1, None]).reshape(-1) for b in obs])
        assert np.array_equal(hb._read(8, hb.subs * hb.centres, np.int32), cen)
        assert np.array_equal(_bits(read_f(hb, _lib.F_EDGE_W, hb.edges)), _bits(np.concatenate([b.ew for b in obs] + [np.zeros(0, f32)])))
        assert np.array_equal(_bits(read_f(hb, _lib.F_EDGE_W_T, hb.edges)), _bits(np.concatenate([b.by_source()[2] for b in obs] + [np.zeros(0, f32)])))
    config = [('GraphConv', [dims[l], dims[l + 1]]) for l in range(n_gcn)] + [('Linear', [dims[-1], Cn])] + ([('LinkPred', [True])] if link else [])
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=Cn, k_spt=k_spt, k_qry=k_qry, task_num=Tn, update_step=3, update_step_test=3,
                              method='G-Meta', sample_nodes=sample_n, link_pred_mode='True' if link else 'False', task_setup='Shared', h=h)
    torch.manual_seed(seed)
    theta0 = [p.detach().cpu().numpy().copy() for p in gmeta_amd.Meta(args, config).net.parameters()]
    theta0 = [t if t.ndim > 1 else (rng.uniform(0.15, 0.4, size=t.shape) * rng.choice([-1.0, 1.0], size=t.shape)).astype(f32) for t in theta0]      # biases off the relu kink
    oaccs, ograd, lq = ew.meta_step(feats, ospt, oqry, ys, yq, theta0, config, k_spt, 0.05, 1e-3, 3)
    og_flat = np.concatenate([g.reshape(-1) for g in ograd])
    tys = [torch.from_numpy(y.astype(np.int64)) for y in ys]; tyq = [torch.from_numpy(y.astype(np.int64)) for y in yq]
    for name, flags in SCHEDULES:
        m = gmeta_amd.Meta(args, config).to('cuda')
        for k, v in flags.items():
            setattr(m, k, v)
        with torch.no_grad():
            for p_, v_ in zip(m.net.parameters(), theta0):
                p_.copy_(torch.from_numpy(v_))
        out, P, _ = m._run(S.views(), tys, Q.views(), tyq, 3, True)
        out = out.cpu().numpy()
        np.testing.assert_allclose(out[P:P + 4] / Tn, lq, atol=TOL, rtol=1e-4, err_msg=name)
        np.testing.assert_allclose(out[:P] / Tn, og_flat, atol=TOL * max(1.0, float(np.abs(og_flat).max())), rtol=1e-3, err_msg=name)
        assert np.abs(out[P + 4:P + 8] / Tn - np.asarray(oaccs)).max() <= 1.0 / (Cn * k_qry) + 1e-6, name
