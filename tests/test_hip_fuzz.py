"""GPU (-m gpu): randomised differential test of the whole path against the oracle on small ragged multigraphs --
self-loops, parallel edges, isolated nodes, zero-in-degree centres, h = 1, 2, 3, link-pred pairs, sampling on and off,
odd feature widths, 1-3 GCN layers in both branch orders -- through the C ABI: extraction bit-exact, then one meta-step
for the dense schedule and the flagged exact ones.  Besides the 1e-4 comparisons against the fp32 oracle, every schedule's meta-gradient (per parameter tensor) and
losses_q are held to 4 x the fp32 yardstick against the oracle's fp64 statement of the step (tests/step_bar.py, tests/test_hip_step_numerics.py)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, ROOT)
import gmeta_oracle as orc      # noqa: E402  (the checker)
import step_bar as sb           # noqa: E402  (its fp64 statement of the step and the bar)

pytestmark = pytest.mark.gpu
TOL = 1e-4                       # north_star tolerance on logits / meta-gradients
# Worlds whose fp64 yardstick takes the fmaf-chain order of k_gemm_nn / k_wgrad (orc.sequential_products; every fuzz world is served by those kernels) beside
# numpy's blocked order, with what numpy's order alone left above the bar of 4: the device's error against the yardstick, in u.  Per-kernel bars of that order:
# test_hip_gemm_numerics.py / test_hip_gemm_epilogue.py / test_hip_wgrad_numerics.py.
FMAF_CHAIN_SEEDS = {0: 'losses_q 2.48 u against 0.50 u (the floor: the oracle was exact by chance)', 11: 'grad/0 12.09 u against 2.62 u'}


def _graph(rng, n):
    m = int(rng.integers(n, 6 * n))
    src = rng.integers(0, n, size=m); dst = rng.integers(0, n, size=m)
    hub = int(rng.integers(0, n))                                      # one hub: most nodes point at it
    k = int(rng.integers(n // 2, n))
    src = np.concatenate([src, rng.integers(0, n, size=k), [hub, hub]]); dst = np.concatenate([dst, np.full(k, hub), [hub, hub]])   # + parallel self-loops
    iso = rng.integers(0, n, size=max(1, n // 20))                     # isolated nodes: drop every edge touching them
    keep = ~(np.isin(src, iso) | np.isin(dst, iso))
    return n, src[keep].astype(np.int64), dst[keep].astype(np.int64)


def _launches(category):
    """launches of one category of the launch accounting in the last meta-step (gm_profile_read)"""
    import ctypes as C
    from gmeta_amd import _lib
    ms, n, wk = C.c_double(), C.c_int64(), C.c_int64()
    _lib.lib().gm_profile_read(category, C.byref(ms), C.byref(n), C.byref(wk))
    return int(n.value)


@pytest.mark.parametrize('seed', list(range(int(os.environ.get('GMETA_FUZZ_SEEDS', '14')))))
def test_random_multigraph_matches_oracle(seed):
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    rng = np.random.default_rng(1000 + seed)
    link = seed % 4 == 3
    h = int(rng.integers(1, 4))
    n_graphs = int(rng.integers(1, 4))
    F0 = int(rng.choice([1, 5, 12, 32, 50, 64]))
    graphs = [_graph(rng, int(rng.integers(25, 160))) for _ in range(n_graphs)]
    feats = [rng.standard_normal((g[0], F0)).astype(np.float32) for g in graphs]
    sample_n = int(rng.choice([6, 15, 40, 10000]))
    T, C = int(rng.integers(1, 4)), int(rng.integers(2, 4))
    k_spt, k_qry = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    n_gcn = 2 if link else int(rng.integers(1, 4))                     # the model's layer count need not equal h for the kernels
    dims = [F0] + [int(rng.choice([8, 16, 20, 32, 64])) for _ in range(n_gcn)]
    if seed % 3 == 0 and F0 >= 32:
        dims[1] = 8                                                     # multiply-first first layer (in > out)

    def seeds_for(count):
        out = []
        for _ in range(count):
            g = int(rng.integers(0, n_graphs)); n = graphs[g][0]
            i = int(rng.integers(0, n)); j = int(rng.integers(0, n)) if link else -1
            if link and j == i:
                j = (i + 1) % n
            out.append((g, i, j))
        return np.array(out, np.int32)
    store = gmeta_amd.GraphStore(graphs, feats)
    og = [orc.Graph(*g) for g in graphs]
    spt_seeds = [seeds_for(C * k_spt) for _ in range(T)]
    qry_seeds = [seeds_for(C * k_qry) for _ in range(T)]
    ys = [np.repeat(np.arange(C), k_spt).astype(np.int32) for _ in range(T)]
    yq = [np.repeat(np.arange(C), k_qry).astype(np.int32) for _ in range(T)]
    S = SubgraphBatch.extract(store, np.concatenate(spt_seeds), np.arange(T + 1) * C * k_spt, h, sample_n, 222, link)
    Q = SubgraphBatch.extract(store, np.concatenate(qry_seeds), np.arange(T + 1) * C * k_qry, h, sample_n, 222, link)
    ospt = [orc.extract_batch(og, s, h, sample_n, 222, link) for s in spt_seeds]
    oqry = [orc.extract_batch(og, s, h, sample_n, 222, link) for s in qry_seeds]
    # ---- integer work: bit-exact (node lists, CSR, centres)
    for hb, obs in ((S, ospt), (Q, oqry)):
        assert np.array_equal(hb.parent(), np.concatenate([b.parent for b in obs]))
        ip, ix = hb.csr()
        r0 = e0 = 0
        for b in obs:
            assert np.array_equal(ip[r0:r0 + b.n + 1] - e0, b.indptr) and np.array_equal(ix[e0:e0 + len(b.indices)] - r0, b.indices)
            r0 += b.n; e0 += len(b.indices)
        cen = np.concatenate([(b.centre_rows - b.sub_off[:-1, None]).reshape(-1) for b in obs])      # local index inside each subgraph
        assert np.array_equal(hb._read(8, hb.subs * hb.centres, np.int32), cen)
    # ---- one meta-step per schedule
    config = [('GraphConv', [dims[l], dims[l + 1]]) for l in range(n_gcn)] + [('Linear', [dims[-1], C])] + ([('LinkPred', [True])] if link else [])
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=C, k_spt=k_spt, k_qry=k_qry, task_num=T, update_step=3, update_step_test=3,
                              method='G-Meta', sample_nodes=sample_n, link_pred_mode='True' if link else 'False', task_setup='Shared', h=h)
    torch.manual_seed(seed)
    theta0 = None
    res = {}
    for name, kw in (('full', {}), ('hoist', dict(hoist_z1=1)), ('sparse', dict(sparse_bwd=1)), ('cone', dict(cone=1)), ('cone+hoist', dict(cone=1, hoist_z1=1))):
        torch.manual_seed(seed)
        m = gmeta_amd.Meta(args, config).to('cuda')
        for k, v in kw.items():
            setattr(m, k, v)
        if theta0 is None:
            # biases start at zero in the reference (learner.py:96): an isolated centre then sits exactly on the relu kink and
            # fp noise in the (mathematically zero) bias gradient decides relu' in later inner steps -- a property of the model,
            # not of an implementation.  Move every bias well off the kink so that the comparison is conditioned.
            theta0 = [p.detach().cpu().numpy().copy() for p in m.net.parameters()]
            theta0 = [t if t.ndim > 1 else rng.uniform(0.15, 0.4, size=t.shape).astype(np.float32) * rng.choice([-1.0, 1.0], size=t.shape).astype(np.float32)
                      for t in theta0]
        with torch.no_grad():
            for p_, v_ in zip(m.net.parameters(), theta0):
                p_.copy_(torch.from_numpy(v_))
        grads = {}
        orig = m.meta_optim.step
        m.meta_optim.step = lambda *a, _g=grads, _m=m, _o=orig, **k: (_g.setdefault('g', torch.cat([p.grad.reshape(-1) for p in _m.net.parameters()]).cpu().numpy().copy()), _o(*a, **k))[1]
        chain = seed in FMAF_CHAIN_SEEDS
        if chain:
            gmeta_amd._lib.lib().gm_profile_enable(1)
        try:
            accs = m(S.views(), [torch.from_numpy(y.astype(np.int64)) for y in ys], Q.views(), [torch.from_numpy(y.astype(np.int64)) for y in yq],
                     None, None, None, None, None, None, feats)
            if chain:      # the exact-fp32 kernels (launch category 1: k_gemm_nn) served this world, the split kernels (4 / 5) took no launch: the order its yardstick models
                torch.cuda.synchronize()
                assert _launches(1) > 0 and _launches(4) == 0 and _launches(5) == 0, name
        finally:
            if chain:
                gmeta_amd._lib.lib().gm_profile_enable(0)
        res[name] = (accs, grads.get('g'), m.last_stats['losses_q'])
    oaccs, ograd, _, lq = orc.meta_step(og, feats, ospt, oqry, ys, yq, theta0, config, k_spt, 0.05, 1e-3, 3, adam_state={})
    og_flat = np.concatenate([g.reshape(-1) for g in ograd])
    scale = max(1.0, float(np.abs(og_flat).max()))
    for name, (accs, g, losses) in res.items():
        np.testing.assert_allclose(losses, lq, atol=TOL, rtol=1e-4, err_msg=name)
        assert g is not None, name
        np.testing.assert_allclose(g, og_flat, atol=TOL * scale, rtol=1e-3, err_msg=name)
        # accuracies are argmax decisions: equal unless two distances tie within noise
        assert np.abs(np.asarray(accs) - np.asarray(oaccs)).max() <= 1.0 / (C * k_qry) + 1e-9, name
    # ---- and against fp64, per tensor, at 4 x what the fp32 oracle itself misses fp64 by
    ref = sb.reference(sb.device_sets(S, feats), sb.device_sets(Q, feats), ys, yq, theta0, config, k_spt, 0.05, 3, sequential=seed in FMAF_CHAIN_SEEDS)
    report = sb.Report()
    for name, (accs, g, losses) in res.items():
        sb.hold_step(report, 'fuzz %d %s' % (seed, name), ref, theta0, g, losses)
    report.assert_ok()


@pytest.mark.parametrize('dims', [[512, 128, 128], [64, 512, 512], [100, 300, 60], [2048, 64]])
def test_wide_and_odd_layer_shapes_match_oracle(dims):
    """Shapes outside the specialised kernels' sweet spot (Fold-PPI's 512 -> 128 multiply-first layer, 512-wide hidden
    layers, widths that are not multiples of 32, the 2048 limit): generic kernels, same results."""
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    rng = np.random.default_rng(77)
    n_gcn = len(dims) - 1
    graphs = [_graph(rng, 90)]
    feats = [(0.3 * rng.standard_normal((90, dims[0]))).astype(np.float32)]
    T, C, k_spt, k_qry, h = 2, 2, 2, 3, 2
    store = gmeta_amd.GraphStore(graphs, feats)
    og = [orc.Graph(*g) for g in graphs]
    mk = lambda cnt: np.array([(0, int(rng.integers(0, 90)), -1) for _ in range(cnt)], np.int32)      # noqa: E731
    spt_seeds = [mk(C * k_spt) for _ in range(T)]; qry_seeds = [mk(C * k_qry) for _ in range(T)]
    ys = [np.repeat(np.arange(C), k_spt).astype(np.int32) for _ in range(T)]
    yq = [np.repeat(np.arange(C), k_qry).astype(np.int32) for _ in range(T)]
    S = SubgraphBatch.extract(store, np.concatenate(spt_seeds), np.arange(T + 1) * C * k_spt, h, 1000, 222, False)
    Q = SubgraphBatch.extract(store, np.concatenate(qry_seeds), np.arange(T + 1) * C * k_qry, h, 1000, 222, False)
    ospt = [orc.extract_batch(og, s, h, 1000, 222, False) for s in spt_seeds]
    oqry = [orc.extract_batch(og, s, h, 1000, 222, False) for s in qry_seeds]
    config = [('GraphConv', [dims[l], dims[l + 1]]) for l in range(n_gcn)] + [('Linear', [dims[-1], C])]
    args = argparse.Namespace(update_lr=0.02, meta_lr=1e-3, n_way=C, k_spt=k_spt, k_qry=k_qry, task_num=T, update_step=2, update_step_test=2,
                              method='G-Meta', sample_nodes=1000, link_pred_mode='False', task_setup='Shared', h=h)
    theta0 = None
    report = sb.Report()
    for kw in ({}, dict(cone=1)):
        torch.manual_seed(3)
        m = gmeta_amd.Meta(args, config).to('cuda')
        for k, v in kw.items():
            setattr(m, k, v)
        if theta0 is None:
            theta0 = [p.detach().cpu().numpy().copy() for p in m.net.parameters()]
            theta0 = [t if t.ndim > 1 else (rng.uniform(0.15, 0.4, size=t.shape) * rng.choice([-1.0, 1.0], size=t.shape)).astype(np.float32) for t in theta0]
        with torch.no_grad():
            for p_, v_ in zip(m.net.parameters(), theta0):
                p_.copy_(torch.from_numpy(v_))
        grads = {}
        orig = m.meta_optim.step
        m.meta_optim.step = lambda *a, _g=grads, _m=m, _o=orig, **k: (_g.setdefault('g', torch.cat([p.grad.reshape(-1) for p in _m.net.parameters()]).cpu().numpy().copy()), _o(*a, **k))[1]
        m(S.views(), [torch.from_numpy(y.astype(np.int64)) for y in ys], Q.views(), [torch.from_numpy(y.astype(np.int64)) for y in yq],
          None, None, None, None, None, None, feats)
        oaccs, ograd, _, lq = orc.meta_step(og, feats, ospt, oqry, ys, yq, theta0, config, k_spt, 0.02, 1e-3, 2, adam_state={})
        og_flat = np.concatenate([g.reshape(-1) for g in ograd])
        np.testing.assert_allclose(m.last_stats['losses_q'], lq, atol=TOL, rtol=1e-4)
        np.testing.assert_allclose(grads['g'], og_flat, atol=TOL * max(1.0, float(np.abs(og_flat).max())), rtol=1e-3)
        if not kw:
            ref = sb.reference(sb.device_sets(S, feats), sb.device_sets(Q, feats), ys, yq, theta0, config, k_spt, 0.02, 2)
        sb.hold_step(report, 'fuzz dims %s %s' % ('x'.join(str(d) for d in dims), 'cone' if kw else 'full'), ref, theta0, grads['g'], m.last_stats['losses_q'])
    report.assert_ok()
