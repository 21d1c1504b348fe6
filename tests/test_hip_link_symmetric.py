"""GPU (-m gpu): the symmetric pair mode of the extraction (link_pred mode 2 = GM_LINK_SYMMETRIC: h hops around BOTH endpoints) against its
restatement out of the oracle's pieces (tests/link_sym_ref.py) -- node lists, CSR and centre indices bit for bit on every launch shape of k_nodes, the
whole meta-step on every schedule within the project's 1e-4, the Python surface, and the default modes unchanged.  Every case first checks that its
restated batches are NOT the reference mode's, so a build that ignores the mode fails."""
import argparse
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
import link_sym_ref as ref      # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4                       # the project's tolerance on losses / meta-gradients (tests/test_hip_fuzz.py)
SYM = 2                          # GM_LINK_SYMMETRIC


def _extract(store, seeds, h, sample_n, mode, off=None):
    from gmeta_amd.subgraphs import SubgraphBatch
    return SubgraphBatch.extract(store, seeds, [0, len(seeds)] if off is None else off, h, sample_n, ref.RNG_SEED, mode)


# ---------------------------------------------------------------------------------------------------- 1. random multigraphs
@pytest.mark.parametrize('seed', ref.FUZZ_SEEDS)
def test_random_multigraphs_match_restatement(seed):
    import gmeta_amd
    c = ref.fuzz_case(seed)
    assert ref.differs_from_reference_mode(c['og'], c['seeds'], c['h'], c['sample_n']) >= 1
    store = gmeta_amd.GraphStore(c['graphs'], [np.zeros((g[0], 3), np.float32) for g in c['graphs']])
    B = _extract(store, c['seeds'], c['h'], c['sample_n'], SYM)
    ref.assert_batch_matches(B, [ref.extract_batch(c['og'], c['seeds'], c['h'], c['sample_n'])])


# ---------------------------------------------------------------------------------------------------- 2. hubs on the second root
@pytest.mark.parametrize('h,sample_n', ref.HUB_CASES)
def test_hubs_reached_from_the_second_root(h, sample_n):
    import gmeta_amd
    c = ref.hub_case()
    assert ref.differs_from_reference_mode(c['og'], c['seeds'], h, sample_n) >= 1
    store = gmeta_amd.GraphStore(c['graphs'], [np.zeros((c['graphs'][0][0], 3), np.float32)])
    B = _extract(store, c['seeds'], h, sample_n, SYM)
    ref.assert_batch_matches(B, [ref.extract_batch(c['og'], c['seeds'], h, sample_n)])


# ---------------------------------------------------------------------------------------------------- 3. joint build
@pytest.mark.parametrize('seed', [1, 5])
def test_joint_build_equals_two_builds(seed):
    import gmeta_amd
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    c = ref.fuzz_case(seed)
    assert ref.differs_from_reference_mode(c['og'], c['seeds'], c['h'], c['sample_n']) >= 1
    store = gmeta_amd.GraphStore(c['graphs'], [np.zeros((g[0], 3), np.float32) for g in c['graphs']])
    sa, sb = c['seeds'][:4], c['seeds'][4:]
    oa, ob = [0, 1, 4], [0, len(sb)]
    A1, B1 = _extract(store, sa, c['h'], c['sample_n'], SYM, oa), _extract(store, sb, c['h'], c['sample_n'], SYM, ob)
    A2, B2 = SubgraphBatch.extract_pair(store, sa, oa, sb, ob, c['h'], c['sample_n'], ref.RNG_SEED, SYM)
    ref.assert_batch_matches(A2, [ref.extract_batch(c['og'], sa[:1], c['h'], c['sample_n']), ref.extract_batch(c['og'], sa[1:], c['h'], c['sample_n'])])
    for one, two in ((A1, A2), (B1, B2)):
        assert (one.rows, one.edges, one.subs, one.sets, one.centres) == (two.rows, two.edges, two.subs, two.sets, two.centres)
        for field, count, dt in ((0, one.subs + 1, np.int32), (1, one.sets + 1, np.int32), (2, one.rows, np.int32), (3, one.subs, np.int32),
                                 (4, one.rows + 1, np.int32), (5, one.edges, np.int32), (6, one.rows + 1, np.int32), (7, one.edges, np.int32),
                                 (8, one.subs * 2, np.int32), (9, one.rows, np.uint32), (10, one.rows, np.int32), (11, one.rows, np.uint32),
                                 (12, one.rows, np.uint32)):
            x, y = np.empty(count, dt), np.empty(count, dt)
            for b, dst in ((one, x), (two, y)):
                rc = _lib.lib().gm_batch_read(b.handle, field, _lib.ptr(dst), dst.nbytes)
                assert rc == 0, field
            assert np.array_equal(x, y), field


# ---------------------------------------------------------------------------------------------------- 4. global-memory bitmap
def test_global_bitmap_path_on_a_800k_node_graph():
    import gmeta_amd
    c = ref.large_case()
    n, src, dst = c['graphs'][0]
    G = orc.Graph(n, src, dst)
    lists = ref.node_lists([G], c['seeds'], c['h'], c['sample_n'])
    quirk = [orc.sample_nodes(orc.linkpred_nodes(G, int(i), int(j)), c['sample_n'], ref.RNG_SEED, 0, int(i), int(j)) for _, i, j in c['seeds']]
    assert sum(not np.array_equal(a, b) for a, b in zip(lists, quirk)) >= 1
    store = gmeta_amd.GraphStore(c['graphs'], [np.zeros((n, 4), np.float32)])
    B = _extract(store, c['seeds'], c['h'], c['sample_n'], SYM)
    assert B.centres == 2
    par, sub = B.parent(), B.sub_off
    ip, ix = B.csr()
    cen = B._read(8, B.subs * 2, np.int32).reshape(-1, 2)
    for k, (_, i, j) in enumerate(c['seeds']):
        want = lists[k]
        assert np.array_equal(par[sub[k]:sub[k + 1]], want), k
        oip, oix = orc.induce(G, want)
        assert np.array_equal(ip[sub[k]:sub[k + 1] + 1] - ip[sub[k]], oip)
        assert np.array_equal(ix[ip[sub[k]]:ip[sub[k + 1]]] - sub[k], oix)
        assert want[cen[k, 0]] == i and want[cen[k, 1]] == j


# ---------------------------------------------------------------------------------------------------- 5. whole path
@pytest.mark.parametrize('seed', ref.WHOLE_PATH_SEEDS)
def test_meta_step_on_every_schedule_matches_oracle(seed):
    """Mode 2 with an h-layer model (what train.py builds from --h): one meta-step per schedule against orc.meta_step on the restated batches, with
    the conditioning and tolerances of tests/test_hip_fuzz.py (biases moved off the relu kink; 1e-4 on losses and gradients, one tie on accuracies)."""
    import gmeta_amd
    c = ref.whole_path_case(seed)
    rng, h, sample_n, T, C_, k_spt, k_qry, dims, feats, og = (c[k] for k in ('rng', 'h', 'sample_n', 'T', 'C', 'k_spt', 'k_qry', 'dims', 'feats', 'og'))
    assert ref.differs_from_reference_mode(og, np.concatenate(c['spt_seeds'] + c['qry_seeds']), h, sample_n) >= 1
    store = gmeta_amd.GraphStore(c['graphs'], feats)
    ys = [np.repeat(np.arange(C_), k_spt).astype(np.int32) for _ in range(T)]
    yq = [np.repeat(np.arange(C_), k_qry).astype(np.int32) for _ in range(T)]
    S = _extract(store, np.concatenate(c['spt_seeds']), h, sample_n, SYM, np.arange(T + 1) * C_ * k_spt)
    Q = _extract(store, np.concatenate(c['qry_seeds']), h, sample_n, SYM, np.arange(T + 1) * C_ * k_qry)
    ospt = [ref.extract_batch(og, s, h, sample_n) for s in c['spt_seeds']]
    oqry = [ref.extract_batch(og, s, h, sample_n) for s in c['qry_seeds']]
    ref.assert_batch_matches(S, ospt)
    ref.assert_batch_matches(Q, oqry)
    config = [('GraphConv', [dims[l], dims[l + 1]]) for l in range(h)] + [('Linear', [dims[-1], C_]), ('LinkPred', [True])]
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=C_, k_spt=k_spt, k_qry=k_qry, task_num=T, update_step=3, update_step_test=3,
                              method='G-Meta', sample_nodes=sample_n, link_pred_mode='True', task_setup='Shared', h=h)
    theta0 = None
    res = {}
    for name, kw in (('full', {}), ('hoist', dict(hoist_z1=1)), ('sparse', dict(sparse_bwd=1)), ('cone', dict(cone=1)), ('cone+hoist', dict(cone=1, hoist_z1=1))):
        torch.manual_seed(seed)
        m = gmeta_amd.Meta(args, config).to('cuda')
        for k, v in kw.items():
            setattr(m, k, v)
        if theta0 is None:
            theta0 = [p.detach().cpu().numpy().copy() for p in m.net.parameters()]
            theta0 = [t if t.ndim > 1 else rng.uniform(0.15, 0.4, size=t.shape).astype(np.float32) * rng.choice([-1.0, 1.0], size=t.shape).astype(np.float32)
                      for t in theta0]
        with torch.no_grad():
            for p_, v_ in zip(m.net.parameters(), theta0):
                p_.copy_(torch.from_numpy(v_))
        grads = {}
        orig = m.meta_optim.step
        m.meta_optim.step = lambda *a, _g=grads, _m=m, _o=orig, **k: (_g.setdefault('g', torch.cat([p.grad.reshape(-1) for p in _m.net.parameters()]).cpu().numpy().copy()), _o(*a, **k))[1]
        accs = m(S.views(), [torch.from_numpy(y.astype(np.int64)) for y in ys], Q.views(), [torch.from_numpy(y.astype(np.int64)) for y in yq],
                 None, None, None, None, None, None, feats)
        res[name] = (accs, grads.get('g'), m.last_stats['losses_q'])
    oaccs, ograd, _, lq = orc.meta_step(og, feats, ospt, oqry, ys, yq, theta0, config, k_spt, 0.05, 1e-3, 3, adam_state={})
    og_flat = np.concatenate([g.reshape(-1) for g in ograd])
    scale = max(1.0, float(np.abs(og_flat).max()))
    for name, (accs, g, losses) in res.items():
        np.testing.assert_allclose(losses, lq, atol=TOL, rtol=1e-4, err_msg=name)
        assert g is not None, name
        np.testing.assert_allclose(g, og_flat, atol=TOL * scale, rtol=1e-3, err_msg=name)
        assert np.abs(np.asarray(accs) - np.asarray(oaccs)).max() <= 1.0 / (C_ * k_qry) + 1e-9, name


# ---------------------------------------------------------------------------------------------------- 6. public surface
def _surface_db(d, store, h, **kw):
    import gmeta_amd
    s = ref.SURFACE
    np.random.seed(222); random.seed(222)
    over = kw.pop('args', {})
    args = argparse.Namespace(update_lr=0.05, meta_lr=1e-3, n_way=s['n_way'], k_spt=s['k_spt'], k_qry=s['k_qry'], task_num=s['tasks'], update_step=2,
                              update_step_test=2, method='G-Meta', sample_nodes=s['sample_nodes'], link_pred_mode='True', task_setup='Shared', h=h)
    for k, v in over.items():
        setattr(args, k, v)
    db = gmeta_amd.Subgraphs(None, 'train', d['info'], n_way=s['n_way'], k_shot=s['k_spt'], k_query=s['k_qry'], batchsz=s['tasks'], args=args,
                             adjs=store, h=h, tables=d['tables'], verbose=False, **kw)
    return args, db


@pytest.mark.parametrize('h', ref.SURFACE_HOPS)
def test_subgraphs_link_hops_symmetric(h, monkeypatch):
    import gmeta_amd
    s = ref.SURFACE
    d = ref.surface_dataset()
    og = [orc.Graph(*g) for g in d['graphs']]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    args, db = _surface_db(d, store, h, link_hops='symmetric')
    assert db.link_hops == 'symmetric'
    idx = list(range(s['tasks']))
    arrs = [db._task_arrays(i) for i in idx]
    ospt = [ref.extract_batch(og, a[0], h, s['sample_nodes']) for a in arrs]
    oqry = [ref.extract_batch(og, a[1], h, s['sample_nodes']) for a in arrs]
    assert ref.differs_from_reference_mode(og, np.concatenate([a[0] for a in arrs] + [a[1] for a in arrs]), h, s['sample_nodes']) >= 1
    batch = db.get_batch(idx)
    ref.assert_batch_matches(batch[0][0].view_of, ospt)
    ref.assert_batch_matches(batch[2][0].view_of, oqry)
    # every other way the dataset extracts: one task, the two-call variants, the prefetching iterator
    one = db[1]
    ref.assert_batch_matches(one[0], ospt[1:2])
    ref.assert_batch_matches(one[2], oqry[1:2])
    for mode in ('serial', 'threads'):
        monkeypatch.setenv('GMETA_EXTRACT_MODE', mode)
        b2 = db.get_batch(idx)
        ref.assert_batch_matches(b2[0][0].view_of, ospt)
        ref.assert_batch_matches(b2[2][0].view_of, oqry)
    monkeypatch.delenv('GMETA_EXTRACT_MODE')
    for b3 in db.batches([idx[:2], idx[2:], idx[:1]], prefetch=1):
        pass
    ref.assert_batch_matches(b3[0][0].view_of, ospt[:1])
    # unlabelled pairs
    names = ref.surface_query_names(d)
    seeds = [np.array([[int(x) for x in nm.split('_')] for nm in task], np.int32) for task in names]
    assert ref.differs_from_reference_mode(og, np.concatenate(seeds), h, s['sample_nodes']) >= 1
    QB = db.query_batch(names)
    ref.assert_batch_matches(QB, [ref.extract_batch(og, sd, h, s['sample_nodes']) for sd in seeds])
    torch.manual_seed(5)
    from gmeta_amd import synth
    m = gmeta_amd.Meta(args, synth.make_config(s['F0'], 16, h, 2, link=True)).to('cuda')
    pr = m.predict(batch[0], batch[1], QB)
    assert [len(p) for p in pr.pred] == [len(t) for t in names]
    assert all(np.isfinite(lp).all() and set(np.unique(p)) <= {0, 1} for lp, p in zip(pr.log_probs, pr.pred))
    # args.link_hops is the fallback of the keyword
    _, db2 = _surface_db(d, store, h, args=dict(link_hops='symmetric'))
    assert db2.link_hops == 'symmetric' and db2.link_mode == SYM
    ref.assert_batch_matches(db2.query_batch(names), [ref.extract_batch(og, sd, h, s['sample_nodes']) for sd in seeds])


def test_subgraphs_link_hops_errors():
    import gmeta_amd
    d = ref.surface_dataset()
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    with pytest.raises(ValueError, match='link_hops'):
        _surface_db(d, store, 2, link_hops='both')
    with pytest.raises(ValueError, match='link_pred_mode'):
        _surface_db(d, store, 2, link_hops='symmetric', args=dict(link_pred_mode='False'))
    with pytest.raises(ValueError, match='sample_mode'):
        _surface_db(d, store, 2, link_hops='symmetric', sample_mode='reference')
    _, db = _surface_db(d, store, 2)
    assert db.link_hops == 'reference' and db.link_mode == 1


def test_c_abi_modes():
    """link_pred is a mode: 2 needs h in 1..3, anything but 0 / 1 / 2 is refused (GM_EINVAL -> ValueError, with a message); gm_batch_from_nodes keeps
    treating any non-zero value as "two centres"."""
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    c = ref.fuzz_case(4)
    store = gmeta_amd.GraphStore(c['graphs'], [np.zeros((g[0], 3), np.float32) for g in c['graphs']])
    for h in (0, 4, -1):
        with pytest.raises(ValueError, match='symmetric'):
            _extract(store, c['seeds'], h, 40, SYM)
        with pytest.raises(ValueError, match='symmetric'):
            SubgraphBatch.extract_pair(store, c['seeds'][:3], [0, 3], c['seeds'][3:], [0, len(c['seeds']) - 3], h, 40, ref.RNG_SEED, SYM)
    for mode in (3, -1, 7):
        with pytest.raises(ValueError, match='mode'):
            _extract(store, c['seeds'], 2, 40, mode)
    lists = ref.node_lists(c['og'], c['seeds'], c['h'], c['sample_n'])
    want = [ref.extract_batch(c['og'], c['seeds'], c['h'], c['sample_n'])]
    for mode in (1, 2, 5, True):
        ref.assert_batch_matches(SubgraphBatch.from_nodes(store, c['seeds'], [0, len(c['seeds'])], lists, mode), want)


# ---------------------------------------------------------------------------------------------------- 7. default unchanged
@pytest.mark.parametrize('seed', [1, 2, 7])
def test_reference_pair_mode_unchanged(seed):
    """True, 1 and a dataset without link_hops give the reference's pairs (i two hops, j one, h ignored), bit for bit."""
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    c = ref.fuzz_case(seed)
    store = gmeta_amd.GraphStore(c['graphs'], [np.zeros((g[0], 3), np.float32) for g in c['graphs']])
    for h in (1, 2, 3, 9):
        want = [orc.extract_batch(c['og'], c['seeds'], h, c['sample_n'], ref.RNG_SEED, True)]
        for mode in (True, 1, np.bool_(True)):
            ref.assert_batch_matches(_extract(store, c['seeds'], h, c['sample_n'], mode), want)
    sa, sb = c['seeds'][:5], c['seeds'][5:]
    A, B = SubgraphBatch.extract_pair(store, sa, [0, 5], sb, [0, len(sb)], 3, c['sample_n'], ref.RNG_SEED, True)
    ref.assert_batch_matches(A, [orc.extract_batch(c['og'], sa, 3, c['sample_n'], ref.RNG_SEED, True)])
    ref.assert_batch_matches(B, [orc.extract_batch(c['og'], sb, 3, c['sample_n'], ref.RNG_SEED, True)])


def test_dataset_without_link_hops_unchanged():
    import gmeta_amd
    s = ref.SURFACE
    d = ref.surface_dataset()
    og = [orc.Graph(*g) for g in d['graphs']]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    _, db = _surface_db(d, store, 3)
    idx = list(range(s['tasks']))
    arrs = [db._task_arrays(i) for i in idx]
    batch = db.get_batch(idx)
    ref.assert_batch_matches(batch[0][0].view_of, [orc.extract_batch(og, a[0], 3, s['sample_nodes'], ref.RNG_SEED, True) for a in arrs])
    ref.assert_batch_matches(batch[2][0].view_of, [orc.extract_batch(og, a[1], 3, s['sample_nodes'], ref.RNG_SEED, True) for a in arrs])
    names = ref.surface_query_names(d)
    seeds = [np.array([[int(x) for x in nm.split('_')] for nm in task], np.int32) for task in names]
    ref.assert_batch_matches(db.query_batch(names), [orc.extract_batch(og, sd, 3, s['sample_nodes'], ref.RNG_SEED, True) for sd in seeds])
