"""Meta.adapt / Adapted.predict / Meta.predict (gm_meta_adapt, gm_proto_predict, k_head_predict): labelling query subgraphs with a
fine-tuned model.  Checked against finetunning_batch (exact: the same kernels score the same subgraphs), against an oracle composed from the
CPU restatement, on unlabelled ragged query sets, at 10^5 subgraphs per call, for state isolation, under the flagged schedules, and for its
argument errors."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from golden_util import CASES, NAN_CASES, WIDE_CASES, Fixture      # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def _hu():
    import hip_util
    return hip_util


def _labels(fx, tag):
    return [torch.from_numpy(y.astype(np.int64)) for y in fx.z['y_' + tag]]


def _setup(case, hoist=0, sparse_bwd=0, cone=0):
    hu = _hu()
    fx = Fixture(case)
    store = hu.make_store(fx)
    S, Q = hu.fixture_batches(fx, store, True)
    m = hu.fixture_meta(fx)
    m.hoist_z1, m.sparse_bwd, m.cone = hoist, sparse_bwd, cone
    return fx, store, S, Q, m


def _check_agreement(fx, S, Q, m):
    """For every j in 0..K_test: the correct labels of predict(K=j) per task == finetunning_batch accs[:, j] * Q_t, as fp32 count / Q."""
    ys, yq = _labels(fx, 'spt'), _labels(fx, 'qry')
    ft = m.finetunning_batch(S.views(), ys, Q.views(), yq)
    for j in range(fx.K_test + 1):
        pr = m.predict(S.views(), ys, Q.views(), K=j)
        for t in range(fx.T):
            y = yq[t].numpy()
            got = f32(np.count_nonzero(pr.labels[t] == y)) / f32(len(y))
            assert got == f32(ft[t, j]), (fx.name, j, t, got, ft[t, j])
    return ft


@pytest.mark.parametrize('case', CASES)
def test_predict_agrees_with_finetunning(case):
    fx, store, S, Q, m = _setup(case)
    _check_agreement(fx, S, Q, m)


@pytest.mark.parametrize('case', WIDE_CASES)
def test_predict_agrees_with_finetunning_split_and_exact(case):
    from gmeta_amd import _lib
    lib = _lib.lib()
    fx, store, S, Q, m = _setup(case)
    old = lib.gm_get_tuning(b'GM_GEMM_SPLIT_MIN_TILES')
    lib.gm_set_tuning(b'GM_GEMM_SPLIT_MIN_TILES', 0)
    try:
        _check_agreement(fx, S, Q, m)
    finally:
        lib.gm_set_tuning(b'GM_GEMM_SPLIT_MIN_TILES', old)
    mode = lib.gm_get_gemm_mode()
    lib.gm_set_gemm_mode(0)
    try:
        _check_agreement(fx, S, Q, m)
    finally:
        lib.gm_set_gemm_mode(mode)


# ---------------------------------------------------------------------------------------------------- oracle
def _orc_adapt(fx, spt, xs, ys, K):
    """Support chain of the oracle (classifier_forward -> proto_loss_spt -> classifier_backward -> SGD) K times: fw_K and the prototypes of the
    support pass at fw_{max(K-1, 0)}."""
    import gmeta_oracle as orc
    fw = [v.copy() for v in fx.vars0]
    protos = None
    for k in range(max(K, 1)):
        logit_s, cs = orc.classifier_forward(spt, xs, fw, fx.config)
        _, _, protos, dls = orc.proto_loss_spt(logit_s, ys, fx.args['k_spt'], need_grad=K > 0)
        if K > 0:
            g = orc.classifier_backward(spt, fw, fx.config, cs, dls)
            fw = [w - f32(fx.args['update_lr']) * gg for w, gg in zip(fw, g)]
    return fw, protos


def _orc_logp(fx, qb, feats, fw, protos):
    import gmeta_oracle as orc
    z, _ = orc.classifier_forward(qb, qb.features(feats), fw, fx.config)
    d = ((z[:, None, :] - protos[None, :, :]) ** 2).sum(2)
    return orc._log_softmax(-d)


def _close(a, b, tol=1e-4, nan_subset=False):
    """Within tol, NaN at the same positions.  nan_subset (the inf-feature fixtures): NaN(a) must lie inside NaN(b) -- the oracle masks relu'
    by multiplication (dh * (h > 0): inf * 0 = NaN), the kernels and torch's threshold_backward by selection, so the oracle's fast weights can
    hold NaN where the kernels' hold numbers; those positions are not compared."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if nan_subset:
        assert not (np.isnan(a) & ~np.isnan(b)).any()
    else:
        assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a) & ~np.isnan(b)
    np.testing.assert_allclose(a[ok], b[ok], atol=tol, rtol=0)


def _orc_batches(fx, tag):
    import gmeta_oracle as orc
    graphs = fx.graphs()
    return [orc.extract_batch(graphs, fx.z[tag + '_seeds'][t], fx.args['h'], fx.args['sample_nodes'], 222, fx.link,
                              replay_nodes=fx.replay_lists(tag, t)) for t in range(fx.T)]


@pytest.mark.parametrize('case', CASES)
def test_adapt_and_predict_match_oracle(case):
    fx, store, S, Q, m = _setup(case)
    ys = _labels(fx, 'spt')
    spt, qry = _orc_batches(fx, 'spt'), _orc_batches(fx, 'qry')
    sub = case in NAN_CASES
    for K in sorted({0, 1, fx.K_test}):
        ad = m.adapt(S.views(), ys, K=K)
        pr = ad.predict(Q.views())
        fw_h, pt_h = ad.fast_weights.cpu().numpy(), ad.prototypes.cpu().numpy()
        for t in range(fx.T):
            fw, protos = _orc_adapt(fx, spt[t], spt[t].features(fx.feats), fx.z['y_spt'][t], K)
            _close(fw_h[t], np.concatenate([w.reshape(-1) for w in fw]), nan_subset=sub)
            n = len(ad.classes[t])
            _close(pt_h[t, :n], protos, nan_subset=sub)
            assert not pt_h[t, n:].any()
            _close(pr.log_probs[t], _orc_logp(fx, qry[t], fx.feats, fw, protos), nan_subset=sub)


# ---------------------------------------------------------------------------------------------------- unlabelled, ragged query sets
def _ragged_seeds(fx, rng, n):
    out = []
    for _ in range(n):
        g = int(rng.integers(len(fx.edges)))
        nn = fx.edges[g][0]
        i = int(rng.integers(nn))
        j = -1
        if fx.link:
            j = int(rng.integers(nn - 1)); j += j >= i
        out.append((g, i, j))
    return np.asarray(out, np.int32)


@pytest.mark.parametrize('case', ['g0_disjoint_h1', 'g1_sampled_h2', 'g1_h3', 'g3_linkpred', 'g5_in_gt_out'])
def test_predict_ragged_unlabelled_queries_match_oracle(case):
    import gmeta_oracle as orc
    from gmeta_amd.subgraphs import SubgraphBatch
    fx, store, S, Q, m = _setup(case)
    rng = np.random.default_rng(7)
    sizes = [1, 7, 300]
    seeds = [_ragged_seeds(fx, rng, n) for _ in range(fx.T) for n in sizes]          # arbitrary nodes: classes outside the support included
    off = np.cumsum([0] + [len(s) for s in seeds])
    QB = SubgraphBatch.extract(store, np.concatenate(seeds), off, fx.args['h'], fx.args['sample_nodes'], 222, fx.link)
    tasks = [t for t in range(fx.T) for _ in sizes]
    ad = m.adapt(S.views(), _labels(fx, 'spt'))
    pr = ad.predict(QB, tasks=tasks, logits=True)
    spt = _orc_batches(fx, 'spt')
    graphs = fx.graphs()
    for i, t in enumerate(tasks):
        fw, protos = _orc_adapt(fx, spt[t], spt[t].features(fx.feats), fx.z['y_spt'][t], fx.K_test)
        qb = orc.extract_batch(graphs, seeds[i], fx.args['h'], fx.args['sample_nodes'], 222, fx.link)
        lp = _orc_logp(fx, qb, fx.feats, fw, protos)
        assert pr.log_probs[i].shape == (sizes[i % 3], len(ad.classes[t])) and pr.logits[i].shape[0] == sizes[i % 3]
        _close(pr.log_probs[i], lp)
        srt = np.sort(lp, 1)
        sure = (srt[:, -1] - srt[:, -2] > 1e-4) if lp.shape[1] > 1 else np.ones(len(lp), bool)
        assert np.array_equal(pr.labels[i][sure], ad.classes[t][lp.argmax(1)][sure])
        assert np.array_equal(pr.labels[i], ad.classes[t][pr.pred[i]])


# ---------------------------------------------------------------------------------------------------- large
def _arxiv_db(T, sample_nodes):
    import gmeta_amd
    from gmeta_amd import synth
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args('arxiv', task_num=T, sample_nodes=sample_nodes)
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=3, k_shot=3, k_query=24, batchsz=T, args=args, adjs=store, h=2,
                             tables=data['tables'], verbose=False)
    return args, cfg, data, store, db


def test_predict_large_query_batch():
    import gmeta_amd
    import gmeta_oracle as orc
    from gmeta_amd import synth
    T, NQ = 2, 50000                                    # 100,000 query subgraphs in one call
    args, cfg, data, store, db = _arxiv_db(T, 16)      # (16 sampled nodes per subgraph: ~2M rows, the workspace of one forward stays ~12 GB)
    batch = db.get_batch(list(range(T)))
    m = gmeta_amd.Meta(args, synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], synth.n_out(cfg))).to('cuda')
    ad = m.adapt(batch[0], batch[1], K=2)
    rng = np.random.default_rng(3)
    n = data['graphs'][0][0]
    names = [['0_%d' % v for v in rng.integers(0, n, NQ)] for _ in range(T)]
    QB = db.query_batch(names)
    assert QB.subs == T * NQ
    full = ad.predict(QB)
    # the same queries in four chunks
    parts = [db.query_batch([nm[c * NQ // 2:(c + 1) * NQ // 2]]) for nm in names for c in range(2)]
    chunked = [ad.predict(p, tasks=[k // 2]) for k, p in enumerate(parts)]
    for t in range(T):
        lp = np.concatenate([chunked[2 * t + c].log_probs[0] for c in range(2)])
        lab = np.concatenate([chunked[2 * t + c].labels[0] for c in range(2)])
        _close(full.log_probs[t], lp)
        srt = np.sort(lp, 1)
        sure = srt[:, -1] - srt[:, -2] > 1e-4
        assert np.array_equal(full.labels[t][sure], lab[sure])
    # 256 sampled subgraphs per task against the oracle (a subgraph's logits depend on its own subgraph only)
    graphs = [orc.Graph(*g) for g in data['graphs']]
    fw_h, pt_h = ad.fast_weights.cpu().numpy(), ad.prototypes.cpu().numpy()
    shapes = [p.shape for p in m.net.parameters()]
    cfg_l = synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], synth.n_out(cfg))

    class _Fx:
        config = cfg_l
    for t in range(T):
        pick = np.sort(rng.choice(NQ, 256, replace=False))
        seeds = np.asarray([(0, int(names[t][k].split('_')[1]), -1) for k in pick], np.int32)
        qb = orc.extract_batch(graphs, seeds, args.h, args.sample_nodes, 222, False)
        fw, off = [], 0
        for s in shapes:
            k = int(np.prod(s)); fw.append(fw_h[t, off:off + k].reshape(s)); off += k
        nc = len(ad.classes[t])
        _close(full.log_probs[t][pick], _orc_logp(_Fx, qb, data['feats'], fw, pt_h[t, :nc]))


# ---------------------------------------------------------------------------------------------------- state
def test_predict_leaves_training_state_alone():
    import copy
    fx, store, S, Q, m = _setup('g2_shared')
    ys, yq = _labels(fx, 'spt'), _labels(fx, 'qry')
    m(S.views(), ys, Q.views(), yq, None, None, None, None, None, None, fx.feats)        # Adam state and .grad exist
    twin = copy.deepcopy(m)                                                             # train.py's snapshot: never predicts
    snap = lambda mm: ([p.detach().clone() for p in mm.net.parameters()], [p.grad.clone() for p in mm.net.parameters()],    # noqa: E731
                       {k: {n: v.clone() for n, v in s.items()} for k, s in enumerate(mm.meta_optim.state.values())})
    before = snap(m)
    p1 = m.predict(S.views(), ys, Q.views(), logits=True)
    ad = m.adapt(S.views(), ys)
    p2, p3 = ad.predict(Q.views(), logits=True), ad.predict(Q.views(), logits=True)
    after = snap(m)
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert torch.equal(a, b)
    for k in before[2]:
        for n in before[2][k]:
            assert torch.equal(before[2][k][n], after[2][k][n])
    for a, b in ((p1, p2), (p2, p3)):
        for t in range(fx.T):
            assert np.array_equal(a.log_probs[t], b.log_probs[t], equal_nan=True) and np.array_equal(a.pred[t], b.pred[t])
            assert np.array_equal(a.logits[t], b.logits[t], equal_nan=True)
    # a meta-step after the interleaved predictions == the same meta-step on a twin that never predicted
    a1 = m(S.views(), ys, Q.views(), yq, None, None, None, None, None, None, fx.feats)
    a2 = twin(S.views(), ys, Q.views(), yq, None, None, None, None, None, None, fx.feats)
    assert np.array_equal(a1, a2)
    for p, q in zip(m.net.parameters(), twin.net.parameters()):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad)


# ---------------------------------------------------------------------------------------------------- flagged schedules
@pytest.mark.parametrize('flag', ['hoist_z1', 'cone', 'sparse_bwd'])
@pytest.mark.parametrize('case', ['g1_sampled_h2', 'g3_linkpred', 'g7_wide_h2'])
def test_predict_flagged_schedules(flag, case):
    fx, store, S, Q, m = _setup(case, **{'hoist': 0, 'sparse_bwd': 0, 'cone': 0})
    ys = _labels(fx, 'spt')
    dense = m.predict(S.views(), ys, Q.views())
    setattr(m, flag, 1)
    _check_agreement(fx, S, Q, m)
    flagged = m.predict(S.views(), ys, Q.views())
    for t in range(fx.T):
        _close(flagged.log_probs[t], dense.log_probs[t])


# ---------------------------------------------------------------------------------------------------- errors
def test_predict_errors():
    import ctypes as C
    from gmeta_amd import _lib
    hu = _hu()
    fx, store, S, Q, m = _setup('g1_sampled_h2')
    ys = _labels(fx, 'spt')
    ad = m.adapt(S.views(), ys, K=1)
    with pytest.raises(ValueError, match='tasks'):
        ad.predict(Q.views(), tasks=list(range(fx.T + 1)))
    with pytest.raises(ValueError, match='tasks'):
        ad.predict(Q.views(), tasks=[fx.T] * fx.T)
    with pytest.raises(ValueError, match='K must be'):
        m.adapt(S.views(), ys, K=-1)
    bad = [y.clone() for y in ys]
    bad[0][0] = 99                                      # a class with one row < k_spt = 2
    with pytest.raises(ValueError, match='n_support'):
        m.adapt(S.views(), bad)
    other = hu.make_store(fx)
    S2, Q2 = hu.fixture_batches(fx, other, True)
    with pytest.raises(ValueError, match='store'):
        ad.predict(Q2.views())
    # C ABI: c_task too small, parameter strides below P
    lib = _lib.lib()
    model = m.net.model
    P = int(lib.gm_model_param_count(C.byref(model)))
    hp = _lib.HParams(float(m.update_lr), 1, int(m.k_spt), 0, 0, 0, 0, 0)
    ws = torch.empty(int(lib.gm_adapt_ws_bytes(S.handle, C.byref(model), C.byref(hp))), dtype=torch.uint8, device='cuda')
    theta = m._flat_theta()
    fw = torch.empty(fx.T, P, device='cuda'); pt = torch.empty(fx.T, 8, model.n_out, device='cuda')
    yy = np.concatenate([y.numpy() for y in ys]).astype(np.int32)
    ncls = min(len(c) for c in ad.classes)
    rc = lib.gm_meta_adapt(S.handle, _lib.ptr(yy), C.byref(model), C.byref(hp), _lib.ptr(theta), _lib.ptr(fw), P, _lib.ptr(pt), ncls - 1,
                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == -1 and b'c_task' in lib.gm_last_error()
    rc = lib.gm_meta_adapt(S.handle, _lib.ptr(yy), C.byref(model), C.byref(hp), _lib.ptr(theta), _lib.ptr(fw), P - 1, _lib.ptr(pt), 8,
                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == -1 and b'fw_stride' in lib.gm_last_error()
    hp_g = _lib.HParams(float(m.update_lr), 1, int(m.k_spt), 1, 0, 0, 0, 0)
    rc = lib.gm_meta_adapt(S.handle, _lib.ptr(yy), C.byref(model), C.byref(hp_g), _lib.ptr(theta), _lib.ptr(fw), P, _lib.ptr(pt), 8,
                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == -1 and b'need_meta_grad' in lib.gm_last_error()
    wq = torch.empty(int(lib.gm_predict_ws_bytes(Q.handle, C.byref(model), C.byref(hp))), dtype=torch.uint8, device='cuda')
    nq = np.full(Q.sets, 2, np.int32)
    lp = torch.empty(Q.subs, 8, device='cuda'); pd = torch.empty(Q.subs, dtype=torch.int32, device='cuda')
    rc = lib.gm_proto_predict(Q.handle, C.byref(model), C.byref(hp), _lib.ptr(fw), P - 1, _lib.ptr(pt), _lib.ptr(nq), 8, None, _lib.ptr(lp), _lib.ptr(pd),
                              _lib.ptr(wq), wq.numel(), _lib.stream_ptr())
    assert rc == -1 and b'param_stride' in lib.gm_last_error()
    nq[0] = 9
    rc = lib.gm_proto_predict(Q.handle, C.byref(model), C.byref(hp), _lib.ptr(fw), P, _lib.ptr(pt), _lib.ptr(nq), 8, None, _lib.ptr(lp), _lib.ptr(pd),
                              _lib.ptr(wq), wq.numel(), _lib.stream_ptr())
    assert rc == -1 and b'c_task' in lib.gm_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- driver
def test_train_driver_predict_out(tmp_path):
    sys.path.insert(0, ROOT)
    import train as drv
    from test_train_driver import _dataset
    _, _, info = _dataset(tmp_path)
    out = str(tmp_path / 'pred.npz')
    args = drv.parse(['--data_dir', str(tmp_path) + '/', '--task_setup', 'Disjoint', '--epoch', '2', '--n_way', '3', '--k_spt', '2',
                      '--k_qry', '6', '--task_num', '4', '--update_step', '3', '--update_step_test', '4', '--update_lr', '0.05',
                      '--meta_lr', '0.01', '--hidden_dim', '32', '--batchsz', '40', '--h', '2', '--eval_tasks', '10',
                      '--train_result_report_steps', '5', '--predict_out', out])
    res = drv.main(args)
    z = np.load(out)
    off = z['task_off']
    assert len(off) == 11 and off[-1] == len(z['names']) == len(z['true']) == len(z['pred']) == z['log_probs'].shape[0] == 10 * 3 * 6
    assert z['log_probs'].shape[1] == 3 and np.array_equal(z['class_off'], np.arange(11) * 3)
    assert all(info[str(n)] == int(t) for n, t in zip(z['names'], z['true']))
    assert set(np.unique(z['pred'])) <= {3, 4, 5} and set(np.unique(z['true'])) <= {3, 4, 5}       # label values of the test split
    for t in range(10):
        cl = z['classes'][z['class_off'][t]:z['class_off'][t + 1]]
        assert np.array_equal(z['pred'][off[t]:off[t + 1]], cl[z['log_probs'][off[t]:off[t + 1]].argmax(1)])
    acc = np.mean([np.mean(z['pred'][off[t]:off[t + 1]] == z['true'][off[t]:off[t + 1]]) for t in range(10)])
    assert abs(acc - res['early_stopped_test_acc']) <= 1e-6, (acc, res)
