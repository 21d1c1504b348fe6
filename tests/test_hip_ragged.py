"""GPU (-m gpu): ragged-task mode (gm_set_ragged_classes / Meta.ragged / train.py --ragged): tasks whose classes have unequal or short row
counts.  The reference cannot score such a task, so the yardsticks are (a) the pinned balanced path, bit for bit, wherever the task is
balanced, and (b) the CPU restatement tests/ragged_ref.py, itself held to the oracle and to fp64 autograd by tests/test_ragged_restatement.py.
Floats within the north-star tolerance 1e-4 (TOL) unless a test derives its own."""
import argparse
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gmeta_oracle as orc                                                    # noqa: E402
import ragged_ref as rr                                                       # noqa: E402
from golden_util import CASES, NAN_CASES, WIDE_CASES, Fixture                 # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
f32 = np.float32
GOLD = os.path.join(ROOT, 'tests', 'golden')
SCHEDULES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)]          # (hoist_z1, sparse_bwd, cone): the five of test_hip_parity.py


def _hu():
    import hip_util
    return hip_util


def _batches(fx, store, masks):
    """Support / query batches (one set per task) of the fixture's tasks restricted to `masks`, from the reference's node lists."""
    from gmeta_amd.subgraphs import SubgraphBatch
    out = []
    for which, tag in enumerate(('spt', 'qry')):
        seeds, lists, off = [], [], [0]
        for t in range(fx.T):
            keep = masks[t][which]
            seeds.append(fx.z[tag + '_seeds'][t][keep].reshape(-1, 3))
            lists += [l for l, k in zip(fx.replay_lists(tag, t), keep) if k]
            off.append(off[-1] + int(keep.sum()))
        out.append(SubgraphBatch.from_nodes(store, np.concatenate(seeds), off, lists, fx.link))
    return out


def _labels(fx, masks):
    ys = [torch.from_numpy(fx.z['y_spt'][t][masks[t][0]].astype(np.int64)) for t in range(fx.T)]
    yq = [torch.from_numpy(fx.z['y_qry'][t][masks[t][1]].astype(np.int64)) for t in range(fx.T)]
    return ys, yq


def _meta(fx, ragged, sched=(0, 0, 0)):
    m = _hu().fixture_meta(fx)
    m.ragged = ragged
    m.hoist_z1, m.sparse_bwd, m.cone = sched
    return m


def _step(m, S, Q, ys, yq):
    accs = m(S.views(), ys, Q.views(), yq, None, None, None, None, None, None, None)
    grad = torch.cat([p.grad.reshape(-1) for p in m.net.parameters()]).clone()
    return np.asarray(accs), grad, [p.detach().clone() for p in m.net.parameters()], dict(m.last_stats)


def _teq(a, b):
    """torch.equal with NaN == NaN (the inf-feature fixtures carry NaN gradients)."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _short_class_db():
    """tests/golden/r4_shared_short_class: the Shared data set whose sampler tops a short class up (as tests/test_hip_round3.py sets it up)."""
    import gmeta_amd
    from gmeta_amd import synth
    z = np.load(os.path.join(GOLD, 'r4_shared_short_class.npz'), allow_pickle=False)
    args = argparse.Namespace(**json.loads(str(z['args'])))
    graphs = [(int(z['g%d_n' % k]), z['g%d_src' % k], z['g%d_dst' % k]) for k in range(int(z['n_graphs']))]
    tables = {'train': ([str(x) for x in z['csv_train.csv_names']], [str(x) for x in z['csv_train.csv_labels']])}
    info = {str(k): int(v) for k, v in zip(z['info_names'], z['info_labels'])}
    rng = np.random.default_rng(0)
    feats = [rng.standard_normal((n, 8)).astype(np.float32) for n, _, _ in graphs]
    store = gmeta_amd.GraphStore(graphs, feats)
    torch.manual_seed(222); np.random.seed(222); random.seed(222)
    db = gmeta_amd.Subgraphs(None, 'train', info, n_way=args.n_way, k_shot=args.k_spt, k_query=args.k_qry, batchsz=int(z['T']), args=args,
                             adjs=store, h=args.h, tables=tables, verbose=False)
    qry = json.loads(str(z['qry_json']))
    bad = [t for t in range(int(z['T'])) if any(len(sub) != args.k_qry for sub in qry[t])]
    config = synth.make_config(8, 16, args.h, 3)
    return args, graphs, feats, store, db, bad, config


# ---------------------------------------------------------------------------------------------------- 1. off is off
def test_off_is_off():
    import gmeta_amd
    args, graphs, feats, store, db, bad, config = _short_class_db()
    assert bad
    m = gmeta_amd.Meta(args, config).to('cuda')
    assert m.ragged == 0
    with pytest.raises(ValueError, match='unequal row counts'):
        m(*db.get_batch(bad[:1]), feats)


# ---------------------------------------------------------------------------------------------------- 2. balanced tasks are bit-identical
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('sched', SCHEDULES)
def test_balanced_meta_step_is_bit_identical(case, sched):
    fx = Fixture(case)
    store = _hu().make_store(fx)
    masks = rr.all_masks(fx, ragged=False)
    S, Q = _batches(fx, store, masks)
    ys, yq = _labels(fx, masks)
    a = _step(_meta(fx, 0, sched), S, Q, ys, yq)
    b = _step(_meta(fx, 1, sched), S, Q, ys, yq)
    assert np.array_equal(a[0], b[0], equal_nan=True)
    assert _teq(a[1], b[1])
    assert all(_teq(x, y) for x, y in zip(a[2], b[2]))
    assert np.array_equal(a[3]['losses_q'], b[3]['losses_q'], equal_nan=True)


@pytest.mark.parametrize('case', CASES)
def test_balanced_finetunning_and_adapt_are_bit_identical(case):
    fx = Fixture(case)
    store = _hu().make_store(fx)
    masks = rr.all_masks(fx, ragged=False)
    S, Q = _batches(fx, store, masks)
    ys, yq = _labels(fx, masks)
    m0, m1 = _meta(fx, 0), _meta(fx, 1)
    assert np.array_equal(m0.finetunning_batch(S.views(), ys, Q.views(), yq), m1.finetunning_batch(S.views(), ys, Q.views(), yq), equal_nan=True)
    a0, a1 = m0.adapt(S.views(), ys), m1.adapt(S.views(), ys)
    assert _teq(a0.fast_weights, a1.fast_weights) and _teq(a0.prototypes, a1.prototypes)


# ---------------------------------------------------------------------------------------------------- 3. ragged tasks match the restatement
def _check_accs(fx, got, masks):
    """got [T, K_test+1] from finetunning_batch against the restated fine-tuning run.  A query scoring (one row at one step) whose two largest
    restated log-probabilities are closer than 1e-4 is left out: the correct count of the step may then differ by it.  At most two per case."""
    margins = []
    res = rr.run_tasks(fx, masks, True, fx.K_test, False, margins)
    left_out = 0
    for t in range(fx.T):
        n = int(masks[t][1].sum())
        for j in range(fx.K_test + 1):
            tied = int((~(margins[t * (fx.K_test + 1) + j] >= 1e-4)).sum())
            left_out += tied
            want, have = float(res[t][1][j]) * n, float(got[t, j]) * n
            print('acc', fx.name, t, j, 'restated', want, 'kernel', have, 'tied', tied)
            assert abs(have - round(have)) < 1e-3
            assert abs(have - want) <= tied + 1e-3, (fx.name, t, j, want, have, tied)
    assert left_out <= 2, left_out


def _check_step(fx, sched, split):
    from gmeta_amd import _lib
    lib = _lib.lib()
    store = _hu().make_store(fx)
    masks = rr.all_masks(fx)
    S, Q = _batches(fx, store, masks)
    ys, yq = _labels(fx, masks)
    old = lib.gm_get_tuning(b'GM_GEMM_SPLIT_MIN_TILES')
    if split:
        lib.gm_set_tuning(b'GM_GEMM_SPLIT_MIN_TILES', 0)
    try:
        m = _meta(fx, 1, sched)
        before = [p.detach().clone() for p in m.net.parameters()]
        accs, grad, after, stats = _step(m, S, Q, ys, yq)
        ft = _meta(fx, 1, sched).finetunning_batch(S.views(), ys, Q.views(), yq) if fx.name not in NAN_CASES else None
    finally:
        lib.gm_set_tuning(b'GM_GEMM_SPLIT_MIN_TILES', old)
    if fx.name in NAN_CASES:                                 # NaN query loss, no optimiser step (as in test_hip_parity.py)
        assert np.isnan(stats['loss_q'])
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        for st in m.meta_optim.state.values():
            assert float(st['step']) == 0.0 and float(st['exp_avg'].abs().max()) == 0.0
        return
    lq, aq, g_ref, new = rr.meta_step(fx, masks)
    g_ref_flat = np.concatenate([g.reshape(-1) for g in g_ref])
    print(fx.name, sched, split, 'max |losses_q - restated|', np.abs(stats['losses_q'] - lq).max(), 'max |grad - restated|',
          np.abs(grad.cpu().numpy() - g_ref_flat).max())
    np.testing.assert_allclose(stats['losses_q'], lq, atol=TOL, rtol=0)
    np.testing.assert_allclose(grad.cpu().numpy(), g_ref_flat, atol=TOL, rtol=0)
    for a, b, g in zip(after, new, g_ref):
        ok = np.abs(g) > 1e-5           # Adam's first step is sign(g) * lr: only comparable where g is well away from 0 (as test_hip_parity.py)
        np.testing.assert_allclose(a.cpu().numpy()[ok], b[ok], atol=TOL, rtol=0)
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    if fx.name != 'g8_wide_scales':      # (tiny logits: most of its scorings tie; its accuracies are held by the predict agreement below)
        _check_accs(fx, ft, masks)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('sched', [(0, 0, 0), (1, 0, 1)])
def test_ragged_meta_step_matches_restatement(case, sched):
    _check_step(Fixture(case), sched, False)


@pytest.mark.parametrize('case', WIDE_CASES)
@pytest.mark.parametrize('sched', [(0, 0, 0), (1, 0, 1)])
def test_ragged_meta_step_matches_restatement_split_kernels(case, sched):
    _check_step(Fixture(case), sched, True)


def test_ragged_meta_step_unstaged_head_kernel():
    """The head / loss kernel with everything in global memory (what a task too large for LDS takes; forced here with GM_HEAD_STAGE=0):
    the class starts are read from global memory instead of LDS."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    old = lib.gm_get_tuning(b'GM_HEAD_STAGE')
    lib.gm_set_tuning(b'GM_HEAD_STAGE', 0)
    try:
        _check_step(Fixture('g2_shared'), (0, 0, 0), False)
    finally:
        lib.gm_set_tuning(b'GM_HEAD_STAGE', old)


# ---------------------------------------------------------------------------------------------------- 4. the sampler's own task trains
def test_topped_up_task_of_the_sampler_trains():
    import gmeta_amd
    args, graphs, feats, store, db, bad, config = _short_class_db()
    args.ragged = 1
    torch.manual_seed(5)
    m = gmeta_amd.Meta(args, config).to('cuda')
    theta0 = [p.detach().cpu().numpy().copy() for p in m.net.parameters()]
    t = bad[0]
    b = db.get_batch([t])
    accs = np.asarray(m(*b, feats))
    assert accs.shape == (args.update_step + 1,) and np.isfinite(accs).all()
    assert any(not np.array_equal(a, p.detach().cpu().numpy()) for a, p in zip(theta0, m.net.parameters()))
    # the restatement of the same task: the batch's own node lists, the oracle's inner loop with the ragged losses
    og = [orc.Graph(n, s, d) for n, s, d in graphs]
    seeds_s, seeds_q, ys, yq = db._task_arrays(t)
    assert len(yq) == len(np.unique(ys)) * args.k_qry + 1                    # topped up: one row more than a balanced query set
    sb = orc.extract_batch(og, seeds_s, args.h, args.sample_nodes, 222, False, replay_nodes=[np.asarray(l) for l in b[6][0]])
    qb = orc.extract_batch(og, seeds_q, args.h, args.sample_nodes, 222, False, replay_nodes=[np.asarray(l) for l in b[7][0]])
    with rr.patched(ys):
        lq, aq, mg = orc.task_inner_loop(sb, qb, sb.features(feats), qb.features(feats), ys, yq, theta0, config, args.k_spt, args.update_lr,
                                         args.update_step, True)
    grad = torch.cat([p.grad.reshape(-1) for p in m.net.parameters()]).cpu().numpy()
    np.testing.assert_allclose(m.last_stats['losses_q'], lq, atol=TOL, rtol=0)
    np.testing.assert_allclose(grad, np.concatenate([g.reshape(-1) for g in mg]), atol=TOL, rtol=0)


# ---------------------------------------------------------------------------------------------------- 5. adapt and predict on ragged support
@pytest.mark.parametrize('case', CASES)
def test_adapt_and_predict_on_ragged_support(case):
    fx = Fixture(case)
    store = _hu().make_store(fx)
    masks = rr.all_masks(fx)
    S, Q = _batches(fx, store, masks)
    ys, yq = _labels(fx, masks)
    m = _meta(fx, 1)
    if case not in NAN_CASES:
        ad = m.adapt(S.views(), ys)
        fw_h, pt_h = ad.fast_weights.cpu().numpy(), ad.prototypes.cpu().numpy()
        for t in range(fx.T):
            sb, _ = rr.oracle_batches(fx, t, *masks[t])
            fw, protos = rr.support_chain(fx, sb, ys[t].numpy(), fx.K_test)
            np.testing.assert_allclose(fw_h[t], np.concatenate([w.reshape(-1) for w in fw]), atol=TOL, rtol=0)
            n = len(ad.classes[t])
            np.testing.assert_allclose(pt_h[t, :n], protos, atol=TOL, rtol=0)
            assert not pt_h[t, n:].any()
    # predict agrees with finetunning_batch exactly, as tests/test_hip_predict.py holds it for balanced sets
    ft = m.finetunning_batch(S.views(), ys, Q.views(), yq)
    for j in range(fx.K_test + 1):
        pr = m.predict(S.views(), ys, Q.views(), K=j)
        for t in range(fx.T):
            y = yq[t].numpy()
            got = f32(np.count_nonzero(pr.labels[t] == y)) / f32(len(y))
            assert got == f32(ft[t, j]), (case, j, t, got, ft[t, j])


# ---------------------------------------------------------------------------------------------------- 6. the kernels directly
def _ref64(z, rows, protos=None):
    """fp64 statement: rows = per class the scored rows; support role when protos is None.  loss, acc, protos, dlogits, dprotos."""
    z = z.astype(np.float64)
    mode0 = protos is None
    if mode0:
        protos = np.stack([z[r].mean(0) for r in rows])
    protos = protos.astype(np.float64)
    idx = np.concatenate(rows); tgt = np.concatenate([np.full(len(r), c) for c, r in enumerate(rows)]).astype(np.int64)
    q = z[idx]; Q = len(idx)
    a = -((q[:, None, :] - protos[None]) ** 2).sum(2)
    mx = a.max(1, keepdims=True)
    logp = a - mx - np.log(np.exp(a - mx).sum(1, keepdims=True))
    loss = -logp[np.arange(Q), tgt].mean(); acc = (logp.argmax(1) == tgt).mean()
    G = np.exp(logp); G[np.arange(Q), tgt] -= 1; G /= Q
    diff = q[:, None, :] - protos[None]
    dl = np.zeros_like(z)
    np.add.at(dl, idx, (G[:, :, None] * (-2 * diff)).sum(1))
    dp = (G[:, :, None] * (2 * diff)).sum(0)
    if mode0:
        for c, r in enumerate(rows):
            dl[r] += dp[c] / len(r)
    return loss, acc, protos, dl, dp


def _kernel_sets(rng):
    """Per set the (class label, row count) pairs: 1..24 classes of 1..40 rows, a set with a single-row class, and one whose rows x classes
    exceed PROTO_A_MAX = 8192 (no A table) while its rows stay within the 8192 limit."""
    sets = [[(int(l), int(rng.integers(1, 41))) for l in rng.choice(1000, size=nc, replace=False)] for nc in (1, 2, 3, 7, 12, 24)]
    sets.append([(5, 1), (9, 17), (2, 6)])
    sets.append([(int(l), int(rng.integers(20, 81))) for l in rng.choice(1000, size=20, replace=False)])      # ~1000 rows x 20 classes
    assert sum(n for _, n in sets[-1]) * 20 > 8192
    return sets


def test_proto_loss_kernels_on_ragged_sets_against_fp64():
    """loss, accuracy, prototypes, dlogits, dprotos of gm_proto_loss_spt / _qry on random logits.  The tolerance is derived, not chosen: per quantity,
    the fp32 restatement's own distance to fp64 on the same inputs -- its largest over the sets of the batch; a single small set's is a sample of a
    handful of roundings and can be zero by luck -- times four.  That bound holds the pass in which every row counts (n_support = 40).  A second
    pass with n_support = 3 checks WHICH rows count -- the first three of a class next to classes that have fewer -- at the 1e-5 / 1e-6 of
    tests/test_hip_parity.py::test_proto_losses_match_oracle: most of its support sets are balanced and run the balanced code, which the golden
    fixtures pin bit for bit and which is not this test's subject."""
    import gmeta_amd
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    lib = _lib.lib()
    rng = np.random.default_rng(11)
    D = 6
    sets = _kernel_sets(rng)
    y, off = [], [0]
    for s in sets:
        lab = np.concatenate([np.full(n, l) for l, n in s])
        y.append(lab[rng.permutation(len(lab))])
        off.append(off[-1] + len(lab))
    y = np.concatenate(y).astype(np.int32)
    n_sub = off[-1]
    n = 64
    src, dst = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    store = gmeta_amd.GraphStore([(n, src.astype(np.int64), dst.astype(np.int64))], [rng.standard_normal((n, 8)).astype(np.float32)])
    nodes = rng.integers(0, n, n_sub)
    B = SubgraphBatch.from_nodes(store, np.array([(0, int(v), -1) for v in nodes], np.int32), off, [np.array([v], np.int32) for v in nodes], False)
    T, cmax = len(sets), max(len(s) for s in sets)
    z = rng.standard_normal((n_sub, D)).astype(f32)
    zq = rng.standard_normal((n_sub, D)).astype(f32)
    dz, dzq = torch.from_numpy(z).cuda(), torch.from_numpy(zq).cuda()

    def close(name, got, r32, r64):
        """Records, per quantity, the kernel's and the fp32 restatement's largest distance to fp64 over the sets of the batch."""
        w = worst.setdefault(name, [0.0, 0.0])
        w[0] = max(w[0], float(np.abs(np.asarray(got, np.float64) - r64).max()))
        w[1] = max(w[1], float(np.abs(np.asarray(r32, np.float64) - r64).max()))

    lib.gm_set_ragged_classes(1)
    try:
        for n_support in (40, 3):
            worst = {}
            loss, acc = torch.empty(T, device='cuda'), torch.empty(T, device='cuda')
            protos = torch.zeros(T, cmax, D, device='cuda'); dl = torch.empty(n_sub, D, device='cuda')
            _lib.check(lib.gm_proto_loss_spt(B.handle, _lib.ptr(dz), D, _lib.ptr(y), n_support, _lib.ptr(loss), _lib.ptr(acc), _lib.ptr(protos), _lib.ptr(dl),
                                             _lib.stream_ptr()), 'gm_proto_loss_spt')
            lossq, accq = torch.empty(T, device='cuda'), torch.empty(T, device='cuda')
            dq = torch.empty(n_sub, D, device='cuda'); dp = torch.zeros(T, cmax, D, device='cuda')
            _lib.check(lib.gm_proto_loss_qry(B.handle, _lib.ptr(dzq), D, _lib.ptr(y), _lib.ptr(protos), cmax, _lib.ptr(lossq), _lib.ptr(accq), _lib.ptr(dq),
                                             _lib.ptr(dp), _lib.stream_ptr()), 'gm_proto_loss_qry')
            torch.cuda.synchronize()
            for t in range(T):
                a, b = off[t], off[t + 1]
                yt = y[a:b]; classes = np.unique(yt); nc = len(classes)
                spt, qry, _ = rr.make(yt)
                l32, a32, p32, g32 = spt(z[a:b], yt, n_support)
                l64, a64, p64, g64, _ = _ref64(z[a:b], rr.class_rows(yt, classes, n_support))
                pk = protos[t, :nc].cpu().numpy()
                close('spt loss', loss[t].item(), l32, l64); close('spt acc', acc[t].item(), a32, a64); close('protos', pk, p32, p64)
                close('spt dlogits', dl[a:b].cpu().numpy(), g32, g64)
                # query role: all rows, against the kernel's own prototypes (the same fp32 input for the three of them)
                l32, a32, q32, d32 = qry(zq[a:b], yt, pk, need_grad=True)
                l64, a64, _, q64, d64 = _ref64(zq[a:b], rr.class_rows(yt, classes), pk)
                close('qry loss', lossq[t].item(), l32, l64); close('qry acc', accq[t].item(), a32, a64)
                close('qry dlogits', dq[a:b].cpu().numpy(), q32, q64); close('dprotos', dp[t, :nc].cpu().numpy(), d32, d64)
                assert not protos[t, nc:].any() and not dp[t, nc:].any()          # nothing written past the set's classes
            for k, (err, ref) in worst.items():
                print('n_support', n_support, k, 'kernel vs fp64 %.3e' % err, 'fp32 restatement vs fp64 %.3e' % ref)
            if n_support == 40:
                assert all(err <= 4 * ref for err, ref in worst.values()), worst
            else:
                assert all(err <= (1e-6 if k in ('spt acc', 'qry acc', 'protos') else 1e-5) for k, (err, ref) in worst.items()), worst
    finally:
        lib.gm_set_ragged_classes(0)


# ---------------------------------------------------------------------------------------------------- 7. errors
def test_ragged_errors():
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    lib = _lib.lib()
    fx = Fixture('g2_shared')
    store = _hu().make_store(fx)
    masks = rr.all_masks(fx)
    S, Q = _batches(fx, store, masks)
    ys, yq = _labels(fx, masks)
    m = _meta(fx, 1)
    outside = int(max(int(y.max()) for y in ys)) + 7
    bad = [y.clone() for y in yq]; bad[1][0] = outside
    with pytest.raises(ValueError, match=r'task 1 has a query row of label %d' % outside):
        m.finetunning_batch(S.views(), ys, Q.views(), bad)
    with pytest.raises(ValueError, match=r'task 1 has a query row of label %d' % outside):
        m(S.views(), ys, Q.views(), bad, None, None, None, None, None, None, None)
    assert lib.gm_get_ragged_classes() == 0                                   # put back after a failed call too
    # a task without query rows
    empty = [(ks, kq.copy()) for ks, kq in masks]
    empty[fx.T - 1][1][:] = False
    S2, Q2 = _batches(fx, store, empty)
    ys2, yq2 = _labels(fx, empty)
    with pytest.raises(ValueError, match=r'task %d has no query rows' % (fx.T - 1)):
        m.finetunning_batch(S2.views(), ys2, Q2.views(), yq2)
    # more than 8192 scored rows in a set
    n_sub = 8200
    nodes = np.arange(n_sub) % fx.edges[0][0]
    B = SubgraphBatch.from_nodes(store, np.array([(0, int(v), -1) for v in nodes], np.int32), [0, n_sub], [np.array([v], np.int32) for v in nodes], False)
    y = (np.arange(n_sub) % 3 == 0).astype(np.int32)                          # two classes of unequal size
    z = torch.zeros(n_sub, 2, device='cuda')
    loss, acc = torch.empty(1, device='cuda'), torch.empty(1, device='cuda')
    lib.gm_set_ragged_classes(1)
    try:
        rc = lib.gm_proto_loss_spt(B.handle, _lib.ptr(z), 2, _lib.ptr(y), n_sub, _lib.ptr(loss), _lib.ptr(acc), None, None, _lib.stream_ptr())
        assert rc == -4 and b'8200 rows' in lib.gm_last_error(), (rc, lib.gm_last_error())
    finally:
        lib.gm_set_ragged_classes(0)


# ---------------------------------------------------------------------------------------------------- 8. tasks stay independent
def test_ragged_tasks_stay_independent():
    fx = Fixture('g2_shared')
    store = _hu().make_store(fx)
    masks = rr.all_masks(fx)
    S, Q = _batches(fx, store, masks)
    ys, yq = _labels(fx, masks)
    m = _meta(fx, 1)
    together = m.finetunning_batch(S.views(), ys, Q.views(), yq)
    assert together.shape == (fx.T, fx.K_test + 1)
    from gmeta_amd.subgraphs import SubgraphBatch
    for t in range(fx.T):
        one = []
        for which, tag in enumerate(('spt', 'qry')):
            keep = masks[t][which]
            lists = [l for l, k in zip(fx.replay_lists(tag, t), keep) if k]
            one.append(SubgraphBatch.from_nodes(store, fx.z[tag + '_seeds'][t][keep].reshape(-1, 3), [0, int(keep.sum())], lists, fx.link))
        alone = m.finetunning_batch([one[0]], ys[t:t + 1], [one[1]], yq[t:t + 1])
        assert np.array_equal(alone[0], together[t]), (t, alone[0], together[t])


# ---------------------------------------------------------------------------------------------------- train.py --ragged
def _shared_datadir(tmp, seed=0):
    """Six small graphs with one label set {0, 1, 2}; Shared splits are by graph (train: 0-2, val: 3-4, test: 5).  In training graph 1 class 2 has
    five members: k_spt = 3 <= 5 < k_spt + k_qry = 7, the sampler's top-up branch."""
    from gmeta_amd import datadir, synth
    rng = np.random.default_rng(seed)
    graphs, feats, info, rows = [], [], {}, {'train': ([], []), 'val': ([], []), 'test': ([], [])}
    proto = rng.standard_normal((3, 8)).astype(np.float32) * 2
    for g in range(6):
        n = 90
        e = synth.pa_edges(n, 3, rng)
        graphs.append((n, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])))
        lab = rng.integers(0, 2, size=n)
        lab[rng.permutation(n)[:5 if g == 1 else 30]] = 2
        feats.append((proto[lab] + 0.3 * rng.standard_normal((n, 8))).astype(np.float32))
        split = 'train' if g < 3 else ('val' if g < 5 else 'test')
        for v in range(n):
            nm = '%d_%d' % (g, v)
            info[nm] = int(lab[v]); rows[split][0].append(nm); rows[split][1].append(str(int(lab[v])))
    datadir.write_datadir(str(tmp), graphs, feats, info, rows)


def test_train_driver_runs_a_short_class_dataset_with_ragged(tmp_path, monkeypatch):
    import gmeta_amd
    import train as drv
    _shared_datadir(tmp_path)
    made = []
    real = gmeta_amd.Subgraphs

    class Recording(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append((a[1], self))

    monkeypatch.setattr(gmeta_amd, 'Subgraphs', Recording)
    argv = ['--data_dir', str(tmp_path) + '/', '--task_setup', 'Shared', '--epoch', '1', '--n_way', '3', '--k_spt', '3', '--k_qry', '4', '--task_num', '4',
            '--update_step', '2', '--update_step_test', '2', '--update_lr', '0.05', '--meta_lr', '0.01', '--hidden_dim', '16', '--batchsz', '24', '--h', '1',
            '--eval_tasks', '6', '--train_result_report_steps', '2']
    with pytest.raises(ValueError, match='unequal row counts'):
        drv.main(drv.parse(argv))
    train_db = [db for mode, db in made if mode == 'train'][0]
    assert any(len(sub) == 5 for task in train_db.query_x_batch for sub in task)          # a sampled task really was topped up (k_qry + 1 entries)
    del made[:]
    res = drv.main(drv.parse(argv + ['--ragged', '1']))
    train_db = [db for mode, db in made if mode == 'train'][0]
    assert any(len(sub) == 5 for task in train_db.query_x_batch for sub in task)
    assert np.isfinite([res['test_acc'], res['early_stopped_test_acc'], res['val_best']]).all()
