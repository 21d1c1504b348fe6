"""GPU (-m gpu): the opt-in mean-pooled readout (include/gmeta_hip.h, gm_set_readout; config entry ('Readout', ['mean'])) from the two pooling kernels
to train.py, against the CPU restatement tests/readout_ref.py (held to fp64 autograd by tests/test_readout_restatement.py) on the ten golden fixtures
with a pair model's head cut to Wl[:, :H].

Tolerances: those of tests/test_hip_hop_labels.py (TOL = 1e-4, assert_step_close's forms).  Accuracies: the rule of tests/test_hip_ragged.py::_check_accs
with a cap of ZERO rows left out, on the six fixtures of ACC_CASES (the restatement has no query scoring whose two largest log-probabilities are closer
than 1e-4 there: tests/test_readout_restatement.py); g1_h3 and g8_wide_scales collapse under mean pooling (24 of 72 and 100 of 150 scorings tied) and are
checked on losses and gradients."""
import argparse
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import gmeta_oracle as orc                                                    # noqa: E402
import hop_label_ref as hl                                                    # noqa: E402
import ragged_ref as rr                                                       # noqa: E402
import readout_ref as ro                                                      # noqa: E402
from golden_util import CASES, NAN_CASES, WIDE_CASES, Fixture                 # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
f32 = np.float32
ACC_CASES = ('g0_disjoint_h1', 'g1_sampled_h2', 'g2_shared', 'g3_linkpred', 'g5_in_gt_out', 'g7_wide_h2')
SCHEDULES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)]          # (hoist_z1, sparse_bwd, cone): the five of tests/test_hip_parity.py
FORCE = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
MEAN = ('Readout', ['mean'])


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


def _hu():
    import hip_util
    return hip_util


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def close(got, want, what, rtol=1e-4):
    np.testing.assert_allclose(got, want, atol=TOL * max(1.0, float(np.abs(want).max())), rtol=rtol, err_msg=what)


# ---------------------------------------------------------------------------------------------------- 1. the kernels through Classifier
SIZES = (1, 2, 63, 64, 65, 1500)      # rows per subgraph; a chunk covers 64 rows: one row, one chunk less / exactly / plus one row, 24 chunks
NG = 1600


def hub_graph():
    """Node 0 has the 1,499 in-neighbours 1..1499; node NG - 1 is isolated; random edges (self loops and parallel edges among them) elsewhere."""
    rng = np.random.default_rng(21)
    e = [(k, 0) for k in range(1, 1500)] + [(int(u), int(v)) for u, v in rng.integers(1, NG - 1, size=(4 * NG, 2))]
    e = np.array(e, np.int64)
    return NG, e[:, 0], e[:, 1]


def hub_batch(store, link):
    """Two sets of three subgraphs with the node lists given: sizes 1 (the isolated node, alone), 2, 63 | 64, 65, 1500 (the hub and all of its
    in-neighbours: what a 1-hop extraction with sample_nodes above 1,500 returns).  Pairs: the second centre is another node of the list -- the same
    node (i == j) in the one-row subgraph and in the hub's."""
    from gmeta_amd.subgraphs import SubgraphBatch
    rng = np.random.default_rng(22)
    lists, seeds = [], []
    for k, n in enumerate(SIZES):
        if n == 1:
            nodes = np.array([NG - 1])
        elif n == 1500:
            nodes = np.arange(1500)
        else:
            nodes = np.sort(rng.choice(np.arange(1, NG - 1), n, replace=False))
        i = int(nodes[0])
        j = -1 if not link else (i if n in (1, 1500) else int(nodes[-1]))
        lists.append(nodes.astype(np.int32)); seeds.append((0, i, j))
    seeds = np.array(seeds, np.int32)
    B = SubgraphBatch.from_nodes(store, seeds, [0, 3, 6], lists, link)
    assert [int(v) for v in np.diff(B.sub_off)] == list(SIZES)
    return B, orc.Batch([orc.Graph(*hub_graph())], seeds, lists)


def _theta(rng, dims, n_out):
    th = []
    for fi, fo in zip(dims[:-1], dims[1:]):
        th += [(rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(f32), (rng.uniform(0.15, 0.4, fo) * rng.choice([-1.0, 1.0], fo)).astype(f32)]
    return th + [(rng.standard_normal((n_out, dims[-1])) / np.sqrt(dims[-1])).astype(f32), (rng.uniform(0.15, 0.4, n_out) * rng.choice([-1.0, 1.0], n_out)).astype(f32)]


@pytest.mark.parametrize('dims,link,force', [((8, 10, 10), False, False), ((8, 16, 16), False, False), ((64, 128, 128), False, True), ((16, 32, 8), False, False),
                                             ((8, 16, 16), True, False), ((64, 128, 128), True, True), ((8, 258), False, False), ((8, 1028), False, False)])
def test_pooling_kernels_through_classifier_forward_and_backward(dims, link, force):
    """Hd = 10 takes the scalar path, 16 and 128 the 16-byte one (128 with the split GEMM / weight-gradient kernels forced); 16 -> 32 -> 8 ends in a
    multiply-first layer, whose aggregate is what writes H_L; the pair batch holds i == j twice; Hd = 258 / 1028 are more column vectors than a workgroup
    has threads (scalar / 16-byte path): the kernels' loop over column passes."""
    import gmeta_amd
    n, src, dst = hub_graph()
    rng = np.random.default_rng(sum(dims))
    feats = [(0.3 * rng.standard_normal((n, dims[0]))).astype(f32)]
    cfg = [('GraphConv', [a, b]) for a, b in zip(dims[:-1], dims[1:])] + [('Linear', [dims[-1], 3]), MEAN] + ([('LinkPred', [True])] if link else [])
    th = _theta(rng, dims, 3)
    with tuning(**(FORCE if force else {})):
        store = gmeta_amd.GraphStore([(n, src, dst)], feats)
        B, ob = hub_batch(store, link)
        net = gmeta_amd.Classifier(cfg).to('cuda')
        assert net.readout == 'mean' and tuple(net.vars[-2].shape) == (3, dims[-1])
        with torch.no_grad():
            for p, v in zip(net.parameters(), th):
                p.copy_(torch.from_numpy(v))
        R = rng.standard_normal((B.subs, 3)).astype(f32)
        got = []
        for _ in range(2):
            net.zero_grad()
            logits, _ = net(B, None, None)
            (logits * torch.from_numpy(R).cuda()).sum().backward()
            got.append((logits.detach().cpu().numpy(), torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu().numpy()))
        # to_fetch is accepted and not used
        other, _ = net(B, np.zeros((B.subs, 2) if link else B.subs, np.int64), None)
    from gmeta_amd import _lib
    assert _lib.lib().gm_get_readout() == 0
    fwd, bwd = ro.make()
    want_l, cache = fwd(ob, ob.features(feats), th, cfg)
    want_g = np.concatenate([g.reshape(-1) for g in bwd(ob, th, cfg, cache, R)])
    print(dims, link, 'max |logits - restated|', np.abs(got[0][0] - want_l).max(), 'max |grad - restated|', np.abs(got[0][1] - want_g).max(), 'at', np.abs(want_g).max())
    close(got[0][0], want_l, 'logits')
    close(got[0][1], want_g, 'gradients')
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))      # one fixed summation order
    assert np.array_equal(_bits(other.detach().cpu().numpy()), _bits(got[0][0]))


# ---------------------------------------------------------------------------------------------------- 2. meta-step and fine-tuning on the fixtures
class Pooled:
    """A golden fixture as the pooled model sees it (config with the Readout entry, a pair head cut to Wl[:, :H]), its batches from the reference's
    node lists, and the restated training step / fine-tuning run, computed once per fixture."""

    def __init__(self, case):
        self.fx = fx = Fixture(case)
        fx.vars0, fx.config = ro.mean_vars(fx.vars0, fx.config), ro.mean_config(fx.config)      # (hip_util.fixture_meta and ragged_ref read these two)
        self.nan = case in NAN_CASES
        self._ref = {}

    def batches(self):
        hu = _hu()
        self.store = hu.make_store(self.fx)
        return hu.fixture_batches(self.fx, self.store, True)

    def labels(self):
        fx = self.fx
        return ([torch.from_numpy(y.astype(np.int64)) for y in fx.z['y_spt']], [torch.from_numpy(y.astype(np.int64)) for y in fx.z['y_qry']])

    def meta(self, sched=(0, 0, 0), **flags):
        m = _hu().fixture_meta(self.fx)
        assert m.net.readout == 'mean'
        m.hoist_z1, m.sparse_bwd, m.cone = sched
        for k, v in flags.items():
            setattr(m, k, v)
        return m

    def step(self, S, Q, need_grad, sched=(0, 0, 0)):
        """gm_meta_step's whole `out` (host copy), P, K."""
        ys, yq = self.labels()
        K = self.fx.K if need_grad else self.fx.K_test
        out, P, _ = self.meta(sched)._run(S.views(), ys, Q.views(), yq, K, need_grad)
        return out.cpu().numpy().copy(), P, K

    def reference(self, need_grad):
        """Per task (losses_q, accs_q, meta-gradient list) of the restatement, and the margins of every query scoring."""
        if need_grad not in self._ref:
            margins = []
            fx = self.fx
            res = ro.run_tasks(fx, fx.K if need_grad else fx.K_test, need_grad, margins, theta=fx.vars0)
            self._ref[need_grad] = (res, margins)
        return self._ref[need_grad]


_POOLED = {}


def pooled(case):
    if case not in _POOLED:
        _POOLED[case] = Pooled(case)
    return _POOLED[case]


def check_out(pw, out, P, K, need_grad, what):
    """A gm_meta_step `out` against the restatement: losses and the meta-gradient in assert_step_close's forms; accuracies by the correct counts of
    every task and step, exactly (no scoring is left out on ACC_CASES), on the fixtures that have them."""
    fx = pw.fx
    T, K1 = fx.T, K + 1
    assert out[-1] == 0, what
    res, margins = pw.reference(need_grad)
    lq = sum(r[0].astype(np.float64) for r in res) / T
    got_l = out[P:P + K1] / T
    if pw.nan:                                                                   # inf features: a NaN query loss on both sides
        assert np.isnan(got_l[-1]) and np.isnan(lq[-1]), what
        return
    print(what, 'max |losses_q - restated|', np.abs(got_l - lq).max())
    np.testing.assert_allclose(got_l, lq, atol=TOL, rtol=1e-4, err_msg=what)
    if need_grad:
        gsum = [np.zeros_like(g) for g in res[0][2]]
        for r in res:
            gsum = [a + b for a, b in zip(gsum, r[2])]
        grad = np.concatenate([(g / f32(T)).astype(f32).reshape(-1) for g in gsum])
        print(what, 'max |grad - restated|', np.abs(out[:P] / T - grad).max(), 'at', np.abs(grad).max())
        np.testing.assert_allclose(out[:P] / T, grad, atol=TOL * max(1.0, float(np.abs(grad).max())), rtol=1e-3, err_msg=what)
    if fx.name in ACC_CASES:
        per_task = out[P + 2 * K1 + 1:P + 2 * K1 + 1 + T * K1].reshape(T, K1)
        for t in range(T):
            n = len(fx.z['y_qry'][t])
            for j in range(K1):
                tied = int((~(margins[t * K1 + j] >= 1e-4)).sum())
                assert tied == 0, (what, t, j, tied)                              # the cap: zero rows left out
                want, have = float(res[t][1][j]) * n, float(per_task[t, j]) * n
                assert abs(have - round(have)) < 1e-3 and abs(have - want) <= tied + 1e-3, (what, t, j, want, have)


@pytest.mark.parametrize('case', CASES)
def test_meta_step_and_finetunning_match_the_restatement_on_every_schedule(case):
    """Training step and fine-tuning, the five schedule flag combinations, the fused aggregate + GEMM on and off (the hidden-128 fixtures with the
    split kernels forced, as tests/test_hip_ragged.py forces them); under the mean readout sparse_bwd and cone are ignored: those runs are the dense
    run (cone + hoist_z1: the hoist_z1 run) bit for bit."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    pw = pooled(case)
    with tuning(**(FORCE if case in WIDE_CASES else {})):
        S, Q = pw.batches()
        for need_grad in (True, False):
            for fuse in (1, 0):
                outs = {}
                for sched in SCHEDULES:
                    lib.gm_set_fuse_agg(fuse)
                    try:
                        out, P, K = pw.step(S, Q, need_grad, sched)
                    finally:
                        lib.gm_set_fuse_agg(-1)
                    outs[sched] = out
                    check_out(pw, out, P, K, need_grad, '%s, sched=%s, fuse_agg=%d, need_grad=%s' % (case, sched, fuse, need_grad))
                for flagged, plain in (((0, 1, 0), (0, 0, 0)), ((0, 0, 1), (0, 0, 0)), ((1, 0, 1), (1, 0, 0))):
                    assert np.array_equal(_bits(outs[flagged]), _bits(outs[plain])), (case, flagged, fuse, need_grad)
    assert lib.gm_get_readout() == 0


@pytest.mark.parametrize('case', ['g2_shared', 'g3_linkpred', 'g7_wide_h2', 'g6_nan_skip'])
def test_three_steps_twice_are_bitwise_identical(case):
    """Two runs of three meta-steps (Adam included) from the same state; the NaN fixture: a NaN query loss and no optimiser step, as tests/test_hip_parity.py
    checks it on the centre path."""
    pw = pooled(case)
    runs = []
    with tuning(**(FORCE if case in WIDE_CASES else {})):
        S, Q = pw.batches()
        ys, yq = pw.labels()
        for _ in range(2):
            m = pw.meta()
            before = [p.detach().clone() for p in m.net.parameters()]
            accs = [np.asarray(m(S.views(), ys, Q.views(), yq, None, None, None, None, None, None, None)) for _ in range(3)]
            after = [p.detach().clone() for p in m.net.parameters()]
            runs.append((np.concatenate(accs), torch.cat([p.reshape(-1) for p in after]).cpu().numpy(), m.last_stats['losses_q']))
            if pw.nan:
                assert np.isnan(m.last_stats['loss_q'])
                assert all(torch.equal(a, b) for a, b in zip(before, after))
                for st in m.meta_optim.state.values():
                    assert float(st['step']) == 0.0 and float(st['exp_avg'].abs().max()) == 0.0
            else:
                assert any(not torch.equal(a, b) for a, b in zip(before, after))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(_bits(np.asarray(a, f32)), _bits(np.asarray(b, f32)))


# ---------------------------------------------------------------------------------------------------- 3. adapt / predict
@pytest.mark.parametrize('case', ACC_CASES)
def test_adapt_and_predict_agree_with_finetunning(case):
    pw = pooled(case)
    fx = pw.fx
    with tuning(**(FORCE if case in WIDE_CASES else {})):
        S, Q = pw.batches()
        ys, yq = pw.labels()
        m = pw.meta()
        fb = m.finetunning_batch(S.views(), ys, Q.views(), yq)
        for j in range(fx.K_test + 1):
            pr = m.adapt(S.views(), ys, K=j).predict(Q.views())
            for t in range(fx.T):
                y = yq[t].numpy()
                assert f32(np.count_nonzero(pr.labels[t] == y)) / f32(len(y)) == f32(fb[t, j]), (case, j, t)
        pr2 = m.predict(S.views(), ys, Q.views())
        assert all(np.array_equal(a, b) for a, b in zip(pr.labels, pr2.labels))
    res, _ = pw.reference(False)
    for t in range(fx.T):                                                        # ... and those accuracies are the restated ones
        n = len(fx.z['y_qry'][t])
        assert np.abs(fb[t] * n - res[t][1].astype(np.float64) * n).max() < 1e-3, (case, t)


# ---------------------------------------------------------------------------------------------------- 4. two-piece mode requested
def test_two_piece_mode_is_ignored_under_the_mean_readout():
    """gm_set_split_pieces(2) with the two-piece threshold at zero: the pooled step is the three-piece step bit for bit, violation word 0 -- and the knob
    does engage on the centre-readout twin of the same fixture (its result differs), so the guard is what kept the pooled step."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    pw = pooled('g7_wide_h2')
    centre = Fixture('g7_wide_h2')
    ys, yq = pw.labels()

    def centre_step(S, Q):
        out, _, _ = _hu().fixture_meta(centre)._run(S.views(), ys, Q.views(), yq, centre.K, True)
        return out.cpu().numpy().copy()
    with tuning(GM_SPLIT16_MIN_ROWS=0, **FORCE):
        S, Q = pw.batches()
        three_m, three_c = pw.step(S, Q, True)[0], centre_step(S, Q)
        lib.gm_set_split_pieces(2)
        try:
            assert lib.gm_get_split_pieces() == 2
            two_m, two_c = pw.step(S, Q, True)[0], centre_step(S, Q)
        finally:
            lib.gm_set_split_pieces(-1)
    assert np.array_equal(_bits(two_m), _bits(three_m)) and two_m[-1] == 0
    assert not np.array_equal(_bits(two_c), _bits(three_c))


# ---------------------------------------------------------------------------------------------------- 5. composition
@pytest.mark.parametrize('case', ['g2_shared', 'g3_linkpred'])
def test_ragged_tasks_under_the_mean_readout(case):
    """Ragged-task mode lives in the class tables: tests/ragged_ref.py's losses and tests/readout_ref.py's model patched into the oracle together."""
    from test_hip_ragged import _batches, _labels
    pw = pooled(case)
    fx = pw.fx
    masks = rr.all_masks(fx)
    store = _hu().make_store(fx)
    S, Q = _batches(fx, store, masks)
    ys, yq = _labels(fx, masks)
    m = pw.meta(ragged=1)
    out, P, _ = m._run(S.views(), ys, Q.views(), yq, fx.K, True)
    out = out.cpu().numpy()
    with ro.patched():
        lq, aq, g_ref, _ = rr.meta_step(fx, masks)
    grad = np.concatenate([g.reshape(-1) for g in g_ref])
    K1 = fx.K + 1
    print(case, 'max |losses_q - restated|', np.abs(out[P:P + K1] / fx.T - lq).max(), 'max |grad - restated|', np.abs(out[:P] / fx.T - grad).max())
    assert out[-1] == 0
    np.testing.assert_allclose(out[P:P + K1] / fx.T, lq, atol=TOL, rtol=1e-4)
    np.testing.assert_allclose(out[:P] / fx.T, grad, atol=TOL * max(1.0, float(np.abs(grad).max())), rtol=1e-3)


def test_symmetric_pairs_with_hop_labels_under_the_mean_readout():
    """The SEAL configuration: link_hops='symmetric' + hop_labels=3 + the mean readout, against tests/hop_label_ref.py's inner loop on the labelled rows
    with the pooled model patched in."""
    import test_hip_hop_labels as thl
    w = thl.world('link_sym')
    cfg = ro.mean_config(w.config)
    th = ro.mean_vars(w.theta, w.config)
    spt, qry = w.ref_batches()
    with tuning(**FORCE):
        S, Q = w.batches(w.store())
        assert S.hop_labels_cap == thl.D and S.centres == 2
        for need_grad in (True, False):
            with ro.patched():
                accs, grad, lq = hl.meta_step(w.feats, spt, qry, w.ys, w.yq, th, cfg, thl.K_SPT, thl.LR, thl.K, thl.D, need_grad)
            grad = np.concatenate([x.reshape(-1) for x in grad]) if need_grad else None
            for sched in ({}, dict(hoist_z1=1), dict(cone=1)):
                out, P = w.step(S, Q, need_grad, th, cfg, **sched)
                thl.assert_step_close(out, P, np.asarray(accs), grad, np.asarray(lq), 'seal, %s, need_grad=%s' % (sched, need_grad))


def test_unit_edge_weights_give_the_unweighted_floats_under_the_mean_readout():
    import gmeta_amd
    import test_hip_hop_labels as thl
    w = thl.world('node')
    cfg = ro.mean_config(w.config_for(w.F0))
    th = [w.theta[0][:w.F0]] + w.theta[1:]
    with tuning(**FORCE):
        plain = gmeta_amd.GraphStore([(w.n, w.src, w.dst)], w.feats)
        unit = gmeta_amd.GraphStore([(w.n, w.src, w.dst)], w.feats, edge_weights=[np.ones(len(w.src), f32)])
        outs = []
        for store in (plain, unit):
            S, Q = w.batches(store, 0)
            outs.append([w.step(S, Q, need_grad, th, cfg)[0] for need_grad in (True, False)])
        assert Q.weighted and outs[1][0][-1] == 0
    for a, b in zip(*outs):
        assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- 6. mode hygiene
def test_a_centre_step_after_a_mean_call_and_the_switch_after_an_exception():
    from gmeta_amd import _lib
    lib = _lib.lib()
    pw = pooled('g3_linkpred')
    centre = Fixture('g3_linkpred')
    ys, yq = pw.labels()
    S, Q = pw.batches()

    def centre_step(into):
        out, _, _ = _hu().fixture_meta(centre)._run(S.views(), ys, Q.views(), yq, centre.K, True)
        torch.cuda.synchronize()
        into.append((out.cpu().numpy().copy(), int(lib.gm_get_readout())))
    fresh = []
    th = threading.Thread(target=centre_step, args=(fresh,))                     # a thread that never switched
    th.start(); th.join()
    assert lib.gm_get_readout() == 0
    mean_out = pw.step(S, Q, True)[0]
    assert lib.gm_get_readout() == 0
    here = []
    centre_step(here)
    assert fresh[0][1] == 0 and np.array_equal(_bits(fresh[0][0]), _bits(here[0][0]))
    assert len(mean_out) != len(here[0][0])                                       # (the pooled pair head is [C, H]: another parameter count)
    # an exception inside the switched block: a model whose dims[0] is not the store's feature width
    bad = Fixture('g3_linkpred')
    bad.config = ro.mean_config([(n, ([p[0] + 1, p[1]] if k == 0 else p)) for k, (n, p) in enumerate(bad.config)])
    bad.vars0 = ro.mean_vars([np.vstack([bad.vars0[0], np.zeros((1, bad.vars0[0].shape[1]), f32)])] + bad.vars0[1:], bad.config)
    m = _hu().fixture_meta(bad)
    for call in (lambda: m._run(S.views(), ys, Q.views(), yq, bad.K, True), lambda: m.adapt(S.views(), ys), lambda: m.net(S, None, None)):
        with pytest.raises(ValueError, match='dims'):
            call()
        assert lib.gm_get_readout() == 0


# ---------------------------------------------------------------------------------------------------- 7. end to end
def test_subgraphs_collate_meta_forward_with_the_mean_readout(tmp_path):
    import random
    import gmeta_amd
    from gmeta_amd import _lib, datadir
    from test_train_driver import _dataset
    np.random.seed(1); random.seed(1); torch.manual_seed(1)
    _dataset(tmp_path)
    root = str(tmp_path) + '/'
    feat, graphs, info = datadir.load_features(root), datadir.load_graphs(root), datadir.load_labels(root)
    store = gmeta_amd.GraphStore(graphs, feat)
    args = argparse.Namespace(update_lr=0.05, meta_lr=0.01, n_way=3, k_spt=2, k_qry=6, task_num=4, update_step=3, update_step_test=4, method='G-Meta',
                              sample_nodes=1000, link_pred_mode='False', task_setup='Disjoint', h=2)
    db = gmeta_amd.Subgraphs(root, 'train', info, n_way=3, k_shot=2, k_query=6, batchsz=8, args=args, adjs=store, h=2, verbose=False)
    config = [('GraphConv', [feat[0].shape[1], 32]), ('GraphConv', [32, 32]), ('Linear', [32, 3]), MEAN]
    maml = gmeta_amd.Meta(args, config).to('cuda')
    batch = gmeta_amd.collate([db[i] for i in range(4)])
    accs = maml(*batch, feat)
    assert np.isfinite(accs).all() and len(accs) == 4
    # the restatement of the first task on the batch's own node lists
    theta0 = None
    maml2 = gmeta_amd.Meta(args, config).to('cuda')
    theta0 = [p.detach().cpu().numpy().copy() for p in maml2.net.parameters()]
    one = gmeta_amd.collate([db[0]])
    maml2(*one, feat)
    og = [orc.Graph(*gr) for gr in graphs]
    seeds_s, seeds_q, ys, yq = db._task_arrays(0)
    sb = orc.extract_batch(og, seeds_s, 2, 1000, db.rng_seed, False)
    qb = orc.extract_batch(og, seeds_q, 2, 1000, db.rng_seed, False)
    with ro.patched():
        lq, aq, mg = orc.task_inner_loop(sb, qb, sb.features(feat), qb.features(feat), ys, yq, theta0, config, 2, 0.05, 3, True)
    grad = torch.cat([p.grad.reshape(-1) for p in maml2.net.parameters()]).cpu().numpy()
    want = np.concatenate([g.reshape(-1) for g in mg])
    np.testing.assert_allclose(maml2.last_stats['losses_q'], lq, atol=TOL, rtol=1e-4)
    np.testing.assert_allclose(grad, want, atol=TOL * max(1.0, float(np.abs(want).max())), rtol=1e-3)
    joint = db.get_batch([0, 1, 2, 3])
    assert np.isfinite(maml(*joint, feat)).all()
    assert _lib.lib().gm_get_readout() == 0


def _train(tmp_path, extra):
    sys.path.insert(0, ROOT)
    import train as drv
    args = drv.parse(['--data_dir', str(tmp_path) + '/', '--epoch', '2', '--k_spt', '2', '--k_qry', '6', '--task_num', '4', '--update_step', '3',
                      '--update_step_test', '4', '--update_lr', '0.05', '--meta_lr', '0.01', '--hidden_dim', '32', '--batchsz', '40', '--h', '2',
                      '--eval_tasks', '10', '--train_result_report_steps', '5', '--readout', 'mean'] + extra)
    return drv.main(args)


def test_train_driver_with_the_mean_readout_on_nodes(tmp_path):
    from test_train_driver import _dataset
    _dataset(tmp_path)
    res = _train(tmp_path, ['--task_setup', 'Disjoint', '--n_way', '3'])
    assert res['test_acc'] > 0.6, res            # 3-way chance is 0.33; the classes are homophilous and their features separable, pooled too


def _link_dataset(tmp, n_graphs=6, n=120, F0=8, seed=0):
    """Shared link prediction laid out like synth.link_dataset (names 'g_i_j', every listed pair stored as an edge, *_spt / *_qry tables), with a
    signal a pooled readout can see: every graph has two communities with separable features; label-1 pairs lie inside the one, label-0 pairs
    inside the other.

    Why not synth.link_dataset itself: it is made for shapes and timings, not for learning.  Its features are i.i.d. N(0, 1), independent of the
    graph and of the labels, and its negative pairs are stored as edges exactly like the positive ones (the reference's data layout), so a pair's
    subgraph looks the same for either label but for degree statistics; nothing in the suite holds any head, centre or mean, to learning it, and a
    'learns above chance' bound on it would have to come from a run of the code under test.  The node run above likewise trains on
    test_train_driver._dataset (class-separable features), not on synth.node_dataset, whose labels are uniform noise."""
    from gmeta_amd import datadir, synth
    rng = np.random.default_rng(seed)
    half = n // 2
    proto = (2 * rng.standard_normal((2, F0))).astype(f32)
    graphs, feats, info = [], [], {}
    splits = {}
    for g in range(n_graphs):
        mode = ('train', 'train', 'train', 'train', 'val', 'test')[g]
        src, dst = [], []
        for lab in (0, 1):
            e = synth.pa_edges(half, 3, rng) + lab * half
            e = e[e[:, 0] != e[:, 1]]
            e = np.unique(np.sort(e, axis=1), axis=0)
            src.append(e[:, 0]); dst.append(e[:, 1])
            spt = np.zeros(len(e), bool)
            spt[rng.choice(len(e), int(0.3 * len(e)), replace=False)] = True
            for (a, b), s in zip(e.tolist(), spt.tolist()):
                nm = '%d_%d_%d' % (g, a, b)
                info[nm] = lab
                for key in (mode, mode + ('_spt' if s else '_qry')):
                    names, labels = splits.setdefault(key, ([], []))
                    names.append(nm); labels.append(str(lab))
        graphs.append((n, np.concatenate(src), np.concatenate(dst)))
        com = (np.arange(n) >= half).astype(np.int64)
        feats.append((proto[com] + 0.3 * rng.standard_normal((n, F0))).astype(f32))
    datadir.write_datadir(str(tmp), graphs, feats, info, splits)


def test_train_driver_with_the_mean_readout_on_pairs(tmp_path):
    _link_dataset(tmp_path)
    res = _train(tmp_path, ['--task_setup', 'Shared', '--link_pred_mode', 'True', '--n_way', '2'])
    assert res['test_acc'] > 0.6, res            # 2-way chance is 0.5
