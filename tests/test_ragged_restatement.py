"""CPU: the restatement of ragged-task mode (tests/ragged_ref.py) is validated before the GPU tests trust it -- against the pinned oracle on
balanced tasks (bitwise) and against fp64 autograd of a literal statement of the loss on a ragged task -- and the new public surface exists
(exported symbols, train.py --ragged, Meta.ragged)."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gmeta_oracle as orc
import ragged_ref as rr
from golden_util import CASES, Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize('case', CASES)
def test_patched_inner_loop_equals_the_oracle_on_balanced_tasks(case):
    """Fed the fixture's own (balanced) tasks, the inner loop with the three ragged functions patched in returns exactly the arrays of the
    unpatched one: query losses, accuracies and every meta-gradient array, NaN positions included."""
    fx = Fixture(case)
    masks = rr.all_masks(fx, ragged=False)
    a = rr.run_tasks(fx, masks, False, fx.K, True)
    b = rr.run_tasks(fx, masks, True, fx.K, True)
    for x, y in zip(a, b):
        assert _same(x[0], y[0]) and _same(x[1], y[1])
        assert len(x[2]) == len(y[2]) and all(_same(g, h) for g, h in zip(x[2], y[2]))
    saved = (orc.proto_loss_spt, orc.proto_loss_qry, orc.protos_to_dlogits)
    with rr.patched(fx.z['y_spt'][0]):
        assert orc.proto_loss_spt is not saved[0]
    assert (orc.proto_loss_spt, orc.proto_loss_qry, orc.protos_to_dlogits) == saved          # restored


def _literal(z_s, y_s, z_q, y_q, k_spt):
    """The definition, literally (torch, any dtype): support loss, query loss."""
    classes = sorted(set(y_s.tolist()))
    sup = [[i for i in range(len(y_s)) if y_s[i] == c][:k_spt] for c in classes]
    protos = torch.stack([z_s[r].mean(0) for r in sup])
    rows_s = [i for r in sup for i in r]
    tgt_s = torch.tensor([c for c, r in enumerate(sup) for _ in r])
    logp_s = torch.log_softmax(-((z_s[rows_s][:, None, :] - protos[None]) ** 2).sum(2), 1)
    tgt_q = torch.tensor([classes.index(int(v)) for v in y_q])
    logp_q = torch.log_softmax(-((z_q[:, None, :] - protos[None]) ** 2).sum(2), 1)
    return -logp_s[torch.arange(len(rows_s)), tgt_s].mean(), -logp_q[torch.arange(len(y_q)), tgt_q].mean(), protos


def test_ragged_gradients_match_fp64_autograd():
    """A hand-made task: class 7 has fewer than k_spt support rows, class 4 more (only its first k_spt count), class 9 has no query rows."""
    rng = np.random.default_rng(3)
    k_spt, D = 3, 5
    y_s = np.array([4, 9, 7, 4, 4, 9, 7, 4, 9], np.int32)          # 4: four rows (three count), 9: three, 7: two
    y_q = np.array([7, 4, 4, 7, 4, 7, 4], np.int32)                # 9: none
    z_s = rng.standard_normal((len(y_s), D)).astype(f32)
    z_q = rng.standard_normal((len(y_q), D)).astype(f32)
    spt, qry, p2d = rr.make(y_s)
    loss_s, acc_s, protos, dl_s = spt(z_s, y_s, k_spt)
    loss_q, acc_q, dl_q, dp = qry(z_q, y_q, protos, need_grad=True)
    dl_sp = p2d(y_s, k_spt, dp, z_s.shape)

    ts = torch.tensor(z_s.astype(np.float64), requires_grad=True)
    tq = torch.tensor(z_q.astype(np.float64), requires_grad=True)
    Ls, Lq, P = _literal(ts, y_s, tq, y_q, k_spt)
    gs, = torch.autograd.grad(Ls, ts, retain_graph=True)
    gq, gsp = torch.autograd.grad(Lq, [tq, ts])
    tol = 1e-6
    assert abs(float(loss_s) - float(Ls)) < tol and abs(float(loss_q) - float(Lq)) < tol
    for got, want in ((protos, P.detach().numpy()), (dl_s, gs.numpy()), (dl_q, gq.numpy()), (dl_sp, gsp.numpy())):
        assert np.abs(got.astype(np.float64) - want).max() < tol
    # the prototype gradient itself: dL_q/dp through a leaf
    pl = torch.tensor(protos.astype(np.float64), requires_grad=True)
    classes = sorted(set(y_s.tolist()))
    tgt = torch.tensor([classes.index(int(v)) for v in y_q])
    lp = torch.log_softmax(-((torch.tensor(z_q.astype(np.float64))[:, None, :] - pl[None]) ** 2).sum(2), 1)
    gp, = torch.autograd.grad(-lp[torch.arange(len(y_q)), tgt].mean(), pl)
    assert np.abs(dp.astype(np.float64) - gp.numpy()).max() < tol
    assert not dl_s[3 + 4].any() and not dl_sp[7].any()            # row 7: the fourth row of class 4 takes no part
    assert 0.0 <= acc_s <= 1.0 and 0.0 <= acc_q <= 1.0


def test_restatement_rejects_what_the_library_rejects():
    spt, qry, _ = rr.make(np.array([0, 1, 0, 1]))
    protos = np.zeros((2, 3), f32)
    with pytest.raises(ValueError, match='outside the support classes'):
        qry(np.zeros((2, 3), f32), np.array([0, 2]), protos)
    with pytest.raises(ValueError, match='without query rows'):
        qry(np.zeros((0, 3), f32), np.array([], np.int64), protos)


@pytest.mark.parametrize('case,left_out,scored', [('g0_disjoint_h1', 0, None), ('g1_sampled_h2', 0, None), ('g2_shared', 0, None), ('g3_linkpred', 0, None),
                                                  ('g5_in_gt_out', 0, None), ('g1_h3', 1, 51), ('g7_wide_h2', 1, 68)])
def test_drop_rule_leaves_few_ties(case, left_out, scored):
    """The ragged tasks cut out of the fixtures: how many query scorings (one query row at one step) have their two best log-probabilities
    closer than 1e-4, in the training run (update_step) and in the fine-tuning run (update_step_test).  The GPU accuracy comparison leaves
    those scorings out, at most two per case."""
    fx = Fixture(case)
    for K, grad in ((fx.K, True), (fx.K_test, False)):
        margins = []
        rr.run_tasks(fx, rr.all_masks(fx), True, K, grad, margins)
        assert len(margins) == fx.T * (K + 1)
        m = np.concatenate(margins)
        tied = int((~(m >= 1e-4)).sum())
        assert tied <= 2
        if grad:
            assert tied == left_out and (scored is None or len(m) == scored)


def test_new_symbols_are_declared_and_exported():
    from gmeta_amd import _lib
    assert 'gm_set_ragged_classes' in _lib.PROTOTYPES and 'gm_get_ragged_classes' in _lib.PROTOTYPES
    hdr = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    assert 'void gm_set_ragged_classes(int32_t on);' in hdr and 'int32_t gm_get_ragged_classes(void);' in hdr
    lib = _lib.lib()                      # (raises AttributeError when a declared symbol is not exported)
    assert lib.gm_get_ragged_classes() == 0
    lib.gm_set_ragged_classes(1)
    try:
        import threading
        seen = []
        th = threading.Thread(target=lambda: seen.append(lib.gm_get_ragged_classes()))
        th.start(); th.join()
        assert lib.gm_get_ragged_classes() == 1 and seen == [0]          # per calling thread
    finally:
        lib.gm_set_ragged_classes(0)


def test_train_help_lists_ragged():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--help'], capture_output=True, text=True, check=True).stdout
    assert '--ragged' in out and 'imbalanced' in out


def test_meta_ragged_defaults_to_off():
    import gmeta_amd
    from gmeta_amd import synth
    args = argparse.Namespace(update_lr=0.01, meta_lr=0.001, n_way=3, k_spt=3, k_qry=4, task_num=2, update_step=2, update_step_test=3, method='G-Meta')
    cfg = synth.make_config(8, 16, 2, 3)
    assert gmeta_amd.Meta(args, cfg).ragged == 0
    args.ragged = 1
    assert gmeta_amd.Meta(args, cfg).ragged == 1
