"""CPU (-m "not gpu"): the restatement of the mean readout (tests/readout_ref.py) against fp64 torch autograd of a literal statement of the pooled
model, the stability of its accuracies under the summation order, the tied-row counts the GPU tests rely on, and the host side of the feature:
config parsing, Classifier shapes, the C ABI switch."""
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
import readout_ref as ro                                                      # noqa: E402
from golden_util import CASES, NAN_CASES, Fixture                             # noqa: E402

f32 = np.float32
ACC_CASES = ('g0_disjoint_h1', 'g1_sampled_h2', 'g2_shared', 'g3_linkpred', 'g5_in_gt_out', 'g7_wide_h2')      # the fixtures whose accuracies the GPU tests check
COLLAPSED = {'g1_h3': (24, 72), 'g8_wide_scales': (100, 150)}                 # tied rows / scored rows of a training step under mean pooling


def _perturbed(fx, seed):
    """The fixture's pooled weights moved off their recorded values, every bias off the relu kink (tests/test_hip_fuzz.py: why)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, v in enumerate(ro.mean_vars(fx.vars0, fx.config)):
        if v.ndim == 2:
            out.append((v + 0.05 * rng.standard_normal(v.shape) * max(float(np.abs(v).max()), 1e-3)).astype(f32))
        else:
            out.append((v + rng.uniform(0.05, 0.2, v.shape) * rng.choice([-1.0, 1.0], v.shape)).astype(f32))
    return out


def _fp64_autograd(batch, x0, vars_, config, R):
    """logits and d sum(logits * R) / d vars of the pooled model, stated literally in fp64 torch."""
    gcn, lin, link = orc.parse_config(config)
    th = [torch.tensor(v.astype(np.float64), requires_grad=True) for v in vars_]
    n = batch.n
    dst = torch.from_numpy(np.repeat(np.arange(n), np.diff(batch.indptr)))
    src = torch.from_numpy(np.asarray(batch.indices, np.int64))
    agg = lambda x: torch.zeros(n, x.shape[1], dtype=torch.float64).index_add(0, dst, x[src])      # noqa: E731
    norm = torch.from_numpy(batch.norm.astype(np.float64))[:, None]
    h = torch.from_numpy(np.asarray(x0, np.float64))
    for l, (fi, fo) in enumerate(gcn):
        W, b = th[2 * l], th[2 * l + 1]
        xs = h * norm
        pre = agg(xs @ W) if fi > fo else agg(xs) @ W
        h = torch.relu(pre * norm + b)
    sub = torch.from_numpy(np.repeat(np.arange(batch.S), np.diff(batch.sub_off)))
    cnt = torch.from_numpy(np.diff(batch.sub_off).astype(np.float64))[:, None]
    p = torch.zeros(batch.S, h.shape[1], dtype=torch.float64).index_add(0, sub, h) / cnt          # dgl.mean_nodes(g, 'h')
    logits = p @ th[2 * len(gcn)].T + th[2 * len(gcn) + 1]
    (logits * torch.from_numpy(R.astype(np.float64))).sum().backward()
    return logits.detach().numpy(), [t.grad.numpy() for t in th]


@pytest.mark.parametrize('case', ['g1_h3', 'g3_linkpred', 'g5_in_gt_out', 'g7_wide_h2'])
def test_restatement_matches_fp64_autograd(case):
    """Within 1e-5 * max(1, max |want|): measured on g1_h3 the logits differ by 2e-8 and the gradients by at most 6.2e-6 at magnitude 1.2 -- the bound leaves
    a margin of 1.6 over that for the other fixtures (a pair model, a multiply-first last layer, hidden 128)."""
    fx = Fixture(case)
    cfg, th = ro.mean_config(fx.config), _perturbed(fx, 3)
    fwd, bwd = ro.make()
    rng = np.random.default_rng(5)
    for t in range(fx.T):
        sb, _ = ro.fixture_batches(fx, t)
        x0 = sb.features(fx.feats)
        R = rng.standard_normal((sb.S, fx.config[[n for n, _ in fx.config].index('Linear')][1][1])).astype(f32)
        logits, cache = fwd(sb, x0, th, cfg)
        grads = bwd(sb, th, cfg, cache, R)
        want_l, want_g = _fp64_autograd(sb, x0, th, cfg, R)
        worst = [float(np.abs(logits - want_l).max() / max(1.0, np.abs(want_l).max()))]
        worst += [float(np.abs(g - w).max() / max(1.0, np.abs(w).max())) for g, w in zip(grads, want_g)]
        print(case, t, 'max scaled error', max(worst))
        assert max(worst) <= 1e-5, (case, t, worst)


def test_patched_restores_the_oracle_and_composes_with_the_ragged_patch():
    import ragged_ref as rr
    saved = (orc.classifier_forward, orc.classifier_backward, orc.proto_loss_spt)
    with pytest.raises(RuntimeError):
        with ro.patched(), rr.patched(np.arange(3)):
            assert orc.classifier_forward is not saved[0] and orc.proto_loss_spt is not saved[2]
            raise RuntimeError('inside')
    assert (orc.classifier_forward, orc.classifier_backward, orc.proto_loss_spt) == saved


def _ties(fx, K, need_grad, **how):
    margins = []
    res = ro.run_tasks(fx, K, need_grad, margins, **how)
    m = np.concatenate(margins)
    return res, int((~(m >= 1e-4)).sum()), len(m), float(np.nanmin(m)) if not np.isnan(m).all() else float('nan')


def test_tied_rows_of_the_pooled_fixtures():
    """What tests/test_hip_readout.py's accuracy rule relies on: on the six fixtures it checks accuracies on, no query scoring of the restated training
    step or fine-tuning run has its two largest log-probabilities closer than 1e-4 (774 and 1,016 scorings: rows x (K + 1) steps; the smallest gap is
    1.2e-4, on g5_in_gt_out); g1_h3 and g8_wide_scales collapse under mean pooling from their recorded weights and are checked on losses and gradients only.

    The feature request quoted 720 scorings for the training step.  Counted here it is 774 = sum over the six fixtures of T x Q x (K + 1):
    240 (g0_disjoint_h1: 4 x 10 x 6) + 150 (g2_shared: 3 x 10 x 5) + 4 x 96 (the other four: 2 x 12 x 4).  720 is what comes out with g2_shared at 96
    like its neighbours; the fine-tuning count (1,016), the zero tied rows and the smallest gap agree with the request."""
    total = [0, 0]
    gaps = {}
    for case in ACC_CASES:
        fx = Fixture(case)
        for which, (K, need_grad) in enumerate(((fx.K, True), (fx.K_test, False))):
            _, tied, rows, gap = _ties(fx, K, need_grad)
            assert tied == 0, (case, which, tied)
            total[which] += rows
            gaps[case] = min(gaps.get(case, np.inf), gap)
    assert total == [774, 1016], total
    assert min(gaps, key=gaps.get) == 'g5_in_gt_out' and 1.2e-4 <= gaps['g5_in_gt_out'] < 1.3e-4, gaps
    for case, (tied_want, rows_want) in COLLAPSED.items():
        fx = Fixture(case)
        _, tied, rows, _ = _ties(fx, fx.K, True)
        assert (tied, rows) == (tied_want, rows_want), (case, tied, rows)


@pytest.mark.parametrize('case', [c for c in CASES if c not in NAN_CASES])
def test_summation_order_moves_the_meta_gradient_by_rounding_only(case):
    """Pooling in reversed row order or in fp64 is another rounding of the same sums: the meta-gradient stays within the bound the restatement is held to
    against fp64 above, 1e-5 * max(1, max |g|) (measured: at most 9e-7), and no accuracy changes."""
    fx = Fixture(case)
    lq, aq, g = ro.meta_step(fx)
    for how in (dict(reverse=True), dict(dtype=np.float64)):
        lq2, aq2, g2 = ro.meta_step(fx, **how)
        print(case, how, 'max |d grad|', float(np.abs(g - g2).max()))
        assert np.abs(g - g2).max() <= 1e-5 * max(1.0, float(np.abs(g).max()))
        assert np.array_equal(aq, aq2)


# ---------------------------------------------------------------------------------------------------- host side
GCN = [('GraphConv', [8, 16]), ('GraphConv', [16, 16]), ('Linear', [16, 3])]


def test_make_model_accepts_the_readout_entry_and_names_what_it_does_not_know():
    from gmeta_amd import _lib
    for cfg, readout, link in ((GCN, 'centre', 0), (GCN + [('Readout', ['centre'])], 'centre', 0), (GCN + [('Readout', ['mean'])], 'mean', 0),
                               (GCN + [('Readout', ['mean']), ('LinkPred', [True])], 'mean', 1), (GCN[:2] + [('Readout', ['mean'])] + GCN[2:], 'mean', 0)):
        m = _lib.make_model(cfg)
        assert _lib.config_readout(cfg) == readout and m.link_pred == link and m.n_gcn == 2 and m.n_out == 3
    for bad in (GCN + [('Readout', ['max'])], GCN + [('Readout', 'mean')], GCN + [('Readout', ['mean', 'mean'])], GCN + [('Readout', [])],
                GCN + [('Readout', ['mean']), ('Readout', ['mean'])], GCN + [('LinkPred', [True]), ('Readout', ['mean'])]):
        with pytest.raises(ValueError, match='Readout'):
            _lib.make_model(bad)
    with pytest.raises(ValueError) as ei:
        _lib.make_model(GCN + [('Dropout', [0.5]), ('BatchNorm', [16])])
    assert 'BatchNorm' in str(ei.value) and 'Dropout' in str(ei.value)


def test_classifier_shapes_under_the_mean_readout():
    import gmeta_amd
    from gmeta_amd import _lib
    for tail, readout, wl in (([], 'centre', (3, 16)), ([('LinkPred', [True])], 'centre', (3, 32)), ([('Readout', ['mean'])], 'mean', (3, 16)),
                              ([('Readout', ['mean']), ('LinkPred', [True])], 'mean', (3, 16))):
        net = gmeta_amd.Classifier(GCN + tail)
        assert net.readout == readout and net.LinkPred_mode == bool(tail and tail[-1][0] == 'LinkPred')
        assert tuple(net.vars[4].shape) == wl and tuple(net.vars[5].shape) == (3,)
        assert [tuple(v.shape) for v in net.vars[:4]] == [(8, 16), (16,), (16, 16), (16,)]
        with _lib.readout_switch(readout):                     # the library's parameter count under the same mode is the Classifier's
            assert int(_lib.lib().gm_model_param_count(__import__('ctypes').byref(net.model))) == sum(v.numel() for v in net.vars)
    assert __import__('ctypes').sizeof(_lib.Model) == 32 and __import__('ctypes').sizeof(_lib.HParams) == 32      # the switch is not a struct field


def test_the_library_exports_the_readout_switch():
    from gmeta_amd import _lib
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    for name in ('gm_set_readout', 'gm_get_readout'):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert 'void gm_set_readout(int32_t mode);' in hdr and 'int32_t gm_get_readout(void);' in hdr
    assert '#define GM_READOUT_CENTRE 0' in hdr and '#define GM_READOUT_MEAN 1' in hdr
    assert lib.gm_get_readout() == 0                              # off by default
    try:
        lib.gm_set_readout(1)
        assert lib.gm_get_readout() == 1
        for bad in (-1, 2, 7):
            lib.gm_set_readout(bad)
            assert lib.gm_get_readout() == 1 and b'gm_set_readout' in lib.gm_last_error()
        seen = []
        th = threading.Thread(target=lambda: seen.append(lib.gm_get_readout()))       # per calling thread
        th.start(); th.join()
        assert seen == [0]
        with pytest.raises(KeyError):
            with _lib.readout_switch('centre'):
                assert lib.gm_get_readout() == 0
                raise KeyError('inside')
        assert lib.gm_get_readout() == 1                          # the block restores what it found, after an exception too
    finally:
        lib.gm_set_readout(0)
