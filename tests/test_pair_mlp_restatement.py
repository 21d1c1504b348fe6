"""CPU (-m "not gpu"): the float64 restatement of the BUDDY pair predictor (tests/pair_mlp_ref.py; the definition is in include/gmeta_hip.h) against torch's
float64 autograd of the same formula, the condition its tolerance puts on the GPU tests' inputs (few near-kink entries), and the bound itself."""
import os
import re

import numpy as np
import pytest
import torch

import hop_feature_ref as hop
import pair_mlp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_ASSUMED = 128          # the cases are sized by the kernels' pair tile; the CPU checks take the value the header of the kernels names and check that it does


def small():
    """30 nodes, random directed edges with weights, F = 6, hops = 2, S = 3, Hd = 7, 40 pairs with a == b, a duplicate and both orientations"""
    rng = np.random.default_rng(3)
    N, F, hops, S, Hd, n = 30, 6, 2, 3, 7, 40
    src, dst = rng.integers(0, N, 90), rng.integers(0, N, 90)
    w = np.exp2(rng.uniform(-2, 2, 90)).astype(np.float32)
    g = hop.csr(N, src, dst, w)
    X = hop.features(N, F, 1)
    x, E = hop.levels(*g, X, hops, True), hop.bound(*g, X, hops, True)
    small.graph = (g, X, hops)
    pairs = ref.case_pairs(N, n, 4)
    extra = rng.integers(0, 6, (n, S)).astype(np.float32)
    labels = rng.random(n).astype(np.float32)
    params = ref.init_params((hops + 1) * F + S, Hd, 5)
    return x, E, pairs, extra, labels, params, Hd


def small_levels_fp32():
    g, X, hops = small.graph
    return hop.levels_fp32(*g, X, hops, True, order='reversed')


@pytest.mark.parametrize('op', hop.OPS)
def test_the_restatement_equals_float64_autograd_of_the_same_formula(op):
    x, E, pairs, extra, labels, params, Hd = small()
    got = ref.evaluate(x, pairs, op, extra, params, Hd, labels)
    xt = torch.from_numpy(x)
    a, b = xt[:, pairs[:, 0]], xt[:, pairs[:, 1]]
    z = (a * b if op == 'hadamard' else (a - b).abs()).permute(1, 0, 2).reshape(len(pairs), -1)
    z = torch.cat([z, torch.from_numpy(extra).double()], dim=1)
    w = torch.from_numpy(params).double().requires_grad_(True)
    K = z.shape[1]
    W1, b1, w2, b2 = w[:K * Hd].view(K, Hd), w[K * Hd:K * Hd + Hd], w[K * Hd + Hd:K * Hd + 2 * Hd], w[-1]
    logits = torch.relu(z @ W1 + b1) @ w2 + b2
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).double())
    loss.backward()

    def close(u, v):
        u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
        return np.abs(u - v).max() <= 1e-12 * max(np.abs(v).max(), 1e-300)

    assert close(got['z'], z.numpy()) and close(got['logits'], logits.detach().numpy()) and close(got['loss'], loss.item())
    K_Hd = K * Hd
    for lo, hi in ((0, K_Hd), (K_Hd, K_Hd + Hd), (K_Hd + Hd, K_Hd + 2 * Hd), (K_Hd + 2 * Hd, K_Hd + 2 * Hd + 1)):
        assert close(got['grad'][lo:hi], w.grad.numpy()[lo:hi])
    assert np.abs(got['grad']).min() >= 0 and np.abs(got['grad'][:K_Hd]).max() > 0
    # both orientations, and the duplicate of case_pairs: the same logits
    flip = ref.evaluate(x, pairs[:, ::-1], op, extra, params, Hd)['logits']
    assert np.array_equal(flip, got['logits'])
    # n = 0: loss 0, a zero gradient
    none = ref.evaluate(x, pairs[:0], op, extra[:0], params, Hd, labels[:0])
    assert none['loss'] == 0.0 and not none['grad'].any() and len(none['logits']) == 0


def test_the_bound_is_finite_positive_and_covers_plain_fp32_evaluations():
    x, E, pairs, extra, labels, params, Hd = small()
    X32 = small_levels_fp32()
    assert (np.abs(X32.astype(np.float64) - x) <= E).all()
    for op in hop.OPS:
        tol = ref.bound(x, E, pairs, op, extra, params, Hd, labels)
        want = ref.evaluate(x, pairs, op, extra, params, Hd, labels)
        for k in ('logits', 'grad'):
            assert np.isfinite(tol[k]).all() and (tol[k] > 0).all(), k
        assert np.isfinite(tol['loss']) and tol['loss'] > 0
        assert (tol['logits'] < 1e-3 * (1 + np.abs(want['logits']))).all() and tol['loss'] < 1e-4                      # ... and it is a tight one
        # plain numpy fp32 evaluations (the levels by hop.levels_fp32, which hop.bound covers; K in forward and in reversed order) stay inside it
        z = hop.pair_features(X32[:, pairs[:, 0]], X32[:, pairs[:, 1]], op).transpose(1, 0, 2).reshape(len(pairs), -1)
        z = np.concatenate([z, extra], axis=1)
        K = z.shape[1]
        W1, b1, w2, b2 = (params[:K * Hd].reshape(K, Hd), params[K * Hd:K * Hd + Hd], params[K * Hd + Hd:K * Hd + 2 * Hd], params[-1])
        for order in (np.arange(K), np.arange(K)[::-1]):
            pre = np.zeros((len(pairs), Hd), np.float32)
            for k in order:
                pre = (pre + z[:, k:k + 1] * W1[k:k + 1]).astype(np.float32)
            h = np.maximum(pre + b1, 0).astype(np.float32)
            l = np.zeros(len(pairs), np.float32)
            for j in range(Hd):
                l = (l + h[:, j] * w2[j]).astype(np.float32)
            l = (l + b2).astype(np.float32)
            assert (np.abs(l.astype(np.float64) - want['logits']) <= tol['logits']).all()
    empty = ref.bound(x, E, pairs[:0], 'hadamard', extra[:0], params, Hd, labels[:0])
    assert empty['loss'] == 0.0 and not empty['grad'].any()


def test_the_gpu_cases_cover_every_value_and_keep_near_kink_entries_rare():
    cases = ref.CASES
    assert {c[1] for c in cases} == {5, 64, 100, 300} and {c[2] for c in cases} == {1, 3} and {c[3] for c in cases} == {0, 1, 25}
    assert {c[4] for c in cases} == {1, 8, 100, 256} and {c[6] for c in cases} == set(hop.OPS) and {c[7] for c in cases} == {True, False} == {c[8] for c in cases}
    assert {c[5] for c in cases} == {(0, 0), (0, 1), (1, -1), (1, 0), (1, 1), (3, 7)} and {c[0] for c in cases} == {'hub', 'multigraph', 'chain'}
    assert any(c[1:6] == (5, 1, 0, 1, (0, 1)) for c in cases) and any((c[1], c[3], c[4], c[5]) == (300, 25, 256, (3, 7)) for c in cases)
    src = open(os.path.join(ROOT, 'g-meta_amd', 'csrc', 'pair_mlp.hip')).read()
    assert int(re.search(r'#define PM_T (\d+)', src).group(1)) == T_ASSUMED
    levels = {}
    for c, name in zip(cases, ref.CASE_IDS):
        inp = ref.case_inputs(c, T_ASSUMED)
        key = (c[0], c[1], c[7], c[8], c[2])
        if key not in levels:
            levels[key] = (hop.levels(*inp['csr'], inp['X'], c[2], c[8]), hop.bound(*inp['csr'], inp['X'], c[2], c[8]))
        x, E = levels[key]
        p = inp['pairs']
        if inp['n'] >= 5:
            assert p[0, 0] == p[0, 1] and (p[1] == p[2]).all() and (p[3] == p[4][::-1]).all()
        assert ((inp['labels'] >= 0) & (inp['labels'] <= 1)).all()
        tol = ref.bound(x, E, p, inp['op'], inp['extra'], inp['params'], inp['Hd'], inp['labels'])
        share = float(tol['near'].mean()) if tol['near'].size else 0.0
        print('%s: %d of %d (pair, unit) entries near the kink' % (name, int(tol['near'].sum()), tol['near'].size))
        assert share <= 0.01, (name, share)
        assert np.isfinite(tol['logits']).all() and np.isfinite(tol['grad']).all() and np.isfinite(tol['loss'])
        if inp['n']:
            assert (tol['logits'] > 0).all() and (tol['grad'] >= 0).all() and tol['loss'] > 0      # (a dead unit far from its kink has gradient 0 exactly: bound 0)


def test_header_prototypes_knob_and_python_surface():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name, n_args in (('gm_prop_pair_mlp_dims', 5), ('gm_prop_pair_mlp_tile', 0), ('gm_prop_pair_mlp_forward', 10), ('gm_prop_pair_mlp_step', 13)):
        assert re.search(r'\b%s\s*\(' % name, code) and name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    assert 'tests/pair_mlp_ref.py' in txt and 'pair_mlp_rows' in txt and 'GM_PAIR_MLP_ROWS' in txt
    lib = _lib.lib()
    assert lib.gm_prop_pair_mlp_tile() == T_ASSUMED
    for knob in (b'pair_mlp_rows', b'GM_PAIR_MLP_ROWS'):
        assert lib.gm_get_tuning(knob) == 0 and lib.gm_set_tuning(knob, 77) == 0 and lib.gm_get_tuning(b'pair_mlp_rows') == 77 and lib.gm_set_tuning(knob, 0) == 0
    assert gmeta_amd.PairPredictor is gmeta_amd.predictor.PairPredictor and 'PairPredictor' in gmeta_amd.__all__
    for m in ('scores', 'step', 'fit', 'auc', 'W1', 'b1', 'w2', 'b2'):
        assert hasattr(gmeta_amd.PairPredictor, m)


def test_train_flag_takes_the_epochs_of_the_pair_predictor():
    import train as drv
    base = ['--data_dir', 'x', '--task_setup', 'Shared']
    assert drv.parse(base).buddy == 0 and drv.parse(base + ['--link_pred_mode', 'True']).buddy == 0
    assert drv.parse(base + ['--link_pred_mode', 'True', '--buddy', '5']).buddy == 5
    with pytest.raises(SystemExit, match='link_pred_mode'):
        drv.parse(base + ['--buddy', '5'])                                            # refused before any data is read: node tasks have no pairs
    with pytest.raises(SystemExit, match='buddy'):
        drv.parse(base + ['--link_pred_mode', 'True', '--buddy', '-1'])


def test_no_kernel_of_the_predictor_uses_scratch_memory():
    """private_segment_fixed_size (bytes 4..7 of every kernel descriptor of the built object) is 0: nothing spills."""
    import struct
    import subprocess
    import tempfile
    import test_kernel_resources as kr
    missing = [t for t in kr.TOOLS if not os.path.exists(os.path.join(kr.LLVM, t))]
    assert not missing, 'the LLVM tools that come with the compiler of the build are not under %s: %s' % (kr.LLVM, ', '.join(missing))
    obj = os.path.join(ROOT, 'g-meta_amd', 'csrc', 'build', 'pair_mlp.o')
    if not os.path.exists(obj):
        import __graft_entry__
        __graft_entry__.build()
    with tempfile.TemporaryDirectory() as tmp:
        dev = kr._device_elf(obj, tmp)
        sec = subprocess.run([os.path.join(kr.LLVM, 'llvm-readelf'), '-S', '-W', dev], check=True, capture_output=True, text=True).stdout
        addr, off, size = (int(v, 16) for v in re.search(r'\]\s+\.rodata\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', sec).groups())
        data = open(dev, 'rb').read()
        sym = subprocess.run([os.path.join(kr.LLVM, 'llvm-readelf'), '-s', '-W', dev], check=True, capture_output=True, text=True).stdout
    scratch = {}
    for line in sym.splitlines():
        f = line.split()
        if len(f) >= 8 and f[-1].endswith('.kd'):
            a = int(f[1], 16)
            assert addr <= a < addr + size
            scratch[f[-1][:-3]] = struct.unpack_from('<I', data, off + (a - addr) + 4)[0]
    assert all('k_pmlp_' in k for k in scratch) and all(any(name in k for k in scratch) for name in ('k_pmlp_fwd', 'k_pmlp_wgrad', 'k_pmlp_reduce')), scratch
    assert not any(scratch.values()), scratch
