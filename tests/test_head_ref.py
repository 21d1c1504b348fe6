"""CPU: tests/head_ref.py is what tests/test_hip_head_numerics.py takes it for -- its fp64 statement of a head-and-loss launch against the oracle (balanced
sets), tests/ragged_ref.py (ragged sets) and central finite differences of the loss; its fp32 restatement next to it; and every random case of the GPU test
decided (no scored row whose two best log-probabilities are within the fp32 error of each other)."""
import types

import numpy as np
import pytest

import gmeta_oracle as orc
import head_ref as hr
import ragged_ref as rr

f32, f64 = np.float32, np.float64
BY_NAME = {c['name']: c for c in hr.CASES}
BALANCED = [c['name'] for c in hr.CASES if not c['ragged'] and not c['tie'] and c['name'] not in ('table_off_ct24_n16', 'table_edge_ct16_n32', 'size_unstaged')]
RAGGED = [c['name'] for c in hr.CASES if c['ragged']]


def _whole(d, **over):
    a = dict(H=d['H'], Wl=d['Wl'], bl=d['bl'], protos=d['protos'])
    a.update(over)
    return hr.whole64(a['H'], d['crow'], d['set_off'], a['Wl'], a['bl'], d['tables'], a['protos'])


def test_cases_cover_the_axes():
    """The table of the GPU test: every value of every axis is there (each case runs every launch path)."""
    cs = hr.CASES
    assert {c['Hd'] for c in cs} == {6, 8, 20, 96, 256} and {c['pair'] for c in cs} == {'1', '2', '2s'}
    assert {1, 2, 3, 5, 8, 9, 64} <= {c['C'] for c in cs}
    assert {c['out'] for c in cs} == {'dQ', 'Gc', 'Gcc', 'none'} and {c['mode'] for c in cs} == {0, 1}
    assert {(c['sgd'], c['amax']) for c in cs} >= {(True, False), (False, True), (False, False)}
    assert any(c['mode'] == 1 and not c['grad'] for c in cs) and any(c['mode'] == 1 and c['grad'] for c in cs)
    assert any(c['ragged'] and c['spt_extra'] for c in cs) and any(c['compact_nc'] for c in cs) and any(c['tie'] for c in cs)
    assert len({c['name'] for c in cs}) == len(cs)
    for name, fast in (('hd8_pair_shared_fast_amax', True), ('hd20_pair_shared_c9', False)):
        c = BY_NAME[name]
        assert c['pair'] == '2s' and c['out'] == 'dQ' and (1024 % c['Hd'] == 0 and c['C'] <= 8) == fast
    t = BY_NAME['table_off_ct24_n16']
    assert 24 * 16 * 24 > 8192 and t['C'] * 24 == 576 and t['mode'] == 1
    assert 16 * 32 * 16 == 8192


@pytest.mark.parametrize('name', BALANCED)
def test_fp64_reference_matches_the_oracle_on_balanced_sets(name):
    """classifier_forward / classifier_backward (a head without GCN layers below it: logits, dWl, dbl) and proto_loss_spt / proto_loss_qry, set by set, in the
    oracle's fp32; dQ has no oracle of its own without the layers below and is held by the finite differences."""
    d = hr.build(BY_NAME[name]); case = d['case']
    ref = _whole(d)
    config = [('Linear', [d['nc'] * case['Hd'], case['C']])]
    for t in range(len(case['sets'])):
        a, b = int(d['set_off'][t]), int(d['set_off'][t + 1])
        p = 0 if case['shared_params'] else t
        batch = types.SimpleNamespace(centre_rows=d['crow'][a:b], norm=np.ones(len(d['H']), f32))
        vars_ = [d['Wl'][p], d['bl'][p]]
        logits, cache = orc.classifier_forward(batch, d['H'], vars_, config)
        np.testing.assert_allclose(logits, ref['logits'][a:b], rtol=1e-5, atol=1e-5)
        y = d['y'][a:b]
        r = ref['sets'][t]
        if case['mode'] == 0:
            loss, acc, protos, dl = orc.proto_loss_spt(logits, y, case['n_support'])
            np.testing.assert_allclose(protos, r['protos'], rtol=1e-5, atol=1e-5)
        else:
            loss, acc, dl, dp = orc.proto_loss_qry(logits, y, d['protos'][t], need_grad=True)
            np.testing.assert_allclose(dp, r['dprotos'], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(loss, r['loss'], rtol=1e-5, atol=1e-5)
        assert acc == f32(r['acc'])
        np.testing.assert_allclose(dl, ref['dlogits'][a:b], rtol=1e-4, atol=1e-5)
        g = orc.classifier_backward(batch, vars_, config, cache, dl)
        np.testing.assert_allclose(g[0], ref['dWl'][t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(g[1], ref['dbl'][t], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('name', RAGGED)
def test_fp64_reference_matches_the_ragged_restatement(name):
    d = hr.build(BY_NAME[name]); case = d['case']
    sub_set = d['sub_set']
    z, _ = hr.logits64(d['H'], d['crow'], sub_set, d['Wl'], d['bl'])
    z = z.astype(f32)
    res = hr.loss64(z, d['tables'], d['protos'])
    for t in range(len(case['sets'])):
        a, b = int(d['set_off'][t]), int(d['set_off'][t + 1])
        y = d['y'][a:b]
        if case['mode'] == 0:
            spt, _, _ = rr.make(y)
            loss, acc, protos, dl = spt(z[a:b], y, case['n_support'])
            np.testing.assert_allclose(protos, res[t]['protos'], rtol=1e-5, atol=1e-5)
        else:
            _, qry, _ = rr.make(np.asarray(d['spt_classes'][t] if d['spt_classes'] else np.unique(y)))
            n_cls = len(d['tables'][t][0])
            loss, acc, dl, dp = qry(z[a:b], y, d['protos'][t, :n_cls], need_grad=True)
            np.testing.assert_allclose(dp, res[t]['dprotos'], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(loss, res[t]['loss'], rtol=1e-5, atol=1e-5)
        assert acc == f32(res[t]['acc'])
        np.testing.assert_allclose(dl, res[t]['dlogits'][a:b], rtol=1e-4, atol=1e-5)
        assert not res[t]['dlogits'][:a].any() and not res[t]['dlogits'][b:].any()


@pytest.mark.parametrize('name', ['hd6_pair_shared_ragged_amax', 'hd6_pair_c1_qry_gc', 'hd8_pair_shared_fast_amax', 'hd20_pair_ragged_qry_empty_class'])
def test_fp64_reference_against_finite_differences(name):
    """Central differences in fp64 of the summed loss with respect to the logits, the prototypes, Wl, bl and H.  The head is linear in H, so the difference
    quotient is dL/dH itself; the reference's dQ is that times relu'(H), summed where a pair's centres share a row, and zero off the centre rows."""
    d = hr.build(BY_NAME[name])
    rng = np.random.default_rng(3)
    H, Wl, bl = d['H'].astype(f64), d['Wl'].astype(f64), d['bl'].astype(f64)
    protos = None if d['protos'] is None else d['protos'].astype(f64)
    ref = _whole(d, H=H, Wl=Wl, bl=bl, protos=protos)
    eps = 1e-6

    def fd(arr, key, idx):
        old = arr[idx]
        arr[idx] = old + eps; up = _whole(d, **{'H': H, 'Wl': Wl, 'bl': bl, 'protos': protos})['loss'].sum()
        arr[idx] = old - eps; dn = _whole(d, **{'H': H, 'Wl': Wl, 'bl': bl, 'protos': protos})['loss'].sum()
        arr[idx] = old
        return (up - dn) / (2 * eps)

    def some(shape, k=24):
        flat = rng.choice(int(np.prod(shape)), size=min(k, int(np.prod(shape))), replace=False)
        return [tuple(int(v) for v in np.unravel_index(f, shape)) for f in flat]

    tol = dict(rtol=1e-6, atol=1e-8)
    for idx in some(Wl.shape):
        np.testing.assert_allclose(ref['dWl'][idx], fd(Wl, 'Wl', idx), **tol)
    for idx in some(bl.shape):
        np.testing.assert_allclose(ref['dbl'][idx], fd(bl, 'bl', idx), **tol)
    hit_rows = np.nonzero(ref['hit'])[0]
    for r in list(hit_rows[:6]) + [int(d['crow'][int(d['set_off'][1]) + 1, 0])]:          # among them a row two centres share ('2s')
        for col in range(H.shape[1]):
            np.testing.assert_allclose(ref['dQ'][r, col], fd(H, 'H', (r, col)) if d['H'][r, col] > 0 else 0.0, **tol)
    for r in np.nonzero(~ref['hit'])[0][:3]:
        assert fd(H, 'H', (int(r), 0)) == 0.0 and not ref['dQ'][r].any()
    if protos is not None:
        for t, (cl, _) in enumerate(d['tables']):
            for c in range(len(cl)):
                for k in range(protos.shape[2]):
                    np.testing.assert_allclose(ref['sets'][t]['dprotos'][c, k], fd(protos, 'protos', (t, c, k)), **tol)
    # dlogits: the nonlinear stage alone
    z = ref['logits'].copy()
    for idx in some(z.shape):
        old = z[idx]
        z[idx] = old + eps; up = sum(r['loss'] for r in hr.loss64(z, d['tables'], protos))
        z[idx] = old - eps; dn = sum(r['loss'] for r in hr.loss64(z, d['tables'], protos))
        z[idx] = old
        np.testing.assert_allclose(ref['dlogits'][idx], (up - dn) / (2 * eps), **tol)


@pytest.mark.parametrize('name', [c['name'] for c in hr.CASES])
def test_cases_are_decided_and_the_restatement_is_close(name):
    """Every random case: no scored row within 64 u max_c dist of a tie (the designed tie case: every row tied); the class tables say which launcher runs; the
    fp32 restatement is fp32-close to the fp64 statement on the same logits."""
    d = hr.build(BY_NAME[name]); case = d['case']
    z, _ = hr.logits64(d['H'], d['crow'], d['sub_set'], d['Wl'], d['bl'])
    z = z.astype(f32)
    res = hr.loss64(z, d['tables'], d['protos'])
    assert hr.is_ragged(d['tables']) == case['ragged']
    for t, (r, (_, rows)) in enumerate(zip(res, d['tables'])):
        if case['tie']:
            assert not r['gap'].any() and hr.undecided(r) == r['Q']
            continue
        assert hr.undecided(r) == 0, (name, t, hr.undecided(r))
        r32 = hr.set_loss32(z, rows, None if d['protos'] is None else d['protos'][t])
        for k in ('protos', 'loss', 'dlogits', 'dprotos'):
            np.testing.assert_allclose(r32[k], r[k], rtol=1e-4, atol=2e-5)
        assert r32['acc'] == f32(r['correct']) / f32(r['Q'])
