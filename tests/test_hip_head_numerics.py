"""GPU (-m gpu): the classifier head with the prototypical loss -- k_head_loss and the device code it shares (head_fwd_sub, proto_set, head_bwd_set), and the
unfused k_head_fwd / k_proto / k_head_bwd -- against fp64, one launch at a time through the test-only export gm_dense_head_loss, whose sizing and dispatch are
head_loss()'s own.  tests/head_ref.py holds the fp64 statement, the fp32 restatement and the cases (tests/test_head_ref.py holds THEM to the oracle, the
ragged restatement and finite differences).  Every case runs every launch path: GM_HEAD_STAGE x GM_HEAD_THREADS for the fused kernel, and the unfused trio;
every launch asserts the instantiation it reports.  Every output is pre-filled with sentinels (floats NaN, amax padding words 0x5A5A5A5A), so an element nobody
writes, a write past a set's own classes / parameter range / centre rows, or into another set's slot fails.

Linear quantities, each referenced in fp64 from the kernel's OWN fp32 inputs to that stage (logits from H and the parameters; dWl, dbl, dQ / Gc from H, Wl and
the dlogits the kernel copied out, so the loss's error does not enter), per element, derived, not fitted:
    |got - ref| <= (C_DET + LAMBDA sqrt(K)) u scale,   u = 2^-24,   scale = sum |products| (+ |bias|),   K = the terms summed (hc; the set's subgraphs; C).
  - LAMBDA sqrt(K): the fp32 accumulation in whatever tree the kernel uses.  Every rounding is below u |partial sum| <= u scale and a term passes at most
    K - 1 of them; independent roundings stay below lambda sqrt(K) u scale except with probability ~2K exp(-lambda^2 / 2) (Higham and Mary, SIAM J. Sci.
    Comput. 41, 2019; LAMBDA = 8 as in test_hip_gemm_epilogue.py) -- and 8 sqrt(K) >= K - 1 up to K = 64, where the bar is the deterministic one.
  - C_DET = 3, the roundings that do not depend on K: one per product where the compiler does not contract it into an fma (sum over the terms <= u scale);
    the bias added to a logit after the reduction; the (0 + v0) + v1 of a pair whose centres share a row.  There is no operand split here.
  relu' does not widen the bar: it is decided on the input H, so a masked element is exactly 0 on both sides.
SGD: |next - (cur - lr g)| <= 2u (|cur| + |lr g|) with the kernel's own g: the product and the subtraction round once each, or once together as an fma.
Nonlinear quantities (prototypes, loss, dlogits, dprotos), by the method of test_hip_ragged.py: on the kernel's own fp32 logits, the kernel's largest distance
to fp64 over the sets of a case is at most 4 x the fp32 restatement's own (head_ref.set_loss32: the yardstick, never the kernel).
Accuracy: the kernel predicts the FIRST maximum of the fp32 log-probabilities lp_c = (a_c - m) - lg, a_c = -dist(q, c).  In fp32 a D-term squared distance
carries 3 roundings per term (subtract, counted twice by the square, and the multiply) and the running sum's: |da_c| <~ (3 + lambda sqrt(D)) u dist(q, c), the
typical size (lambda ~ 1.5) being ~15 u at D = 64; m is one of the a_c (exact), a_c - m rounds once (<= u dist), lg moves by at most the largest |d(a_c - m)|
plus its own two roundings, (a_c - m) - lg rounds once more.  Two log-probabilities therefore move against each other by less than ~4 x 15 u max_c dist:
a scored row is DECIDED when the fp64 gap between its two best log-probabilities exceeds 64 u max_c dist(q, c).  Over decided rows the kernel's count of
correct rows must be the fp64 one exactly; test_head_ref.py asserts that no random case has an undecided row, so here the accuracy is exact.  The designed
tie (H = 0: every logit is the bias, every distance equal) must predict class 0 for every row.
dq_amax: the bits of max |dQ| over what the launch wrote for the set.
Across paths: one association (model.hip: head_fwd_sub), so every output of every path is bitwise the default launch's (staged, 1024 threads)."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_ref as hr

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
U = hr.U
C_DET, LAMBDA = 3, 8
GM_EINVAL, GM_ERANGE = -1, -4
BOUND_PAD = 64
PAD_WORD = 0x5A5A5A5A
LR = 0.37
# (GM_HEAD_STAGE, GM_HEAD_THREADS, path); the first is the default launch every other one must equal bit for bit
LAUNCHES = [(1, 0, 0), (1, 256, 0), (1, 512, 0), (0, 0, 0), (0, 256, 0), (0, 512, 0), (1, 0, 1)]


def bar(K):
    return (C_DET + LAMBDA * K ** 0.5) * U


def within(got, ref, scale, K, what):
    got = np.asarray(got, f64)
    assert np.isfinite(got).all(), what
    bad = np.abs(got - ref) > bar(K) * scale
    assert not bad.any(), (what, int(bad.sum()), float((np.abs(got - ref) / np.maximum(scale, 1e-300)).max() / U), 'u; bar', bar(K) / U)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Setup:
    """A case's batch and device inputs, built once; launch() runs one path into fresh sentinel-filled outputs."""

    def __init__(self, case):
        import gmeta_amd
        from gmeta_amd import _lib
        from gmeta_amd.subgraphs import SubgraphBatch
        self._lib, self.lib = _lib, _lib.lib()
        d = self.d = hr.build(case)
        self.case = case
        self.store = gmeta_amd.GraphStore([(hr.N_NODES, d['src'].astype(np.int64), d['dst'].astype(np.int64))], [d['feats']])
        self.B = SubgraphBatch.from_nodes(self.store, d['seeds'], d['set_off'], d['lists'], d['nc_batch'] == 2)
        B = self.B
        assert B.subs == d['subs'] and B.rows == d['rows'] and B.sets == len(case['sets']) and B.centres == d['nc_batch']
        assert np.array_equal(B.sub_off, d['sub_off']) and np.array_equal(np.asarray(B.centres_local()).reshape(d['subs'], -1), d['centre'])
        Cn, hc = case['C'], d['nc'] * case['Hd']
        self.sets = B.sets
        self.wl_off, self.bl_off = 3, 3 + Cn * hc + 2
        self.stride = self.bl_off + Cn + 5
        n_par = len(d['Wl'])
        par = np.full((n_par, self.stride), np.nan, f32)          # the gaps are NaN: a read outside Wl / bl shows
        par[:, self.wl_off:self.wl_off + Cn * hc] = d['Wl'].reshape(n_par, -1)
        par[:, self.bl_off:self.bl_off + Cn] = d['bl']
        self.par = par
        rng = np.random.default_rng(5)
        self.cur = rng.standard_normal((self.sets, self.stride)).astype(f32)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.dH, self.dpar, self.dcur, self.dprotos_in, self.dcentre = dev(d['H']), dev(par), dev(self.cur), dev(d['protos']), dev(d['centre_local'])
        if d['spt_classes'] is not None:
            self.spt_labels = np.concatenate([np.asarray(c, np.int32) for c in d['spt_classes']]).astype(np.int32)
            self.spt_counts = np.asarray([len(c) for c in d['spt_classes']], np.int32)
        else:
            self.spt_labels = self.spt_counts = None

    def launch(self, stage, threads, path):
        case, d, lib, _lib = self.case, self.d, self.lib, self._lib
        Cn, Hd, sets, subs = case['C'], case['Hd'], self.sets, d['subs']
        bwd = case['out'] != 'none'
        nan = lambda *shape: torch.full(shape, float('nan'), device='cuda', dtype=torch.float32)
        o = dict(logits=nan(subs, Cn), loss=nan(sets), acc=nan(sets))
        if case['grad']:
            o['dlogits'] = nan(subs, Cn)
        if case['mode'] == 1 and case['grad']:
            o['dprotos'] = nan(sets, d['c_task'], Cn)
        if case['mode'] == 0:
            o['protos_out'] = nan(sets, d['c_task'], Cn)
        if bwd:
            o['dparams'] = nan(sets, self.stride)
            if case['out'] == 'dQ':
                o['dQ'] = nan(len(d['H']), Hd)
            else:
                o['Gc'] = nan(subs * d['nc'], Hd)
        sgd = case['sgd'] and path == 0
        if sgd:
            o['next'] = nan(sets, self.stride)
        if case['amax']:
            am = np.full(sets * BOUND_PAD, PAD_WORD, np.uint32); am[::BOUND_PAD] = 0
            o['amax'] = torch.from_numpy(am.view(np.int32)).cuda()
        launched = np.full(3, -1, np.int32)
        p = lambda k: _lib.ptr(o.get(k))
        lib.gm_set_ragged_classes(1 if case['ragged'] else 0)
        try:
            _lib.check(lib.gm_set_tuning(b'GM_HEAD_STAGE', stage), 'set_tuning'); _lib.check(lib.gm_set_tuning(b'GM_HEAD_THREADS', threads), 'set_tuning')
            rc = lib.gm_dense_head_loss(self.B.handle, _lib.ptr(self.dH), Hd, d['nc'], 1 if d['compact'] else 0, Cn, _lib.ptr(self.dpar),
                                        0 if case['shared_params'] else self.stride, self.wl_off, self.bl_off, _lib.ptr(self.dcentre), _lib.ptr(d['y']),
                                        case['mode'], case['n_support'], _lib.ptr(self.dprotos_in), d['c_task'] if case['mode'] == 1 else 0,
                                        _lib.ptr(self.spt_labels), _lib.ptr(self.spt_counts), p('logits'), p('dlogits'), p('dprotos'), p('protos_out'), p('loss'),
                                        p('acc'), 1 if bwd else 0, p('dparams'), self.stride, p('dQ'), p('Gc'), _lib.ptr(self.dcur) if sgd else None, p('next'),
                                        self.stride, LR, p('amax'), path, _lib.ptr(launched), _lib.stream_ptr())
            _lib.check(rc, 'gm_dense_head_loss')
        finally:
            lib.gm_set_tuning(b'GM_HEAD_STAGE', 1); lib.gm_set_tuning(b'GM_HEAD_THREADS', 0); lib.gm_set_ragged_classes(0)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in o.items()}
        if 'amax' in out:
            out['amax'] = out['amax'].view(np.uint32)
        nt = 256 if path == 1 else (threads if threads in (256, 512) else 1024)
        want = (nt, 0 if path == 1 else (stage and case['staged']), 1 if case['ragged'] else 0)
        assert tuple(int(v) for v in launched) == want, (case['name'], (stage, threads, path), launched, want)
        return out


def check_against_fp64(S, o):
    """The default launch of a case against the references and the sentinels."""
    case, d = S.case, S.d
    Cn, Hd, nc, sets, set_off, tables = case['C'], case['Hd'], d['nc'], S.sets, d['set_off'], d['tables']
    hc = nc * Hd
    name = case['name']
    # ---- logits
    ref, scale = hr.logits64(d['H'], d['crow'], d['sub_set'], d['Wl'], d['bl'])
    within(o['logits'], ref, scale, hc, (name, 'logits'))
    # ---- the nonlinear stage on the kernel's own logits
    z = o['logits']
    worst = {}

    def close(q, got, r32, r64):
        w = worst.setdefault(q, [0.0, 0.0])
        w[0] = max(w[0], float(np.abs(np.asarray(got, f64) - r64).max())); w[1] = max(w[1], float(np.abs(np.asarray(r32, f64) - r64).max()))

    in_table = np.zeros(d['subs'], bool)
    for t, (classes, rows) in enumerate(tables):
        a, b = int(set_off[t]), int(set_off[t + 1])
        pr = None if d['protos'] is None else d['protos'][t]
        r64, r32 = hr.set_loss64(z, rows, pr), hr.set_loss32(z, rows, pr)
        n_cls = len(classes)
        in_table[np.concatenate(rows)] = True
        assert np.isfinite(o['loss'][t]) and np.isfinite(o['acc'][t])
        close('loss', o['loss'][t], r32['loss'], r64['loss'])
        if case['mode'] == 0:
            close('protos', o['protos_out'][t, :n_cls], r32['protos'], r64['protos'])
            assert np.isnan(o['protos_out'][t, n_cls:]).all(), (name, t, 'prototypes past the set classes')
        if case['grad']:
            close('dlogits', o['dlogits'][a:b], r32['dlogits'][a:b], r64['dlogits'][a:b])
            assert not r64['dlogits'][:a].any() and not r64['dlogits'][b:].any()
            if case['mode'] == 1:
                close('dprotos', o['dprotos'][t, :n_cls], r32['dprotos'], r64['dprotos'])
                assert np.isnan(o['dprotos'][t, n_cls:]).all(), (name, t, 'dprotos past the set classes')
        # accuracy: exact over decided rows -- and every row is decided; the tie predicts class 0 everywhere
        if case['tie']:
            assert o['acc'][t] == f32(len(rows[0])) / f32(r64['Q']), (name, t, o['acc'][t])
        else:
            assert hr.undecided(r64) == 0, (name, t)
            assert o['acc'][t] == f32(r64['correct']) / f32(r64['Q']), (name, t, o['acc'][t], r64['correct'], r64['Q'])
    for q, (err, yard) in sorted(worst.items()):
        print('%-34s %-8s kernel vs fp64 %.3e   fp32 restatement vs fp64 %.3e   ratio %s' % (name, q, err, yard, '%.2f' % (err / yard) if yard else ('0/0' if not err else 'inf')))
    assert all(err <= 4 * yard for err, yard in worst.values()), (name, worst)
    if case['grad']:
        assert (bits(o['dlogits'][~in_table]) << 1 == 0).all(), (name, 'dlogits of subgraphs outside the class tables')      # exactly zero
    # ---- the head's backward from the kernel's own dlogits
    if case['out'] == 'none':
        return
    dW, dWs, db, dbs, G, Gs = hr.bwd64(d['H'], d['crow'], set_off, d['Wl'], o['dlogits'])
    expect_nan = np.ones((sets, S.stride), bool)
    for t in range(sets):
        K = int(set_off[t + 1] - set_off[t])
        within(o['dparams'][t, S.wl_off:S.wl_off + Cn * hc], dW[t].reshape(-1), dWs[t].reshape(-1), K, (name, t, 'dWl'))
        within(o['dparams'][t, S.bl_off:S.bl_off + Cn], db[t], dbs[t], K, (name, t, 'dbl'))
        expect_nan[t, S.wl_off:S.wl_off + Cn * hc] = False; expect_nan[t, S.bl_off:S.bl_off + Cn] = False
    assert np.isnan(o['dparams'][expect_nan]).all(), (name, 'dparams outside Wl / bl')
    if 'next' in o:
        g = o['dparams'].astype(f64); cur = S.cur.astype(f64)
        want = cur - f64(f32(LR)) * g
        tol = 2 * U * (np.abs(cur) + np.abs(f64(f32(LR)) * g))
        ok = ~expect_nan
        assert (np.abs(o['next'].astype(f64) - want)[ok] <= tol[ok]).all(), (name, 'SGD step')
        assert np.isnan(o['next'][expect_nan]).all(), (name, 'SGD step outside Wl / bl')
    if 'Gc' in o:
        within(o['Gc'], G.reshape(-1, Hd), Gs.reshape(-1, Hd), Cn, (name, 'Gc'))
        return
    dQ, dQs, hit = hr.scatter_dq(G, Gs, d['crow'], len(d['H']))
    assert np.isnan(o['dQ'][~hit]).all(), (name, 'dQ rows that are no centre were written')
    within(o['dQ'][hit], dQ[hit], dQs[hit], Cn, (name, 'dQ'))
    if 'amax' in o:
        am = o['amax'].reshape(sets, BOUND_PAD)
        assert (am[:, 1:] == PAD_WORD).all(), (name, 'amax padding')
        for t in range(sets):
            rows_t = np.unique(d['crow'][int(set_off[t]):int(set_off[t + 1])])
            m = np.abs(o['dQ'][rows_t]).max()
            assert am[t, 0] == (bits(np.array([m], f32))[0] if m > 0 else 0), (name, t, 'dq_amax', hex(int(am[t, 0])), m)


@pytest.mark.parametrize('case', hr.CASES, ids=[c['name'] for c in hr.CASES])
def test_head_loss_launch_against_fp64_on_every_path(case):
    S = Setup(case)
    base = S.launch(*LAUNCHES[0])
    check_against_fp64(S, base)
    for stage, threads, path in LAUNCHES[1:]:
        o = S.launch(stage, threads, path)
        for k, v in base.items():
            if k == 'next' and path == 1:
                continue                                        # the unfused backward has no SGD step
            assert np.array_equal(bits(o[k]), bits(v)), (case['name'], (stage, threads, path), k, int((bits(o[k]) != bits(v)).sum()))


def test_head_loss_export_refuses_bad_arguments():
    S = Setup(hr.CASES[0])
    lib, _lib, d, case = S.lib, S._lib, S.d, S.case
    Cn, Hd = case['C'], case['Hd']
    z = lambda *shape: torch.zeros(shape, device='cuda')
    logits, dlogits, loss, acc, dpar, dQ, Gc = z(d['subs'], Cn), z(d['subs'], Cn), z(S.sets), z(S.sets), z(S.sets, S.stride), z(d['rows'], Hd), z(d['subs'], Hd)
    protos = z(S.sets, 3, Cn); nxt = z(S.sets, S.stride); am = torch.zeros(S.sets * BOUND_PAD, dtype=torch.int32, device='cuda')
    good = dict(b=S.B.handle, H=S.dH, Hd=Hd, nc=1, compact=0, C=Cn, params=S.dpar, pstride=S.stride, wl=S.wl_off, bl=S.bl_off, centre=None, y=d['y'], mode=0, ns=2,
                protos=None, c_task=0, sl=None, sc=None, logits=logits, dlogits=dlogits, dprotos=None, pout=None, loss=loss, acc=acc, bwd=1, dpar=dpar,
                dstride=S.stride, dQ=dQ, Gc=None, cur=None, nxt=None, sstride=S.stride, lr=0.1, am=None, path=0, launched=None)
    order = list(good)

    def call(**over):
        a = dict(good); a.update(over)
        args = [a[k] if k == 'b' or isinstance(a[k], (int, float)) else _lib.ptr(a[k]) for k in order]
        return lib.gm_dense_head_loss(*args, _lib.stream_ptr())

    assert call() == 0
    for what, over in (('dQ with Gc', dict(Gc=Gc)), ('bwd without dQ / Gc', dict(dQ=None)), ('bwd without dlogits', dict(dlogits=None)),
                       ('mode 1 without protos', dict(mode=1, c_task=3)), ('mode 0 with protos', dict(protos=protos)), ('dprotos in mode 0', dict(dprotos=protos)),
                       ('dQ without bwd', dict(bwd=0)), ('SGD on the unfused path', dict(cur=S.dcur, nxt=nxt, path=1)), ('SGD without cur', dict(nxt=nxt)),
                       ('dq_amax without dQ', dict(am=am, dQ=None, Gc=Gc)), ('nc the batch does not have', dict(nc=2)), ('path', dict(path=2)),
                       ('short dparam_stride', dict(dstride=S.stride - 6)), ('overlapping Wl and bl', dict(bl=S.wl_off + 1)), ('n_support 0', dict(ns=0)),
                       ('support classes outside ragged mode 1', dict(sl=np.zeros(3, np.int32), sc=np.ones(3, np.int32))),
                       ('a class with fewer rows than n_support', dict(ns=5)), ('NULL H', dict(H=None))):
        assert call(**over) == GM_EINVAL, what
        assert lib.gm_last_error(), what
    assert call(C=65) == GM_ERANGE and call(Hd=0) == GM_ERANGE
