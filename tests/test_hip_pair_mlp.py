"""GPU (-m gpu): the BUDDY pair predictor (gm_prop_pair_mlp_forward, gm_prop_pair_mlp_step, gmeta_amd.PairPredictor) against the float64 restatement of the
definition (tests/pair_mlp_ref.py; the definition itself is in include/gmeta_hip.h).  Logits, loss and every gradient are held to the DERIVED tolerance
ref.bound (no measurement; the tests print the worst error / bound ratio); everything the definition promises bit for bit is compared as bits.  The cases
(ref.CASES) are a pruned cross product over the graphs of the hop-feature tests, sized by the kernels' own pair tile (gm_prop_pair_mlp_tile)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hop_feature_ref as hop
import pair_mlp_ref as ref
from test_hip_pair_pagerank import _stream, tuning

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = -7.5
PAD = 64


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def tile():
    from gmeta_amd import _lib
    return int(_lib.lib().gm_prop_pair_mlp_tile())


@functools.lru_cache(maxsize=None)
def made(which, F, weighted):
    import gmeta_amd
    N, src, dst, w = ref.graph(which)
    X = hop.features(N, F, 100 + F)
    store = gmeta_amd.GraphStore([(N, src, dst)], [X], edge_weights=[w] if weighted else None)
    g = hop.csr(N, src, dst, w if weighted else None)
    assert np.array_equal(store.host_csr[0][0], g[0]) and np.array_equal(store.host_csr[0][1], g[1])
    return store, g, X


@functools.lru_cache(maxsize=None)
def want_levels(which, F, weighted, self_loops, hops):
    """-> float64 [hops + 1, N, F] levels by the definition and their tolerance, computed once and left unchanged"""
    _, g, X = made(which, F, weighted)
    x, E = hop.levels(*g, X, hops, self_loops), hop.bound(*g, X, hops, self_loops)
    x.setflags(write=False); E.setflags(write=False)
    return x, E


@functools.lru_cache(maxsize=None)
def case(i):
    """-> inputs of case i, its float64 reference and its bound"""
    c = ref.CASES[i]
    inp = ref.case_inputs(c, tile())
    x, E = want_levels(c[0], c[1], c[7], c[8], c[2])
    want = ref.evaluate(x, inp['pairs'], inp['op'], inp['extra'], inp['params'], inp['Hd'], inp['labels'])
    tol = ref.bound(x, E, inp['pairs'], inp['op'], inp['extra'], inp['params'], inp['Hd'], inp['labels'])
    return inp, want, tol


class handle:
    """gm_store_propagate_build through the C ABI, destroyed at the end of the block; .forward / .step are the C ABI itself with poisoned outputs."""

    def __init__(self, store, hops, self_loops):
        from gmeta_amd import _lib
        self.lib = _lib
        self.h = C.c_void_p()
        _lib.check(_lib.lib().gm_store_propagate_build(store.handle, 0, hops, 1 if self_loops else 0, _lib.stream_ptr(), C.byref(self.h)), 'gm_store_propagate_build')
        self.K0 = (hops + 1) * store.feat_dim

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.lib().gm_prop_destroy(self.h)
        self.h = None
        return False

    def _dev(self, pairs, extra, params):
        p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.int32)
        n = len(p)
        d_p = torch.from_numpy(p).cuda() if n else None
        S = 0 if extra is None else np.asarray(extra).shape[1]
        d_e = torch.from_numpy(np.ascontiguousarray(extra, f32)).cuda() if (S and n) else None
        d_w = torch.from_numpy(np.ascontiguousarray(params, f32)).cuda()
        return d_p, d_e, d_w, n, S

    def forward(self, pairs, op, extra, params, Hd, stream=None):
        """float32 [n] logits; PAD poisoned floats in front of them and behind them must stay poisoned"""
        lib, P = self.lib.lib(), self.lib.ptr
        d_p, d_e, d_w, n, S = self._dev(pairs, extra, params)
        out = torch.full((PAD + n + PAD,), POISON, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        self.lib.check(lib.gm_prop_pair_mlp_forward(self.h, P(d_p), n, ref.hop.OPS.index(op), P(d_e), S, P(d_w), Hd, P(out[PAD:]), _stream(stream)), 'gm_prop_pair_mlp_forward')
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert (out[:PAD] == POISON).all() and (out[PAD + n:] == POISON).all()
        return out[PAD:PAD + n]

    def step(self, pairs, op, extra, labels, params, Hd, stream=None, logits=True):
        """-> logits [n] (or None), loss (fp32 scalar), grad [n_params]; all three buffers poisoned beforehand, with PAD floats in front and behind that must stay so"""
        lib, P = self.lib.lib(), self.lib.ptr
        d_p, d_e, d_w, n, S = self._dev(pairs, extra, params)
        n_params = len(params)
        d_y = torch.from_numpy(np.ascontiguousarray(labels, f32)).cuda() if n else None
        lg = torch.full((PAD + n + PAD,), POISON, dtype=torch.float32, device='cuda')
        ls = torch.full((PAD + 1 + PAD,), POISON, dtype=torch.float32, device='cuda')
        gr = torch.full((PAD + n_params + PAD,), POISON, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        self.lib.check(lib.gm_prop_pair_mlp_step(self.h, P(d_p), n, ref.hop.OPS.index(op), P(d_e), S, P(d_y), P(d_w), Hd, P(lg[PAD:]) if logits else None, P(ls[PAD:]), P(gr[PAD:]),
                                                 _stream(stream)), 'gm_prop_pair_mlp_step')
        torch.cuda.synchronize()
        lg, ls, gr = lg.cpu().numpy(), ls.cpu().numpy(), gr.cpu().numpy()
        for buf, m in ((lg, n if logits else -PAD), (ls, 1), (gr, n_params)):
            assert (buf[:PAD] == POISON).all() and (buf[PAD + m:] == POISON).all()
        return (lg[PAD:PAD + n] if logits else None), ls[PAD], gr[PAD:PAD + n_params]


def ratio(got, want, tol):
    """the worst |got - want| / tol, with 0 / 0 = 0; asserts got within tol"""
    err = np.abs(np.asarray(got, np.float64) - want)
    tol = np.asarray(tol, np.float64)
    assert np.isfinite(np.asarray(got, np.float64)).all()
    assert (err <= tol).all(), 'worst error / bound %.3f' % float((err / np.maximum(tol, 1e-300)).max())
    return float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0


def check_step(inp, want, tol, lg, ls, gr, tag):
    K, Hd = inp['K'], inp['Hd']
    r = {'logits': ratio(lg, want['logits'], tol['logits']), 'loss': ratio(ls, want['loss'], tol['loss'])}
    cut = {'dW1': (0, K * Hd), 'db1': (K * Hd, K * Hd + Hd), 'dw2': (K * Hd + Hd, K * Hd + 2 * Hd), 'db2': (K * Hd + 2 * Hd, K * Hd + 2 * Hd + 1)}
    for name, (a, b) in cut.items():
        r[name] = ratio(gr[a:b], want['grad'][a:b], tol['grad'][a:b])
    print('%s: worst error / bound  %s' % (tag, '  '.join('%s %.2g' % kv for kv in r.items())))


# ---------------------------------------------------------------------------------------------------- against the restatement, C ABI and PairPredictor
@pytest.mark.parametrize('i', range(len(ref.CASES)), ids=ref.CASE_IDS)
def test_logits_loss_and_gradients_within_the_derived_bound(i):
    import gmeta_amd
    inp, want, tol = case(i)
    c = ref.CASES[i]
    store, _, _ = made(c[0], c[1], c[7])
    n, Hd, op = inp['n'], inp['Hd'], inp['op']
    with handle(store, inp['hops'], inp['self_loops']) as p:
        fw = p.forward(inp['pairs'], op, inp['extra'], inp['params'], Hd)
        lg, ls, gr = p.step(inp['pairs'], op, inp['extra'], inp['labels'], inp['params'], Hd)
        _, ls2, gr2 = p.step(inp['pairs'], op, inp['extra'], inp['labels'], inp['params'], Hd, logits=False)
    assert np.array_equal(bits(fw), bits(lg))                                                       # forward and step: the same tile code
    assert np.array_equal(bits(gr), bits(gr2)) and bits(ls) == bits(ls2)                            # two calls, one knob: the same bits
    if n == 0:
        assert ls == 0.0 and not gr.any() and len(fw) == 0
    else:
        assert np.abs(gr).max() > 0 and ls > 0
    check_step(inp, want, tol, lg, ls, gr, ref.CASE_IDS[i])
    # through PairPredictor: the same calls, hence the same bits
    model = gmeta_amd.PairPredictor(inp['F'], inp['hops'], hidden=Hd, extra_dim=inp['S'], op=op, seed=3)
    assert model.params.shape == (len(inp['params']),) and model.W1.shape == (inp['K'], Hd) and model.b2.shape == (1,)
    model.params.data.copy_(torch.from_numpy(inp['params']))
    with store.propagated_features(0, hops=inp['hops'], self_loops=inp['self_loops']) as props:
        sc = model.scores(props, inp['pairs'], inp['extra'])
        sct = model.scores(props, inp['pairs'], None if inp['extra'] is None else torch.from_numpy(inp['extra']).cuda(), as_torch=True)
        loss = model.step(props, inp['pairs'], inp['labels'], None if inp['extra'] is None else inp['extra'].astype(np.float64))
    assert sct.is_cuda and np.array_equal(bits(sc), bits(fw)) and np.array_equal(bits(sct.cpu().numpy()), bits(fw))
    assert bits(f32(loss)) == bits(ls) and np.array_equal(bits(model.params.grad.cpu().numpy()), bits(gr))


# ---------------------------------------------------------------------------------------------------- what the definition promises bit for bit
def test_a_logit_is_the_same_bits_alone_in_any_batch_and_for_both_orientations():
    i = 1                                                                                           # F 300, hops 3, S 25, Hd 256, n = 3 T + 7
    inp, _, _ = case(i)
    c = ref.CASES[i]
    store, _, _ = made(c[0], c[1], c[7])
    T, n, Hd, op = tile(), inp['n'], inp['Hd'], inp['op']
    with handle(store, inp['hops'], inp['self_loops']) as p:
        full = p.forward(inp['pairs'], op, inp['extra'], inp['params'], Hd)
        flip = p.forward(inp['pairs'][:, ::-1], op, inp['extra'], inp['params'], Hd)
        assert np.array_equal(bits(full), bits(flip))
        for k in (0, 1, T - 1, T, T + 1, 2 * T + 5, n - 1):
            alone = p.forward(inp['pairs'][k:k + 1], op, inp['extra'][k:k + 1], inp['params'], Hd)
            assert bits(alone[0]) == bits(full[k]), k
        perm = np.random.default_rng(5).permutation(n)                                              # another place in another batch
        mixed = p.forward(inp['pairs'][perm], op, inp['extra'][perm], inp['params'], Hd)
        assert np.array_equal(bits(mixed), bits(full[perm]))
        part = p.forward(inp['pairs'][7:T + 9], op, inp['extra'][7:T + 9], inp['params'], Hd)
        assert np.array_equal(bits(part), bits(full[7:T + 9]))


def test_duplicate_pairs_with_equal_columns_share_their_bits():
    i = 4                                                                                           # S = 0: rows 1 and 2 of case_pairs are the same input
    inp, _, _ = case(i)
    c = ref.CASES[i]
    store, _, _ = made(c[0], c[1], c[7])
    with handle(store, inp['hops'], inp['self_loops']) as p:
        lg = p.forward(inp['pairs'], inp['op'], None, inp['params'], inp['Hd'])                     # S = 0 with extra = NULL
    assert bits(lg[1]) == bits(lg[2]) and bits(lg[3]) == bits(lg[4])                               # the duplicate; the two orientations


def test_logits_do_not_depend_on_pair_mlp_rows_or_the_stream_and_sums_only_on_the_knob():
    i = 5                                                                                           # chain, F 100, n = 3 T + 7
    inp, want, tol = case(i)
    c = ref.CASES[i]
    store, _, _ = made(c[0], c[1], c[7])
    T, Hd, op = tile(), inp['Hd'], inp['op']
    side = torch.cuda.Stream()
    seen = {}
    with handle(store, inp['hops'], inp['self_loops']) as p:
        fw = p.forward(inp['pairs'], op, inp['extra'], inp['params'], Hd)
        assert np.array_equal(bits(p.forward(inp['pairs'], op, inp['extra'], inp['params'], Hd, stream=side)), bits(fw))
        for rows in (0, 1, T, 2 ** 30):
            with tuning(pair_mlp_rows=rows):
                lg, ls, gr = p.step(inp['pairs'], op, inp['extra'], inp['labels'], inp['params'], Hd)
                lg2, ls2, gr2 = p.step(inp['pairs'], op, inp['extra'], inp['labels'], inp['params'], Hd, stream=side)
            assert np.array_equal(bits(lg), bits(fw)) and np.array_equal(bits(lg2), bits(fw))
            assert np.array_equal(bits(gr), bits(gr2)) and bits(ls) == bits(ls2)                    # one knob: the same bits, on any stream
            check_step(inp, want, tol, lg, ls, gr, 'pair_mlp_rows %d' % rows)                       # across knobs: each within the bound of the definition
            seen[rows] = (ls, gr)
    assert np.array_equal(bits(seen[0][1]), bits(seen[2 ** 30][1]))                                 # n < the library's choice: one chunk either way
    for a in seen:                                                                                  # across knobs: loss and gradients agree within the bound
        for b in seen:
            assert abs(float(seen[a][0]) - float(seen[b][0])) <= tol['loss'], (a, b)
            assert (np.abs(seen[a][1].astype(np.float64) - seen[b][1]) <= tol['grad']).all(), (a, b)
    from gmeta_amd import _lib
    assert _lib.lib().gm_get_tuning(b'pair_mlp_rows') == 0


def test_a_short_last_chunk_behind_a_chunk_of_more_than_262144_rows():
    """pair_mlp_rows = 262,272 and n = 262,272 + 262,144: the full chunk's ranges are 1,056 rows long (249 of them), and ranges of 1,024 rows would cut the last
    chunk into 256 -- more than the scratch of the partials holds.  The call keeps ONE range length, so the last chunk has 249 too.  A narrow model (K = 11,
    Hd = 8) keeps it quick; logits, loss and gradients against the restatement, and the logits against a plain forward."""
    c = ('chain', 5, 1, 1, 8, (0, 0), 'abs_diff', False, True)
    R = 262272
    n = R + 262144
    inp = ref.case_inputs(c, tile())
    store, _, _ = made(c[0], c[1], c[7])
    x, E = want_levels(c[0], c[1], c[7], c[8], c[2])
    rng = np.random.default_rng(12)
    pairs, extra, labels = ref.case_pairs(inp['N'], n, 13), rng.integers(0, 6, (n, 1)).astype(f32), (rng.random(n) < 0.5).astype(f32)
    want = ref.evaluate(x, pairs, inp['op'], extra, inp['params'], inp['Hd'], labels)
    tol = ref.bound(x, E, pairs, inp['op'], extra, inp['params'], inp['Hd'], labels)
    assert float(tol['near'].mean()) <= 0.01
    with handle(store, inp['hops'], inp['self_loops']) as p:
        fw = p.forward(pairs, inp['op'], extra, inp['params'], inp['Hd'])
        with tuning(pair_mlp_rows=R):
            lg, ls, gr = p.step(pairs, inp['op'], extra, labels, inp['params'], inp['Hd'])
            _, ls2, gr2 = p.step(pairs, inp['op'], extra, labels, inp['params'], inp['Hd'], logits=False)
    assert np.array_equal(bits(lg), bits(fw)) and np.array_equal(bits(gr), bits(gr2)) and bits(ls) == bits(ls2)
    check_step(dict(inp, n=n), want, tol, lg, ls, gr, 'pair_mlp_rows %d, n %d' % (R, n))


def test_a_logit_equals_b2_exactly_when_w2_is_zero():
    i = 3
    inp, _, _ = case(i)
    c = ref.CASES[i]
    store, _, _ = made(c[0], c[1], c[7])
    K, Hd = inp['K'], inp['Hd']
    params = inp['params'].copy()
    params[K * Hd + Hd:K * Hd + 2 * Hd] = 0.0
    with handle(store, inp['hops'], inp['self_loops']) as p:
        lg = p.forward(inp['pairs'], inp['op'], inp['extra'], params, Hd)
    assert params[-1] != 0 and (bits(lg) == bits(params[-1])).all()


# ---------------------------------------------------------------------------------------------------- errors
def test_argument_errors_return_their_code_and_write_nothing():
    import gmeta_amd
    from gmeta_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    store, _, _ = made('chain', 64, False)
    st = _lib.stream_ptr()
    n, S, Hd, hops = 5, 3, 8, 1
    K = (hops + 1) * 64 + S
    n_params = K * Hd + 2 * Hd + 1

    def fails(rc, text):
        assert rc == -1, rc
        msg = lib.gm_last_error().decode()
        assert text in msg, msg

    with handle(store, hops, True) as p:
        k, npar = C.c_int32(), C.c_int64()
        assert lib.gm_prop_pair_mlp_dims(p.h, S, Hd, C.byref(k), C.byref(npar)) == 0 and (k.value, npar.value) == (K, n_params)
        assert lib.gm_prop_pair_mlp_dims(p.h, S, Hd, None, None) == 0
        fails(lib.gm_prop_pair_mlp_dims(None, S, Hd, C.byref(k), C.byref(npar)), 'prop is NULL')
        fails(lib.gm_prop_pair_mlp_dims(p.h, S, 0, C.byref(k), C.byref(npar)), 'Hd = 0')
        fails(lib.gm_prop_pair_mlp_dims(p.h, 257, Hd, C.byref(k), C.byref(npar)), 'S = 257')
        d_p = torch.zeros((n, 2), dtype=torch.int32, device='cuda')
        d_e = torch.zeros((n, S), dtype=torch.float32, device='cuda')
        d_y = torch.zeros((n,), dtype=torch.float32, device='cuda')
        d_w = torch.zeros((n_params,), dtype=torch.float32, device='cuda')
        lg = torch.full((n,), POISON, dtype=torch.float32, device='cuda')
        ls = torch.full((1,), POISON, dtype=torch.float32, device='cuda')
        gr = torch.full((n_params,), POISON, dtype=torch.float32, device='cuda')

        def fwd(h=p.h, pairs=d_p, n=n, op=0, e=d_e, S=S, w=d_w, Hd=Hd, out=lg):
            return lib.gm_prop_pair_mlp_forward(h, P(pairs), n, op, P(e), S, P(w), Hd, P(out), st)

        def step(h=p.h, pairs=d_p, n=n, op=0, e=d_e, S=S, y=d_y, w=d_w, Hd=Hd, out=lg, loss=ls, grad=gr):
            return lib.gm_prop_pair_mlp_step(h, P(pairs), n, op, P(e), S, P(y), P(w), Hd, P(out), P(loss), P(grad), st)

        for call in (fwd, step):
            fails(call(h=None), 'prop is NULL')
            fails(call(Hd=0), 'Hd = 0'); fails(call(Hd=257), 'Hd = 257'); fails(call(Hd=-3), 'Hd = -3')
            fails(call(S=-1), 'S = -1'); fails(call(S=257), 'S = 257')
            fails(call(op=2), 'op = 2'); fails(call(op=-1), 'op = -1')
            fails(call(n=-1), 'n = -1'); fails(call(n=2 ** 31), 'n = 2147483648')
            fails(call(pairs=None), 'NULL argument'); fails(call(w=None), 'NULL argument'); fails(call(e=None), 'NULL argument')
        fails(fwd(out=None), 'd_logits is NULL')
        fails(step(y=None), 'd_labels is NULL'); fails(step(loss=None), 'NULL argument'); fails(step(grad=None), 'NULL argument')
        fails(step(n=0, loss=None), 'NULL argument')
        with tuning(pair_mlp_rows=-1):
            fails(step(), 'pair_mlp_rows = -1')
        torch.cuda.synchronize()
        assert (lg == POISON).all() and (ls == POISON).all() and (gr == POISON).all()               # nothing was written
        assert fwd(n=0, pairs=None, e=None, w=None, out=None) == 0                                  # n = 0: a no-op with NULL pointers too
        assert step(out=None) == 0 and fwd() == 0                                                   # after the errors: good calls are unaffected
        torch.cuda.synchronize()
        assert torch.isfinite(lg).all() and torch.isfinite(gr).all() and torch.isfinite(ls).all()

    # the Python layer: ValueErrors that name the value
    model = gmeta_amd.PairPredictor(64, 1, hidden=8, extra_dim=S)
    pairs = np.array([[0, 1], [2, 3]])
    ex = np.zeros((2, S), f32)
    with store.propagated_features(0, hops=1) as props, store.propagated_features(0, hops=2) as deeper:
        with pytest.raises(ValueError, match=r'hops = 2; the predictor has feat_dim = 64, hops = 1'):
            model.scores(deeper, pairs, ex)
        with pytest.raises(ValueError, match=r'extra of shape \(2, 4\); \[2, 3\]'):
            model.scores(props, pairs, np.zeros((2, 4), f32))
        with pytest.raises(ValueError, match=r'extra of dtype int64'):
            model.scores(props, pairs, np.zeros((2, S), np.int64))
        with pytest.raises(ValueError, match=r'torch.float64'):
            model.scores(props, pairs, torch.zeros((2, S), dtype=torch.float64, device='cuda'))
        with pytest.raises(ValueError, match=r'extra is None; the predictor has extra_dim = 3'):
            model.scores(props, pairs)
        with pytest.raises(ValueError, match=r'label outside \[0, 1\] \(min 0.0, max 1.5\)'):
            model.step(props, pairs, [0.0, 1.5], ex)
        with pytest.raises(ValueError, match=r'node id outside the graph'):
            model.scores(props, [[0, 331]], ex[:1])
        assert model.params.grad is None
        closed = props
    with pytest.raises(ValueError, match=r'closed'):
        model.scores(closed, pairs, ex)
    with pytest.raises(ValueError, match=r'feat_dim = 32'):
        with made('chain', 5, False)[0].propagated_features(0, hops=1) as narrow:
            gmeta_amd.PairPredictor(32, 1).scores(narrow, pairs)
    for bad, text in ((dict(hidden=0), 'hidden = 0'), (dict(hidden=257), 'hidden = 257'), (dict(extra_dim=-1), 'extra_dim = -1'), (dict(op='sum'), "op = 'sum'"),
                      (dict(hops=0), 'hops = 0')):
        kw = dict(feat_dim=8, hops=1)
        kw.update(bad)
        with pytest.raises(ValueError, match=text):
            gmeta_amd.PairPredictor(**kw)


# ---------------------------------------------------------------------------------------------------- training
def test_fit_on_a_planted_two_community_graph_learns_and_replays_bit_for_bit():
    import gmeta_amd
    rng = np.random.default_rng(9)
    N, F = 200, 16
    side = np.arange(N) >= N // 2
    cand = rng.integers(0, N, (6000, 2))
    cand = cand[cand[:, 0] != cand[:, 1]]
    same = side[cand[:, 0]] == side[cand[:, 1]]
    edges = np.unique(np.sort(cand[same | (rng.random(len(cand)) < 0.03)][:1200], axis=1), axis=0)
    X = (rng.standard_normal((N, F)) + np.where(side, 1.0, -1.0)[:, None]).astype(f32)             # the community shows in the features' mean
    src, dst = np.concatenate([edges[:, 0], edges[:, 1]]), np.concatenate([edges[:, 1], edges[:, 0]])
    store = gmeta_amd.GraphStore([(N, src, dst)], [X])
    neg = store.negative_pairs(0, len(edges), seed=5)
    names = ['0_%d_%d' % (a, b) for a, b in np.concatenate([edges, neg]).tolist()]
    labels = np.concatenate([np.ones(len(edges)), np.zeros(len(neg))])
    curves = []
    with store.propagated_features(0, hops=2) as props:
        for _ in range(2):
            model = gmeta_amd.PairPredictor(F, 2, hidden=32, seed=11)
            before = model.auc([props], names, labels)
            curve = model.fit([props], names, labels, epochs=6, batch=500, lr=0.01)
            after = model.auc([props], names, labels)
            curves.append(curve)
            print('planted graph: %d edges, AUC %.4f -> %.4f, loss %.4f -> %.4f' % (len(edges), before, after, curve[0], curve[-1]))
            assert after > before and curve[-1] < curve[0] and len(curve) == 6
    assert np.array_equal(np.asarray(curves[0], np.float64).view(np.uint64), np.asarray(curves[1], np.float64).view(np.uint64))


def test_train_driver_fits_and_reports_the_buddy_auc(tmp_path, capsys):
    import gmeta_amd
    from gmeta_amd import datadir, synth
    from test_hip_pair_scores import DRIVER, _positives_only, _splits
    import train as drv
    d = synth.link_dataset(2, 60, 2, 5, seed=11, inject_negatives=False)
    pos, info1 = _positives_only(d)
    root = str(tmp_path / 'pos')
    datadir.write_datadir(root, d['graphs'], d['feats'], info1, _splits({'tables': pos}))
    base = ['--data_dir', root + '/'] + DRIVER + ['--negatives', 'uniform', '--mask_target', '1', '--link_hops', 'symmetric']
    res = drv.main(drv.parse(base + ['--buddy', '3', '--heuristics', '1']))
    text = capsys.readouterr().out
    assert 0.0 <= res['buddy_auc'] <= 1.0 and 'BUDDY test AUC: %.4f' % res['buddy_auc'] in text
    assert text.index('Heuristic test AUC:') < text.index('BUDDY test AUC:')
    # the same fit by hand over the completed tables: seeded, hence the same number
    from gmeta_amd.negatives import read_link_tables
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    tables, _ = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root + '/'), info1, mode='uniform')
    assert drv.buddy_auc(store, tables['train'], tables['test'], 3) == res['buddy_auc']
    plain = drv.main(drv.parse(base + ['--heuristics', '1']))
    text = capsys.readouterr().out
    assert 'BUDDY' not in text and plain == {k: v for k, v in res.items() if k != 'buddy_auc'}     # the flag changes nothing else
