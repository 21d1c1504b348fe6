"""GPU (-m gpu): GM_DEAD_ROWS=3 -- the passes nobody differentiates stop forming and storing rows no centre reads.

All anyone reads of a forward-only pass (the query evaluations of a meta-step, the evaluation leg, Meta.predict) is H_L at the centre rows.  So Z_L is
observable at the centre rows only, and H_{L-1} and Z_{L-1} only at the sources of the centres' in-edges.  At 3 (the default) the fused loaders read
through per-batch tables that send every other row to the zero row, the partial aggregates form the observable rows only (a +-1 flag vector with
keep_signed: a scale of exactly 1), and the update below the last stores the rows GM_F_NORM_E1 keeps.  Every tile and every MFMA is still issued and no
product or sum that reaches a stored value is dropped or reordered, so everything below is compared BITWISE.

Fixtures: the worlds of tests/test_hip_dead_rows_bwd.py, rebuilt here (20,000-node preferential-attachment graph, m = 7, F0 128, hidden 256, h = 2, 8 tasks,
K = 2, sample_nodes 160, every edge stored both ways; the same graph stored low id -> high id with the forced-split knobs), and two joined 300-leaf stars for
the kernels alone: there the 301-edge hub rows are split over two workgroups, one kept and one flagged."""
import argparse
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, K_STEPS = 8, 2
SENTINEL = 0x7fc12345      # a NaN no kernel produces: "this output row was never stored"
FUSE_ZERO, FUSE_SELF, MAXDEG = 0x20000000, 0x40000000, 2
ONE = 0x3f800000


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


def _world(both_directions):
    import gmeta_amd
    from gmeta_amd import synth
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args('arxiv', task_num=T, k_qry=4, update_step=K_STEPS, sample_nodes=160 if both_directions else 1000)
    data = synth.node_dataset(20000, 7, cfg['F0'], cfg['classes'], both_directions=both_directions)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=3, k_shot=3, k_query=4, batchsz=T, args=args, adjs=store, h=2,
                             tables={'train': (data['names'], data['labels'])}, verbose=False)
    batch = db.get_batch(list(range(T)))
    force = {} if both_directions else dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
    one = db.get_batch([0])      # the first task alone: what Meta.finetunning evaluates
    return dict(args=args, cfg=cfg, store=store, db=db, batch=batch, one=one, S=batch[0][0].view_of, Q=batch[2][0].view_of, force=force, results={})


N_LEAF = 300


def _star():
    """Hubs A = 0 and B = 1 joined by an edge, 300 leaves each, every edge stored both ways; one set of five subgraphs around A, two of A's leaves, B and one
    of B's leaves.  Around A the subgraph holds all 602 nodes: A's own row (301 in-edges) is the centre and not the source of an edge into it (there is no
    self-loop), B's row (301 in-edges) is no centre and the source of one."""
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    la, lb = 2 + np.arange(N_LEAF), 2 + N_LEAF + np.arange(N_LEAF)
    u = np.concatenate([np.zeros(N_LEAF, np.int64), np.ones(N_LEAF, np.int64), [0]])
    v = np.concatenate([la, lb, [1]])
    n = 2 + 2 * N_LEAF
    feats = [np.random.default_rng(3).standard_normal((n, 128)).astype(np.float32)]
    store = gmeta_amd.GraphStore([(n, np.concatenate([u, v]), np.concatenate([v, u]))], feats)
    seeds = [(0, c, -1) for c in (0, 2, 3, 1, 2 + N_LEAF)]
    B = SubgraphBatch.extract(store, seeds, [0, len(seeds)], 2, 1000, 222, False)
    return dict(store=store, S=B, Q=B, force={}, cfg=dict(hidden=256, F0=128))


@pytest.fixture(scope='module')
def undirected():
    return _world(True)


@pytest.fixture(scope='module')
def directed():
    return _world(False)


@pytest.fixture(scope='module')
def star():
    return _star()


@pytest.fixture(params=['undirected', 'directed'])
def world(request):
    return request.getfixturevalue(request.param)


@pytest.fixture(params=['undirected', 'directed', 'star'])
def kworld(request):
    return request.getfixturevalue(request.param)


def _n_tiles(B):
    so = [int(v) for v in B.sub_off[B.set_sub_off]]
    return sum((so[t + 1] - so[t] + 127) // 128 for t in range(B.sets))


def _need_split(w, *batches):
    """The paths under test run where the split kernels engage: n_tiles >= CUs / 4 (unless the fixture forces them)."""
    if w['force']:
        return
    need = torch.cuda.get_device_properties(0).multi_processor_count // 4
    for B in batches:
        if _n_tiles(B) < need:
            pytest.skip('batch of %d row tiles is below the split threshold of this device (%d)' % (_n_tiles(B), need))


def _centre_rows(B):
    from gmeta_amd import _lib
    return (B.sub_off[:-1].astype(np.int64)[:, None] + B._read(_lib.F_CENTRE, B.subs * B.centres, np.int32).reshape(B.subs, B.centres)).reshape(-1)


def _sets(B):
    """(is_centre [rows], e1 [rows]: the row is the source of an in-edge of a centre) from the in-edge CSR and the centre rows."""
    ip, ix = B.csr()
    ip = ip.astype(np.int64)
    is_c = np.zeros(B.rows, bool); is_c[_centre_rows(B)] = True
    dst = np.repeat(np.arange(B.rows), np.diff(ip))
    e1 = np.zeros(B.rows, bool); e1[ix[is_c[dst]]] = True
    return is_c, e1


def _source_tables(B):
    """gm_batch's per-row source tables recomputed from the in-edge CSR, the norms and the feature rows: (over batch rows, over feature rows), [rows, 4] uint32."""
    from gmeta_amd import _lib
    ip, ix = B.csr()
    ip = ip.astype(np.int64); ix = ix.astype(np.int64)
    deg = np.diff(ip)
    norm = B._read(_lib.F_NORM, B.rows, np.float32).view(np.uint32)
    frow = B._read(_lib.F_FEAT_ROW, B.rows, np.int32).astype(np.int64)
    r = np.arange(B.rows)
    t = np.zeros((B.rows, 4), np.uint32)
    t[:, 0] = t[:, 1] = r | FUSE_SELF; t[:, 2] = ONE                      # more than two sources: the row's own finished row
    z = deg == 0
    t[z, 0] = t[z, 1] = FUSE_ZERO
    few = (deg >= 1) & (deg <= MAXDEG)
    u0 = ix[np.minimum(ip[:-1], len(ix) - 1)]
    u1 = np.where(deg >= 2, ix[np.minimum(ip[:-1] + 1, len(ix) - 1)], u0)
    tf = t.copy()
    t[few, 0] = u0[few]; t[few, 1] = u1[few]
    tf[few, 0] = frow[u0[few]]; tf[few, 1] = frow[u1[few]]
    for tab in (t, tf):
        tab[few, 2] = norm[u0[few]]
        tab[few, 3] = np.where(deg[few] >= 2, norm[u1[few]], 0)
    return t, tf, deg


def _read_table(B, which):
    from gmeta_amd import _lib
    t = torch.empty(B.rows, 4, dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().gm_dense_agg_table(B.handle, which, 0, _lib.ptr(t), B.rows, _lib.stream_ptr()), 'gm_dense_agg_table')
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the tables
def test_tables_equal_their_recomputation(kworld):
    """Tables 7 / 8 / 9 of gm_dense_agg_table carry the source-table entry on the centre rows / on the sources of the centres' in-edges (over batch rows and
    over feature rows) and {ZERO, ZERO, 0, 0} on every other row; GM_F_OBS_CENTRE / GM_F_OBS_E1 are +1 there and -1 elsewhere.  Both from the in-edge CSR and
    the centre rows; the unrestricted tables 4 / 5 are checked against the same recomputation first."""
    from gmeta_amd import _lib
    fused_kept = 0
    for side in ('S', 'Q'):
        B = kworld[side]
        is_c, e1 = _sets(B)
        t, tf, deg = _source_tables(B)
        assert np.array_equal(_read_table(B, 4), t) and np.array_equal(_read_table(B, 5), tf)
        zero = np.array([FUSE_ZERO, FUSE_ZERO, 0, 0], np.uint32)
        for which, keep, src in ((7, is_c, t), (8, e1, t), (9, e1, tf)):
            want = np.where(keep[:, None], src, zero[None, :])
            got = _read_table(B, which)
            bad = np.nonzero((got != want).any(1))[0]
            assert len(bad) == 0, (side, which, bad[:5], got[bad[:5]], want[bad[:5]])
        for field, keep in ((_lib.F_OBS_CENTRE, is_c), (_lib.F_OBS_E1, e1)):
            got = B._read(field, B.rows, np.float32)
            assert np.array_equal(got.view(np.uint32), np.where(keep, 1.0, -1.0).astype(np.float32).view(np.uint32))
        e1_bit = B._read(_lib.F_NORM_E1, B.rows, np.float32).view(np.uint32) >> 31 == 0
        assert np.array_equal(e1_bit, e1)                                 # the same set the backward's flag vector keeps
        # not vacuous: both flags occur on rows the partial aggregate writes ...
        for keep in (is_c, e1):
            assert keep.any() and not keep.all()
            assert (keep & (deg > MAXDEG)).any() and (~keep & (deg > MAXDEG)).any()
        fused_kept += int(((is_c | e1) & (deg >= 1) & (deg <= MAXDEG)).sum())
    # ... and some kept row is one the loaders form (one or two sources) -- but in the directed world, whose kept rows all have no source or at least three
    assert fused_kept > 0 or bool(kworld['force'])


def test_star_holds_split_hub_rows_of_both_flags(star):
    B = star['S']
    is_c, e1 = _sets(B)
    deg = np.diff(B.csr()[0].astype(np.int64))
    split = deg >= 192
    for keep in (is_c, e1):
        assert (split & keep).any() and (split & ~keep).any()


# ---------------------------------------------------------------------------------------------------------------- the step
def _meta(w, config=None, **attrs):
    import gmeta_amd
    from gmeta_amd import synth
    a = argparse.Namespace(**vars(w['args']))
    cfg = w['cfg']
    torch.manual_seed(222)
    m = gmeta_amd.Meta(a, config or synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], cfg['n_way'])).to('cuda')
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _flat(m, grad=False):
    return torch.cat([(p.grad if grad else p.detach()).reshape(-1) for p in m.net.parameters()]).cpu().numpy().copy()


def _run(w, poison_bytes=0, inf_weight=False, config=None, pieces=3, **knobs):
    """One Meta.forward from identical seeds: accuracies, losses_q, the meta-gradient that reached Adam, the parameters before and after its step, and the
    aggregate launches' bytes (category 0 of the launch accounting)."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    if pieces == 2:
        knobs = dict(knobs, GM_SPLIT16_MIN_ROWS=0)
    with tuning(**dict(w['force'], **knobs)):
        lib.gm_set_split_pieces(pieces)
        try:
            m = _meta(w, config)
            cfg = w['cfg']
            if inf_weight:
                with torch.no_grad():
                    W_L = [p for p in m.net.parameters() if p.dim() == 2 and tuple(p.shape) == (cfg['hidden'], cfg['hidden'])]
                    assert len(W_L) == 1
                    W_L[0][3, 5] = float('inf')
            theta0 = _flat(m)
            if poison_bytes:
                m._ws = torch.full((poison_bytes,), 0xFF, dtype=torch.uint8, device='cuda')      # every float of the step's workspace a NaN
            lib.gm_profile_enable(1)
            accs = np.asarray(m(*w['batch'], None)).copy()
            torch.cuda.synchronize()
            ms, n, wk = C.c_double(), C.c_int64(), C.c_int64()
            lib.gm_profile_read(0, C.byref(ms), C.byref(n), C.byref(wk))
            assert not poison_bytes or m._ws.numel() == poison_bytes      # (the step ran in the poisoned block)
        finally:
            lib.gm_profile_enable(0)
            lib.gm_set_split_pieces(3)
    return dict(accs=accs, losses=np.asarray(m.last_stats['losses_q']).copy(), grad=_flat(m, True), theta0=theta0, theta=_flat(m), ws_bytes=m._ws.numel(),
                agg_bytes=int(wk.value), found_inf=float(m._found_inf) if m._found_inf is not None else None)


def _cached(w, name, **kw):
    if name not in w['results']:
        w['results'][name] = _run(w, **kw)
    return w['results'][name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype.itemsize == 1 else 'u%d' % a.dtype.itemsize)


def _assert_bitwise(a, b, keys=('accs', 'losses', 'grad', 'theta')):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize('ref_level', [2, 0])
def test_step_is_bitwise_the_step_of_the_lower_levels(world, ref_level):
    _need_split(world, world['S'], world['Q'])
    on = _cached(world, 'dr3', GM_DEAD_ROWS=3)
    ref = _cached(world, 'dr%d' % ref_level, GM_DEAD_ROWS=ref_level)
    assert np.isfinite(on['grad']).all() and np.isfinite(on['losses']).all()
    assert np.abs(on['grad']).max() > 0
    _assert_bitwise(on, ref)


def test_step_over_a_poisoned_workspace_is_unchanged_and_finite(world):
    """Every byte of the workspace 0xFF before the step at level 3: the rows the forward-only passes no longer write hold NaNs, and no unwritten row reaches
    a stored value."""
    _need_split(world, world['S'], world['Q'])
    on = _cached(world, 'dr3', GM_DEAD_ROWS=3)
    poisoned = _run(world, poison_bytes=on['ws_bytes'], GM_DEAD_ROWS=3)
    for k in ('accs', 'losses', 'grad', 'theta'):
        assert np.isfinite(poisoned[k]).all(), k
    _assert_bitwise(poisoned, on)


def _eval(w, level, poison=False, config=None, **attrs):
    """The evaluation leg (the first task, then all tasks: every query evaluation forward-only) and Meta.predict from identical seeds; with `poison` the
    workspace is 0xFF before one more evaluation of all tasks and the bytes still 0xFF afterwards are counted."""
    b = w['batch']
    with tuning(**dict(w['force'], GM_DEAD_ROWS=level)):
        m = _meta(w, config, **attrs)
        first = np.asarray(m.finetunning(*w['one'], None)).copy()
        accs = np.asarray(m.finetunning_batch(b[0], b[1], b[2], b[3])).copy()
        untouched = None
        if poison:
            m._ws = torch.full((m._ws.numel(),), 0xFF, dtype=torch.uint8, device='cuda')
            again = np.asarray(m.finetunning_batch(b[0], b[1], b[2], b[3])).copy()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(again), _bits(accs))
            untouched = int((m._ws == 0xFF).sum())
        out = dict(first=first, accs=accs, untouched=untouched)
        if not poison:
            p = m.predict(b[0], b[1], b[2], logits=True)
            out.update(logp=np.concatenate(p.log_probs), pred=np.concatenate(p.pred), logits=np.concatenate(p.logits))
    return out


def test_evaluation_leg_and_predict_are_bitwise(world):
    _need_split(world, world['S'], world['Q'])
    res = {lv: _eval(world, lv) for lv in (3, 2, 0)}
    assert np.isfinite(res[3]['logits']).all()
    for lv in (2, 0):
        _assert_bitwise(res[3], res[lv], keys=('first', 'accs', 'logp', 'pred', 'logits'))


def _h1_rows_dropped(w):
    """rows of H_{L-1} level 2 stores (an out-edge) and level 3 does not (no out-edge into a centre), in the query batch"""
    from gmeta_amd import _lib
    Q = w['Q']
    _, e1 = _sets(Q)
    src = Q._read(_lib.F_NORM_SRC, Q.rows, np.float32).view(np.uint32) >> 31 == 0
    assert not (e1 & ~src).any()
    return int(src.sum() - e1.sum())


def test_forward_only_passes_leave_unobservable_rows_unwritten(world):
    """The evaluation leg over a 0xFF workspace: at level 3 at least the rows of H_{L-1} that are a source but not a source of a centre's in-edge stay
    unwritten beyond what level 2 leaves (a written byte is 0xFF by chance in fewer than 1 of 10: the bound takes 0.9 of them), with the same accuracies."""
    _need_split(world, world['S'], world['Q'])
    three, two = _eval(world, 3, poison=True), _eval(world, 2, poison=True)
    _assert_bitwise(three, two, keys=('accs',))
    dropped = _h1_rows_dropped(world)
    assert dropped > 0
    gain = three['untouched'] - two['untouched']
    print('bytes left unwritten at 3 / at 2: %d / %d; H_{L-1} rows no longer stored: %d' % (three['untouched'], two['untouched'], dropped))
    assert gain >= 0.9 * 4 * world['cfg']['hidden'] * dropped, (gain, dropped)


@pytest.mark.parametrize('case', ['mean_readout', 'cone'])
def test_off_where_it_must_be_off(world, case):
    """Mean readout and the cone schedule: level 3 runs what level 2 runs -- the same accuracies and, over a 0xFF workspace, the same bytes left unwritten
    (the every-row stores of H_{L-1} happen)."""
    from gmeta_amd import synth
    _need_split(world, world['S'], world['Q'])
    cfg = world['cfg']
    kw = {}
    if case == 'mean_readout':
        kw['config'] = synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], cfg['n_way']) + [('Readout', ['mean'])]
    else:
        kw['cone'] = 1
    three, two = _eval(world, 3, poison=True, **kw), _eval(world, 2, poison=True, **kw)
    _assert_bitwise(three, two, keys=('first', 'accs'))
    assert three['untouched'] == two['untouched'], (three['untouched'], two['untouched'])


def test_off_under_the_two_piece_kernels(world):
    """The opt-in two-piece kernels record the largest stored |H_l| of every row, so every row stays observable: the step at level 3 equals level 2 bitwise
    and its aggregate launches are priced as at level 2 -- where under the three-piece kernels level 3 prices less."""
    _need_split(world, world['S'], world['Q'])
    three, two = _run(world, pieces=2, GM_DEAD_ROWS=3), _run(world, pieces=2, GM_DEAD_ROWS=2)
    _assert_bitwise(three, two)
    assert three['agg_bytes'] == two['agg_bytes'], (three['agg_bytes'], two['agg_bytes'])
    on, ref = _cached(world, 'dr3', GM_DEAD_ROWS=3), _cached(world, 'dr2', GM_DEAD_ROWS=2)
    print('two-piece step differs from the three-piece step:', not np.array_equal(_bits(three['grad']), _bits(on['grad'])))
    assert 0 < on['agg_bytes'] < ref['agg_bytes'], (on['agg_bytes'], ref['agg_bytes'])


def test_user_supplied_centres_take_the_every_row_pass(world):
    """gm_gcn_forward with a caller's centre list: the same logits and the same bytes left unwritten at levels 3 and 2."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    Q = world['Q']
    res = {}
    for lv in (3, 2):
        with tuning(**dict(world['force'], GM_DEAD_ROWS=lv)):
            m = _meta(world)
            model = m.net.model
            theta = m._flat_theta()
            centre = torch.from_numpy(Q._read(_lib.F_CENTRE, Q.subs * Q.centres, np.int32)).cuda()
            ws = torch.full((int(lib.gm_gcn_ws_bytes(Q.handle, C.byref(model))),), 0xFF, dtype=torch.uint8, device='cuda')
            logits = torch.empty(Q.subs, model.n_out, device='cuda')
            _lib.check(lib.gm_gcn_forward(Q.handle, C.byref(model), _lib.ptr(theta), 0, None, _lib.ptr(centre), _lib.ptr(logits), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr()), 'gm_gcn_forward')
            torch.cuda.synchronize()
            res[lv] = (logits.cpu().numpy(), int((ws == 0xFF).sum()))
    assert np.isfinite(res[3][0]).all()
    assert np.array_equal(_bits(res[3][0]), _bits(res[2][0])) and res[3][1] == res[2][1]


def test_three_layer_model_restricts_the_last_two_layers_only(world):
    """Three GraphConv layers: the step at level 3 equals level 0 bitwise, and of the three partial aggregate launches of a forward-only pass the first is
    priced as at level 2, the other two on their observable rows."""
    from gmeta_amd import synth
    _need_split(world, world['S'], world['Q'])
    cfg = world['cfg']
    config = synth.make_config(cfg['F0'], cfg['hidden'], 3, cfg['n_way'])
    on, off = _run(world, config=config, GM_DEAD_ROWS=3), _run(world, config=config, GM_DEAD_ROWS=0)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0
    _assert_bitwise(on, off)
    Q = world['Q']
    F0, H = cfg['F0'], cfg['hidden']
    w3, w2 = _predict_launch_bytes(world, 3, config), _predict_launch_bytes(world, 2, config)
    assert w2 == [_price(Q, F0), _price(Q, H), _price(Q, H)], w2
    assert w3 == [_price(Q, F0), _price(Q, H, 1), _price(Q, H, 0)], w3


def test_non_finite_weight_gives_the_lower_levels_results(world):
    """One +Inf in W_L: level 3 equals level 2 in accuracies, losses_q and parameters (NaNs compare equal), and the update is skipped."""
    _need_split(world, world['S'], world['Q'])
    three = _run(world, inf_weight=True, GM_DEAD_ROWS=3)
    two = _run(world, inf_weight=True, GM_DEAD_ROWS=2)
    for k in ('accs', 'losses', 'theta'):
        assert np.array_equal(three[k], two[k], equal_nan=True), k
    assert not np.isfinite(three['losses']).all()
    for r in (three, two):
        assert np.array_equal(_bits(r['theta']), _bits(r['theta0']))      # the update was skipped
        assert r['found_inf'] is None or r['found_inf'] != 0


# ---------------------------------------------------------------------------------------------------------------- the launch accounting
def _price(B, width, obs=None):
    """Category-0 bytes of a fused pass's partial aggregate launch over rows of `width` floats: every indptr entry; of the rows of more than two sources the
    edge-table entries, a row-scale entry, the row written once and their distinct sources read once (obs None) -- or, restricted to the observable rows
    (obs 0: centres, 1: sources of the centres' in-edges), the list entry and the flag of every such row and only the observable ones' edges, rows and sources."""
    ip, ix = B.csr()
    ip = ip.astype(np.int64)
    deg = np.diff(ip)
    big = deg > MAXDEG
    U = int(big.sum())
    rows_w = big if obs is None else big & _sets(B)[obs]
    dst = np.repeat(np.arange(B.rows), deg)
    e = int(deg[rows_w].sum()); n = int(rows_w.sum()); s = len(np.unique(ix[rows_w[dst]]))
    if obs is None:
        return 4 * (B.rows + 1) + 4 * e + 4 * U + 4 * n * width + 4 * s * width
    return 4 * (B.rows + 1) + 8 * U + 4 * e + 4 * n * width + 4 * s * width


def _predict_launch_bytes(w, level, config=None):
    """the category-0 work of every aggregate launch of one gm_proto_predict (one forward-only pass over the query batch)"""
    from gmeta_amd import _lib
    lib = _lib.lib()
    b = w['batch']
    with tuning(**dict(w['force'], GM_DEAD_ROWS=level)):
        m = _meta(w, config)
        adapted = m.adapt(b[0], b[1])
        torch.cuda.synchronize()
        lib.gm_profile_enable(1)
        try:
            adapted.predict(b[2])
            torch.cuda.synchronize()
            ms, work = (C.c_double * 16)(), (C.c_int64 * 16)()
            n = lib.gm_profile_read_launches(0, ms, work, 16)
        finally:
            lib.gm_profile_enable(0)
    return [int(work[k]) for k in range(n)]


def test_launch_accounting_prices_the_touched_rows(world):
    """With the launch accounting on, the two partial aggregate launches of a forward-only pass carry the host-side formula on the rows they touch, and less
    than at level 2."""
    _need_split(world, world['S'], world['Q'])
    Q = world['Q']
    F0, H = world['cfg']['F0'], world['cfg']['hidden']
    w3, w2 = _predict_launch_bytes(world, 3), _predict_launch_bytes(world, 2)
    print('partial aggregate bytes at 3 / at 2:', w3, w2)
    assert w2 == [_price(Q, F0), _price(Q, H)], (w2, _price(Q, F0), _price(Q, H))
    assert w3 == [_price(Q, F0, 1), _price(Q, H, 0)], (w3, _price(Q, F0, 1), _price(Q, H, 0))
    assert all(a < b for a, b in zip(w3, w2))


# ---------------------------------------------------------------------------------------------------------------- the kernels alone
def _sentinel(rows, width):
    return torch.full((rows, width), SENTINEL, device='cuda', dtype=torch.int32)


def _partial_aggregate(B, x_src, x, width, flags, out):
    """gcn_forward's partial launch of a fused pass: rows of more than two sources, over the batch's list of window rows and its schedule where it has one;
    flags: the keep vector (device pointer) of a restricted launch, or None"""
    from gmeta_amd import _lib
    lib = _lib.lib()
    info = (C.c_int64 * 16)()
    _lib.check(lib.gm_dense_agg_info(B.handle, 0, info), 'gm_dense_agg_info')
    n_mid, mid_win, has_sched, n_heavy = int(info[6]), int(info[7]), int(info[8]), int(info[1])
    use_list = n_mid > 0 and (n_heavy == 0 or has_sched)
    lst = None
    if use_list:
        lst = torch.empty(n_mid, dtype=torch.int32, device='cuda')
        _lib.check(lib.gm_dense_agg_table(B.handle, 2, 0, _lib.ptr(lst), n_mid, _lib.stream_ptr()), 'gm_dense_agg_table')
    _lib.check(lib.gm_dense_aggregate(B.handle, 0, x_src, _lib.ptr(x), x.shape[1] if x is not None else 0, width, 2, None, flags, 1 if flags else 0, None, 0, 0,
                                      None, None, None, 2, _lib.ptr(lst), n_mid if use_list else 0, mid_win if use_list else 0,
                                      1 if (use_list and n_heavy > 0) else 0, 0, MAXDEG, 0, _lib.ptr(out), None, _lib.stream_ptr()), 'gm_dense_aggregate')
    torch.cuda.synchronize()


def test_restricted_partial_aggregates_alone(kworld):
    """The partial aggregate with the +-1 keep vector against the unrestricted launch, over sentinel-filled outputs: it writes exactly the rows of more than
    two sources that are observable, bitwise the unrestricted launch's -- over an input that is NaN on every row no observable row reads -- and a later
    unrestricted launch on the same batch still gives what the first gave (the split hub rows' arrival counters are back at 0)."""
    from gmeta_amd import _lib
    B = kworld['S']
    H, F0 = kworld['cfg']['hidden'], kworld['cfg']['F0']
    is_c, e1 = _sets(B)
    ip, ix = B.csr()
    deg = np.diff(ip.astype(np.int64))
    big = deg > MAXDEG
    g = torch.Generator(device='cuda'); g.manual_seed(11)
    x = torch.randn(B.rows, H, device='cuda', generator=g)
    x[0, :4] = torch.tensor([-0.0, 0.0, 1e-40, 3e30], device='cuda')
    cases = ((is_c, _lib.F_OBS_CENTRE, 0, H, e1), (e1, _lib.F_OBS_E1, 0, H, None), (e1, _lib.F_OBS_E1, 2, F0, None))
    for keep, field, x_src, width, readers in cases:
        xin = x if x_src == 0 else None
        full = _sentinel(B.rows, width)
        _partial_aggregate(B, x_src, xin, width, None, full)
        dirty = xin
        if readers is not None:      # the last layer's launch reads H_{L-1} on the sources of the centres' in-edges only
            dirty = torch.where(torch.from_numpy(readers).cuda()[:, None], x, torch.full_like(x, float('nan')))
        part = _sentinel(B.rows, width)
        _partial_aggregate(B, x_src, dirty, width, B.device_ptr(field), part)
        again = _sentinel(B.rows, width)
        _partial_aggregate(B, x_src, xin, width, None, again)
        big_t, w_t = torch.from_numpy(big).cuda(), torch.from_numpy(big & keep).cuda()
        assert bool((full[~big_t] == SENTINEL).all()) and bool((full[big_t] != SENTINEL).any(1).all())
        assert (big & keep).any() and (big & ~keep).any()
        assert torch.equal(part[w_t], full[w_t])
        assert bool((part[~w_t] == SENTINEL).all())
        assert torch.equal(again, full)


def test_update_below_the_last_stores_the_kept_rows_alone(kworld):
    """The K = 128 update GEMM with GM_F_NORM_E1 as the keep vector stores exactly the rows it keeps, each equal to the every-row launch."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    B = kworld['S']
    H, F0 = kworld['cfg']['hidden'], kworld['cfg']['F0']
    _, e1 = _sets(B)
    g = torch.Generator(device='cuda'); g.manual_seed(5)
    z = torch.randn(B.rows, F0, device='cuda', generator=g)
    W = torch.randn(F0, H, device='cuda', generator=g) * 0.1
    bias = torch.randn(H, device='cuda', generator=g)
    outs = []
    with tuning(**kworld['force']):
        for keep in (None, B.device_ptr(_lib.F_NORM_E1)):
            out = _sentinel(B.rows, H)
            _lib.check(lib.gm_dense_gemm(B.handle, _lib.ptr(z), F0, F0, _lib.ptr(W), 0, 0, H, _lib.ptr(out), H, B.device_ptr(_lib.F_NORM), keep, _lib.ptr(bias), 0, 1,
                                         None, None, None, None, None, 1, None, _lib.stream_ptr()), 'gm_dense_gemm')
            torch.cuda.synchronize()
            outs.append(out)
    full, part = outs
    kept = torch.from_numpy(e1).cuda()
    assert bool((full != SENTINEL).any(1).all())
    assert torch.equal(part[kept], full[kept])
    assert bool((part[~kept] == SENTINEL).all())
