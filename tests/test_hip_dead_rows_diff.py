"""GPU (-m gpu): GM_DEAD_ROWS=4 -- the passes the dense backward differentiates form and store only the rows a gradient reaches.

A differentiated pass (the support passes, the last query evaluation of a meta-step) is read by the head at the centre rows and by its backward, whose dQ_L is
zero outside the centre rows and whose dQ_{L-1} is zero outside the sources of the centres' in-edges.  At 4 (the default) such a pass runs level 3's forward
(tables that send every other row to the zero row, +-1 keep vectors on the partial aggregates, the GM_F_NORM_E1 store below the last layer) and its weight
gradients read Z_l through the same tables.  The last support pass is differentiated twice -- by support_bwd behind the head/loss launch and again, over the
same stored Z / H / relu' bits, by the meta-gradient through the prototypes, which fills dQ_L itself: both go through the tables.  No kernel changed, no
product or sum that reaches a stored value is dropped or reordered, so everything below is compared BITWISE.

Worlds and helpers: those of tests/test_hip_dead_rows_fwd.py (20,000-node preferential-attachment graph, m = 7, F0 128, hidden 256, h = 2, 8 tasks, K = 2,
sample_nodes 160, every edge stored both ways; the same graph stored low id -> high id with the forced-split knobs), plus one
link-prediction world (two centres per subgraph) cut from synth's FirstMM-shaped config.

Not here: the GM_REQUIRE of plan_backward (csrc/model.hip) that refuses a restricted layer whose weight gradient gets neither flagged rows of G nor a dQ the call
filled.  It guards the backward plan's own consistency; the test exports gm_dense_wgrad_fused / gm_dense_fused_gemm launch the kernels below it and cannot reach it."""
import argparse
import ctypes as C
import random

import numpy as np
import pytest
import torch

from test_hip_dead_rows_fwd import (K_STEPS, _assert_bitwise, _bits, _eval, _flat, _h1_rows_dropped, _meta, _need_split, _price, _world, tuning)

pytestmark = pytest.mark.gpu

WGRAD_BYTES = 14      # launch-accounting category: the A and G rows of every weight-gradient launch


@pytest.fixture(scope='module')
def undirected():
    return _world(True)


@pytest.fixture(scope='module')
def directed():
    return _world(False)


@pytest.fixture(params=['undirected', 'directed'])
def world(request):
    return request.getfixturevalue(request.param)


def _step(w, poison=False, inf_weight=False, config=None, pieces=3, attrs=None, **knobs):
    """_run of test_hip_dead_rows_fwd.py with Meta attributes (cone, sparse_bwd, hoist_z1), the weight gradients' accounted bytes (category 14) and, with
    `poison`, the whole workspace 0xFF before the step and the bytes still 0xFF after it (the workspace size comes from an unpoisoned run of the same case)."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    if poison:
        poison = _step(w, False, inf_weight, config, pieces, attrs, **knobs)['ws_bytes']
    if pieces == 2:
        knobs = dict(knobs, GM_SPLIT16_MIN_ROWS=0)
    with tuning(**dict(w['force'], **knobs)):
        lib.gm_set_split_pieces(pieces)
        try:
            m = _meta(w, config, **(attrs or {}))
            cfg = w['cfg']
            if inf_weight:
                with torch.no_grad():
                    W_L = [p for p in m.net.parameters() if p.dim() == 2 and tuple(p.shape) == (cfg['hidden'], cfg['hidden'])]
                    assert len(W_L) == 1
                    W_L[0][3, 5] = float('inf')
            theta0 = _flat(m)
            if poison:
                m._ws = torch.full((poison,), 0xFF, dtype=torch.uint8, device='cuda')
            ms, n, wk0, wk, wg = C.c_double(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
            lib.gm_profile_enable(1)
            lib.gm_profile_read(WGRAD_BYTES, C.byref(ms), C.byref(n), C.byref(wk0))
            accs = np.asarray(m(*w['batch'], None)).copy()
            torch.cuda.synchronize()
            lib.gm_profile_read(0, C.byref(ms), C.byref(n), C.byref(wk))
            lib.gm_profile_read(WGRAD_BYTES, C.byref(ms), C.byref(n), C.byref(wg))
            assert not poison or m._ws.numel() == poison      # (the step ran in the poisoned block)
            untouched = int((m._ws == 0xFF).sum()) if poison else None
        finally:
            lib.gm_profile_enable(0)
            lib.gm_set_split_pieces(3)
    return dict(accs=accs, losses=np.asarray(m.last_stats['losses_q']).copy(), grad=_flat(m, True), theta0=theta0, theta=_flat(m), ws_bytes=m._ws.numel(),
                agg_bytes=int(wk.value), wgrad_bytes=int(wg.value - wk0.value), untouched=untouched,
                found_inf=float(m._found_inf) if m._found_inf is not None else None)


def _cached(w, name, **kw):
    if name not in w['results']:
        w['results'][name] = _step(w, **kw)
    return w['results'][name]


def _level(w, level, fuse_diff=1, poison=False):
    return _cached(w, 'dr%d fd%d%s' % (level, fuse_diff, ' poisoned' if poison else ''), poison=poison, GM_DEAD_ROWS=level, GM_FUSE_DIFF=fuse_diff)


# ---------------------------------------------------------------------------------------------------------------- 1. the step
@pytest.mark.parametrize('fuse_diff', [1, 2])
@pytest.mark.parametrize('ref_level', [3, 0])
def test_step_is_bitwise_the_step_of_the_lower_levels(world, ref_level, fuse_diff):
    """Meta.forward at level 4 against levels 3 and 0: accuracies, losses_q, the meta-gradient (which runs the second backward of the last support pass) and
    the parameters after Adam."""
    _need_split(world, world['S'], world['Q'])
    on, ref = _level(world, 4, fuse_diff), _level(world, ref_level, fuse_diff)
    assert np.isfinite(on['grad']).all() and np.isfinite(on['losses']).all()
    assert np.abs(on['grad']).max() > 0
    _assert_bitwise(on, ref)


# ---------------------------------------------------------------------------------------------------------------- 2. the poisoned workspace
def test_step_over_a_poisoned_workspace_is_unchanged_and_leaves_more_unwritten(world):
    """Every byte of the workspace 0xFF before the step at level 4: every output is finite and bitwise the unpoisoned one, and at least the rows of H_{L-1}
    of the query batch that have an out-edge but none into a centre stay unwritten beyond what level 3 leaves (the last query evaluation stored them at
    level 3; a written byte is 0xFF by chance in fewer than 1 of 10: the bound takes 0.9 of them)."""
    _need_split(world, world['S'], world['Q'])
    on, four, three = _level(world, 4), _level(world, 4, poison=True), _level(world, 3, poison=True)
    for k in ('accs', 'losses', 'grad', 'theta'):
        assert np.isfinite(four[k]).all(), k
    _assert_bitwise(four, on)
    _assert_bitwise(three, on)
    dropped = _h1_rows_dropped(world)
    assert dropped > 0
    gain = four['untouched'] - three['untouched']
    print('bytes left unwritten at 4 / at 3: %d / %d; H_{L-1} rows of the query batch no longer stored: %d' % (four['untouched'], three['untouched'], dropped))
    assert gain >= 0.9 * 4 * world['cfg']['hidden'] * dropped, (gain, dropped)


# ---------------------------------------------------------------------------------------------------------------- 3. adapt / predict / the evaluation leg
def _adapt(w, level, K):
    b = w['batch']
    with tuning(**dict(w['force'], GM_DEAD_ROWS=level, GM_FUSE_DIFF=1)):
        m = _meta(w)
        ad = m.adapt(b[0], b[1], K=K)
        p = ad.predict(b[2], logits=True)
        torch.cuda.synchronize()
        return dict(fw=ad.fast_weights.cpu().numpy(), protos=ad.prototypes.cpu().numpy(), logp=np.concatenate(p.log_probs), pred=np.concatenate(p.pred),
                    logits=np.concatenate(p.logits))


@pytest.mark.parametrize('K', [2, 0])
def test_adapt_and_predict_are_bitwise(world, K):
    """Meta.adapt (the support chain alone: K = 0 runs the forward and the prototypes only) and Meta.predict on the adapted weights."""
    _need_split(world, world['S'], world['Q'])
    four, three = _adapt(world, 4, K), _adapt(world, 3, K)
    assert np.isfinite(four['fw']).all() and np.isfinite(four['logits']).all()
    _assert_bitwise(four, three, keys=('fw', 'protos', 'logp', 'pred', 'logits'))


def test_evaluation_leg_is_bitwise(world):
    _need_split(world, world['S'], world['Q'])
    four, three = _eval(world, 4), _eval(world, 3)
    assert np.isfinite(four['logits']).all()
    _assert_bitwise(four, three, keys=('first', 'accs', 'logp', 'pred', 'logits'))


# ---------------------------------------------------------------------------------------------------------------- 4. the off cases
def _mean_config(w):
    from gmeta_amd import synth
    cfg = w['cfg']
    return synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], cfg['n_way']) + [('Readout', ['mean'])]


OFF = {
    'mean_readout': lambda w: dict(config=_mean_config(w)),
    'cone': lambda w: dict(attrs=dict(cone=1)),
    'sparse_bwd': lambda w: dict(attrs=dict(sparse_bwd=1)),
    'hoist_z1': lambda w: dict(attrs=dict(hoist_z1=1)),
    'two_piece': lambda w: dict(pieces=2),
    'centre_store_0': lambda w: dict(GM_CENTRE_STORE=0),
    'centre_store_1': lambda w: dict(GM_CENTRE_STORE=1),
    'fuse_diff_0': lambda w: dict(GM_FUSE_DIFF=0),
}


@pytest.mark.parametrize('case', sorted(OFF))
def test_off_where_it_must_be_off(world, case):
    """Level 4 runs what level 3 runs: the same results, the same bytes left unwritten over a 0xFF workspace, the same category-0 accounted bytes."""
    _need_split(world, world['S'], world['Q'])
    kw = dict(dict(GM_FUSE_DIFF=1), **OFF[case](world))
    four, three = _step(world, poison=True, GM_DEAD_ROWS=4, **kw), _step(world, poison=True, GM_DEAD_ROWS=3, **kw)
    _assert_bitwise(four, three)
    assert four['untouched'] == three['untouched'], (four['untouched'], three['untouched'])
    assert four['agg_bytes'] == three['agg_bytes'], (four['agg_bytes'], three['agg_bytes'])


def test_off_through_the_public_abi_with_user_centres(world):
    """gm_gcn_forward + gm_gcn_backward with a caller's centre list: the same logits, gradients, bytes left unwritten and category-0 bytes at levels 4 and 3."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    Q = world['Q']
    res = {}
    for lv in (4, 3):
        with tuning(**dict(world['force'], GM_DEAD_ROWS=lv, GM_FUSE_DIFF=1)):
            m = _meta(world)
            model = m.net.model
            theta = m._flat_theta()
            centre = torch.from_numpy(Q._read(_lib.F_CENTRE, Q.subs * Q.centres, np.int32)).cuda()
            ws = torch.full((int(lib.gm_gcn_ws_bytes(Q.handle, C.byref(model))),), 0xFF, dtype=torch.uint8, device='cuda')
            logits = torch.empty(Q.subs, model.n_out, device='cuda')
            g = torch.Generator(device='cuda'); g.manual_seed(7)
            dlogits = torch.randn(Q.subs, model.n_out, device='cuda', generator=g)
            dparams = torch.full((Q.sets, theta.numel()), float('nan'), device='cuda')      # one gradient vector per set, dparam_stride apart
            ms, n, wk = C.c_double(), C.c_int64(), C.c_int64()
            lib.gm_profile_enable(1)
            try:
                _lib.check(lib.gm_gcn_forward(Q.handle, C.byref(model), _lib.ptr(theta), 0, None, _lib.ptr(centre), _lib.ptr(logits), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr()), 'gm_gcn_forward')
                _lib.check(lib.gm_gcn_backward(Q.handle, C.byref(model), _lib.ptr(theta), 0, None, _lib.ptr(centre), _lib.ptr(dlogits), _lib.ptr(dparams),
                                               theta.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), 'gm_gcn_backward')
                torch.cuda.synchronize()
                lib.gm_profile_read(0, C.byref(ms), C.byref(n), C.byref(wk))
            finally:
                lib.gm_profile_enable(0)
            res[lv] = dict(logits=logits.cpu().numpy(), grad=dparams.cpu().numpy(), untouched=int((ws == 0xFF).sum()), agg_bytes=int(wk.value))
    assert np.isfinite(res[4]['logits']).all() and np.isfinite(res[4]['grad']).all() and np.abs(res[4]['grad']).max() > 0
    _assert_bitwise(res[4], res[3], keys=('logits', 'grad'))
    assert res[4]['untouched'] == res[3]['untouched'] and res[4]['agg_bytes'] == res[3]['agg_bytes']


# ---------------------------------------------------------------------------------------------------------------- 5. three layers
def _launches(w, config, level, n_max=256):
    """the category-0 work of every aggregate launch of one Meta.forward, in launch order"""
    from gmeta_amd import _lib
    lib = _lib.lib()
    with tuning(**dict(w['force'], GM_DEAD_ROWS=level, GM_FUSE_DIFF=1)):
        m = _meta(w, config, serialize=1)
        lib.gm_profile_enable(1)
        try:
            m(*w['batch'], None)
            torch.cuda.synchronize()
            ms, work = (C.c_double * n_max)(), (C.c_int64 * n_max)()
            n = lib.gm_profile_read_launches(0, ms, work, n_max)
        finally:
            lib.gm_profile_enable(0)
    assert 0 < n < n_max
    return [int(work[k]) for k in range(n)]


def test_three_layer_model_restricts_the_last_layer_only(world):
    """Three GraphConv layers: the step at level 4 equals level 0 bitwise.  Below the last layer dQ_{L-1} is the A operand of a plain dZ GEMM and stays whole,
    so only the last layer is restricted: of every pass's aggregate launches, in launch order, the first layer's (every third forward launch: the smallest
    width, F0 < hidden) are priced exactly as at level 3."""
    from gmeta_amd import synth
    _need_split(world, world['S'], world['Q'])
    cfg = world['cfg']
    config = synth.make_config(cfg['F0'], cfg['hidden'], 3, cfg['n_way'])
    on, off = _step(world, config=config, GM_DEAD_ROWS=4, GM_FUSE_DIFF=1), _step(world, config=config, GM_DEAD_ROWS=0, GM_FUSE_DIFF=1)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0
    _assert_bitwise(on, off)
    l4, l3 = _launches(world, config, 4), _launches(world, config, 3)
    assert len(l4) == len(l3)
    # the first layer's partial launch of a fused pass carries _price(batch, F0) at every level: one per support pass, one per query evaluation, in place
    for B, passes in ((world['S'], K_STEPS), (world['Q'], K_STEPS + 1)):
        at3, at4 = ([k for k, v in enumerate(l) if v == _price(B, cfg['F0'])] for l in (l3, l4))
        assert len(at3) >= passes and at4 == at3, (at3, at4)
    assert sum(l4) < sum(l3)      # ... and the last layer's launches of the differentiated passes are priced on their observable rows


# ---------------------------------------------------------------------------------------------------------------- 6. a non-finite weight
def test_non_finite_weight_gives_level_3s_results(world):
    """One +Inf in W_L: level 4 equals level 3 in accuracies, losses_q and parameters (NaNs compare equal), and the update is skipped."""
    _need_split(world, world['S'], world['Q'])
    four = _step(world, inf_weight=True, GM_DEAD_ROWS=4, GM_FUSE_DIFF=1)
    three = _step(world, inf_weight=True, GM_DEAD_ROWS=3, GM_FUSE_DIFF=1)
    for k in ('accs', 'losses', 'theta'):
        assert np.array_equal(four[k], three[k], equal_nan=True), k
    assert not np.isfinite(four['losses']).all()
    for r in (four, three):
        assert np.array_equal(_bits(r['theta']), _bits(r['theta0']))      # the update was skipped
        assert r['found_inf'] is None or r['found_inf'] != 0


# ---------------------------------------------------------------------------------------------------------------- 7. link prediction
@pytest.fixture(scope='module')
def link_world():
    """synth's FirstMM-shaped link config (its only one) cut to 4 tasks, 4-shot 8-query, K = 2: two centres per subgraph, F0 = 5 (the first layer gathers
    padded feature rows and is never fused), hidden 128; the split kernels forced."""
    import gmeta_amd
    from gmeta_amd import synth
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args('firstmm', task_num=4, k_spt=4, k_qry=8, update_step=2, update_step_test=2, n_graphs=6)
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=cfg['n_way'], k_shot=cfg['k_spt'], k_query=cfg['k_qry'], batchsz=4, args=args, adjs=store,
                             h=cfg['h'], tables=data['tables'], verbose=False)
    batch = db.get_batch(list(range(4)))
    config = synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], synth.n_out(cfg), link=True)
    return dict(args=args, cfg=cfg, store=store, db=db, batch=batch, S=batch[0][0].view_of, Q=batch[2][0].view_of, config=config,
                force=dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0), results={})


def test_link_prediction_step_is_bitwise_level_0(link_world):
    w = link_world
    assert w['Q'].centres == 2 and w['S'].centres == 2

    def run(level):
        with tuning(**dict(w['force'], GM_DEAD_ROWS=level, GM_FUSE_DIFF=1)):
            a = argparse.Namespace(**vars(w['args']))
            torch.manual_seed(222)
            import gmeta_amd
            m = gmeta_amd.Meta(a, w['config']).to('cuda')
            accs = np.asarray(m(*w['batch'], None)).copy()
            torch.cuda.synchronize()
            return dict(accs=accs, losses=np.asarray(m.last_stats['losses_q']).copy(), grad=_flat(m, True), theta=_flat(m))
    on, off = run(4), run(0)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0
    _assert_bitwise(on, off)


# ---------------------------------------------------------------------------------------------------------------- 8. the launch accounting
def test_launch_accounting_prices_the_touched_rows(world):
    """Where level 4 engages, the step's aggregate launches are priced below level 3's (the restricted partial launches of the differentiated passes) and its
    weight gradients' A and G rows not above."""
    _need_split(world, world['S'], world['Q'])
    four, three = _level(world, 4), _level(world, 3)
    print('category 0 at 4 / at 3: %d / %d; category 14: %d / %d' % (four['agg_bytes'], three['agg_bytes'], four['wgrad_bytes'], three['wgrad_bytes']))
    assert 0 < four['agg_bytes'] < three['agg_bytes']
    assert 0 < four['wgrad_bytes'] <= three['wgrad_bytes']
