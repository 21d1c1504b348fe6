"""GPU (-m gpu): GM_AGG_OBS_LIST -- the aggregate launches that GM_DEAD_ROWS 2-4 restrict to the observable rows walk compact lists of those rows.

Three ascending lists are built with every batch, next to its list of window rows: the rows of 3 .. hub-threshold sources that are centres (list 0: the last
layer's partial aggregate), the same that are sources of a centre's in-edge (list 1: the layer below), and every source of a centre's in-edge in the by-source
orientation (list 2: the last layer's transposed aggregate of a backward).  Lists 1 and 2 are sized by a bound the host knows (at most one row per in-edge of a
centre); the launch reads the length the device counted.  A row's chain does not depend on the wave that forms it and a split hub row is summed in part order
either way, so everything below is compared BITWISE, list against descriptor walk.

Fixtures: the worlds of tests/test_hip_dead_rows_fwd.py rebuilt here (20,000-node preferential-attachment graph, 8 tasks, K = 2, sample_nodes 160, both ways and
low id -> high id; the two joined 300-leaf stars whose 301-edge hub rows are split over two workgroups, one kept and one flagged), the first of them with edge
weights, the link-prediction world of tests/test_hip_dead_rows_diff.py (two centres per subgraph), and a path graph, where no centre has more than two sources."""
import argparse
import ctypes as C
import random

import numpy as np
import pytest
import torch

from test_hip_dead_rows_fwd import (MAXDEG, SENTINEL, T, K_STEPS, _assert_bitwise, _bits, _eval, _flat, _need_split, _partial_aggregate, _run, _sentinel, _sets,
                                    _star, _world, tuning)

pytestmark = pytest.mark.gpu

FORCE = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)


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


def _node_world(data, sample_nodes=160):
    """_world of tests/test_hip_dead_rows_fwd.py over a caller's dataset, the split kernels forced"""
    import gmeta_amd
    from gmeta_amd import synth
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args('arxiv', task_num=T, k_qry=4, update_step=K_STEPS, sample_nodes=sample_nodes)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=3, k_shot=3, k_query=4, batchsz=T, args=args, adjs=store, h=2,
                             tables={'train': (data['names'], data['labels'])}, verbose=False)
    batch = db.get_batch(list(range(T)))
    one = db.get_batch([0])
    return dict(args=args, cfg=cfg, store=store, db=db, batch=batch, one=one, S=batch[0][0].view_of, Q=batch[2][0].view_of, force=dict(FORCE), results={})


@pytest.fixture(scope='module')
def weighted():
    from gmeta_amd import synth
    _, cfg = synth.make_args('arxiv', task_num=T)
    data = synth.node_dataset(20000, 7, cfg['F0'], cfg['classes'])
    data['graphs'] = synth.with_edge_weights(data['graphs'], seed=5)
    w = _node_world(data)
    assert w['Q'].weighted and w['S'].weighted
    return w


@pytest.fixture(scope='module')
def path():
    """One path of 20,000 nodes, every edge stored both ways: no row has more than two sources, so both forward lists are empty and the host knows it."""
    from gmeta_amd import synth
    _, cfg = synth.make_args('arxiv', task_num=T)
    data = synth.node_dataset(20000, 7, cfg['F0'], cfg['classes'])
    n = 20000
    a = np.arange(n - 1, dtype=np.int64)
    data['graphs'] = [(n, np.concatenate([a, a + 1]), np.concatenate([a + 1, a]))]
    return _node_world(data)


@pytest.fixture(scope='module')
def link_world():
    """the link-prediction world of tests/test_hip_dead_rows_diff.py: synth's FirstMM-shaped link config cut to 4 tasks, two centres per subgraph"""
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
    return dict(args=args, cfg=cfg, store=store, db=db, batch=batch, S=batch[0][0].view_of, Q=batch[2][0].view_of, config=config, force=dict(FORCE), results={})


# ---------------------------------------------------------------------------------------------------------------- the lists
def _info(B):
    """gm_dense_obs_lists as a dict per list, the reference counts, and the hub threshold of the batch"""
    from gmeta_amd import _lib
    lib = _lib.lib()
    v = (C.c_int64 * 16)()
    _lib.check(lib.gm_dense_obs_lists(B.handle, v, _lib.stream_ptr()), 'gm_dense_obs_lists')
    a = (C.c_int64 * 16)()
    _lib.check(lib.gm_dense_agg_info(B.handle, 0, a), 'gm_dense_agg_info')
    lists = [dict(n=int(v[4 * k]), cap=int(v[4 * k + 1]), win=int(v[4 * k + 2]), take=int(v[4 * k + 3]) & 3, sched=bool(int(v[4 * k + 3]) & 4)) for k in range(3)]
    return lists, dict(fwd=(int(v[12]), int(v[13])), e1_rows=int(v[14])), int(a[0])


def _read_list(B, k, n):
    from gmeta_amd import _lib
    t = torch.empty(max(n, 1), dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().gm_dense_agg_table(B.handle, 10 + k, 0, _lib.ptr(t), n, _lib.stream_ptr()), 'gm_dense_agg_table')
    torch.cuda.synchronize()
    return t[:n].cpu().numpy()


def _selections(B, heavy):
    """the three lists from the exported row bounds and flag vectors, and the observable hub rows of the two forward sets"""
    from gmeta_amd import _lib
    deg = np.diff(B.csr()[0].astype(np.int64))
    mid = (deg > MAXDEG) & (deg <= heavy)
    obs_c = B._read(_lib.F_OBS_CENTRE, B.rows, np.float32) > 0
    obs_e = B._read(_lib.F_OBS_E1, B.rows, np.float32) > 0
    e1 = B._read(_lib.F_NORM_E1, B.rows, np.float32).view(np.uint32) >> 31 == 0
    return [np.nonzero(mid & obs_c)[0], np.nonzero(mid & obs_e)[0], np.nonzero(e1)[0]], [int(((deg > heavy) & obs_c).sum()), int(((deg > heavy) & obs_e).sum())]


@pytest.mark.parametrize('which', ['S', 'Q'])
def test_lists_are_the_numpy_selections(kworld, which):
    """Each list read back is the ascending selection from the exported indptr / flag vectors, no longer than its bound; the lengths are the library's own
    counts (gm_batch_fwd_counts less the observable hub rows, gm_batch_e1_rows)."""
    B = kworld[which]
    lists, counts, heavy = _info(B)
    want, hubs = _selections(B, heavy)
    for k in range(3):
        L = lists[k]
        assert L['n'] == len(want[k]) and L['n'] <= max(L['cap'], 0), (k, L, len(want[k]))
        if L['n']:
            got = _read_list(B, k, L['n'])
            assert np.array_equal(got, want[k]) and (np.diff(got) > 0).all(), k
        assert L['win'] in (0, 2, 4, 8, 16, 32, 64)
    assert lists[0]['n'] + hubs[0] == counts['fwd'][0] and lists[1]['n'] + hubs[1] == counts['fwd'][1]
    assert lists[2]['n'] == counts['e1_rows']
    is_c, e1 = _sets(B)
    assert np.array_equal(want[2], np.nonzero(e1)[0])


def test_fixtures_cover_the_cases(undirected, directed, star):
    """A list shorter than its bound (the unused tail), a last partial window, lists the batch takes, and in the star batch split hub rows of either flag in
    both orientations (their blocks ride in the list's own schedule)."""
    tails = partial = taken = 0
    for w in (undirected, directed):
        for B in (w['S'], w['Q']):
            lists, _, _ = _info(B)
            for k in (1, 2):
                tails += lists[k]['cap'] > lists[k]['n'] > 0
            for L in lists:
                partial += L['n'] > 0 and L['n'] % L['win'] != 0
                taken += L['take'] == 1
    assert tails >= 2 and partial >= 1 and taken >= 6, (tails, partial, taken)
    B = star['S']
    lists, _, heavy = _info(B)
    assert all(L['sched'] and L['take'] == 1 for L in lists), lists
    is_c, e1 = _sets(B)
    for tr, keeps in ((False, (is_c, e1)), (True, (e1,))):
        split = np.diff(B.csr(transposed=tr)[0].astype(np.int64)) >= 192
        for keep in keeps:
            assert (split & keep).any() and (split & ~keep).any()


# ---------------------------------------------------------------------------------------------------------------- the kernel alone
def _forward_launch(B, k, x, width, flags, out):
    """the partial aggregate of a fused pass over list k of the batch (selector 2 + k of gm_dense_aggregate)"""
    from gmeta_amd import _lib
    _lib.check(_lib.lib().gm_dense_aggregate(B.handle, 0, 0, _lib.ptr(x), x.shape[1], width, 2, None, flags, 1, None, 0, 0, None, None, None, 2, None, 0, 0, 2 + k,
                                             0, MAXDEG, 0, _lib.ptr(out), None, _lib.stream_ptr()), 'gm_dense_aggregate')
    torch.cuda.synchronize()


def _transposed_launch(B, Tm, width, mask, out, listed):
    """the last layer's transposed aggregate of a restricted backward: T through the centre-edge table, GM_F_NORM_E1 as keep vector, packed relu' bits"""
    from gmeta_amd import _lib
    _lib.check(_lib.lib().gm_dense_aggregate(B.handle, 1, 3, _lib.ptr(Tm), width, width, 0, None, B.device_ptr(_lib.F_NORM_E1), 1, None, 0, 0, None, None,
                                             _lib.ptr(mask), 2, None, 0, 0, 4 if listed else 0, 1, 0, 0, _lib.ptr(out), None, _lib.stream_ptr()), 'gm_dense_aggregate')
    torch.cuda.synchronize()


@pytest.mark.parametrize('width', [128, 256])
def test_list_launches_alone(kworld, width):
    """Each of the three launches over its list and then as the descriptor walk, into sentinel-filled outputs: the same bits everywhere -- the observable rows
    with work written, every other row still the sentinel -- and the walk once more afterwards gives what it gave (the split hub rows' arrival counters are
    back at zero behind a list launch)."""
    from gmeta_amd import _lib
    B = kworld['S']
    lists, _, heavy = _info(B)
    is_c, e1 = _sets(B)
    big = np.diff(B.csr()[0].astype(np.int64)) > MAXDEG
    g = torch.Generator(device='cuda'); g.manual_seed(13 + width)
    x = torch.randn(B.rows, width, device='cuda', generator=g)
    x[0, :4] = torch.tensor([-0.0, 0.0, 1e-40, 3e30], device='cuda')
    ran = 0
    for k, keep, field in ((0, is_c, _lib.F_OBS_CENTRE), (1, e1, _lib.F_OBS_E1)):
        if lists[k]['cap'] == 0 and not lists[k]['sched']:
            continue      # (no list of this kind in the batch)
        walk, listed, again = _sentinel(B.rows, width), _sentinel(B.rows, width), _sentinel(B.rows, width)
        _partial_aggregate(B, 0, x, width, B.device_ptr(field), walk)
        _forward_launch(B, k, x, width, B.device_ptr(field), listed)
        _partial_aggregate(B, 0, x, width, B.device_ptr(field), again)
        w_t = torch.from_numpy(big & keep).cuda()
        assert (big & keep).any()
        assert bool((walk[w_t] != SENTINEL).any(1).all()) and bool((walk[~w_t] == SENTINEL).all())
        assert torch.equal(listed, walk) and torch.equal(again, walk), k
        ran += 1
    if lists[2]['cap'] > 0:
        crow = torch.from_numpy(np.nonzero(is_c)[0]).cuda()
        Tm = torch.zeros(B.rows + 1, width, device='cuda')
        Tm[crow] = torch.randn(len(crow), width, device='cuda', generator=g)
        mask = torch.randint(0, 16, (B.rows * width // 4,), device='cuda', generator=g, dtype=torch.int32).to(torch.uint8)
        walk, listed, again = _sentinel(B.rows, width), _sentinel(B.rows, width), _sentinel(B.rows, width)
        _transposed_launch(B, Tm, width, mask, walk, False)
        _transposed_launch(B, Tm, width, mask, listed, True)
        _transposed_launch(B, Tm, width, mask, again, False)
        k_t = torch.from_numpy(e1).cuda()
        assert bool((walk[k_t] != SENTINEL).all()) and bool((walk[~k_t] == SENTINEL).all())
        assert walk.view(torch.float32)[k_t].abs().max() > 0
        assert torch.equal(listed, walk) and torch.equal(again, walk)
        ran += 1
    assert ran == 3, (ran, lists)


# ---------------------------------------------------------------------------------------------------------------- the empty list
def _predict(w, **knobs):
    """one Meta.adapt + predict over the world's batch: the logits, and the category-0 work of every aggregate launch of the prediction"""
    from gmeta_amd import _lib
    from test_hip_dead_rows_fwd import _meta
    lib = _lib.lib()
    b = w['batch']
    with tuning(**dict(w['force'], **knobs)):
        m = _meta(w)
        adapted = m.adapt(b[0], b[1])
        torch.cuda.synchronize()
        lib.gm_profile_enable(1)
        try:
            p = adapted.predict(b[2], logits=True)
            torch.cuda.synchronize()
            ms, work = (C.c_double * 16)(), (C.c_int64 * 16)()
            n = lib.gm_profile_read_launches(0, ms, work, 16)
        finally:
            lib.gm_profile_enable(0)
    return dict(logits=np.concatenate(p.logits), logp=np.concatenate(p.log_probs), launches=[int(work[k]) for k in range(n)])


def test_empty_lists_launch_nothing(path):
    """A path graph: no row has more than two sources, the host knows both forward lists empty (no hub rows either), and the two partial aggregate launches of a
    forward-only pass are gone from the launch accounting -- with the same logits."""
    Q = path['Q']
    assert (np.diff(Q.csr()[0].astype(np.int64)) <= MAXDEG).all()
    lists, _, _ = _info(Q)
    assert lists[0]['take'] == 2 and lists[1]['take'] == 2 and lists[0]['n'] == 0 and lists[1]['n'] == 0, lists
    on, off = _predict(path, GM_AGG_OBS_LIST=1), _predict(path, GM_AGG_OBS_LIST=0)
    assert len(off['launches']) == 2 and len(on['launches']) == 0, (off['launches'], on['launches'])
    assert np.isfinite(on['logits']).all()
    _assert_bitwise(on, off, keys=('logits', 'logp'))


# ---------------------------------------------------------------------------------------------------------------- the whole step
def _both(w, level, config=None, **knobs):
    """Meta.forward, the evaluation leg and Meta.predict with the lists and without"""
    res = []
    for on in (1, 0):
        r = _run(w, config=config, GM_DEAD_ROWS=level, GM_AGG_OBS_LIST=on, **knobs)
        with tuning(GM_AGG_OBS_LIST=on, **knobs):
            r.update(('ev_' + k, v) for k, v in _eval(w, level, config=config).items() if v is not None)
        res.append(r)
    return res


STEP_KEYS = ('accs', 'losses', 'grad', 'theta', 'ev_first', 'ev_accs', 'ev_logp', 'ev_pred', 'ev_logits')


@pytest.mark.parametrize('level', [2, 3, 4])
def test_step_evaluation_and_predict_are_bitwise(world, level):
    """Meta.forward (accuracies, losses_q, every .grad, the parameters after Adam), finetunning and Meta.predict with GM_AGG_OBS_LIST 1 against 0."""
    _need_split(world, world['S'], world['Q'])
    on, off = _both(world, level)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0 and np.isfinite(on['ev_logits']).all()
    _assert_bitwise(on, off, keys=STEP_KEYS)
    assert on['agg_bytes'] == off['agg_bytes']      # (a list launch is priced as the walk it replaces)


def test_weighted_step_is_bitwise(weighted):
    on, off = _both(weighted, 4)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0
    _assert_bitwise(on, off, keys=STEP_KEYS)


def test_link_prediction_step_is_bitwise(link_world):
    w = link_world
    assert w['Q'].centres == 2 and w['S'].centres == 2

    def run(on):
        import gmeta_amd
        with tuning(**dict(w['force'], GM_DEAD_ROWS=4, GM_AGG_OBS_LIST=on)):
            a = argparse.Namespace(**vars(w['args']))
            torch.manual_seed(222)
            m = gmeta_amd.Meta(a, w['config']).to('cuda')
            accs = np.asarray(m(*w['batch'], None)).copy()
            torch.cuda.synchronize()
            return dict(accs=accs, losses=np.asarray(m.last_stats['losses_q']).copy(), grad=_flat(m, True), theta=_flat(m))
    on, off = run(1), run(0)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0
    _assert_bitwise(on, off)


def test_second_hub_set_keeps_the_descriptor_walk(world):
    """GM_QUERY_STREAMS=2: the contexts on the second hub set fall back to today's launches, and the step stays bitwise either way."""
    _need_split(world, world['S'], world['Q'])
    on = _run(world, GM_DEAD_ROWS=4, GM_QUERY_STREAMS=2, GM_AGG_OBS_LIST=1)
    off = _run(world, GM_DEAD_ROWS=4, GM_QUERY_STREAMS=2, GM_AGG_OBS_LIST=0)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0
    _assert_bitwise(on, off)
