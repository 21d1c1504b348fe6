"""GPU (-m gpu): GM_DEAD_ROWS=2 -- the dense backward stops storing and fetching rows that are zero by construction.

With dQ_L on its centre rows only (GM_DEAD_ROWS=1), T = norm (dQ_L W_L^T) is zero outside the centre rows and dQ_{L-1} = relu' norm A^T T is zero outside
the sources of the centres' in-edges.  At 2 (the default) the dZ GEMM stores T's centre rows only, the transposed aggregate reads T through a per-edge table
that sends every other destination to one zero row behind T, stores only the rows of dQ_{L-1} that can be non-zero, and the first layer's weight gradient
selects zeros for the rest.  Every row is still computed and no product or sum is dropped, so everything below is compared BITWISE.

Fixtures: the two worlds of tests/test_hip_dead_rows.py (20,000-node preferential-attachment graph, m = 7, F0 128, hidden 256, h = 2, 8 tasks, K = 2; every
edge stored both ways / stored low id -> high id with the forced-split knobs), and two joined 300-leaf stars for the kernels alone: there a hub row has 301
out-edges, which the aggregate splits over two workgroups (the last arriver runs the epilogue) -- one such row kept, one flagged."""
import argparse
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, K_STEPS = 8, 2
SENTINEL = 0x7fc12345      # a NaN no kernel produces: "this output row was never stored"


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
    return dict(args=args, cfg=cfg, store=store, db=db, batch=batch, S=batch[0][0].view_of, Q=batch[2][0].view_of, force=force, results={})


N_LEAF = 300


def _star():
    """Hubs A = 0 and B = 1 joined by an edge, 300 leaves each, every edge stored both ways; one set of five subgraphs around A, two of A's leaves, B and one
    of B's leaves.  Around A the subgraph holds all 602 nodes: A's own row (301 out-edges, none into the centre: there is no self-loop) is flagged, B's row
    (301 out-edges, one into the centre) is kept.  Around a leaf of A, A's row is kept."""
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


def _heavy_deg(B):
    return 32 if B.edges <= 8 * B.rows else 64      # the batch's hub threshold, by density


def _centre_rows(B):
    from gmeta_amd import _lib
    return (B.sub_off[:-1].astype(np.int64)[:, None] + B._read(_lib.F_CENTRE, B.subs * B.centres, np.int32).reshape(B.subs, B.centres)).reshape(-1)


def _tables(B):
    """(is_centre [rows], kept [rows], ect [edges]) recomputed on the host from the by-source CSR and the centre rows."""
    ipt, ixt = B.csr(transposed=True)
    is_c = np.zeros(B.rows, bool); is_c[_centre_rows(B)] = True
    src = np.repeat(np.arange(B.rows), np.diff(ipt.astype(np.int64)))      # source row of every by-source edge
    kept = np.zeros(B.rows, bool); kept[src[is_c[ixt]]] = True              # rows with an out-edge into a centre row
    ect = np.where(is_c[ixt], ixt, B.rows).astype(np.int32)
    return is_c, kept, ect


# ---------------------------------------------------------------------------------------------------------------- test 1: the tables
def _check_tables(B):
    from gmeta_amd import _lib
    is_c, kept, ect = _tables(B)
    norm = B._read(_lib.F_NORM, B.rows, np.float32).view(np.uint32)
    e1 = B._read(_lib.F_NORM_E1, B.rows, np.float32).view(np.uint32)
    assert np.array_equal(e1 >> 31 == 0, kept)
    assert np.array_equal(e1 & 0x7fffffff, norm)
    assert np.array_equal(B._read(_lib.F_EDGE_CENTRE_T, B.edges, np.int32), ect)
    n = C.c_int64(-1)
    _lib.check(_lib.lib().gm_batch_e1_source_rows(B.handle, C.byref(n)))
    assert n.value == int(kept.sum())
    assert kept.any() and not kept.all(), int(kept.sum())                                   # both orientations of the flag
    assert (ect == B.rows).any() and (ect != B.rows).any()
    return np.diff(B.csr(transposed=True)[0].astype(np.int64)), kept


def test_tables_equal_their_recomputation(world):
    """Sign bits of GM_F_NORM_E1 == "no out-edge into a centre row", magnitudes == GM_F_NORM bitwise, GM_F_EDGE_CENTRE_T and the kept-row count equal their
    recomputation from B.csr(transposed=True) and the centre rows.  Not vacuous: both flags occur in both batches, and the by-source degrees of a world
    cover 0, 1, 2 and >= 3."""
    degs = []
    for side in ('S', 'Q'):
        d, _ = _check_tables(world[side])
        degs.append(d)
    d = np.concatenate(degs)
    assert (d == 0).any() and (d == 1).any() and (d == 2).any() and (d >= 3).any()


def test_fixtures_hold_hub_rows_of_both_flags(undirected, star):
    """Hub rows (by-source degree above the batch's threshold) ride in workgroups of their own: the undirected world holds some, and the star batch holds
    rows that are SPLIT over several workgroups (from 192 edges), one kept and one flagged."""
    d, _ = _check_tables(undirected['Q'])
    assert (d > _heavy_deg(undirected['Q'])).any()
    B = star['S']
    d, kept = _check_tables(B)
    assert _heavy_deg(B) == 32
    split = d >= 192
    assert (split & kept).any() and (split & ~kept).any(), (int((split & kept).sum()), int((split & ~kept).sum()))


# ---------------------------------------------------------------------------------------------------------------- tests 2, 3, 5: the step
def _run(w, poison_bytes=0, inf_weight=False, **knobs):
    """One Meta.forward from identical seeds: accuracies, losses_q, the meta-gradient that reached Adam, the parameters before and after its step, the
    GEMM (13) and aggregate (0) byte counts of the launch accounting."""
    import gmeta_amd
    from gmeta_amd import _lib, synth
    a = argparse.Namespace(**vars(w['args']))
    cfg = w['cfg']
    with tuning(**dict(w['force'], **knobs)):
        torch.manual_seed(222)
        m = gmeta_amd.Meta(a, synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], cfg['n_way'])).to('cuda')
        if inf_weight:
            with torch.no_grad():
                W_L = [p for p in m.net.parameters() if p.dim() == 2 and tuple(p.shape) == (cfg['hidden'], cfg['hidden'])]
                assert len(W_L) == 1
                W_L[0][3, 5] = float('inf')
        theta0 = torch.cat([p.detach().reshape(-1) for p in m.net.parameters()]).cpu().numpy().copy()
        if poison_bytes:
            m._ws = torch.full((poison_bytes,), 0xFF, dtype=torch.uint8, device='cuda')      # every float of the step's workspace a NaN
        lib = _lib.lib()
        lib.gm_profile_enable(1)
        accs = np.asarray(m(*w['batch'], None)).copy()
        torch.cuda.synchronize()
        work = {}
        for cat in (13, 0):
            ms, n, wk = C.c_double(), C.c_int64(), C.c_int64()
            lib.gm_profile_read(cat, C.byref(ms), C.byref(n), C.byref(wk))
            work[cat] = int(wk.value)
        lib.gm_profile_enable(0)
        assert not poison_bytes or m._ws.numel() == poison_bytes      # (the step ran in the poisoned block)
    return dict(accs=accs, losses=np.asarray(m.last_stats['losses_q']).copy(),
                grad=torch.cat([p.grad.reshape(-1) for p in m.net.parameters()]).cpu().numpy().copy(), theta0=theta0,
                theta=torch.cat([p.detach().reshape(-1) for p in m.net.parameters()]).cpu().numpy().copy(), ws_bytes=m._ws.numel(),
                gemm_bytes=work[13], agg_bytes=work[0], found_inf=float(m._found_inf) if m._found_inf is not None else None)


def _cached(w, name, **kw):
    if name not in w['results']:
        w['results'][name] = _run(w, **kw)
    return w['results'][name]


def _bits(a):
    return a.view(np.uint8 if a.dtype.itemsize == 1 else 'u%d' % a.dtype.itemsize)


def _assert_bitwise(a, b, keys=('accs', 'losses', 'grad', 'theta')):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize('ref_level', [1, 0])
def test_step_is_bitwise_the_step_of_the_lower_levels(world, ref_level):
    """One Meta.forward from identical seeds with GM_DEAD_ROWS = 2 against 1 and 0: accuracies, losses_q, the meta-gradient and the parameters after the
    Adam step, bitwise; the gradient finite and non-zero; and at 2 the launch accounting's GEMM and aggregate bytes strictly below those at 1."""
    _need_split(world, world['S'], world['Q'])
    on = _cached(world, 'dr2', GM_DEAD_ROWS=2)
    ref = _cached(world, 'dr%d' % ref_level, GM_DEAD_ROWS=ref_level)
    assert np.isfinite(on['grad']).all() and np.isfinite(on['losses']).all()
    assert np.abs(on['grad']).max() > 0
    _assert_bitwise(on, ref)
    if ref_level == 1:
        print('bytes at 2 / at 1: GEMM %d / %d, aggregate %d / %d' % (on['gemm_bytes'], ref['gemm_bytes'], on['agg_bytes'], ref['agg_bytes']))
        assert 0 < on['gemm_bytes'] < ref['gemm_bytes'], (on['gemm_bytes'], ref['gemm_bytes'])
        assert 0 < on['agg_bytes'] < ref['agg_bytes'], (on['agg_bytes'], ref['agg_bytes'])


def test_step_over_a_poisoned_workspace_is_unchanged_and_finite(world):
    """Every byte of the workspace 0xFF before the step at GM_DEAD_ROWS = 2: whatever the step no longer writes (T outside the centre rows, dQ_{L-1} outside
    the sources of the centres' in-edges, and the rows level 1 already left) holds NaNs, the zero row behind T is the step's own to fill -- and nothing
    reads what is no longer written."""
    _need_split(world, world['S'], world['Q'])
    on = _cached(world, 'dr2', GM_DEAD_ROWS=2)
    poisoned = _run(world, poison_bytes=on['ws_bytes'], GM_DEAD_ROWS=2)
    for k in ('accs', 'losses', 'grad', 'theta'):
        assert np.isfinite(poisoned[k]).all(), k
    _assert_bitwise(poisoned, on)


def test_non_finite_weight_skips_the_update_at_both_levels(world):
    """One +Inf in W_L: the dense pass's structural zeros turn into NaN (0 * Inf), the selected zeros do not -- but the forward over the same weights gives a
    NaN loss and the NaN guard discards the step.  Accuracies, losses_q and the parameters after the step equal those of GM_DEAD_ROWS = 1 (NaNs compare
    equal), and the parameters are the ones the step started from."""
    _need_split(world, world['S'], world['Q'])
    two = _run(world, inf_weight=True, GM_DEAD_ROWS=2)
    one = _run(world, inf_weight=True, GM_DEAD_ROWS=1)
    for k in ('accs', 'losses', 'theta'):
        assert np.array_equal(two[k], one[k], equal_nan=True), k
    assert not np.isfinite(two['losses']).all()
    for r in (two, one):
        assert np.array_equal(_bits(r['theta']), _bits(r['theta0']))      # the update was skipped
        assert r['found_inf'] is None or r['found_inf'] != 0


# ---------------------------------------------------------------------------------------------------------------- test 4: the kernels alone
def test_aggregate_and_weight_gradient_alone(kworld):
    """The masked transposed aggregate through GM_F_EDGE_CENTRE_T + keep_signed over a T that is NaN everywhere but its centre rows (signed zeros, a subnormal
    and 3e30 in one of them) against the plain launch over the clean T: bitwise equal on the kept rows, the output's bytes untouched on the flagged rows
    (which the plain launch leaves all zero).  Beside it the K = 128 flagged-row weight gradient over a dQ that is NaN on the flagged rows against
    gm_dense_wgrad (mode 1) over the zero-filled one."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    B = kworld['S']
    H, F0 = kworld['cfg']['hidden'], kworld['cfg']['F0']
    assert (H, F0) == (256, 128)
    g = torch.Generator(device='cuda'); g.manual_seed(7)
    is_c, kept, _ = _tables(B)
    crow = torch.from_numpy(np.nonzero(is_c)[0]).cuda()
    kept_t = torch.from_numpy(kept).cuda()
    clean = torch.zeros(B.rows + 1, H, device='cuda')
    clean[crow] = torch.randn(len(crow), H, device='cuda', generator=g)
    clean[crow[0], :4] = torch.tensor([-0.0, 0.0, 1e-40, 3e30], device='cuda')      # signed zeros, a subnormal, a huge value
    dirty = torch.full((B.rows + 1, H), float('nan'), device='cuda')
    dirty[crow] = clean[crow]
    mask = torch.randint(0, 16, (B.rows * H // 4,), device='cuda', generator=g, dtype=torch.int32).to(torch.uint8)      # packed relu' bits
    st = _lib.stream_ptr()
    out_plain = torch.empty(B.rows, H, device='cuda')
    out_keep = torch.full((B.rows, H), SENTINEL, device='cuda', dtype=torch.int32)
    _lib.check(lib.gm_dense_agg_centre_t(B.handle, _lib.ptr(clean), H, _lib.ptr(mask), _lib.ptr(out_plain), 0, st), 'gm_dense_agg_centre_t')
    _lib.check(lib.gm_dense_agg_centre_t(B.handle, _lib.ptr(dirty), H, _lib.ptr(mask), _lib.ptr(out_keep), 1, st), 'gm_dense_agg_centre_t')
    torch.cuda.synchronize()
    plain_i = out_plain.view(torch.int32)
    assert out_plain[kept_t].abs().max() > 0
    assert torch.equal(plain_i[kept_t], out_keep[kept_t])
    assert bool((out_keep[~kept_t] == SENTINEL).all())
    assert bool((out_plain[~kept_t] == 0).all())                      # (what the flagged rows are by construction)
    assert bool(torch.isnan(dirty[:B.rows][~torch.from_numpy(is_c).cuda()]).all())      # the launch wrote nothing into T but its zero row
    # ---- the first layer's weight gradient over that dQ_{L-1}: K = 128, N = 256
    with tuning(**kworld['force']):
        x = torch.randn(B.rows, F0, device='cuda', generator=g)
        dq_clean = out_plain
        dq_dirty = torch.where(kept_t[:, None], out_plain, torch.full_like(out_plain, float('nan')))
        norm = B.device_ptr(_lib.F_NORM)
        res = []
        for which in (0, 1):
            dW, db = torch.empty(B.sets, F0, H, device='cuda'), torch.empty(B.sets, H, device='cuda')
            if which == 0:
                _lib.check(lib.gm_dense_wgrad(B.handle, _lib.ptr(x), F0, F0, _lib.ptr(dq_clean), H, H, norm, None, 0, _lib.ptr(dW), F0 * H, _lib.ptr(db), H, 1,
                                              None, None, 0, 0.0, None, None, None, st), 'gm_dense_wgrad')
            else:
                _lib.check(lib.gm_dense_wgrad_e1(B.handle, _lib.ptr(x), F0, _lib.ptr(dq_dirty), H, _lib.ptr(dW), F0 * H, _lib.ptr(db), H, st), 'gm_dense_wgrad_e1')
            torch.cuda.synchronize()
            res.append((dW, db))
    assert torch.isfinite(res[1][0]).all() and torch.isfinite(res[1][1]).all() and res[0][0].abs().max() > 0
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
