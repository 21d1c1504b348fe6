"""GPU (-m gpu): GM_DEAD_ROWS -- rows no later kernel reads are computed and neither stored nor zero-filled.

* H_l below the last layer is read through the edges only, so a row without an out-edge inside the batch is nobody's source: its value is not stored
  (gm_batch's GM_F_NORM_SRC carries the flag in the sign bit of the row scale, as GM_F_NORM_CENTRE does for the last layer).
* dQ_L is no longer zero-filled: the head/loss launch assigns its centre rows, the dZ GEMM reads it through a per-row table on the fused split kernel and
  the weight gradient selects zeros for the rows nobody wrote.
No sum and no product changes, so everything below is compared BITWISE: the switch on, off, and off through GM_CENTRE_STORE=0.

Fixtures (the smallest at which the split kernels engage by themselves on a 256-CU part): a 20,000-node preferential-attachment graph, m = 7, F0 = 128,
hidden 256, h = 2, 3-way 3-shot, 4 queries per class, 8 tasks, K = 2 -- once stored in both directions (a flagged row is an isolated one: the 2-hop
neighbourhoods are sampled down to 160 nodes there, which leaves some centres without any neighbour) and once with every edge stored once, low id -> high id (in- and out-degrees differ; a
centre's subgraph holds its ancestors only, so EVERY centre is flagged).  The directed subgraphs are small (tens of rows): there the split kernels are
forced onto the batch with the tuning knobs the other suites use for that."""
import argparse
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, K_STEPS = 8, 2


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
    # undirected: neighbourhoods above 160 nodes are sampled down to 160 (+ the centre), which leaves some centres without any of their neighbours
    args, cfg = synth.make_args('arxiv', task_num=T, k_qry=4, update_step=K_STEPS, sample_nodes=160 if both_directions else 1000)
    data = synth.node_dataset(20000, 7, cfg['F0'], cfg['classes'], both_directions=both_directions)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=3, k_shot=3, k_query=4, batchsz=T, args=args, adjs=store, h=2,
                             tables={'train': (data['names'], data['labels'])}, verbose=False)
    batch = db.get_batch(list(range(T)))
    # directed: tens of rows per subgraph, far below any launch-size threshold -- the large-launch kernels are forced onto it
    force = {} if both_directions else dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
    return dict(args=args, cfg=cfg, store=store, db=db, batch=batch, S=batch[0][0].view_of, Q=batch[2][0].view_of, force=force, results={})


@pytest.fixture(scope='module')
def undirected():
    return _world(True)


@pytest.fixture(scope='module')
def directed():
    return _world(False)


@pytest.fixture(params=['undirected', 'directed'])
def world(request):
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


# ---------------------------------------------------------------------------------------------------------------- test 1: the flags
def test_source_row_flags_equal_out_degree_zero_of_the_batch(world):
    """Sign bits of GM_F_NORM_SRC == "no out-edge" recomputed from the batch's own by-source CSR; magnitudes == GM_F_NORM bitwise; the count of kept rows
    matches.  Not vacuous: both batches of a fixture hold flagged rows, and the fixture holds centres that are themselves flagged."""
    flagged_centres = sum(_check_flags(world[side]) for side in ('S', 'Q'))
    assert flagged_centres >= 1


def _check_flags(B):
    from gmeta_amd import _lib
    ipt, _ = B.csr(transposed=True)
    dead = np.diff(ipt.astype(np.int64)) == 0
    norm = B._read(_lib.F_NORM, B.rows, np.float32).view(np.uint32)
    src = B._read(_lib.F_NORM_SRC, B.rows, np.float32).view(np.uint32)
    assert np.array_equal(src >> 31 == 1, dead)
    assert np.array_equal(src & 0x7fffffff, norm)
    n = C.c_int64(-1)
    _lib.check(_lib.lib().gm_batch_source_rows(B.handle, C.byref(n)))
    assert n.value == int((~dead).sum())
    crow = B.sub_off[:-1].astype(np.int64) + B._read(_lib.F_CENTRE, B.subs * B.centres, np.int32).reshape(B.subs, B.centres)[:, 0]
    assert dead.any() and not dead.all(), int(dead.sum())
    # the last layer's flag (GM_F_NORM_CENTRE) on the same footing: clear on the centre rows only
    cen = B._read(_lib.F_NORM_CENTRE, B.rows, np.float32).view(np.uint32)
    want = np.ones(B.rows, bool); want[crow] = False
    assert np.array_equal(cen >> 31 == 1, want) and np.array_equal(cen & 0x7fffffff, norm)
    return int(dead[crow].sum())


# ---------------------------------------------------------------------------------------------------------------- tests 2 + 3: the step
def _run(w, poison_bytes=0, **knobs):
    """One Meta.forward from identical seeds: accuracies, losses_q, the meta-gradient that reached Adam, the parameters after its step."""
    import gmeta_amd
    from gmeta_amd import _lib, synth
    a = argparse.Namespace(**vars(w['args']))
    cfg = w['cfg']
    with tuning(**dict(w['force'], **knobs)):
        torch.manual_seed(222)
        m = gmeta_amd.Meta(a, synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], cfg['n_way'])).to('cuda')
        if poison_bytes:
            m._ws = torch.full((poison_bytes,), 0xFF, dtype=torch.uint8, device='cuda')      # every float of the step's workspace a NaN
        lib = _lib.lib()
        lib.gm_profile_enable(1)
        accs = np.asarray(m(*w['batch'], None)).copy()
        torch.cuda.synchronize()
        ms, n, work = C.c_double(), C.c_int64(), C.c_int64()
        lib.gm_profile_read(13, C.byref(ms), C.byref(n), C.byref(work))       # compulsory bytes of every grouped GEMM launch: A read once + the C rows STORED
        lib.gm_profile_enable(0)
        assert not poison_bytes or m._ws.numel() == poison_bytes      # (the step ran in the poisoned block)
    return dict(accs=accs, losses=np.asarray(m.last_stats['losses_q']).copy(),
                grad=torch.cat([p.grad.reshape(-1) for p in m.net.parameters()]).cpu().numpy().copy(),
                theta=torch.cat([p.detach().reshape(-1) for p in m.net.parameters()]).cpu().numpy().copy(), ws_bytes=m._ws.numel(), gemm_bytes=int(work.value))


def _cached(w, name, **kw):
    if name not in w['results']:
        w['results'][name] = _run(w, **kw)
    return w['results'][name]


def _assert_bitwise(a, b):
    for k in ('accs', 'losses', 'grad', 'theta'):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint8 if a[k].dtype.itemsize == 1 else 'u%d' % a[k].dtype.itemsize),
                              b[k].view(np.uint8 if b[k].dtype.itemsize == 1 else 'u%d' % b[k].dtype.itemsize)), k


@pytest.mark.parametrize('off', [dict(GM_DEAD_ROWS=0), dict(GM_CENTRE_STORE=0)], ids=['dead_rows_0', 'centre_store_0'])
def test_step_is_bitwise_the_step_with_every_row_stored(world, off):
    """One Meta.forward from identical seeds with GM_DEAD_ROWS = 1 against GM_DEAD_ROWS = 0 and against GM_CENTRE_STORE = 0: accuracies, losses_q, the
    meta-gradient and the parameters after the Adam step, bitwise."""
    _need_split(world, world['S'], world['Q'])
    on = _cached(world, 'on', GM_DEAD_ROWS=1)
    ref = _cached(world, str(sorted(off.items())), **off)
    assert np.isfinite(on['grad']).all() and np.isfinite(on['losses']).all()
    assert np.abs(on['grad']).max() > 0
    _assert_bitwise(on, ref)
    assert 0 < on['gemm_bytes'] < ref['gemm_bytes'], (on['gemm_bytes'], ref['gemm_bytes'])      # ... and the switch did take stores out


def test_step_over_a_poisoned_workspace_is_unchanged_and_finite(world):
    """Every byte of the workspace 0xFF before the step: whatever the step no longer writes (H_l at rows without an out-edge, dQ_L outside the centre rows)
    holds NaNs -- and nothing reads it."""
    _need_split(world, world['S'], world['Q'])
    on = _cached(world, 'on', GM_DEAD_ROWS=1)
    poisoned = _run(world, poison_bytes=on['ws_bytes'], GM_DEAD_ROWS=1)
    for k in ('accs', 'losses', 'grad', 'theta'):
        assert np.isfinite(poisoned[k]).all(), k
    _assert_bitwise(poisoned, on)


# ---------------------------------------------------------------------------------------------------------------- test 4: dZ through the table
def test_dz_through_the_table_is_bitwise_the_plain_launch(world):
    """T = norm * (dQ W^T) of the support batch: the fused split kernel reading dQ's centre rows through the batch's table -- every other row of dQ holding
    NaNs -- against the plain split launch over the same dQ with zeros there (gm_dense_gemm, mode 1).  And the weight gradient beside it: the flagged-row
    variant over the poisoned dQ against gm_dense_wgrad (mode 1) over the zero-filled one."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    B = world['S']
    _need_split(world, B)
    H = world['cfg']['hidden']
    g = torch.Generator(device='cuda'); g.manual_seed(5)
    crow = torch.from_numpy(B.sub_off[:-1].astype(np.int64) + B._read(_lib.F_CENTRE, B.subs, np.int32)).cuda()
    clean = torch.zeros(B.rows, H, device='cuda')
    clean[crow] = torch.randn(B.subs, H, device='cuda', generator=g)
    clean[crow[0], :4] = torch.tensor([-0.0, 0.0, 1e-40, -3e30], device='cuda')      # signed zeros, a subnormal, a huge value
    dirty = torch.full((B.rows, H), float('nan'), device='cuda')
    dirty[crow] = clean[crow]
    W = torch.randn(B.sets, H, H, device='cuda', generator=g) * 0.05                     # per set, stored [N = fi][K = fo] as the layer's own W
    norm = B.device_ptr(_lib.F_NORM)
    st = _lib.stream_ptr()
    T_plain, T_tab = torch.empty(B.rows, H, device='cuda'), torch.empty(B.rows, H, device='cuda')
    with tuning(**world['force']):
        _lib.check(lib.gm_dense_gemm(B.handle, _lib.ptr(clean), H, H, _lib.ptr(W), H * H, 1, H, _lib.ptr(T_plain), H, norm, None, None, 0, 0,
                                     None, None, None, None, None, 1, None, st), 'gm_dense_gemm')
        _lib.check(lib.gm_dense_dz_centre(B.handle, _lib.ptr(dirty), H, _lib.ptr(W), H * H, H, _lib.ptr(T_tab), st), 'gm_dense_dz_centre')
        torch.cuda.synchronize()
        assert torch.isfinite(T_tab).all() and T_plain.abs().max() > 0
        assert torch.equal(T_plain.view(torch.int32), T_tab.view(torch.int32))
        x = torch.randn(B.rows, H, device='cuda', generator=g)
        out = []
        for which in (0, 1):
            dW, db = torch.empty(B.sets, H, H, device='cuda'), torch.empty(B.sets, H, device='cuda')
            if which == 0:
                _lib.check(lib.gm_dense_wgrad(B.handle, _lib.ptr(x), H, H, _lib.ptr(clean), H, H, norm, None, 0, _lib.ptr(dW), H * H, _lib.ptr(db), H, 1,
                                              None, None, 0, 0.0, None, None, None, st), 'gm_dense_wgrad')
            else:
                _lib.check(lib.gm_dense_wgrad_centre(B.handle, _lib.ptr(x), H, _lib.ptr(dirty), H, _lib.ptr(dW), H * H, _lib.ptr(db), H, st), 'gm_dense_wgrad_centre')
            torch.cuda.synchronize()
            out.append((dW, db))
    assert torch.isfinite(out[1][0]).all() and out[0][0].abs().max() > 0
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32)) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
