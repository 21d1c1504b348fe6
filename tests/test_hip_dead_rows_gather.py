"""GPU (-m gpu): the GM_DEAD_ROWS=2 transposed aggregate leaves the rows nobody can observe alone.

A row of that launch whose GM_F_NORM_E1 carries the sign bit is not stored, and the launch writes no relu' bits: nothing such a row computes has a reader, so
it issues no edge-table load, no row gather and no mask load and skips its epilogue (agg.hip, agg_unobservable) -- in the windows, in the hub rows' own
workgroups (every part of a split one) and in the per-element kernel.  A launch that does write relu' bits still owes them to a flagged row.

Fixture: one batch over a store of two graphs.  Graph 0: hubs A = 0 and B = 1 joined by an edge, 300 leaves each, every edge stored both ways, the leaves of
A on the even ids and those of B on the odd ones -- in the subgraph around A (all 602 nodes, rows in id order) A's leaves are kept and B's are flagged, so the
flags ALTERNATE row by row, inside every side-by-side group of the 64- and 128-wide kernels; A's row (301 out-edges, split over two workgroups) is flagged and
B's is kept.  Graph 1: a 2,000-node preferential-attachment graph (m = 4), every edge stored both ways except those of the last node, which keeps its in-edges
only: as a centre it is a row without an out-edge.  The two-hop subgraphs around two of its large hubs (sampled to 1,000 nodes) hold by-source degrees from
0 to a few tens and hub rows of one workgroup, kept (a hub next to the centre) and flagged.  About 4,300 rows in nine subgraphs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_LEAF = 300
N_PA, M_PA = 2000, 4
SENTINEL = 0x7fc12345      # a NaN no kernel produces: "this output row was never stored"
WIDTHS = [64, 128, 256, 512]
FORCE = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)      # the forced-split knobs of tests/test_hip_dead_rows_bwd.py


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


def graphs_and_seeds():
    """[(n, src, dst)] of the two graphs and the batch's seeds (graph, centre, -1).  Host only."""
    from gmeta_amd import synth
    la, lb = 2 + 2 * np.arange(N_LEAF), 3 + 2 * np.arange(N_LEAF)
    u = np.concatenate([np.zeros(N_LEAF, np.int64), np.ones(N_LEAF, np.int64), [0]])
    v = np.concatenate([la, lb, [1]])
    star = (2 + 2 * N_LEAF, np.concatenate([u, v]), np.concatenate([v, u]))
    e = synth.pa_edges(N_PA, M_PA, np.random.default_rng(5))
    back = e[:, 1] != N_PA - 1                       # (u < v: the last node's edges are stored towards it only)
    pa = (N_PA, np.concatenate([e[:, 0], e[back, 1]]), np.concatenate([e[:, 1], e[back, 0]]))
    hubs = np.argsort(-np.bincount(e.reshape(-1), minlength=N_PA), kind='stable')
    # around A, two of A's leaves, B, one of B's leaves; the last node, a low-degree node, and two of the large hubs (their two-hop sets are sampled)
    seeds = [(0, c, -1) for c in (0, 2, 4, 1, 3)] + [(1, int(c), -1) for c in (N_PA - 1, N_PA - 700, hubs[1], hubs[4])]
    return [star, pa], seeds


@pytest.fixture(scope='module')
def fx():
    import gmeta_amd
    from gmeta_amd import _lib
    from gmeta_amd.subgraphs import SubgraphBatch
    graphs, seeds = graphs_and_seeds()
    rng = np.random.default_rng(3)
    store = gmeta_amd.GraphStore(graphs, [rng.standard_normal((g[0], 128)).astype(np.float32) for g in graphs])
    with tuning(**FORCE):
        B = SubgraphBatch.extract(store, seeds, [0, len(seeds)], 2, 1000, 222, False)
    ipt, ixt = B.csr(transposed=True)
    crow = (B.sub_off[:-1].astype(np.int64)[:, None] + B._read(_lib.F_CENTRE, B.subs * B.centres, np.int32).reshape(B.subs, B.centres)).reshape(-1)
    is_c = np.zeros(B.rows, bool); is_c[crow] = True
    deg = np.diff(ipt.astype(np.int64))
    src = np.repeat(np.arange(B.rows), deg)
    kept = np.zeros(B.rows, bool); kept[src[is_c[ixt]]] = True
    return dict(store=store, B=B, is_c=is_c, kept=kept, deg=deg, cache={})


def test_fixture_holds_what_the_change_touches(fx):
    """The batch is what the tests below take it for: the library's flags are the recomputed ones; by-source degrees 0, 1, 2, 3 and a few tens; a hub row of
    one workgroup kept and one flagged, a split hub row (from 192 edges) kept and one flagged; kept and flagged rows side by side in aligned groups of two and
    of four rows (the rows one wave works on together at widths 128 and 64), all four of a group's positions taken by either flag somewhere."""
    from gmeta_amd import _lib
    B, kept, deg = fx['B'], fx['kept'], fx['deg']
    assert 2000 <= B.rows <= 10000, B.rows
    e1 = B._read(_lib.F_NORM_E1, B.rows, np.float32).view(np.uint32)
    assert np.array_equal(e1 >> 31 == 0, kept)
    for d in (0, 1, 2, 3):
        assert (deg == d).any(), d
    heavy = 32 if B.edges <= 8 * B.rows else 64
    assert ((deg >= 20) & (deg <= heavy)).any()                                  # "a few tens", still a window row
    assert ((deg == 0) & ~kept).any() and ((deg >= 3) & (deg <= heavy) & kept).any() and ((deg >= 3) & (deg <= heavy) & ~kept).any()
    hub, split = (deg > heavy) & (deg < 192), deg >= 192
    for what, m in (('hub', hub), ('split hub', split)):
        assert (m & kept).any() and (m & ~kept).any(), (what, int((m & kept).sum()), int((m & ~kept).sum()))
    n4 = B.rows // 4 * 4
    k2, k4 = kept[:n4].reshape(-1, 2), kept[:n4].reshape(-1, 4)
    assert (k2[:, 0] != k2[:, 1]).sum() >= 100
    mixed = k4[k4.any(1) & ~k4.all(1)]
    assert len(mixed) >= 50 and mixed.any(0).all() and (~mixed).any(0).all()


def _operands(fx, width):
    """clean T (zero outside the centre rows), the same with NaN outside them, packed relu' bits.  One set per width, shared and left unchanged."""
    key = ('ops', width)
    if key not in fx['cache']:
        B = fx['B']
        g = torch.Generator(device='cuda'); g.manual_seed(7 + width)
        crow = torch.from_numpy(np.nonzero(fx['is_c'])[0]).cuda()
        clean = torch.zeros(B.rows + 1, width, device='cuda')
        clean[crow] = torch.randn(len(crow), width, device='cuda', generator=g)
        clean[crow[0], :4] = torch.tensor([-0.0, 0.0, 1e-40, 3e30], device='cuda')      # signed zeros, a subnormal, a huge value
        dirty = torch.full((B.rows + 1, width), float('nan'), device='cuda')
        dirty[crow] = clean[crow]
        mask = torch.randint(0, 16, (B.rows * width // 4,), device='cuda', generator=g, dtype=torch.int32).to(torch.uint8)
        fx['cache'][key] = (clean, dirty, mask)
    return fx['cache'][key]


def _centre_t(fx, T, width, mask, keep):
    from gmeta_amd import _lib
    B = fx['B']
    out = torch.full((B.rows, width), SENTINEL, device='cuda', dtype=torch.int32)
    _lib.check(_lib.lib().gm_dense_agg_centre_t(B.handle, _lib.ptr(T), width, _lib.ptr(mask), _lib.ptr(out), keep, _lib.stream_ptr()), 'gm_dense_agg_centre_t')
    return out


@pytest.mark.parametrize('width', WIDTHS)
def test_kept_rows_are_the_plain_launch_and_flagged_rows_are_left_alone(fx, width):
    """keep = 1 over a T that is NaN outside its centre rows against keep = 0 over the clean T: bitwise equal on the kept rows (hub rows and the split one
    among them), the sentinel untouched on every flagged row, T unwritten but for its zero row."""
    clean, dirty, mask = _operands(fx, width)
    dirty = dirty.clone()
    kept = torch.from_numpy(fx['kept']).cuda()
    not_c = ~torch.from_numpy(fx['is_c']).cuda()
    plain = _centre_t(fx, clean, width, mask, 0)
    keep = _centre_t(fx, dirty, width, mask, 1)
    torch.cuda.synchronize()
    assert bool((plain != SENTINEL).all())                               # the plain launch stores every row
    assert plain.view(torch.float32)[kept].abs().max() > 0
    assert bool((plain[~kept] == 0).all())                               # (what the flagged rows are by construction)
    assert torch.equal(plain[kept], keep[kept])
    assert bool((keep[~kept] == SENTINEL).all())
    B = fx['B']
    assert bool(torch.isnan(dirty[:B.rows][not_c]).all()) and bool((dirty[B.rows] == 0).all())
    assert torch.equal(dirty[:B.rows][~not_c].view(torch.int32), clean[:B.rows][~not_c].view(torch.int32))


@pytest.mark.parametrize('width', WIDTHS)
def test_hub_counters_after_skipped_rows(fx, width):
    """Three keep = 1 launches back to back on the same batch, then a keep = 0 launch: each output bitwise the first launch of its kind.  A flagged split hub
    row whose parts had taken a ticket without completing the round would leave its arrival counter off zero: the later launches would miss their last
    arriver (the row left unstored) or sum an incomplete set of partial rows."""
    clean, dirty, mask = _operands(fx, width)
    plain0 = _centre_t(fx, clean, width, mask, 0)
    keeps = [_centre_t(fx, dirty, width, mask, 1) for _ in range(3)]
    plain1 = _centre_t(fx, clean, width, mask, 0)
    torch.cuda.synchronize()
    assert bool((plain0 != SENTINEL).all())
    for k in keeps[1:]:
        assert torch.equal(k, keeps[0])
    assert torch.equal(plain1, plain0)
    split = torch.from_numpy(fx['deg'] >= 192).cuda()
    kept = torch.from_numpy(fx['kept']).cuda()
    assert torch.equal(keeps[2][split & kept], plain0[split & kept]) and bool((keeps[2][split & ~kept] == SENTINEL).all())


@pytest.mark.parametrize('width', [64, 256])
def test_flagged_rows_still_get_their_relu_bits(fx, width):
    """The pin of tests/test_hip_agg_numerics.py on this batch: a launch with s_out + keep_signed + relu + relu_bits writes the bits of EVERY row, the flagged
    ones included (bitwise those of the launch that stores every row), and leaves the flagged rows' values unstored."""
    from gmeta_amd import _lib
    B = fx['B']
    clean, _, _ = _operands(fx, width)
    kept = torch.from_numpy(fx['kept']).cuda()
    res = []
    for keep_signed, s_out in ((1, B.device_ptr(_lib.F_NORM_E1)), (0, B.device_ptr(_lib.F_NORM))):
        out = torch.full((B.rows, width), SENTINEL, device='cuda', dtype=torch.int32)
        bits = torch.full((B.rows * width // 4,), 0xA5, dtype=torch.uint8, device='cuda')
        launched = C.c_int32(-1)
        _lib.check(_lib.lib().gm_dense_aggregate(B.handle, 1, 3, _lib.ptr(clean), width, width, 0, None, s_out, keep_signed, None, 0, 1, _lib.ptr(bits), None, None,
                                                 2, None, 0, 0, 0, 1, 0, 0, _lib.ptr(out), C.byref(launched), _lib.stream_ptr()), 'gm_dense_aggregate')
        torch.cuda.synchronize()
        assert launched.value >= 0
        res.append((out, bits.view(B.rows, width // 4)))
    (out_k, bits_k), (out_p, bits_p) = res
    assert bool((bits_k < 16).all())
    assert torch.equal(bits_k, bits_p) and bool(bits_p[kept].any()) and bool((bits_p[~kept] == 0).all())
    assert bool((out_k[~kept] == SENTINEL).all()) and torch.equal(out_k[kept], out_p[kept])
    assert out_p.view(torch.float32)[kept].max() > 0
