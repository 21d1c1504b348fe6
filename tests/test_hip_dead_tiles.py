"""GPU (-m gpu): GM_DEAD_TILES -- a fused three-piece split GEMM that stores the rows of a keep vector only (a forward-only layer stored on the centre rows or on
the sources of their in-edges; the table-read dZ launch) takes the batch's tile flags: a 128-row tile without a kept row issues its MFMAs on zero registers and
nothing else -- no table fetch, no operand load, no LDS traffic, no barrier, no epilogue (gemm_split.h: SplitGemmK::tile_live).  A live tile does what it did, so
everything here is compared BITWISE, flags on against flags off.

Stand-alone launches go through gm_dense_fused_gemm_rows (table 0: x over batch rows) on the layouts of tests/dead_tiles_ref.py, with the workgroup count forced
to 1, 2 and 7 so that a workgroup owns many tiles (on an MI355X a small batch otherwise gets one tile per workgroup), and 0 = the library's own rule.  C is
pre-filled with a sentinel; x and zside hold NaN in every row that no kept row's table entry names; kept rows come out bit for bit what the launch without the flags
stores, every other row keeps the sentinel.  test_layouts_cover_the_list_cases asserts on the host that the launches contain: a workgroup whose first / last tile
is dead, runs of three and more dead tiles between live ones, a workgroup without a live tile, every tile live, a dead and a live partial last tile, a
single-tile launch, and a change of set (per-set weights) across a dead run."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dead_tiles_ref as D
import fused_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc12345      # a NaN no kernel produces: "this output row was never stored"
GRIDS = (1, 2, 7, 0)


def _L():
    from gmeta_amd import _lib as L
    return L


class Env:
    pass


@functools.lru_cache(maxsize=None)
def env(name):
    """the batch of layout `name`: subgraph k is the consecutive nodes of one parent graph, its centre where the layout puts it"""
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    L = _L()
    e = Env()
    e.name = name
    e.set_rows, sub_rows, subs_per_set, e.centres = D.layout_rows(D.layout(name))
    rows, src, dst, _ = R.build_sets(sub_rows, 23 + len(name))
    e.rows = rows
    store = gmeta_amd.GraphStore([(rows, src.astype(np.int64), dst.astype(np.int64))], [np.zeros((rows, 8), np.float32)])
    so = np.concatenate([[0], np.cumsum(sub_rows)])
    lists = [np.arange(so[k], so[k + 1], dtype=np.int32) for k in range(len(sub_rows))]
    seeds = np.array([(0, int(c), -1) for c in e.centres], np.int32)
    e.store = store
    e.B = SubgraphBatch.from_nodes(store, seeds, np.concatenate([[0], np.cumsum(subs_per_set)]), lists, False)
    assert e.B.rows == rows and e.B.sets == len(e.set_rows)
    assert [int(v) for v in np.diff(e.B.sub_off[e.B.set_sub_off])] == e.set_rows
    e.n_tiles = len(D.tile_table(e.set_rows))
    e.keep = []
    for field in (L.F_NORM_CENTRE, L.F_NORM_E1):
        e.keep.append(~np.signbit(e.B._read(field, rows, np.float32)))
    is_c = np.zeros(rows, bool); is_c[e.centres] = True
    assert np.array_equal(e.keep[0], is_c)
    e.flags = [D.tile_flags(e.set_rows, k) for k in e.keep]
    e.tabs = []
    for which in (7, 8):
        t = torch.empty(rows, 4, dtype=torch.int32, device='cuda')
        L.check(L.lib().gm_dense_agg_table(e.B.handle, which, 0, L.ptr(t), rows, L.stream_ptr()), 'gm_dense_agg_table')
        torch.cuda.synchronize()
        e.tabs.append(t.cpu().numpy())
    return e


@functools.lru_cache(maxsize=None)
def operands(name, rowset, K, N, inf_w=False):
    """x and zside: finite on the rows the set's table names (sources of kept rows / the kept rows' own finished rows), NaN everywhere else; per-set W and bias"""
    e = env(name)
    g = torch.Generator().manual_seed(1000 * K + N + rowset)
    named, own = R.table_sources(e.tabs[rowset])
    x = torch.full((e.rows, K), float('nan'))
    x[torch.from_numpy(named)] = torch.randn(len(named), K, generator=g)
    zs = torch.full((e.rows, K), float('nan'))
    zs[torch.from_numpy(own)] = torch.randn(int(own.sum()), K, generator=g)
    T = len(e.set_rows)
    W = torch.randn(T, K, N, generator=g) / K ** 0.5
    if inf_w:
        W[:, 3, 5] = float('inf')
    bias = torch.randn(T, N, generator=g)
    return x.cuda(), zs.cuda(), W.cuda(), bias.cuda()


def launch(name, rowset, K, N, live_on, grid, keep=1, relu_bits=False, zero_out=False, mode=1, inf_w=False):
    L = _L()
    e = env(name)
    x, zs, W, bias = operands(name, rowset, K, N, inf_w)
    out = torch.full((e.rows, N), SENTINEL, dtype=torch.int32, device='cuda')
    bits = torch.full((e.rows * N // 4,), 0xA5, dtype=torch.uint8, device='cuda') if relu_bits else None
    zero = torch.full((e.rows, N), SENTINEL, dtype=torch.int32, device='cuda') if zero_out else None
    slots = torch.zeros(len(e.set_rows) * 64, dtype=torch.int32, device='cuda') if mode == 2 else None
    zfull = torch.full((e.rows, K), 16.0, device='cuda') if mode == 2 else None      # (what the two-piece A bounds are taken over: above every |entry| of x and zside)
    launched = C.c_int32(-1)
    L.check(L.lib().gm_dense_fused_gemm_rows(e.B.handle, rowset, keep, 1 if live_on else 0, grid, 0, L.ptr(x), K, K, L.ptr(zs), K, L.ptr(zfull), K, L.ptr(W), K * N, N,
                                             L.ptr(out), N, L.ptr(bias), N, 1, L.ptr(bits), L.ptr(zero), L.ptr(slots), mode, C.byref(launched), L.stream_ptr()),
            'gm_dense_fused_gemm_rows')
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), bits=None if bits is None else bits.cpu().numpy(), zero=None if zero is None else zero.cpu().numpy(), kid=launched.value)


def check_pair(name, rowset, K, N, grid, inf_w=False):
    e = env(name)
    on, off = launch(name, rowset, K, N, True, grid, inf_w=inf_w), launch(name, rowset, K, N, False, grid, inf_w=inf_w)
    want_kid = 40 if N == 256 else 44
    assert on['kid'] == off['kid'] == want_kid
    keep = e.keep[rowset]
    assert (off['out'][keep] != SENTINEL).all() and (off['out'][~keep] == SENTINEL).all()      # the launch without flags: kept rows stored, no other
    assert np.array_equal(on['out'][keep], off['out'][keep])
    assert (on['out'][~keep] == SENTINEL).all()
    return on


# ---------------------------------------------------------------------------------------------------- the cases are there
def test_layouts_cover_the_list_cases():
    need = {'first_dead', 'last_dead', 'run3', 'no_live', 'all_live', 'partial_dead', 'partial_live', 'single', 'set_change_over_run'}
    got = set()
    for name in ('sparse', 'lonely', 'all_live', 'single'):
        e = env(name)
        for G in (1, 2, 7):
            got |= D.patterns(e.set_rows, e.flags[0], G)
    assert need <= got, need - got
    e = env('sparse')
    assert 200 <= e.n_tiles <= 400 and len(e.set_rows) >= 2
    for G in (1, 2, 7):      # the many-tile launches of the K x N sweep hold the list cases themselves
        assert {'first_dead', 'run3', 'set_change_over_run', 'partial_dead', 'partial_live'} <= D.patterns(e.set_rows, e.flags[0], G)
    # the second row set is not the first, and has dead tiles too
    assert not np.array_equal(e.flags[0], e.flags[1]) and 0 < e.flags[1].sum() < e.n_tiles


# ---------------------------------------------------------------------------------------------------- the flags
@pytest.mark.parametrize('name', ['sparse', 'lonely', 'all_live', 'single'])
def test_flags_equal_their_recomputation(name):
    """gm_batch::d_tile_live (tables 13 / 14 of gm_dense_agg_table) against the keep vectors' sign bits, tile by tile"""
    L = _L()
    e = env(name)
    for k in (0, 1):
        t = torch.full((e.n_tiles,), -7, dtype=torch.int32, device='cuda')
        L.check(L.lib().gm_dense_agg_table(e.B.handle, 13 + k, 0, L.ptr(t), e.n_tiles, L.stream_ptr()), 'gm_dense_agg_table')
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        assert np.array_equal((got != 0).astype(np.int32), e.flags[k]), (name, k)
        assert set(np.unique(got)) <= {0, 1}
    t = torch.empty(e.n_tiles + 1, dtype=torch.int32, device='cuda')
    assert L.lib().gm_dense_agg_table(e.B.handle, 13, 0, L.ptr(t), e.n_tiles + 1, L.stream_ptr()) == -1      # GM_EINVAL: more entries than tiles


# ---------------------------------------------------------------------------------------------------- the launches
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('N', [128, 256])
@pytest.mark.parametrize('K', [64, 128, 256])
def test_kept_rows_bitwise_and_nothing_else_stored(K, N, grid):
    check_pair('sparse', 0, K, N, grid)


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('name', ['lonely', 'all_live', 'single'])
def test_special_layouts(name, grid):
    """workgroups without a live tile; every tile live (trivially the launch without flags); one tile"""
    for K, N in ((128, 256), (64, 128)):
        check_pair(name, 0, K, N, grid)


@pytest.mark.parametrize('grid', GRIDS)
def test_sources_of_the_centres_in_edges(grid):
    """the second row set: the flags of GM_F_NORM_E1 under its own table"""
    check_pair('sparse', 1, 128, 256, grid)
    check_pair('lonely', 1, 256, 128, grid)


@pytest.mark.parametrize('grid', [1, 7, 0])
def test_inf_in_the_weights(grid):
    """a non-finite weight makes every row of a live tile NaN and changes nothing about which rows are stored"""
    on = check_pair('sparse', 0, 128, 256, grid, inf_w=True)
    e = env('sparse')
    assert np.isnan(on['out'][e.keep[0]].view(np.float32)).any()


# ---------------------------------------------------------------------------------------------------- eligibility
def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in ('out', 'bits', 'zero'))


@pytest.mark.parametrize('grid', [2, 0])
def test_launches_that_leave_more_than_the_kept_rows_take_the_old_path(grid):
    """relu' bits / the zero fill are written for EVERY row: with flags the launch must still walk every tile.  Without a keep vector every row is stored."""
    e = env('sparse')
    rows_n = e.rows * 256
    for kw in (dict(relu_bits=True), dict(zero_out=True), dict(keep=0)):
        on, off = launch('sparse', 0, 128, 256, True, grid, **kw), launch('sparse', 0, 128, 256, False, grid, **kw)
        assert on['kid'] == off['kid'] == 40 and _same(on, off), kw
        if kw.get('relu_bits'):
            assert on['bits'].size == rows_n // 4 and (on['bits'] < 16).all()      # every byte written (a sentinel byte is 0xA5)
        if kw.get('zero_out'):
            assert (on['zero'] == 0).all()
        if kw.get('keep') == 0:
            assert (on['out'] != SENTINEL).all()


def test_two_piece_launch_ignores_the_flags():
    on, off = launch('sparse', 0, 128, 256, True, 2, mode=2), launch('sparse', 0, 128, 256, False, 2, mode=2)
    assert on['kid'] == off['kid'] == 41 and _same(on, off)
    e = env('sparse')
    assert (on['out'][~e.keep[0]] == SENTINEL).all() and (on['out'][e.keep[0]] != SENTINEL).all()


def test_keep_launch_is_priced_on_the_kept_row_count_it_was_given():
    """launch accounting, category 13 (A rows read once + the C rows the launch stores): a launch with a keep vector prices the kept-row count that comes with the
    vector (gemm_keep_rows of csrc/model.hip sets both).  Through this export that count is every row of the batch, so the launch is priced exactly as the one
    without a keep vector: 4 rows (K + N) bytes -- a count that went missing would price 4 rows K."""
    L = _L()
    e = env('sparse')
    K, N = 128, 256
    for keep in (1, 0):
        ms, n, work = C.c_double(), C.c_int64(), C.c_int64()
        L.lib().gm_profile_enable(1)
        try:
            launch('sparse', 0, K, N, True, 0, keep=keep)
            L.lib().gm_profile_read(13, C.byref(ms), C.byref(n), C.byref(work))
        finally:
            L.lib().gm_profile_enable(0)
        assert work.value == 4 * e.rows * (K + N), (keep, work.value, 4 * e.rows * (K + N))


# ---------------------------------------------------------------------------------------------------- the step
def test_meta_step_is_bitwise_the_step_without_the_flags():
    """one two-layer arxiv-shaped Meta.forward (the world of tests/test_hip_pass_plan.py, split kernels forced) at GM_DEAD_TILES 0 and 1: accuracies, query losses,
    meta-gradient and parameters"""
    from test_hip_dead_rows_diff import _step
    from test_hip_dead_rows_fwd import _assert_bitwise, _world
    w = _world(True)
    force = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
    off, on = _step(w, GM_DEAD_TILES=0, **force), _step(w, GM_DEAD_TILES=1, **force)
    assert all(np.isfinite(off[k]).all() for k in ('accs', 'losses', 'grad', 'theta')) and np.abs(off['grad']).max() > 0
    _assert_bitwise(on, off)
