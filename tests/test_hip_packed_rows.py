"""GPU (-m gpu): GM_PACK_ROWS -- a fused three-piece split GEMM that would take the batch's tile flags (tests/test_hip_dead_tiles.py) takes the row set's PACKED
tiles instead: the kept rows of every set (task), ascending by row, fill the fewest 128-row tiles (gm_batch::pack; tables 15 .. 20 of gm_dense_agg_table), the
launch feeds exactly those and stores row r of a packed tile at its own row of C, and every other tile of the dense schedule issues its MFMAs alone.  An output row
of an MFMA tile depends on its own operand row and the weights only, not on the slot it sits in, and a row's chunk and product order is unchanged, so everything
here is compared BITWISE: packed against the launch without flags, GM_PACK_ROWS 1 against 0.

Layouts (subgraph = consecutive nodes of one parent graph, edges inside it; the centre's in-edges chosen so that the second row set -- the sources of the centres'
in-edges -- keeps a chosen number of rows):
  five    5 sets of 127 / 128 / 129 / 300 / 130 rows whose e1 set keeps 0 / 1 / 128 / 129 (a one-row tail tile) / every row
  ones    2 sets: 129 one-row subgraphs (the centre set keeps every row, 129 = a full tile and a one-row tail), 128 two-row subgraphs (exactly 128 of 256 rows)
  single  1 set of 300 rows
  sparse  the ~300-tile layout of tests/dead_tiles_ref.py (30 sets): workgroups own many tiles at grid 1, 2, 7"""
import argparse
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

import dead_tiles_ref as D

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc12345      # a NaN no kernel produces: "this output row was never stored"
GRIDS = (1, 2, 7, 0)
TILE = 128
F0 = 128                   # feature width of the stores here: the feature-table loader runs at K = 128


def _L():
    from gmeta_amd import _lib as L
    return L


def layout(name):
    """list of sets, each a list of (rows, centre position, distinct sources of the centre's in-edges; -1: every row of the subgraph, the centre included)"""
    if name == 'five':
        return [[(127, 0, 0)], [(128, 5, 1)], [(129, 128, 128)], [(300, 17, 129)], [(130, 64, -1)]]
    if name == 'ones':
        return [[(1, 0, 0)] * 129, [(2, 1, 1)] * 128]
    if name == 'single':
        return [[(300, 299, 40)]]
    assert name == 'sparse'
    rng = np.random.default_rng(11)
    return [[(r, c, int(rng.integers(0, 6))) for r, c in subs] for subs in D.layout('sparse')]


class Env:
    pass


@functools.lru_cache(maxsize=None)
def env(name, link=False):
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    L = _L()
    e = Env()
    sets = layout(name)
    rng = np.random.default_rng(31 + len(name))
    src, dst, lists, seeds, r0 = [], [], [], [], 0
    e.set_rows, e.c_bound, e.e_bound = [], [], []
    for subs in sets:
        n_in = 0
        for rows, c, k in subs:
            others = np.array([r for r in range(rows) if r != c], np.int64)
            into_c = np.arange(rows) if k < 0 else rng.permutation(others)[:k]
            assert k < 0 or len(into_c) == k
            src += list(r0 + into_c); dst += [r0 + c] * len(into_c)
            for r in others:                                  # background edges: zero to three distinct sources per other row
                s = rng.permutation(rows)[:int(rng.integers(0, 4))]
                src += list(r0 + s); dst += [r0 + int(r)] * len(s)
            lists.append(np.arange(r0, r0 + rows, dtype=np.int32))
            seeds.append((0, r0 + c, r0 + c) if link else (0, r0 + c, -1))      # link: the pair (c, c) -- two centres on one row
            n_in += len(into_c) * (2 if link else 1)
            r0 += rows
        e.set_rows.append(sum(s[0] for s in subs))
        e.c_bound.append(min(len(subs) * (2 if link else 1), e.set_rows[-1]))
        e.e_bound.append(min(n_in, e.set_rows[-1]))
    e.rows = r0
    feats = torch.randn(e.rows, F0, generator=torch.Generator().manual_seed(3)).numpy()
    e.store = gmeta_amd.GraphStore([(e.rows, np.array(src, np.int64), np.array(dst, np.int64))], [feats])
    e.B = SubgraphBatch.from_nodes(e.store, np.array(seeds, np.int32), np.concatenate([[0], np.cumsum([len(s) for s in sets])]), lists, link)
    assert e.B.rows == e.rows and e.B.sets == len(sets)
    e.keep = [~np.signbit(e.B._read(f, e.rows, np.float32)) for f in (L.F_NORM_CENTRE, L.F_NORM_E1)]
    e.n_tiles = len(D.tile_table(e.set_rows))
    return e


def _table(e, which, n):
    L = _L()
    t = torch.full((max(n, 1),), -7, dtype=torch.int32, device='cuda')
    L.check(L.lib().gm_dense_agg_table(e.B.handle, which, 0, L.ptr(t), n, L.stream_ptr()), 'gm_dense_agg_table')
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n]


# ---------------------------------------------------------------------------------------------------- the tables
def check_tables(e):
    so = np.concatenate([[0], np.cumsum(e.set_rows)])
    for k in (0, 1):
        kept = [np.flatnonzero(e.keep[k][so[t]:so[t + 1]]) + so[t] for t in range(len(e.set_rows))]
        bound = e.c_bound if k == 0 else e.e_bound
        assert all(len(kept[t]) <= bound[t] for t in range(len(kept))), (k, [len(x) for x in kept], bound)
        base = np.concatenate([[0], np.cumsum(bound)])
        want_tiles = sum((len(x) + TILE - 1) // TILE for x in kept)
        count = int(_table(e, 19 + k, 1)[0])
        assert count == want_tiles, (k, count, want_tiles)
        cap_tiles = sum((b + TILE - 1) // TILE for b in bound)
        assert count <= cap_tiles <= e.n_tiles
        tiles = _table(e, 17 + k, 3 * count).reshape(count, 3)
        rowid = _table(e, 15 + k, int(base[-1]))
        at = 0
        for t, rows_t in enumerate(kept):                     # sets in order; a set without a kept row has no tile
            for j in range(0, len(rows_t), TILE):
                s, off, n = (int(v) for v in tiles[at]); at += 1
                assert s == t and off == base[t] + j and n == min(TILE, len(rows_t) - j), (k, t, j, s, off, n)      # no tile mixes sets; offsets and nrows consistent
                assert np.array_equal(rowid[off:off + n], rows_t[j:j + n])                                        # ascending within the set
        assert at == count
    L = _L()
    t = torch.empty(8, dtype=torch.int32, device='cuda')
    assert L.lib().gm_dense_agg_table(e.B.handle, 19, 0, L.ptr(t), 2, L.stream_ptr()) == -1                      # GM_EINVAL: the count is one word


@pytest.mark.parametrize('name', ['five', 'ones', 'single', 'sparse'])
def test_packed_tables_equal_their_reconstruction(name):
    e = env(name)
    so = np.concatenate([[0], np.cumsum(e.set_rows)])
    per_set = [[int(e.keep[k][so[t]:so[t + 1]].sum()) for t in range(len(e.set_rows))] for k in (0, 1)]
    if name == 'five':                                        # the cases are there: 0 / 1 / 128 / 129 / every row kept; sets of 127, 128, 129 and 300 rows; 5 sets
        assert per_set[1] == [0, 1, 128, 129, 130] and e.set_rows == [127, 128, 129, 300, 130] and per_set[0] == [1] * 5
    if name == 'ones':                                        # 2 sets; every row kept over a tile border; exactly one full tile
        assert per_set[0] == [129, 128] and e.set_rows == [129, 256]
    if name == 'single':
        assert len(e.set_rows) == 1
    check_tables(e)


def test_packed_tables_link_mode_two_centres_on_one_row():
    e = env('five', True)
    assert e.B.centres == 2
    assert int(e.keep[0].sum()) == 5                          # ten centres on five rows
    check_tables(e)


# ---------------------------------------------------------------------------------------------------- the launches
@functools.lru_cache(maxsize=None)
def operands(name, K, N):
    e = env(name)
    g = torch.Generator().manual_seed(1000 * K + N)
    T = len(e.set_rows)
    x, zs = torch.randn(e.rows, K, generator=g), torch.randn(e.rows, K, generator=g)
    W = torch.randn(T, K, N, generator=g) / K ** 0.5
    bias = torch.randn(T, N, generator=g)
    return x.cuda(), zs.cuda(), W.cuda(), bias.cuda()


def launch(name, rowset, table, K, N, packed, grid, epi):
    L = _L()
    e = env(name)
    x, zs, W, bias = operands(name, K, N)
    out = torch.full((e.rows, N), SENTINEL, dtype=torch.int32, device='cuda')
    launched = C.c_int32(-1)
    b = L.ptr(bias) if epi else None
    if packed:
        L.check(L.lib().gm_dense_fused_gemm_packed(e.B.handle, rowset, grid, table, L.ptr(x), K, K, L.ptr(zs), K, L.ptr(W), K * N, N, L.ptr(out), N, b, N, 1 if epi else 0,
                                                   C.byref(launched), L.stream_ptr()), 'gm_dense_fused_gemm_packed')
    else:                                                     # the set's keep vector, no tile flags
        L.check(L.lib().gm_dense_fused_gemm_rows(e.B.handle, rowset, 1, 0, grid, table, L.ptr(x), K, K, L.ptr(zs), K, None, K, L.ptr(W), K * N, N, L.ptr(out), N, b, N,
                                                 1 if epi else 0, None, None, None, 1, C.byref(launched), L.stream_ptr()), 'gm_dense_fused_gemm_rows')
    torch.cuda.synchronize()
    return out.cpu().numpy(), launched.value


def check_pair(name, rowset, table, K, N, grid, epi):
    e = env(name)
    on, kid_on = launch(name, rowset, table, K, N, True, grid, epi)
    off, kid_off = launch(name, rowset, table, K, N, False, grid, epi)
    assert kid_on == kid_off == (40 if N == 256 else 44)
    keep = e.keep[rowset]
    assert (off[keep] != SENTINEL).all() and (off[~keep] == SENTINEL).all()
    assert np.array_equal(on, off)                            # the whole buffer, byte for byte: kept rows as the unpacked launch stores them, no other row touched


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('epi', [False, True])
@pytest.mark.parametrize('rowset', [0, 1])
def test_table_0_k256_n256(rowset, epi, grid):
    for name in ('five', 'sparse'):
        check_pair(name, rowset, 0, 256, 256, grid, epi)


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('epi', [False, True])
def test_feature_table_loader_k128_n256(epi, grid):
    for name in ('five', 'sparse'):
        check_pair(name, 1, 1, F0, 256, grid, epi)


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('rowset', [0, 1])
def test_n128(rowset, grid):
    check_pair('five', rowset, 0, 128, 128, grid, True)
    check_pair('sparse', rowset, 0, 64, 128, grid, rowset == 0)


@pytest.mark.parametrize('grid', GRIDS)
def test_special_layouts(grid):
    """every row of a set kept over a tile border; one set; one-row subgraphs"""
    for name in ('ones', 'single'):
        for rowset in (0, 1):
            check_pair(name, rowset, 0, 128, 256, grid, True)


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('N', [128, 256])
def test_packed_dz_against_dense_dz_centre(N, grid):
    L = _L()
    for name in ('five', 'sparse'):
        e = env(name)
        K = 256
        g = torch.Generator().manual_seed(7 + N)
        dQ = torch.randn(e.rows, K, generator=g).cuda()      # (off the centre rows: bytes nobody reads)
        W = (torch.randn(len(e.set_rows), N, K, generator=g) / K ** 0.5).cuda()
        outs = []
        for kind in ('all', 'rows', 'packed'):
            T = torch.full((e.rows, N), SENTINEL, dtype=torch.int32, device='cuda')
            if kind == 'all':
                L.check(L.lib().gm_dense_dz_centre(e.B.handle, L.ptr(dQ), K, L.ptr(W), N * K, N, L.ptr(T), L.stream_ptr()), 'gm_dense_dz_centre')
            else:
                L.check(L.lib().gm_dense_dz_centre_rows(e.B.handle, L.ptr(dQ), K, L.ptr(W), N * K, N, L.ptr(T), 1 if kind == 'packed' else 0, grid, L.stream_ptr()),
                        'gm_dense_dz_centre_rows')
            torch.cuda.synchronize()
            outs.append(T.cpu().numpy())
        full, rows, packed = outs
        keep = e.keep[0]
        assert (full != SENTINEL).all()
        assert np.array_equal(packed[keep], full[keep]) and (packed[~keep] == SENTINEL).all()
        assert np.array_equal(packed, rows)


# ---------------------------------------------------------------------------------------------------- the step
def test_meta_step_is_bitwise_the_step_without_packing():
    """one two-layer arxiv-shaped Meta.forward (the world of tests/test_hip_pass_plan.py, split kernels forced) at GM_PACK_ROWS 0 and 1: accuracies, query losses,
    meta-gradient and parameters; and on a configuration that is not eligible (two pieces per operand), where the knob changes nothing"""
    from test_hip_dead_rows_diff import _step
    from test_hip_dead_rows_fwd import _assert_bitwise, _world
    w = _world(True)
    force = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
    off, on = _step(w, GM_PACK_ROWS=0, **force), _step(w, GM_PACK_ROWS=1, **force)
    assert all(np.isfinite(off[k]).all() for k in ('accs', 'losses', 'grad', 'theta')) and np.abs(off['grad']).max() > 0
    _assert_bitwise(on, off)
    _assert_bitwise(on, _step(w, GM_PACK_ROWS=1, GM_DEAD_TILES=0, **force))
    off2, on2 = _step(w, pieces=2, GM_PACK_ROWS=0, **force), _step(w, pieces=2, GM_PACK_ROWS=1, **force)
    _assert_bitwise(on2, off2)


def test_link_prediction_step_is_bitwise_the_step_without_packing():
    """the FirstMM-shaped link world of tests/test_hip_dead_rows_diff.py (two centres per subgraph, hidden 128, split kernels forced)"""
    import gmeta_amd
    from gmeta_amd import synth
    from test_hip_dead_rows_diff import _flat, tuning
    from test_hip_dead_rows_fwd import _assert_bitwise
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args('firstmm', task_num=4, k_spt=4, k_qry=8, update_step=2, update_step_test=2, n_graphs=6)
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=cfg['n_way'], k_shot=cfg['k_spt'], k_query=cfg['k_qry'], batchsz=4, args=args, adjs=store,
                             h=cfg['h'], tables=data['tables'], verbose=False)
    batch = db.get_batch(list(range(4)))
    config = synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], synth.n_out(cfg), link=True)

    def run(pack):
        with tuning(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0, GM_PACK_ROWS=pack):
            torch.manual_seed(222)
            m = gmeta_amd.Meta(argparse.Namespace(**vars(args)), config).to('cuda')
            accs = np.asarray(m(*batch, None)).copy()
            torch.cuda.synchronize()
            return dict(accs=accs, losses=np.asarray(m.last_stats['losses_q']).copy(), grad=_flat(m, True), theta=_flat(m))
    on, off = run(1), run(0)
    assert np.isfinite(on['grad']).all() and np.abs(on['grad']).max() > 0
    _assert_bitwise(on, off)
