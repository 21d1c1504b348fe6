"""Helpers of tests/test_hip_dead_tiles.py (GM_DEAD_TILES: a fused split GEMM that stores the rows of a keep vector only issues the MFMAs of a tile without a
kept row and nothing else of it).  No GPU and no library needed here.

Layouts: a batch is a list of sets, a set a list of subgraphs (rows, centre position).  Every subgraph is a run of consecutive rows with its edges inside
(fused_ref.build_sets over the subgraph sizes), so the batch's centre rows -- the only rows the centre keep vector keeps -- sit exactly where the layout puts
them, and a 128-row tile of a set is LIVE for the centre set iff a centre lies in it.

Ownership: workgroup b of a launch of G workgroups walks the hardware tile ids b, b + G, .. in the XCD-contiguous order of k_gemm_split_p (gemm_split.h),
restated in `logical`; `owned` gives every workgroup's tiles in the order it walks them."""
import numpy as np

TILE = 128


def tile_table(set_rows):
    """(set, row0, nrows) of every GEMM tile, in the batch's order"""
    out, r0 = [], 0
    for t, n in enumerate(set_rows):
        for k in range(0, n, TILE):
            out.append((t, r0 + k, min(TILE, n - k)))
        r0 += n
    return out


def tile_flags(set_rows, keep):
    """int32 [tiles]: 1 where some row of the tile is kept (keep: bool [rows])"""
    keep = np.asarray(keep, bool)
    return np.array([1 if keep[r0:r0 + n].any() else 0 for _, r0, n in tile_table(set_rows)], np.int32)


def logical(t, n_tiles):
    """hardware work id -> tile of the batch (the kernel's XCD-contiguous order over n_tiles tiles)"""
    q8, r8 = divmod(n_tiles, 8)
    x, i = t % 8, t // 8
    return (x * (q8 + 1) if x < r8 else r8 * (q8 + 1) + (x - r8) * q8) + i


def owned(n_tiles, G):
    """the tiles of every workgroup of a G-workgroup launch, in walking order"""
    G = min(G, n_tiles)
    return [[logical(t, n_tiles) for t in range(b, n_tiles, G)] for b in range(G)]


def patterns(set_rows, flags, G):
    """which of the situations the kernel's list handling must get right occur in this launch"""
    tt = tile_table(set_rows)
    got = set()
    for tiles in owned(len(tt), G):
        lv = [int(flags[t]) for t in tiles]
        if not any(lv):
            got.add('no_live')
            continue
        if not lv[0]:
            got.add('first_dead')
        if not lv[-1]:
            got.add('last_dead')
        live_at = [i for i, v in enumerate(lv) if v]
        for a, b in zip(live_at, live_at[1:]):
            if b - a - 1 >= 3:
                got.add('run3')
                if tt[tiles[a]][0] != tt[tiles[b]][0]:
                    got.add('set_change_over_run')
        if all(lv):
            got.add('wg_all_live')
    if all(flags):
        got.add('all_live')
    for (_, _, n), f in zip(tt, flags):
        if n < TILE:
            got.add('partial_live' if f else 'partial_dead')
    if len(tt) == 1:
        got.add('single')
    return got


# ---------------------------------------------------------------------------------------------------- layouts
def layout(name):
    """list of sets, each a list of (rows, centre position) subgraphs"""
    rng = np.random.default_rng(5)
    if name == 'sparse':
        # 30 sets of one to three subgraphs of 3 .. 7 tiles: ~300 tiles, about a fifth of them live; some last tiles partial, with and without a centre
        sets = []
        for t in range(30):
            n_sub = 1 + t % 3
            subs = []
            for s in range(n_sub):
                rows = int(rng.integers(3, 8)) * TILE + (int(rng.integers(1, TILE)) if (s == n_sub - 1 and t % 2 == 0) else 0)
                subs.append((rows, int(rng.integers(0, rows))))
            sets.append(subs)
        sets[0][-1] = (sets[0][-1][0], sets[0][-1][0] - 1)       # a live partial last tile: the centre is the set's last row
        sets[2][-1] = (sets[2][-1][0], 0)                        # a dead one: the centre is the subgraph's first row, tiles away
        return sets
    if name == 'lonely':                                         # 41 tiles, two of them live: most workgroups of a 7-workgroup launch own no live tile
        return [[(20 * TILE + 40, 3 * TILE + 9)], [(20 * TILE, 11 * TILE + 127)]]
    if name == 'all_live':                                       # every tile holds a centre, the partial last tiles too
        return [[(TILE, 5)] * 6 + [(77, 76)], [(TILE, 127)] * 9, [(TILE, 0)] * 4 + [(1, 0)]]
    assert name == 'single'
    return [[(90, 17)]]


def layout_rows(sets):
    """(set_rows, subgraph rows, subgraphs per set, centre rows)"""
    set_rows = [sum(r for r, _ in subs) for subs in sets]
    sub_rows = [r for subs in sets for r, _ in subs]
    centres, r0 = [], 0
    for subs in sets:
        for r, c in subs:
            assert 0 <= c < r
            centres.append(r0 + c)
            r0 += r
    return set_rows, sub_rows, [len(s) for s in sets], np.array(centres, np.int64)
