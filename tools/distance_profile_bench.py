"""Time of the joint hop-distance profiles on the device (gm_store_pair_distance_profile), reported with no target: the bit-parallel search of
gm_store_pair_distance over the pairs' columns, one transposition of the level's new bits per level into node-major planes, and a count that reads
2 (D + 1) ceil(N / 64) plane words per pair.  Case: the arxiv-shaped synthetic graph of the other pair benchmarks (synth.CONFIGS['arxiv']).

    python tools/distance_profile_bench.py [--reps 5] [--warmup 2] [--out profiles/distance_profile.txt]

1,000 and 10,000 pairs (half edges, half negatives), masked and unmasked, max_dist 2, 3 and 7.  End to end: HIP events around the C call, median (min - max) of
--reps after --warmup.  Per phase: one more call under GM_TIMING, where the library synchronises the stream behind the search, the transpositions and the count
of every group and prints the three sums (host clock; the sum exceeds the end-to-end time by those synchronisations).  The plane bytes -- written by the
transpositions, read by the count -- per second of their phase against the box's HBM copy rate (bench.py's box_calibration, measured in this process).
The comparison is what a caller did before this call existed: GraphStore.node_distances of both endpoints, 2 N bytes per pair over PCIe, and a 2-D histogram
per pair in numpy; timed on --host_pairs pairs, scaled to the list, and held equal to the device's tables (unmasked only: node_distances has no mask flag).
One JSON line per measurement; --out appends a plain-text table."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gmeta_amd                         # noqa: E402
from gmeta_amd import _lib, synth        # noqa: E402
from pair_distance_bench import timed    # noqa: E402

DISTS = (2, 3, 7)
SIZES = (1000, 10000)
NAME = 'gm_store_pair_distance_profile'


def phases(call):
    """(groups, columns searched with the padding, search ms, transpose ms, count ms) of one call under GM_TIMING: the line the library prints to stderr."""
    lib = _lib.lib()
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as f:
        os.dup2(f.fileno(), 2)
        try:
            assert lib.gm_set_tuning(b'GM_TIMING', 1) == 0
            call()
            torch.cuda.synchronize()
        finally:
            lib.gm_set_tuning(b'GM_TIMING', 0)
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode('utf-8', 'replace')
    m = re.search(r'%s groups (\d+) columns (\d+) search ([\d.]+) us transpose ([\d.]+) us count ([\d.]+) us' % NAME, text)
    assert m, text
    return int(m.group(1)), int(m.group(2)), float(m.group(3)) / 1e3, float(m.group(4)) / 1e3, float(m.group(5)) / 1e3


def host_path(store, pairs, max_dist):
    """The tables of the pairs the way a caller formed them before: both endpoints' rows of node_distances, a 2-D histogram per pair.  -> tables, seconds"""
    side = max_dist + 2
    t0 = time.perf_counter()
    rows = store.node_distances(0, np.concatenate([pairs.min(1), pairs.max(1)]), max_dist=max_dist).astype(np.int64)
    rows = np.where(rows <= max_dist, rows, max_dist + 1)
    n = len(pairs)
    out = np.stack([np.bincount(rows[k] * side + rows[n + k], minlength=side * side).reshape(side, side) for k in range(n)]).astype(np.int32)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host_pairs', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    import bench
    lib = _lib.lib()
    box = bench.box_calibration(lib, _lib, argparse.Namespace(rows=0))       # (rows = 0: the copy only)
    copy_gbps = float(box['hbm_copy']['GBps'])
    cfg = synth.CONFIGS['arxiv']
    d = synth.node_dataset(cfg['n'], cfg['m'], 4, cfg['classes'])
    N, src, dst = d['graphs'][0]
    NW = (N + 63) // 64
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    deg = store.neighbour_degrees(0).astype(np.int64)
    lines = ['arxiv (m = %d): %d nodes (%d node-words), %d directed edges, %d index entries (mean distinct degree %.2f, longest row %d); %s'
             % (cfg['m'], N, NW, len(src), int(deg.sum()), deg.mean(), deg.max(), torch.cuda.get_device_name(0)),
             'box: HBM copy rate %.0f GB/s (1 GiB device copy, bytes read + written per second); end to end: HIP events around the C call, median (min - max) of %d after %d warm-up(s);'
             % (copy_gbps, a.reps, a.warmup),
             'phases: one call under GM_TIMING, the stream synchronised behind every phase of every group (host clock)']
    versus = ['comparison: node_distances of both endpoints + a numpy 2-D histogram per pair on the host (what a caller did before; unmasked only), %d pairs timed, scaled to the list'
              % a.host_pairs]
    rng = np.random.default_rng(5)
    half = len(src) // 2
    for n in SIZES:
        pos = np.stack([src[:half], dst[:half]], 1)[rng.choice(half, n // 2, replace=False)]
        pairs = np.concatenate([pos, store.negative_pairs(0, n - n // 2, seed=222)]).astype(np.int64)
        d_p = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).cuda()
        adjacent = store.has_edges(0, pairs)
        for flags in (0, 1):
            cut = adjacent & bool(flags)
            lo, hi = pairs.min(1), pairs.max(1)
            keys = np.concatenate([np.stack([lo, np.where(cut, hi, -1)], 1), np.stack([hi, np.where(cut, lo, -1)], 1)])
            ncols = len(np.unique(keys, axis=0))
            for D in DISTS:
                out = torch.empty((n, D + 2, D + 2), dtype=torch.int32, device='cuda')
                dist = torch.empty(n, dtype=torch.uint8, device='cuda')
                call = lambda: _lib.check(lib.gm_store_pair_distance_profile(store.handle, 0, _lib.ptr(d_p), n, flags, D, _lib.ptr(out), _lib.stream_ptr()), NAME)      # noqa: E731
                med, tlo, thi = timed(call, a.reps, a.warmup)
                got = out.cpu().numpy()
                assert (got.sum((1, 2)) == N).all()
                groups, cols_run, t_search, t_trans, t_count = phases(call)
                plain = timed(lambda: _lib.check(lib.gm_store_pair_distance(store.handle, 0, _lib.ptr(d_p), n, flags, D, _lib.ptr(dist), _lib.stream_ptr()), 'pair_distance'),
                              a.reps, a.warmup)[0]
                # plane bytes: every level of every group is read once as [N, W] words and written once as [64 W, NW] words (an upper bound: a workgroup without a
                # bit writes nothing); the count reads the D + 1 plane words of both columns of every pair
                trans_bytes = 2.0 * (D + 1) * cols_run * NW * 8
                count_bytes = 2.0 * (D + 1) * NW * 8 * n
                rec = {'what': '%d pairs' % n, 'mask_target': flags, 'max_dist': D, 'columns': ncols, 'groups': groups, 'columns_searched': cols_run, 'ms': round(med, 3), 'min_ms': round(tlo, 3),
                       'max_ms': round(thi, 3), 'search_ms': round(t_search, 3), 'transpose_ms': round(t_trans, 3), 'count_ms': round(t_count, 3),
                       'pair_distance_ms': round(plain, 3), 'transpose_GBps': round(trans_bytes / (t_trans * 1e-3) / 1e9, 1),
                       'count_GBps': round(count_bytes / (t_count * 1e-3) / 1e9, 1), 'hbm_copy_GBps': round(copy_gbps, 1)}
                print(json.dumps(rec), flush=True)
                lines.append('  %6d pairs mask %d max_dist %d  %6d columns (%6d searched in %2d group(s)) %9.3f ms (%.3f - %.3f)   search %8.3f  transpose %8.3f  count %8.3f ms   pair_distance alone %8.3f ms   '
                             'planes: transposed <= %6.1f GB/s = %.3f, counted %6.1f GB/s = %.3f of the copy rate'
                             % (n, flags, D, ncols, cols_run, groups, med, tlo, thi, t_search, t_trans, t_count, plain, rec['transpose_GBps'], rec['transpose_GBps'] / copy_gbps,
                                rec['count_GBps'], rec['count_GBps'] / copy_gbps))
                if not flags:
                    m = min(a.host_pairs, n)
                    want, s = host_path(store, pairs[:m], D)
                    assert np.array_equal(got[:m], want), 'the device tables differ from the histograms of node_distances'
                    scaled = s / m * n
                    print(json.dumps({'what': '%d pairs' % n, 'max_dist': D, 'versus': 'node_distances + numpy', 'pairs_timed': m, 's': round(s, 4), 's_scaled': round(scaled, 3),
                                      'ratio': round(scaled * 1e3 / med, 1)}), flush=True)
                    versus.append('  %6d pairs max_dist %d  device %9.3f ms   host path %.4f s for %d pairs = %.3f s scaled (%.1f MB over PCIe per %d pairs)   %8.1f x   equal tables'
                                  % (n, D, med, s, m, scaled, 2.0 * N * n / 1e6, n, scaled * 1e3 / med))
    lines += versus
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
