"""Time of the shortest-path distances on the device (gm_store_node_distances, gm_store_pair_distance), reported with no target: a bit-parallel multi-source
breadth-first search whose inner step is one gathered row read of the frontier's bit matrix per neighbour -- dist_cols / 8 bytes.  Case: the arxiv-shaped
synthetic graph of the other pair benchmarks (synth.CONFIGS['arxiv']), max_dist 8.

    python tools/pair_distance_bench.py [--reps 5] [--warmup 3] [--out profiles/pair_distance.txt]

The vector call for 64, 256, 1,024 and 4,096 random sources and for the 100 highest-degree sources, the pair call for 10,000 pairs (edges + as many negatives),
masked and unmasked, each per dist_cols and dist_chunk (2^30: no row is cut).  HIP events around the C call, median (min - max) of --reps after --warmup.
Reported per configuration: the time of the call, the levels that ran (the largest finite distance of the result + 1, at most max_dist: the level behind the last
one that found a node still gathers), and the gathered bytes per second -- nnz x 8 bytes per word of 64 columns and level, over the words the rounds hold -- against
the box's HBM copy rate (bench.py's box_calibration, measured in this process).  Results are compared byte for byte across all knob values.
The comparison: gm_store_rooted_pagerank / gm_store_pair_pagerank with iters = 8 over the same sources and pairs in the same process -- what reachability cost
before this call existed -- and the ratio per row.  scipy.sparse.csgraph's unweighted search of a sample of the sources is timed alongside and must give
the device rows.  One JSON line per measurement; --out appends a plain-text table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gmeta_amd                         # noqa: E402
from gmeta_amd import _lib, synth        # noqa: E402

MAX_DIST = 8
COLS = (64, 256, 1024, 4096)
CHUNKS = (64, 128, 256, 1024, 2 ** 30)
LIB_COLS = 4096                          # the library's dist_cols (pair_distance.hip: dist_cols_for), for the round count of the rows that leave the choice to it


def fmt(x):
    return '2^30' if x == 2 ** 30 else '0 (library)' if x == 0 else '%d' % x


def timed(call, reps, warmup):
    ms = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def run(store, kind, d_in, flags, cols, chunk, reps, warmup, out):
    lib = _lib.lib()
    assert lib.gm_set_tuning(b'dist_cols', cols) == 0 and lib.gm_set_tuning(b'dist_chunk', chunk) == 0
    n = d_in.shape[0]
    if kind == 'vector':
        call = lambda: _lib.check(lib.gm_store_node_distances(store.handle, 0, _lib.ptr(d_in), n, MAX_DIST, _lib.ptr(out), _lib.stream_ptr()), 'node_distances')      # noqa: E731
    else:
        call = lambda: _lib.check(lib.gm_store_pair_distance(store.handle, 0, _lib.ptr(d_in), n, flags, MAX_DIST, _lib.ptr(out), _lib.stream_ptr()), 'pair_distance')      # noqa: E731
    res = timed(call, reps, warmup)
    lib.gm_set_tuning(b'dist_cols', 0); lib.gm_set_tuning(b'dist_chunk', 0)
    return res


def run_pagerank(store, kind, d_in, flags, reps, warmup, out):
    lib = _lib.lib()
    n = d_in.shape[0]
    if kind == 'vector':
        call = lambda: _lib.check(lib.gm_store_rooted_pagerank(store.handle, 0, _lib.ptr(d_in), n, 0.15, MAX_DIST, _lib.ptr(out), _lib.stream_ptr()), 'rooted_pagerank')      # noqa: E731
    else:
        call = lambda: _lib.check(lib.gm_store_pair_pagerank(store.handle, 0, _lib.ptr(d_in), n, flags, 0.15, MAX_DIST, _lib.ptr(out), _lib.stream_ptr()), 'pair_pagerank')      # noqa: E731
    return timed(call, reps, warmup)


def report(lines, label, cols, chunk, flags, n, ncols, levels, nnz, res, copy_gbps):
    med, lo, hi = res
    padded = (ncols + 63) // 64 * 64
    B = min(cols if cols else LIB_COLS, padded)
    rounds = max(1, (padded + B - 1) // B)
    gbps = nnz * 8.0 * (padded // 64) * levels / (med * 1e-3) / 1e9
    print(json.dumps({'what': label, 'dist_cols': cols, 'dist_chunk': chunk, 'mask_target': flags, 'n': n, 'columns': ncols, 'rounds': rounds, 'levels': levels, 'ms': round(med, 3),
                      'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'gathered_GBps': round(gbps, 1), 'share_of_hbm_copy': round(gbps / copy_gbps, 3)}), flush=True)
    lines.append('  %-13s dist_cols %-12s dist_chunk %-12s mask %d  %5d columns %3d rounds %d levels %9.3f ms  (%.3f - %.3f)  %7.1f GB/s gathered = %.3f of the copy rate'
                 % (label, fmt(cols), fmt(chunk), flags, ncols, rounds, levels, med, lo, hi, gbps, gbps / copy_gbps))


def levels_of(d):
    """The levels that gather: the largest finite distance + 1 (the level that finds nothing still runs), at most max_dist.  d: a uint8 tensor."""
    d = d[d != gmeta_amd.DIST_UNREACHED]
    return min(MAX_DIST, int(d.max()) + 1) if d.numel() else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no_host', action='store_true')
    ap.add_argument('--no_sweep', action='store_true', help="the library's choice and the comparison only")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    import bench
    box = bench.box_calibration(_lib.lib(), _lib, argparse.Namespace(rows=0))       # (rows = 0: the copy only)
    copy_gbps = float(box['hbm_copy']['GBps'])
    cfg = synth.CONFIGS['arxiv']
    d = synth.node_dataset(cfg['n'], cfg['m'], 4, cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    deg = store.neighbour_degrees(0).astype(np.int64)
    nnz = int(deg.sum())
    lines = ['arxiv (m = %d): %d nodes, %d directed edges, %d index entries (mean distinct degree %.2f, longest row %d); max_dist %d; %s'
             % (cfg['m'], N, len(src), nnz, deg.mean(), deg.max(), MAX_DIST, torch.cuda.get_device_name(0)),
             'box: HBM copy rate %.0f GB/s (1 GiB device copy, bytes read + written per second); HIP events around the C call, median (min - max) of %d after %d warm-up(s)'
             % (copy_gbps, a.reps, a.warmup)]
    versus = ['comparison: the PageRank calls with iters = %d over the same sources and pairs (what reachability within %d hops cost before), same process' % (MAX_DIST, MAX_DIST)]
    rng = np.random.default_rng(5)
    lists = [('%d sources' % m, rng.choice(N, m, replace=False)) for m in (64, 256, 1024, 4096)] + [('100 hubs', np.argsort(-deg, kind='stable')[:100])]
    out = torch.empty((4096, N), dtype=torch.uint8, device='cuda')
    fout = torch.empty((4096, N), dtype=torch.float32, device='cuda')
    for label, sources in lists:
        d_s = torch.from_numpy(np.ascontiguousarray(sources, np.int32)).cuda()
        m = len(sources)
        mine = run(store, 'vector', d_s, 0, 0, 0, a.reps, a.warmup, out)
        base = out[:m].clone()
        levels = levels_of(base)
        report(lines, label, 0, 0, 0, m, m, levels, nnz, mine, copy_gbps)
        theirs = run_pagerank(store, 'vector', d_s, 0, a.reps, a.warmup, fout)
        agree = float(((base != gmeta_amd.DIST_UNREACHED) == (fout[:m] > 0)).float().mean())
        print(json.dumps({'what': label, 'versus': 'rooted_pagerank', 'ms': round(theirs[0], 3), 'min_ms': round(theirs[1], 3), 'max_ms': round(theirs[2], 3), 'ratio': round(theirs[0] / mine[0], 2)}), flush=True)
        versus.append('  %-13s node_distances %9.3f ms (%.3f - %.3f)   rooted_pagerank %9.3f ms (%.3f - %.3f)   %6.2f x   (pi > 0 agrees with reached on %.6f of the entries)'
                      % (label, *mine, *theirs, theirs[0] / mine[0], agree))
        for chunk in CHUNKS if not a.no_sweep else ():
            for cols in COLS:
                report(lines, label, cols, chunk, 0, m, m, levels, nnz, run(store, 'vector', d_s, 0, cols, chunk, a.reps, a.warmup, out), copy_gbps)
                assert torch.equal(out[:m], base), 'dist_chunk %d, dist_cols %d change the result' % (chunk, cols)
    # the pair call: 10,000 pairs, half edges, half negatives
    half = len(src) // 2
    pos = np.stack([src[:half], dst[:half]], 1)[rng.choice(half, 5000, replace=False)]
    pairs = np.concatenate([pos, store.negative_pairs(0, 5000, seed=222)]).astype(np.int64)
    d_p = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).cuda()
    pout = torch.empty(len(pairs), dtype=torch.uint8, device='cuda')
    fpout = torch.empty((len(pairs), 2), dtype=torch.float32, device='cuda')
    adjacent = store.has_edges(0, pairs)
    y = np.concatenate([np.ones(5000), np.zeros(5000)])
    for flags in (0, 1):
        cut = adjacent & bool(flags)                                          # the columns of the call: (smaller endpoint, excluded node or -1), distinct
        ncols = len(np.unique(np.stack([pairs.min(1), np.where(cut, pairs.max(1), -1)], 1), axis=0))
        label = '10,000 pairs'
        mine = run(store, 'pair', d_p, flags, 0, 0, a.reps, a.warmup, pout)
        base = pout.cpu().numpy()
        levels = levels_of(pout)                                              # (the targets' distances bound the levels from below)
        report(lines, label, 0, 0, flags, len(pairs), ncols, levels, nnz, mine, copy_gbps)
        theirs = run_pagerank(store, 'pair', d_p, flags, max(1, a.reps // 2), 1, fpout)
        versus.append('  %-13s mask %d  pair_distance %9.3f ms (%.3f - %.3f)   pair_pagerank  %9.3f ms (%.3f - %.3f)   %6.2f x   distances %s; ROC AUC graph_distance %.4f'
                      % (label, flags, *mine, *theirs, theirs[0] / mine[0], np.bincount(base, minlength=256)[[0, 1, 2, 3, 4, 5, 6, 7, 8, 255]].tolist(),
                         gmeta_amd.link_auc(gmeta_amd.graph_distance_index(base, MAX_DIST), y)))
        print(json.dumps({'what': label, 'mask_target': flags, 'versus': 'pair_pagerank', 'ms': round(theirs[0], 3), 'ratio': round(theirs[0] / mine[0], 2)}), flush=True)
        for cols, chunk in (() if a.no_sweep else tuple((c, 0) for c in COLS) + tuple((0, c) for c in CHUNKS)):
            report(lines, label, cols, chunk, flags, len(pairs), ncols, levels, nnz, run(store, 'pair', d_p, flags, cols, chunk, a.reps, a.warmup, pout), copy_gbps)
            assert np.array_equal(pout.cpu().numpy(), base), 'dist_chunk %d, dist_cols %d change the result' % (chunk, cols)
    lines += versus
    if not a.no_host:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
        S = csr_matrix((np.ones(len(src), np.int32), (src, dst)), shape=(N, N))
        sample = lists[2][1][:16]
        t0 = time.perf_counter()
        want = dijkstra(S, directed=False, indices=sample, unweighted=True, limit=MAX_DIST)
        s = time.perf_counter() - t0
        want = np.where(np.isfinite(want), want, gmeta_amd.DIST_UNREACHED).astype(np.uint8)
        got = store.node_distances(0, sample, max_dist=MAX_DIST)
        assert np.array_equal(got, want), 'the device rows differ from scipy.sparse.csgraph'
        print(json.dumps({'what': 'scipy', 'sources': len(sample), 's': round(s, 4), 's_per_source': round(s / len(sample), 5)}), flush=True)
        lines.append('  host     scipy.sparse.csgraph.dijkstra (unweighted, undirected, limit %d; the matrix given) of %d sources %.4f s: %.2f ms per source, %.2f s scaled to 4,096; '
                     'equal to the device rows' % (MAX_DIST, len(sample), s, s / len(sample) * 1e3, s / len(sample) * 4096))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
