"""Time of rooted PageRank on the device (gm_store_rooted_pagerank, gm_store_pair_pagerank), reported with no target: a repeated sparse-matrix-times-dense-block
product whose inner step is one gathered 256-byte row read of the state per neighbour and slab of 64 columns.  Case: the arxiv-shaped synthetic graph of the
other pair benchmarks (synth.CONFIGS['arxiv']).

    python tools/pair_pagerank_bench.py [--reps 10] [--warmup 2] [--out profiles/pair_pagerank.txt]

The vector call for 64, 256 and 1,024 random sources and for the 100 highest-degree sources, the pair call for 10,000 pairs (edges + as many negatives), masked and
unmasked, each per ppr_cols and ppr_chunk (2^30: no row is cut).  HIP events around the C call, median (min - max) of --reps after --warmup.  Reported per
configuration: the time of the call, the time per iteration and round, and the gathered bytes per second -- nnz x 4 bytes per column and iteration, over the columns
the rounds hold -- against the box's HBM copy rate (bench.py's box_calibration, measured in this process).  Results of one ppr_chunk are compared bit for bit across
ppr_cols.  A numpy float64 restatement of a sample of the sources is timed alongside and the device rows are held against it within the derived bound of
tests/pagerank_ref.py.  One JSON line per measurement; --out appends a plain-text table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gmeta_amd                         # noqa: E402
from gmeta_amd import _lib, synth        # noqa: E402

ALPHA, ITERS = 0.15, 20
COLS = (64, 128, 256)
CHUNKS = (64, 256, 1024, 4096, 2 ** 30)
LIB_COLS = 256                           # the library's ppr_cols (pair_pagerank.hip: ppr_cols_for), for the round count of the rows that leave the choice to it


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
    assert lib.gm_set_tuning(b'ppr_cols', cols) == 0 and lib.gm_set_tuning(b'ppr_chunk', chunk) == 0
    n = d_in.shape[0]
    if kind == 'vector':
        call = lambda: _lib.check(lib.gm_store_rooted_pagerank(store.handle, 0, _lib.ptr(d_in), n, ALPHA, ITERS, _lib.ptr(out), _lib.stream_ptr()), 'rooted_pagerank')      # noqa: E731
    else:
        call = lambda: _lib.check(lib.gm_store_pair_pagerank(store.handle, 0, _lib.ptr(d_in), n, flags, ALPHA, ITERS, _lib.ptr(out), _lib.stream_ptr()), 'pair_pagerank')      # noqa: E731
    res = timed(call, reps, warmup)
    lib.gm_set_tuning(b'ppr_cols', 0); lib.gm_set_tuning(b'ppr_chunk', 0)
    return res


def report(lines, label, cols, chunk, flags, n, ncols, nnz, res, copy_gbps):
    med, lo, hi = res
    B = cols if cols else LIB_COLS
    padded = (ncols + 63) // 64 * 64
    rounds = max(1, (padded + B - 1) // B)
    gbps = nnz * 4.0 * padded * ITERS / (med * 1e-3) / 1e9
    print(json.dumps({'what': label, 'ppr_cols': cols, 'ppr_chunk': chunk, 'mask_target': flags, 'n': n, 'columns': ncols, 'rounds': rounds, 'ms': round(med, 3), 'min_ms': round(lo, 3),
                      'max_ms': round(hi, 3), 'ms_per_iteration': round(med / rounds / ITERS, 4), 'gathered_GBps': round(gbps, 1), 'share_of_hbm_copy': round(gbps / copy_gbps, 3)}), flush=True)
    lines.append('  %-12s ppr_cols %-12s ppr_chunk %-12s mask %d  %5d columns %4d rounds %10.3f ms  (%.3f - %.3f)  %7.4f ms / iteration  %7.1f GB/s gathered = %.3f of the copy rate'
                 % (label, fmt(cols), fmt(chunk), flags, ncols, rounds, med, lo, hi, med / rounds / ITERS, gbps, gbps / copy_gbps))


def host_vector(N, rows, idx, deg, s):
    """pi_(s, -1) in float64 (tests/pagerank_ref.column on arrays built once)."""
    a = float(np.float32(ALPHA)); b = float(np.float32(1.0) - np.float32(ALPHA))
    p = np.zeros(N); p[s] = 1.0
    lone = deg == 0
    for _ in range(ITERS):
        q = p / np.maximum(deg, 1)
        m = np.bincount(rows, weights=q[idx], minlength=N)
        m[lone] = p[lone]
        p = b * m
        p[s] += a
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--pair_reps', type=int, default=3, help='repetitions of the pair call (thousands of columns: seconds per call)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--no_host', action='store_true')
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
    lines = ['arxiv (m = %d): %d nodes, %d directed edges, %d index entries (mean distinct degree %.2f, longest row %d); alpha %.2f, %d iterations; %s'
             % (cfg['m'], N, len(src), nnz, deg.mean(), deg.max(), ALPHA, ITERS, torch.cuda.get_device_name(0)),
             'box: HBM copy rate %.0f GB/s (1 GiB device copy, bytes read + written per second); HIP events around the C call, median (min - max) of %d after %d warm-ups'
             % (copy_gbps, a.reps, a.warmup)]
    rng = np.random.default_rng(5)
    lists = [('%d sources' % m, rng.choice(N, m, replace=False)) for m in (64, 256, 1024)] + [('100 hubs', np.argsort(-deg, kind='stable')[:100])]
    out = torch.empty((1024, N), dtype=torch.float32, device='cuda')
    for label, sources in lists:
        d_s = torch.from_numpy(np.ascontiguousarray(sources, np.int32)).cuda()
        m = len(sources)
        report(lines, label, 0, 0, 0, m, m, nnz, run(store, 'vector', d_s, 0, 0, 0, a.reps, a.warmup, out), copy_gbps)
        base = {}
        for chunk in CHUNKS:
            for cols in COLS:
                report(lines, label, cols, chunk, 0, m, m, nnz, run(store, 'vector', d_s, 0, cols, chunk, a.reps, a.warmup, out), copy_gbps)
                got = out[:m, ::97].cpu().numpy().view(np.uint32)
                assert np.array_equal(base.setdefault(chunk, got), got), 'ppr_chunk %d: ppr_cols %d changes bits' % (chunk, cols)
    # the pair call: 10,000 pairs, half edges, half negatives
    half = len(src) // 2
    pos = np.stack([src[:half], dst[:half]], 1)[rng.choice(half, 5000, replace=False)]
    pairs = np.concatenate([pos, store.negative_pairs(0, 5000, seed=222)]).astype(np.int64)
    d_p = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).cuda()
    pout = torch.empty((len(pairs), 2), dtype=torch.float32, device='cuda')
    adjacent = store.has_edges(0, pairs)
    for flags in (0, 1):
        cut = adjacent & bool(flags)                                          # the columns of the call: (source, excluded node or -1), distinct
        both = np.concatenate([pairs, pairs[:, ::-1]])
        ncols = len(np.unique(np.stack([both[:, 0], np.where(np.concatenate([cut, cut]), both[:, 1], -1)], 1), axis=0))
        for cols, chunk in ((0, 0),) + tuple((c, 0) for c in COLS) + ((0, 2 ** 30),):
            report(lines, '10,000 pairs', cols, chunk, flags, len(pairs), ncols, nnz, run(store, 'pair', d_p, flags, cols, chunk, a.pair_reps, 1, pout), copy_gbps)
    if not a.no_host:
        import pagerank_ref
        und = np.unique(np.concatenate([np.stack([src, dst], 1), np.stack([dst, src], 1)]), axis=0)
        und = und[und[:, 0] != und[:, 1]]
        rows, idx = und[:, 0], und[:, 1]
        assert np.array_equal(np.bincount(rows, minlength=N), deg)
        sample = lists[2][1][:4]
        t0 = time.perf_counter()
        want = np.stack([host_vector(N, rows, idx, deg, int(s)) for s in sample])
        s = time.perf_counter() - t0
        got = store.rooted_pagerank(0, sample).astype(np.float64)
        err = np.abs(got - want) / pagerank_ref.bound(want, ITERS, int(deg.max()))
        assert err.max() <= 1.0, 'the device rows leave the derived bound'
        print(json.dumps({'what': 'restatement', 'sources': len(sample), 's': round(s, 3), 's_per_source': round(s / len(sample), 3), 'largest_error_over_bound': float(err.max())}), flush=True)
        lines.append('  host     numpy float64 restatement (one bincount per iteration, arrays given) of %d sources %.3f s: %.3f s per source, %.0f s scaled to 1,024; the device '
                     'rows of the sample lie within %.2g of the derived bound' % (len(sample), s, s / len(sample), s / len(sample) * 1024, err.max()))
        y = np.concatenate([np.ones(5000), np.zeros(5000)])
        for mask in (False, True):
            lines.append('           ROC AUC over the 10,000 pairs, mask_target %s: rooted_pagerank %.4f' % (mask, gmeta_amd.link_auc(gmeta_amd.rooted_pagerank_index(store.pair_pagerank(0, pairs, mask_target=mask)), y)))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
