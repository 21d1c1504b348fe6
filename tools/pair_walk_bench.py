"""Time of the walk counts on the device (GraphStore.pair_walks -> gm_store_pair_walks), reported with no target: integer and latency work -- per outer
entry of the shorter endpoint row one row intersection (a strided walk over the shorter row, a binary search per entry in the longer) -- whose amount per pair
spans five orders of magnitude, which is why heavy pairs are cut into work items.  Case: the arxiv-shaped synthetic graph and pair list of
tools/pair_score_bench.py (synth.CONFIGS['arxiv']; |E| / 2 edges plus as many pairs from GraphStore.negative_pairs).

    python tools/pair_walk_bench.py [--reps 10] [--warmup 2] [--out profiles/pair_walks.txt]                      # the arxiv case: the sweep, the mask, the hub pairs, the restatement
    python tools/pair_walk_bench.py --density [--pairs 100000] [--out ...]                                       # the lane widths over graphs of mean distinct degree 2 .. 554

HIP events around the C call, median (min - max) of --reps after --warmup.  The sweep covers every built lane width and a range of walk_chunk values that
ends with 2^30 (nothing is cut: one lane group per pair, however heavy).  Every configuration's result is compared with the first one for equality.  One JSON
line per measurement; --out appends a plain-text table."""
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

LANES = (32, 64)
CHUNKS = (8, 16, 32, 64, 128, 256, 1024, 2 ** 30)
# (n, m, pairs at most): the graphs of profiles/pair_scores.txt; the whole pair list where the graph is sparse, a sample where a walk count costs deg^2 / lanes per pair
DENSITY = ((169343, 1, None), (169343, 2, None), (169343, 4, None), (169343, 7, None), (169343, 16, 2000000), (169343, 40, 1000000), (20000, 75, 200000), (20000, 150, 200000),
           (20000, 300, 200000))


def device_ms(store, d_pairs, flags, reps, warmup, lanes, chunk):
    lib = _lib.lib()
    assert lib.gm_set_tuning(b'walk_lanes', lanes) == 0 and lib.gm_set_tuning(b'walk_chunk', chunk) == 0
    n = d_pairs.shape[0]
    out = torch.empty((n, 3), dtype=torch.int64, device='cuda')
    ms = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.gm_store_pair_walks(store.handle, 0, _lib.ptr(d_pairs), n, flags, _lib.ptr(out), _lib.stream_ptr()), 'pair_walks')
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    lib.gm_set_tuning(b'walk_lanes', 0); lib.gm_set_tuning(b'walk_chunk', 0)
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out.cpu().numpy()


def graph_and_pairs(n, m, classes, cap=None):
    d = synth.node_dataset(n, m, 4, classes)
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    half = len(src) // 2                                                     # node_dataset lists u -> v first, then the reverses
    pos = np.stack([src[:half], dst[:half]], 1)
    if cap is not None and 2 * half > cap:
        pos = pos[np.random.default_rng(3).choice(half, cap // 2, replace=False)]
    neg = store.negative_pairs(0, len(pos), seed=222)
    return N, src, dst, store, np.concatenate([pos, neg]).astype(np.int64), len(pos)


def fmt(x):
    return '2^30' if x == 2 ** 30 else '0 (library)' if x == 0 else '%d' % x


def sweep(store, d_pairs, a, lines, label, lanes_list, chunks, flags=0, first=None):
    for lanes in lanes_list:
        for chunk in chunks:
            med, lo, hi, got = device_ms(store, d_pairs, flags, a.reps, a.warmup, lanes, chunk)
            if first is None:
                first = got
            assert np.array_equal(got, first), 'walk_lanes %d, walk_chunk %d: the result differs' % (lanes, chunk)
            n = d_pairs.shape[0]
            print(json.dumps({'what': label, 'walk_lanes': lanes, 'walk_chunk': chunk, 'mask_target': flags, 'n': n, 'ms': round(med, 3), 'min_ms': round(lo, 3),
                              'max_ms': round(hi, 3)}), flush=True)
            lines.append('  %-10s walk_lanes %-12s walk_chunk %-12s mask_target %d %10.3f ms  (%.3f - %.3f)   %.1f pairs / us'
                         % (label, fmt(lanes), fmt(chunk), flags, med, lo, hi, n / med / 1e3))
    return first


def arxiv(a):
    cfg = synth.CONFIGS['arxiv']
    N, src, dst, store, pairs, half = graph_and_pairs(cfg['n'], cfg['m'], cfg['classes'])
    deg = store.neighbour_degrees(0)                                         # (builds the index: timed by tools/pair_score_bench.py)
    lines = ['arxiv (m = %d): %d nodes, %d directed edges, mean distinct degree %.2f, longest row %d; %d pairs = %d edges + %d negative_pairs; %s'
             % (cfg['m'], N, len(src), deg.mean(), deg.max(), len(pairs), half, len(pairs) - half, torch.cuda.get_device_name(0)),
             'device: HIP events around gm_store_pair_walks, median (min - max) of %d after %d warm-ups; every result equal to the first' % (a.reps, a.warmup)]
    d_pairs = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).cuda()
    work = np.minimum(deg[pairs[:, 0]], deg[pairs[:, 1]]).astype(np.int64)
    lines.append('  outer entries per pair (the shorter row): mean %.1f, median %d, 99th percentile %d, largest %d'
                 % (work.mean(), np.median(work), np.percentile(work, 99), work.max()))
    first = sweep(store, d_pairs, a, lines, 'all pairs', (0,), (0,))
    sweep(store, d_pairs, a, lines, 'all pairs', LANES, CHUNKS, 0, first)
    sweep(store, d_pairs, a, lines, 'all pairs', (0,), (0,), 1)
    # the imbalance case: the 1,000 pairs between the highest-degree nodes
    top = np.argsort(-deg.astype(np.int64), kind='stable')[:46]
    hub = np.array([(x, y) for i, x in enumerate(top.tolist()) for y in top[i + 1:].tolist()], np.int64)[:1000]
    d_hub = torch.from_numpy(np.ascontiguousarray(hub, np.int32)).cuda()
    lines.append('  the %d pairs between the %d highest-degree nodes (rows of %d to %d entries):' % (len(hub), len(top), deg[top].min(), deg[top].max()))
    hfirst = sweep(store, d_hub, a, lines, 'hub pairs', (0,), (0,))
    sweep(store, d_hub, a, lines, 'hub pairs', LANES, (16, 64, 256, 2 ** 30), 0, hfirst)
    if not a.no_host:
        import pair_score_ref
        import path_walk_ref
        at = np.random.default_rng(1).choice(len(pairs), 2000, replace=False)
        nb = pair_score_ref.neighbourhoods(N, src, dst)
        t0 = time.perf_counter()
        want = path_walk_ref.pair_walks(N, src, dst, pairs[at], 0, nb)
        s = time.perf_counter() - t0
        assert np.array_equal(first[at], want), 'the device result differs from the restatement'
        assert np.array_equal(hfirst[:50], path_walk_ref.pair_walks(N, src, dst, hub[:50], 0, nb))
        print(json.dumps({'what': 'restatement', 'n': 2000, 's': round(s, 3), 'scaled_s': round(s * len(pairs) / 2000, 1), 'equal': True}), flush=True)
        lines.append('  host     restatement (tests/path_walk_ref.py: Python sets, neighbourhoods given) of a 2,000-pair sample %.3f s: %.0f s scaled to all pairs; '
                     'the device rows of the sample and of 50 hub pairs EQUAL it' % (s, s * len(pairs) / 2000))
        y = np.concatenate([np.ones(half), np.zeros(len(pairs) - half)])
        masked = store.pair_walks(0, pairs, mask_target=True)
        lines.append('           ROC AUC of the masked scores, edges against negatives: local_path %.4f  katz %.4f  (cn, the same pairs: %.4f)'
                     % (gmeta_amd.link_auc(gmeta_amd.local_path_index(masked), y), gmeta_amd.link_auc(gmeta_amd.katz_index(masked), y),
                        gmeta_amd.link_auc(masked[:, 1], y)))
    return lines


def density(a):
    classes = synth.CONFIGS['arxiv']['classes']
    lines = ['lane widths and walk_chunk over preferential-attachment graphs (the graphs of profiles/pair_scores.txt); pairs = edges + as many negatives, %s; median of %d; %s'
             % ('at most %d a graph (sampled)' % a.pairs if a.pairs else 'the whole list on the sparse graphs, a sample on the dense ones', a.reps, torch.cuda.get_device_name(0))]
    for n, m, cap in DENSITY:
        N, src, dst, store, pairs, half = graph_and_pairs(n, m, classes, a.pairs if a.pairs else cap)
        deg = store.neighbour_degrees(0)
        lines.append('  n = %d, m = %d: mean distinct degree %.2f, longest row %d; %d pairs' % (N, m, deg.mean(), deg.max(), len(pairs)))
        d_pairs = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).cuda()
        first = sweep(store, d_pairs, a, lines, 'm = %d' % m, (0,), (0,))
        sweep(store, d_pairs, a, lines, 'm = %d' % m, LANES, (16, 32, 64), 0, first)
        store.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--density', action='store_true', help='the lane-width sweep over graphs of growing density instead of the arxiv case')
    ap.add_argument('--pairs', type=int, default=None, help="--density: pairs per graph at most, for every graph (default: the table's own caps) -- the short-list regime, where the tail of the heaviest pairs decides")
    ap.add_argument('--no_host', action='store_true', help='skip the restatement of the 2,000-pair sample')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = density(a) if a.density else arxiv(a)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
