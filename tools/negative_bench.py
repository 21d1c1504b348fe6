"""Time of drawing negative pairs on the device (GraphStore.negative_pairs -> gm_store_negative_pairs), reported with no target: integer and latency work,
two binary searches per candidate, no roofline to hold it against.  Case: the arxiv-shaped synthetic graph (synth.CONFIGS['arxiv']: 169,343 nodes, stored in
both directions) and a draw of as many negatives as the graph has edges, in both modes.

    python tools/negative_bench.py [--config arxiv] [--reps 10] [--warmup 2] [--out profiles/negative_pairs.txt] [--no_host]

Device time: HIP events around the C call (which reads one counter per round, so the events bracket the whole call), median of --reps after --warmup.
Host time, once each: the numpy restatement of the definition (tests/negative_ref.py) for the same draw, and the host loop of synth.link_dataset on the same
graph (3 |E| candidates through Python sets, as many negatives as undirected edges).  One JSON line per measurement; --out appends a plain-text table."""
import argparse
import ctypes as C
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


def device_ms(store, n, mode, reps, warmup):
    lib = _lib.lib()
    out = torch.empty((n, 2), dtype=torch.int32, device='cuda')
    found = C.c_int64(0)
    ms = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.gm_store_negative_pairs(store.handle, 0, n, 222, _lib.NEG_MODES[mode], None, 0, _lib.ptr(out), C.byref(found), _lib.stream_ptr()), 'negative_pairs')
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out.cpu().numpy()[:found.value]


def link_dataset_host_loop(n_nodes, e, seed=222):
    """The negative-drawing lines of synth.link_dataset, on the undirected edge list e [E, 2]: seconds, pairs kept."""
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    have = set(map(tuple, e.tolist()))
    neg = rng.integers(0, n_nodes, size=(3 * len(e), 2))
    neg = neg[neg[:, 0] != neg[:, 1]]
    keep, seen = [], set()
    for a, b in neg.tolist():
        if (a, b) in have or (b, a) in have or (a, b) in seen or (b, a) in seen:
            continue
        seen.add((a, b)); keep.append((a, b))
        if len(keep) == len(e):
            break
    return time.perf_counter() - t0, len(keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='arxiv')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no_host', action='store_true', help='skip the two host timings (minutes of pure Python at the arxiv size)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = synth.CONFIGS[a.config]
    d = synth.node_dataset(cfg['n'], cfg['m'], 4, cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    n = len(src)
    lines = ['%s: %d nodes, %d directed edges (undirected graph stored in both directions); n = %d negatives per draw; %s'
             % (a.config, N, n, n, torch.cuda.get_device_name(0)),
             'device: HIP events around gm_store_negative_pairs, median (min - max) of %d after %d warm-ups' % (a.reps, a.warmup)]
    pairs = {}
    for mode in ('uniform', 'two_hop'):
        med, lo, hi, pairs[mode] = device_ms(store, n, mode, a.reps, a.warmup)
        r = {'what': 'device', 'mode': mode, 'n': n, 'ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'found': len(pairs[mode]), 'pairs_per_us': round(len(pairs[mode]) / med / 1e3, 2)}
        print(json.dumps(r), flush=True)
        lines.append('  device   %-8s %10.3f ms  (%.3f - %.3f)   %d pairs found, %.1f pairs / us' % (mode, med, lo, hi, len(pairs[mode]), len(pairs[mode]) / med / 1e3))
    agree = True
    if not a.no_host:
        import negative_ref as ref
        for mode in ('uniform', 'two_hop'):
            t0 = time.perf_counter()
            want, found = ref.negative_pairs(N, src, dst, 0, n, 222, mode)
            s = time.perf_counter() - t0
            same = np.array_equal(want, pairs[mode].astype(np.int64))
            print(json.dumps({'what': 'numpy restatement', 'mode': mode, 'n': n, 's': round(s, 2), 'equals_device': bool(same)}), flush=True)
            lines.append('  host     %-8s %10.2f s   numpy restatement (tests/negative_ref.py), same draw; equals the device result: %s' % (mode, s, same))
            agree = agree and same
        e = np.stack([src[:n // 2], dst[:n // 2]], 1)                    # node_dataset lists u -> v first, then the reverses
        s, kept = link_dataset_host_loop(N, e)
        print(json.dumps({'what': 'synth.link_dataset host loop', 'n': kept, 's': round(s, 2)}), flush=True)
        lines.append('  host     %-8s %10.2f s   synth.link_dataset\'s loop on the same graph: %d negatives (one per undirected edge), 3 |E| candidates through Python sets'
                     % ('uniform', s, kept))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    assert agree, 'the device result differs from the restatement'


if __name__ == '__main__':
    main()
