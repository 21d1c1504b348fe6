"""Time of holding edges out of a resident store (GraphStore.split_edges -> gm_store_split_edges, GraphStore.without_edges -> gm_store_without_edges) against the
host route it replaces (numpy filter of host_csr + the GraphStore constructor), reported with no target: integer streaming work held against the box's own
copy rate.  Case: the arxiv-shaped synthetic graph (synth.CONFIGS['arxiv']: 169,343 nodes, stored in both directions, F0 = 128) at held-out shares of 1 %,
15 % and 50 % of its links.

    python tools/holdout_bench.py [--config arxiv] [--reps 10] [--warmup 2] [--out profiles/holdout.txt]

End to end: a host clock around the Python call (both calls return after the device has finished), median of --reps after --warmup.  Phases: the library's own
laps under gm_set_tuning('GM_TIMING', 1), which drains the stream behind every phase (so their sum exceeds the end-to-end time of the untimed call), median of
--reps.  Copy rate: a device-to-device torch copy of 1 GiB, read + written bytes over the event time.  Every route's arrays are compared in both orientations."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gmeta_amd                         # noqa: E402
from gmeta_amd import _lib, synth        # noqa: E402

SHARES = (0.01, 0.15, 0.50)


def timed(fn, reps, warmup):
    ms, out = [], None
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
        if k + 1 < warmup + reps and hasattr(out, 'close'):
            out.close()
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out


def phases(fn, reps):
    """the library's laps of `reps` calls: {'<call>/<phase>': median us, summed over the laps of one name inside a call}"""
    lib = _lib.lib()
    runs = []
    fd = os.dup(2)
    try:
        for _ in range(reps):
            with tempfile.TemporaryFile(mode='w+') as tmp:
                sys.stderr.flush()
                os.dup2(tmp.fileno(), 2)
                assert lib.gm_set_tuning(b'GM_TIMING', 1) == 0
                try:
                    out = fn()
                    torch.cuda.synchronize()
                finally:
                    lib.gm_set_tuning(b'GM_TIMING', 0)
                    os.dup2(fd, 2)
                if hasattr(out, 'close'):
                    out.close()
                tmp.seek(0)
                one = {}
                for call, phase, us in re.findall(r'\[gm timing\] (\w+)/(.+?) ([0-9.]+) us', tmp.read()):
                    if call in ('without_edges', 'split_edges'):
                        one[call + '/' + phase] = one.get(call + '/' + phase, 0.0) + float(us)
                runs.append(one)
    finally:
        os.close(fd)
    return {k: float(np.median([r[k] for r in runs if k in r])) for k in runs[0]}


def copy_rate():
    a = torch.empty(1 << 28, dtype=torch.float32, device='cuda'); b = torch.empty_like(a)
    best = 0.0
    for k in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        if k:
            best = max(best, 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3))
    return best


def host_route(store, feats, removed):
    ptr, idx = store.host_csr[0]
    N = len(ptr) - 1
    keys = store.pair_keys(0, removed)
    t0 = time.perf_counter()
    dst = np.repeat(np.arange(N, dtype=np.int64), np.diff(ptr))
    src = idx.astype(np.int64)
    keep = ~np.isin(np.minimum(src, dst) * N + np.maximum(src, dst), keys)
    nptr = np.zeros(N + 1, np.int64)
    nptr[1:] = np.cumsum(np.bincount(dst[keep], minlength=N))
    nidx = np.ascontiguousarray(idx[keep])
    t1 = time.perf_counter()
    out = gmeta_amd.GraphStore([(nptr, nidx)], feats)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), out


def moved_bytes(T, E, E2, K, feat_bytes):
    """what the device route has to read and write, from the shapes: per orientation the flag pass reads the entries and the row pointers, the compaction reads
    the entries and writes the kept ones, the pointer pass reads and writes T + 1 offsets; the symmetric check reads both new CSRs; the features are read and
    written once; the keep bits and block counts are noise beside these.  (The binary searches re-read the key list: L2 traffic, not counted.)"""
    per = (4 * E + 8 * T) + (4 * E + 4 * E2) + 16 * T
    return 2 * per + 2 * (4 * E2 + 8 * T) + 8 * K + 2 * feat_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='arxiv')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = synth.CONFIGS[a.config]
    d = synth.node_dataset(cfg['n'], cfg['m'], cfg['F0'], cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    E = store.n_edges[0]
    feat_bytes = N * int(d['feats'][0].shape[1]) * 4
    rate = copy_rate()
    store.neighbour_degrees(0)      # the neighbour index is built once per store, at first use: outside the split's time
    lines = ['%s: %d nodes, %d stored edges (undirected graph stored in both directions), feature table %.1f MB; %s'
             % (a.config, N, E, feat_bytes / 1e6, torch.cuda.get_device_name(0)),
             'end to end: host clock around the call, median (min - max) of %d after %d warm-ups; phases: the library\'s laps under GM_TIMING (stream drained behind each), median of %d'
             % (a.reps, a.warmup, a.reps),
             'device-to-device copy rate of this box (1 GiB torch copy, read + written bytes): %.0f GB/s' % (rate / 1e9)]
    print(json.dumps({'what': 'copy rate', 'GB_per_s': round(rate / 1e9, 1)}), flush=True)
    ok = True
    for share in SHARES:
        split = lambda: store.split_edges(0, val=0.0, test=share, seed=222)      # noqa: E731
        med, lo, hi, (_, test) = timed(split, a.reps, a.warmup)
        ph = phases(split, a.reps)
        r = {'what': 'split_edges', 'share': share, 'held_out': len(test), 'ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'phases_us': {k: round(v, 1) for k, v in ph.items()}}
        print(json.dumps(r), flush=True)
        lines.append('share %4.0f %%: %d of %d links held out' % (100 * share, len(test), E // 2))
        lines.append('  split_edges    %9.3f ms  (%.3f - %.3f)   count + fill, pairs copied back;  laps (us, both calls): %s' % (med, lo, hi, '  '.join('%s %.0f' % (k.split('/')[1], v) for k, v in ph.items())))
        cut = lambda: store.without_edges([test])      # noqa: E731
        med, lo, hi, held = timed(cut, a.reps, a.warmup)
        ph = phases(cut, a.reps)
        E2 = held.n_edges[0]
        moved = moved_bytes(N, E, E2, len(test), feat_bytes)
        kern_us = sum(v for k, v in ph.items() if k.split('/')[1] in ('flag', 'scan', 'compact', 'symmetric check', 'feature copy'))
        r = {'what': 'without_edges', 'share': share, 'edges_left': E2, 'ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'phases_us': {k: round(v, 1) for k, v in ph.items()},
             'moved_MB': round(moved / 1e6, 1), 'device_phases_GB_per_s': round(moved / kern_us / 1e3, 1)}
        print(json.dumps(r), flush=True)
        lines.append('  without_edges  %9.3f ms  (%.3f - %.3f)   %d edges left;  laps (us): %s' % (med, lo, hi, E2, '  '.join('%s %.0f' % (k.split('/')[1], v) for k, v in ph.items())))
        lines.append('                 moves %.1f MB (entries, offsets, features; from the shapes): %.0f GB/s over the device laps (%.0f us), %.0f %% of the copy rate'
                     % (moved / 1e6, moved / kern_us / 1e3, kern_us, 100 * moved / kern_us / 1e3 / (rate / 1e9)))
        f_ms, c_ms, host = host_route(store, d['feats'], test)
        same = host.n_edges == held.n_edges and host.dims(0) == held.dims(0)
        for o in (0, 1):
            same = same and all(np.array_equal(x, y) for x, y in zip(host.read_csr(0, o)[:2], held.read_csr(0, o)[:2]))
        ok = ok and same
        print(json.dumps({'what': 'host route', 'share': share, 'numpy_filter_ms': round(f_ms, 1), 'constructor_ms': round(c_ms, 1), 'equals_device': bool(same)}), flush=True)
        lines.append('  host route     %9.1f ms  = numpy filter of host_csr %.1f ms + GraphStore(...) %.1f ms, once;  %.0f x the device call;  equal arrays in both orientations: %s'
                     % (f_ms + c_ms, f_ms, c_ms, (f_ms + c_ms) / med, same))
        host.close(); held.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    assert ok, 'the device result differs from the host route'


if __name__ == '__main__':
    main()
