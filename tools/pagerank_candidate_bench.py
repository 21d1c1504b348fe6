"""Time of the global candidate generator on the device (GraphStore.pagerank_candidates -> gm_store_pagerank_candidates), reported with no target, against what
a user did before it existed: GraphStore.rooted_pagerank (the walk on the device and the copy of the dense fp32 [m, N] result to the host) followed by a numpy
partial sort per row under the same rule, timed in the same process.  Case: the arxiv-shaped synthetic graph of tools/candidate_bench.py
(synth.CONFIGS['arxiv']: 169,343 nodes, stored in both directions); sources: 64 / 256 / 1,024 random nodes and the 100 highest-degree nodes; k = 50.

    python tools/pagerank_candidate_bench.py [--config arxiv] [--reps 10] [--warmup 2] [--base_reps 3] [--sources 64,256,1024] [--hubs 100] [--k 50] [--out profiles/pagerank_candidates.txt]

Per source set, medians (min - max) of --reps after --warmup: the end-to-end wall time of the call (perf_counter around the C call and a device synchronise),
and the time per phase from the library's own phase timer (GM_TIMING switched on through gm_set_tuning for separate calls: the library then synchronises the
stream behind every phase, so the phases add up to a little more than the untimed call).  `plan` is the read-back of the sources and the host's column
plan, `walk` the iterations, `exclusion` the zeroing of the source's and its neighbours' entries, `select` the radix passes, the tie pass, the collection and
the sort.  The select's sweeps read the round's state P[N, B] at most six times (four histogram passes, the tie pass, the collection; a slab whose columns are
closed leaves a pass early): those bytes are held against the device-to-device copy rate measured in the same process.  The baseline is timed in two parts
(the call that ends with the [m, N] matrix on the host; the numpy selection) and its result must equal the device's: nodes, score bits, totals.
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

PHASES = ('plan', 'walk', 'exclusion', 'select')
ALPHA, ITERS = 0.15, 20
SWEEPS = 6                               # reads of a round's state by the select at most


class Call:
    def __init__(self, store, nodes, k):
        self.store, self.m, self.k = store, len(nodes), k
        self.d_a = torch.from_numpy(np.ascontiguousarray(nodes, np.int32)).cuda()
        self.part = torch.empty((self.m, k), dtype=torch.int32, device='cuda')
        self.sc = torch.empty((self.m, k), dtype=torch.float32, device='cuda')
        self.tot = torch.empty(self.m, dtype=torch.int32, device='cuda')

    def __call__(self):
        _lib.check(_lib.lib().gm_store_pagerank_candidates(self.store.handle, 0, _lib.ptr(self.d_a), self.m, self.k, ALPHA, ITERS, _lib.ptr(self.part), _lib.ptr(self.sc),
                                                           _lib.ptr(self.tot), _lib.stream_ptr()), 'gm_store_pagerank_candidates')
        torch.cuda.synchronize()

    def result(self):
        return self.part.cpu().numpy().astype(np.int64), self.sc.cpu().numpy(), self.tot.cpu().numpy().astype(np.int64)


def wall_ms(fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def phase_ms(call, reps):
    """Per call, the library's phase laps ([gm timing] pagerank candidates/<phase> <us> us on stderr) summed by phase; the number of rounds."""
    lib = _lib.lib()
    out = {p: [] for p in PHASES}
    rounds = 0
    for _ in range(reps):
        torch.cuda.synchronize()
        sys.stderr.flush()
        with tempfile.TemporaryFile(mode='w+') as tmp:
            keep = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                assert lib.gm_set_tuning(b'GM_TIMING', 1) == 0
                call()
            finally:
                lib.gm_set_tuning(b'GM_TIMING', 0)
                os.dup2(keep, 2); os.close(keep)
            tmp.seek(0)
            text = tmp.read()
        laps = re.findall(r'\[gm timing\] pagerank candidates/(\w+) ([0-9.]+) us', text)
        assert laps, text
        for p in PHASES:
            out[p].append(sum(float(us) for name, us in laps if name == p) / 1e3)
        rounds = sum(1 for name, _ in laps if name == 'select')
    return out, rounds


def med(x):
    return float(np.median(x)), float(min(x)), float(max(x))


def neighbour_rows(N, src, dst):
    """Host CSR of the distinct-neighbour graph (either direction, no self loops): what the numpy selection excludes."""
    u = np.concatenate([src, dst]).astype(np.int64); v = np.concatenate([dst, src]).astype(np.int64)
    key = np.unique(u[u != v] * N + v[u != v])
    rows, cols = key // N, key % N
    return np.searchsorted(rows, np.arange(N + 1)), cols


def host_select(rows, nodes, ptr, idx, k):
    """The numpy selection a user writes under the definition's rule: per row the positive entries that are neither the source nor its neighbours, the k
    largest keys (score bits << 32 | 0xFFFFFFFF - w) by a partial sort, then sorted."""
    m, N = rows.shape
    part = np.full((m, k), -1, np.int64); sc = np.zeros((m, k), np.float32); tot = np.zeros(m, np.int64)
    low = np.uint64(0xFFFFFFFF) - np.arange(N, dtype=np.uint64)
    for r, a in enumerate(nodes.tolist()):
        bits = rows[r].view(np.uint32).copy()
        bits[a] = 0
        bits[idx[ptr[a]:ptr[a + 1]]] = 0
        tot[r] = t = int(np.count_nonzero(bits))
        key = (bits.astype(np.uint64) << np.uint64(32)) | low
        n = min(k, t)
        if n == 0:
            continue
        top = np.argpartition(key, N - n)[N - n:]
        top = top[np.argsort(key[top])[::-1]]
        part[r, :n] = top; sc[r, :n] = rows[r][top]
    return part, sc, tot


def copy_rate():
    """Device-to-device copy rate, bytes read + written per second: the box's own HBM rate for a plain stream."""
    a = torch.empty(1 << 28, dtype=torch.float32, device='cuda'); b = torch.empty_like(a)      # 1 GiB each: beyond the Infinity Cache
    a.zero_()
    ms = wall_ms(lambda: (b.copy_(a), torch.cuda.synchronize()), 10, 3)
    return 2 * a.numel() * 4 / (np.median(ms) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='arxiv')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--base_reps', type=int, default=3)
    ap.add_argument('--sources', default='64,256,1024')
    ap.add_argument('--hubs', type=int, default=100)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = synth.CONFIGS[a.config]
    d = synth.node_dataset(cfg['n'], cfg['m'], 4, cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    deg = store.neighbour_degrees(0)                                         # builds the neighbour index
    ptr, idx = neighbour_rows(N, np.asarray(src), np.asarray(dst))
    assert np.array_equal(np.diff(ptr), deg)
    rng = np.random.default_rng(222)
    sets = {'random %d' % n: rng.integers(0, N, n) for n in (int(x) for x in a.sources.split(','))}
    sets['hubs %d' % a.hubs] = np.argsort(-deg.astype(np.int64), kind='stable')[:a.hubs]
    rate = copy_rate()
    B = _lib.lib().gm_get_tuning(b'ppr_cols') or 256
    lines = ['%s (m = %d): %d nodes, %d directed edges, mean distinct degree %.2f, longest row %d; k = %d, alpha = %g, iters = %d; %s'
             % (a.config, cfg['m'], N, len(src), deg.mean(), deg.max(), a.k, ALPHA, ITERS, torch.cuda.get_device_name(0)),
             'ms, median (min - max) of %d after %d warm-ups (baseline: %d after 1); wall = perf_counter around the call and a device synchronise; phases = the library\'s phase '
             'timer in separate calls (stream synchronised behind every phase)' % (a.reps, a.warmup, a.base_reps),
             'device-to-device copy of 1 GiB in this process: %.2f TB/s read + written' % (rate / 1e12)]
    ok = True
    for name, nodes in sets.items():
        call = Call(store, nodes, a.k)
        call()
        w = med(wall_ms(call, a.reps, a.warmup))
        ph, rounds = phase_ms(call, a.reps)
        pm = {p: med(ph[p]) for p in PHASES}
        cols = (len(np.unique(nodes)) + 63) // 64 * 64
        state = 4 * N * cols                                                 # bytes of P over all rounds
        swept = SWEEPS * state
        got = call.result()
        # the parent-side path: the [m, N] matrix to the host, then numpy
        t_mat, t_sel, base = [], [], None
        for r in range(1 + a.base_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = store.rooted_pagerank(0, nodes, ALPHA, ITERS)
            t1 = time.perf_counter()
            base = host_select(rows, nodes, ptr, idx, a.k)
            t2 = time.perf_counter()
            if r:
                t_mat.append((t1 - t0) * 1e3); t_sel.append((t2 - t1) * 1e3)
        same = bool(np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32)) and np.array_equal(got[2], base[2]))
        ok = ok and same
        bm, bs = med(t_mat), med(t_sel)
        ratio = (bm[0] + bs[0]) / w[0]
        r = {'what': name, 'sources': len(nodes), 'rounds': rounds, 'columns': cols, 'wall_ms': round(w[0], 3), 'wall_min_ms': round(w[1], 3), 'wall_max_ms': round(w[2], 3),
             'state_mb': round(state / 1e6, 1), 'select_sweep_mb_at_most': round(swept / 1e6, 1), 'select_sweeps_at_copy_rate_ms': round(swept / rate * 1e3, 3),
             'baseline_matrix_ms': round(bm[0], 3), 'baseline_numpy_ms': round(bs[0], 3), 'baseline_over_call': round(ratio, 2), 'matrix_mb': round(4e-6 * len(nodes) * N, 1),
             'mean_total': round(float(got[2].mean()), 1), 'equal_to_baseline': same}
        r.update({p + '_ms': round(pm[p][0], 3) for p in PHASES})
        print(json.dumps(r), flush=True)
        lines.append('%s: %d sources (mean distinct degree %.1f), %d columns in %d round(s) of at most %d, mean |R| %.0f' % (name, len(nodes), deg[nodes].mean(), cols, rounds, B, got[2].mean()))
        lines.append('  call      wall %9.3f (%.3f - %.3f)   plan %7.3f (%.3f - %.3f)   walk %8.3f (%.3f - %.3f)   exclusion %6.3f (%.3f - %.3f)   select %7.3f (%.3f - %.3f)'
                     % (w + pm['plan'] + pm['walk'] + pm['exclusion'] + pm['select']))
        lines.append('            select / walk %.3f; state %.1f MB, at most %d sweeps = %.1f MB: %.3f ms at the copy rate' % (pm['select'][0] / pm['walk'][0], state / 1e6, SWEEPS, swept / 1e6, swept / rate * 1e3))
        lines.append('  baseline  rooted_pagerank to the host (%.1f MB) %9.3f (%.3f - %.3f)   numpy selection %9.3f (%.3f - %.3f)   together %.3f = %.2f x the call; equal result: %s'
                     % ((4e-6 * len(nodes) * N,) + bm + bs + (bm[0] + bs[0], ratio, same)))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    assert ok, 'the device result differs from the numpy selection on the device\'s own rows'


if __name__ == '__main__':
    main()
