"""Time of candidate generation on the device (GraphStore.link_candidates -> gm_store_pair_candidates), reported with no target: integer and latency work --
two walks over the neighbours' neighbour rows into a bitmap, the pair-score kernel over every candidate pair, a radix select and a small sort per source --
with no roofline to hold it against.  Case: the arxiv-shaped synthetic graph of tools/pair_score_bench.py (synth.CONFIGS['arxiv']: 169,343 nodes, stored in
both directions); sources: 10,000 random nodes, and the 100 highest-degree nodes timed separately (the load-imbalance case); k = 50, every score column.

    python tools/candidate_bench.py [--config arxiv] [--reps 10] [--warmup 2] [--sources 10000] [--hubs 100] [--k 50] [--sample 200] [--out profiles/link_candidates.txt] [--no_host]

Per source set and column, medians of --reps after --warmup: the end-to-end wall time of the C call (it returns after the stream has produced the result), and
the time per phase from the library's own phase timer (GM_TIMING switched on through gm_set_tuning for separate calls: the library then synchronises the stream
behind every phase, so the phases add up to a little more than the untimed call).  `enumerate` is the count pass plus the fill passes.  The restatement
(tests/candidate_ref.py over tests/pair_score_ref.py: Python sets) runs once on a --sample of the random sources and is scaled to all of them; on that sample
the device result must equal the restatement fed with the device's own pair scores.  One JSON line per measurement; --out appends a plain-text table."""
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

PHASES = ('enumerate', 'score', 'select')


class Call:
    def __init__(self, store, nodes, k):
        self.store, self.m, self.k = store, len(nodes), k
        self.d_a = torch.from_numpy(np.ascontiguousarray(nodes, np.int32)).cuda()
        self.part = torch.empty((self.m, k), dtype=torch.int32, device='cuda')
        self.sc = torch.empty((self.m, k), dtype=torch.float32, device='cuda')
        self.tot = torch.empty(self.m, dtype=torch.int32, device='cuda')

    def __call__(self, col):
        _lib.check(_lib.lib().gm_store_pair_candidates(self.store.handle, 0, _lib.ptr(self.d_a), self.m, self.k, col, _lib.ptr(self.part), _lib.ptr(self.sc), _lib.ptr(self.tot),
                                                       _lib.stream_ptr()), 'gm_store_pair_candidates')


def wall_ms(call, col, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(col)
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def phase_ms(call, col, reps):
    """Per call, the library's phase laps ([gm timing] pair candidates/<phase> <us> us on stderr) summed by phase."""
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
                call(col)
            finally:
                lib.gm_set_tuning(b'GM_TIMING', 0)
                os.dup2(keep, 2); os.close(keep)
            tmp.seek(0)
            text = tmp.read()
        laps = re.findall(r'\[gm timing\] pair candidates/(\w+) ([0-9.]+) us', text)
        assert laps, text
        for p in PHASES:
            out[p].append(sum(float(us) for name, us in laps if name == p) / 1e3)
        rounds = sum(1 for name, _ in laps if name == 'select')
    return out, rounds


def med(x):
    return float(np.median(x)), float(min(x)), float(max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='arxiv')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sources', type=int, default=10000)
    ap.add_argument('--hubs', type=int, default=100)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--sample', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no_host', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = synth.CONFIGS[a.config]
    d = synth.node_dataset(cfg['n'], cfg['m'], 4, cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    deg = store.neighbour_degrees(0)                                         # builds the neighbour index
    rng = np.random.default_rng(222)
    sets = {'random': rng.integers(0, N, a.sources), 'hubs': np.argsort(-deg.astype(np.int64), kind='stable')[:a.hubs]}
    lines = ['%s (m = %d): %d nodes, %d directed edges, mean distinct degree %.2f, longest row %d; k = %d; %s'
             % (a.config, cfg['m'], N, len(src), deg.mean(), deg.max(), a.k, torch.cuda.get_device_name(0)),
             'ms, median (min - max) of %d after %d warm-ups; wall = perf_counter around the C call; phases = the library\'s phase timer in separate calls (stream synchronised behind every phase)'
             % (a.reps, a.warmup)]
    for name, nodes in sets.items():
        call = Call(store, nodes, a.k)
        call(2)
        pairs = int(call.tot.sum().item())
        biggest = int(call.tot.max().item())
        lines.append('%s: %d sources (mean distinct degree %.1f), %d candidate pairs scored per call (largest set %d)' % (name, len(nodes), deg[nodes].mean(), pairs, biggest))
        for col, score in enumerate(gmeta_amd.PAIR_SCORES):
            w = med(wall_ms(call, col, a.reps, a.warmup))
            ph, rounds = phase_ms(call, col, a.reps)
            pm = {p: med(ph[p]) for p in PHASES}
            r = {'what': name, 'score': score, 'sources': len(nodes), 'pairs': pairs, 'rounds': rounds, 'wall_ms': round(w[0], 3), 'wall_min_ms': round(w[1], 3), 'wall_max_ms': round(w[2], 3)}
            r.update({p + '_ms': round(pm[p][0], 3) for p in PHASES})
            print(json.dumps(r), flush=True)
            lines.append('  %-20s wall %9.3f (%.3f - %.3f)   enumerate %8.3f (%.3f - %.3f)   score %8.3f (%.3f - %.3f)   select %8.3f (%.3f - %.3f)   %d rounds   %.0f pairs / us end to end'
                         % ((score,) + w + pm['enumerate'] + pm['score'] + pm['select'] + (rounds, pairs / w[0] / 1e3)))
    ok = True
    if not a.no_host:
        import candidate_ref as ref
        import pair_score_ref
        sample = sets['random'][:a.sample]
        t0 = time.perf_counter()
        nb = pair_score_ref.neighbourhoods(N, src, dst)
        t_nb = time.perf_counter() - t0
        t0 = time.perf_counter()
        csets = [ref.candidates(N, src, dst, x, nb) for x in sample.tolist()]
        pairs = ref.pairs_of(sample.tolist(), csets)
        t_sets = time.perf_counter() - t0
        t0 = time.perf_counter()
        pair_score_ref.pair_scores(N, src, dst, pairs, 0, nb)
        t_scores = time.perf_counter() - t0
        dev = store.pair_scores(0, pairs)
        t0 = time.perf_counter()
        want = ref.top_k(sample.tolist(), csets, dev[:, 2], a.k)
        t_rank = time.perf_counter() - t0
        got = store.link_candidates(0, sample, k=a.k)
        ok = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(got[2], want[2]))
        per = (t_sets + t_scores + t_rank) / len(sample)
        print(json.dumps({'what': 'restatement', 'sample': len(sample), 'pairs': len(pairs), 'neighbourhoods_s': round(t_nb, 2), 'sets_s': round(t_sets, 3), 'scores_s': round(t_scores, 3),
                          'rank_s': round(t_rank, 3), 'scaled_to_all_sources_s': round(per * a.sources, 1), 'device_equals_restatement': ok}), flush=True)
        lines.append('  host     restatement on %d of the random sources (%d pairs): candidate sets %.3f s, scores %.3f s, ranking %.3f s (+ %.2f s once for the Python sets of the graph); '
                     'scaled to %d sources: %.1f s' % (len(sample), len(pairs), t_sets, t_scores, t_rank, t_nb, a.sources, per * a.sources))
        lines.append('           device (adamic_adar, k = %d) equals the restatement fed with the device\'s pair scores on the sample: %s' % (a.k, ok))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    assert ok, 'the device result differs from the restatement'


if __name__ == '__main__':
    main()
