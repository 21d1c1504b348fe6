"""Time of the neighbourhood heuristic scores on the device (GraphStore.pair_scores -> gm_store_pair_scores), reported with no target: integer and latency
work -- a strided walk over the shorter neighbour row, one binary search per neighbour in the longer one, two 4-byte gathers per hit -- with no roofline to
hold it against.  Case: the arxiv-shaped synthetic graph (synth.CONFIGS['arxiv']: 169,343 nodes, stored in both directions) and the pair list a link
data set brings: |E| / 2 edges (every undirected edge once) plus as many pairs from GraphStore.negative_pairs.

    python tools/pair_score_bench.py [--config arxiv] [--reps 10] [--warmup 2] [--out profiles/pair_scores.txt] [--no_host] [--n N] [--m M]

Three times: the neighbour-index build, once (wall clock around the first call that needs it: download of the two CSRs, per-row merge on the host, upload);
the scoring call (HIP events around the C call, median of --reps after --warmup) for the library's lane choice and for every forced lanes-per-pair value,
with and without the mask flag; the restatement of the definition (tests/pair_score_ref.py) for the same pairs, once, and how the device result sits
inside the tolerances of tests/test_hip_pair_scores.py.  One JSON line per measurement; --out appends a plain-text table."""
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

LANES = (0, 16, 32, 64)


def device_ms(store, d_pairs, flags, reps, warmup):
    lib = _lib.lib()
    n = d_pairs.shape[0]
    out = torch.empty((n, 5), dtype=torch.float32, device='cuda')
    ms = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.gm_store_pair_scores(store.handle, 0, _lib.ptr(d_pairs), n, flags, _lib.ptr(out), _lib.stream_ptr()), 'pair_scores')
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='arxiv')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=None, help="nodes (default: the config's)")
    ap.add_argument('--m', type=int, default=None, help="edges each new node of the preferential-attachment graph brings (default: the config's): the graph's density")
    ap.add_argument('--no_host', action='store_true', help='skip the restatement (a minute or more of pure Python at the arxiv size)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = synth.CONFIGS[a.config]
    m = a.m if a.m is not None else cfg['m']
    d = synth.node_dataset(a.n if a.n is not None else cfg['n'], m, 4, cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    half = len(src) // 2                                                     # node_dataset lists u -> v first, then the reverses
    pos = np.stack([src[:half], dst[:half]], 1)
    neg = store.negative_pairs(0, half, seed=222)
    pairs = np.concatenate([pos, neg]).astype(np.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    deg = store.neighbour_degrees(0)                                         # the first call that needs the index builds it
    build_s = time.perf_counter() - t0
    lines = ['%s (m = %d): %d nodes, %d directed edges (undirected graph stored in both directions), mean distinct degree %.2f, longest row %d; %d pairs = %d edges + %d negative_pairs; %s'
             % (a.config, m, N, len(src), deg.mean(), deg.max(), len(pairs), half, len(neg), torch.cuda.get_device_name(0)),
             '  index build (once per store; wall clock around the first call: download, per-row merge on the host, upload)   %.3f s' % build_s,
             'device: HIP events around gm_store_pair_scores, median (min - max) of %d after %d warm-ups' % (a.reps, a.warmup)]
    print(json.dumps({'what': 'index build', 's': round(build_s, 3), 'mean_degree': round(float(deg.mean()), 2), 'max_degree': int(deg.max())}), flush=True)
    d_pairs = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).cuda()
    lib = _lib.lib()
    got = {}
    for lanes in LANES:
        assert lib.gm_set_tuning(b'pair_lanes', lanes) == 0
        for flags in (0, 1):
            med, lo, hi, got[(lanes, flags)] = device_ms(store, d_pairs, flags, a.reps, a.warmup)
            r = {'what': 'device', 'pair_lanes': lanes, 'mask_target': flags, 'n': len(pairs), 'ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3),
                 'pairs_per_us': round(len(pairs) / med / 1e3, 1)}
            print(json.dumps(r), flush=True)
            lines.append('  device   pair_lanes %-10s mask_target %d %10.3f ms  (%.3f - %.3f)   %.0f pairs / us'
                         % ('%d' % lanes if lanes else '0 (library)', flags, med, lo, hi, len(pairs) / med / 1e3))
    lib.gm_set_tuning(b'pair_lanes', 0)
    for flags in (0, 1):                                                     # the exact columns do not depend on the lanes
        assert all(np.array_equal(got[(l, flags)][:, [0, 4]], got[(0, flags)][:, [0, 4]]) for l in LANES)
    ok = True
    if not a.no_host:
        import pair_score_ref as ref
        t0 = time.perf_counter()
        want = ref.pair_scores(N, src, dst, pairs, 0)
        s = time.perf_counter() - t0
        g = got[(0, 0)].astype(np.float64)
        exact = bool(np.array_equal(got[(0, 0)][:, [0, 4]], want[:, [0, 4]].astype(np.float32)))
        terms = np.minimum(deg[pairs[:, 0]], deg[pairs[:, 1]]) + 8.0
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = np.where(want > 0, np.abs(g - want) / want, np.where(g != want, np.inf, 0.0))
        worst = (float(rel[:, 1].max() * 2.0 ** 22), float((rel[:, 2] / (terms * 2.0 ** -24)).max()), float((rel[:, 3] / (terms * 2.0 ** -24)).max()))
        ok = exact and max(worst) <= 1.0
        print(json.dumps({'what': 'restatement', 'n': len(pairs), 's': round(s, 2), 'cn_and_pref_attachment_equal': exact, 'worst_share_of_tolerance': [round(w, 3) for w in worst]}), flush=True)
        lines.append('  host     restatement (tests/pair_score_ref.py: Python sets, one pair at a time), same pairs, no mask   %.2f s' % s)
        lines.append('           device (library lanes) against it: cn and pref_attachment equal: %s; largest error as a share of the tolerance: jaccard %.3f of 2^-22, '
                     'adamic_adar %.3f and resource_allocation %.3f of (min deg + 8) 2^-24' % ((exact,) + worst))
        y = np.concatenate([np.ones(half), np.zeros(len(neg))])
        auc = {nm: gmeta_amd.link_auc(got[(0, 1)][:, k], y) for k, nm in enumerate(gmeta_amd.PAIR_SCORES)}
        lines.append('           ROC AUC of the masked scores, edges against negatives: ' + '  '.join('%s %.4f' % kv for kv in auc.items()))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    assert ok, 'the device result leaves the tolerances of the definition'


if __name__ == '__main__':
    main()
