"""Cost of target-link masking (GM_LINK_MASK_TARGET), reported with no target: one FirstMM-shaped synthetic pair meta-batch (synth.CONFIGS['firstmm']:
8 tasks, 2-way, 16-shot, 32-query -> 256 support + 512 query pairs, sample_nodes 1000) built with symmetric pairs (h = 2) without the mask and with
it, same process.  Every listed pair of that dataset is an edge of its graph (the negatives are injected), so the mask has work in every subgraph.

    python tools/link_mask_bench.py [--builds 5] [--warmup 2] [--config firstmm] [--link_hops symmetric]

Per setting, one JSON line: the device time of k_nodes, of k_fill and of the finalisation span (gm_profile_read categories 8, 9, 10; means over the
timed builds, ms), the build's wall time (Subgraphs.get_batch with a synchronise, median, ms) and the rows and edges of both batches; the last line
holds the ratios."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gmeta_amd                         # noqa: E402
from gmeta_amd import _lib, synth        # noqa: E402


def _prof(cat):
    ms, n, work = C.c_double(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().gm_profile_read(cat, C.byref(ms), C.byref(n), C.byref(work)), 'gm_profile_read')
    return ms.value / max(n.value, 1), n.value


def measure(name, mask, builds, warmup, link_hops):
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args(name)
    assert cfg.get('link'), 'target-link masking is a pair mode'
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=args.n_way, k_shot=args.k_spt, k_query=args.k_qry, batchsz=args.task_num, args=args,
                             adjs=store, h=args.h, tables=data['tables'], verbose=False, link_hops=link_hops, mask_target=mask)
    idx = list(range(args.task_num))
    lib = _lib.lib()
    for _ in range(warmup):
        db.get_batch(idx)
    torch.cuda.synchronize()
    lib.gm_profile_enable(1)
    tb = []
    for _ in range(builds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = db.get_batch(idx)
        torch.cuda.synchronize()
        tb.append(time.perf_counter() - t0)
    (nodes_ms, n_nodes), (fill_ms, _), (final_ms, _) = _prof(8), _prof(9), _prof(10)
    lib.gm_profile_enable(0)
    S, Q = b[0][0].view_of, b[2][0].view_of
    assert S.mask_target == bool(mask) and Q.mask_target == bool(mask)
    r = {'config': name, 'mask_target': int(bool(mask)), 'link_mode': db.link_mode, 'h': args.h, 'sample_nodes': args.sample_nodes, 'k_nodes_ms': round(nodes_ms, 4),
         'k_fill_ms': round(fill_ms, 4), 'finalize_span_ms': round(final_ms, 4), 'launches': n_nodes, 'build_ms': round(float(np.median(tb)) * 1e3, 3),
         'spt_subs': S.subs, 'qry_subs': Q.subs, 'spt_rows': S.rows, 'spt_edges': S.edges, 'qry_rows': Q.rows, 'qry_edges': Q.edges,
         'device': torch.cuda.get_device_name(0)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--builds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--config', default='firstmm')
    ap.add_argument('--link_hops', default='symmetric', choices=['reference', 'symmetric'])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    plain, masked = measure(a.config, 0, a.builds, a.warmup, a.link_hops), measure(a.config, 1, a.builds, a.warmup, a.link_hops)
    print(json.dumps({k.replace('_ms', '_ratio'): round(masked[k] / max(plain[k], 1e-9), 3) for k in ('k_nodes_ms', 'k_fill_ms', 'finalize_span_ms', 'build_ms')}),
          flush=True)


if __name__ == '__main__':
    main()
