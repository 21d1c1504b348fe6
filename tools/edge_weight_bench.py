"""Cost of edge weights, reported with no target: one FirstMM-shaped synthetic meta-batch (synth.CONFIGS['firstmm']: 8 tasks, 2-way, 16-shot,
32-query pairs) extracted and stepped on the plain store and on the same graphs with log-uniform weights (synth.with_edge_weights).

    python tools/edge_weight_bench.py [--reps 10] [--config firstmm]

Per store, one JSON line: the meta-step (Meta.forward's gm_meta_step, median wall time with a synchronise, ms), gm_extract_pair's k_fill per
launch and the finalisation span (gm_profile_read categories 9 / 10, means over the timed builds), rows and edges of both batches.  The weighted
fill writes 8 more bytes per edge (one fp32 weight in each orientation) beside the 8 bytes of the two index arrays, and reads 4 to 8 more; the
last line is the measured ratio next to that expectation."""
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


def measure(name, weighted, reps):
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args(name)
    data = synth.make_dataset(cfg, edge_weights=weighted)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=args.n_way, k_shot=args.k_spt, k_query=args.k_qry, batchsz=args.task_num, args=args,
                             adjs=store, h=args.h, tables=data['tables'], verbose=False)
    m = gmeta_amd.Meta(args, synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], synth.n_out(cfg), link=bool(cfg.get('link')))).to('cuda')
    idx = list(range(args.task_num))
    lib = _lib.lib()
    for _ in range(2):
        db.get_batch(idx)                                   # warm-up builds
    torch.cuda.synchronize()
    lib.gm_profile_enable(1)
    for _ in range(reps):
        b = db.get_batch(idx)
    torch.cuda.synchronize()
    fill_ms, n_fill = _prof(9)
    final_ms, _ = _prof(10)
    lib.gm_profile_enable(0)
    S, Q = b[0][0].view_of, b[2][0].view_of
    theta = [p.detach().clone() for p in m.net.parameters()]
    ts = []
    for k in range(reps + 2):
        with torch.no_grad():
            for p, v in zip(m.net.parameters(), theta):
                p.copy_(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m(b[0], b[1], b[2], b[3], None, None, None, None, None, None, data['feats'])
        torch.cuda.synchronize()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    r = {'config': name, 'weighted': bool(store.weighted), 'meta_step_ms': round(float(np.median(ts)) * 1e3, 3), 'k_fill_ms_per_launch': round(fill_ms, 4),
         'k_fill_launches': n_fill, 'finalize_span_ms': round(final_ms, 4), 'spt_rows': S.rows, 'spt_edges': S.edges, 'qry_rows': Q.rows, 'qry_edges': Q.edges,
         'device': torch.cuda.get_device_name(0)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--config', default='firstmm')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    plain, wtd = measure(a.config, False, a.reps), measure(a.config, True, a.reps)
    print(json.dumps({'meta_step_ratio': round(wtd['meta_step_ms'] / plain['meta_step_ms'], 3),
                      'k_fill_ratio': round(wtd['k_fill_ms_per_launch'] / max(plain['k_fill_ms_per_launch'], 1e-9), 3),
                      'expectation': 'k_fill writes 16 instead of 8 bytes per edge (+ 4 per row either way); the step reads the same tables'}), flush=True)


if __name__ == '__main__':
    main()
