"""Cost of hop-distance labels, reported with no target: one FirstMM-shaped synthetic meta-batch (synth.CONFIGS['firstmm']: 8 tasks, 2-way, 16-shot,
32-query pairs) built and stepped without labels and with them (Subgraphs(hop_labels=D): two label blocks of D + 2 columns per row), same process.

    python tools/hop_label_bench.py [--reps 10] [--config firstmm] [--D 3] [--link_hops reference]

Per setting, one JSON line: the meta-step (Meta.forward's gm_meta_step, median wall time with a synchronise, ms), the build of both batches
(Subgraphs.get_batch, median wall time with a synchronise, ms), the finalisation span inside it (gm_profile_read category 10, mean over the timed
builds: the labelling kernels run there), rows of both batches, the feature width and the bytes of the labelled batches' own feature tables
(rows x padded width x 4).  A labelled layer 1 reads the batch's table instead of the store's cache-resident one, so the step's ratio is the price of
that; the last line holds both ratios."""
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


def _pad(F):
    return 32 if F <= 32 else (F + 63) // 64 * 64      # gm_pad_feat


def measure(name, D, reps, link_hops):
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args(name)
    link = bool(cfg.get('link'))
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=args.n_way, k_shot=args.k_spt, k_query=args.k_qry, batchsz=args.task_num, args=args,
                             adjs=store, h=args.h, tables=data['tables'], verbose=False, hop_labels=D, link_hops=link_hops if link else None)
    F = cfg['F0'] + gmeta_amd.hop_label_width(D, link)
    m = gmeta_amd.Meta(args, synth.make_config(F, cfg['hidden'], cfg['h'], synth.n_out(cfg), link=link)).to('cuda')
    idx = list(range(args.task_num))
    lib = _lib.lib()
    for _ in range(2):
        db.get_batch(idx)                                   # warm-up builds
    torch.cuda.synchronize()
    lib.gm_profile_enable(1)
    tb = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = db.get_batch(idx)
        torch.cuda.synchronize()
        tb.append(time.perf_counter() - t0)
    final_ms, _ = _prof(10)
    lib.gm_profile_enable(0)
    S, Q = b[0][0].view_of, b[2][0].view_of
    assert S.hop_labels_cap == D and Q.feat_dim == F
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
    r = {'config': name, 'hop_labels': D, 'link_hops': link_hops if link else None, 'meta_step_ms': round(float(np.median(ts)) * 1e3, 3),
         'build_ms': round(float(np.median(tb)) * 1e3, 3), 'finalize_span_ms': round(final_ms, 4), 'spt_rows': S.rows, 'qry_rows': Q.rows, 'feat_dim': F,
         'feat_ld': _pad(F), 'own_table_bytes': (S.rows + Q.rows) * _pad(F) * 4 if D else 0, 'device': torch.cuda.get_device_name(0)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--config', default='firstmm')
    ap.add_argument('--D', type=int, default=3)
    ap.add_argument('--link_hops', default='reference', choices=['reference', 'symmetric'])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    plain, lab = measure(a.config, 0, a.reps, a.link_hops), measure(a.config, a.D, a.reps, a.link_hops)
    print(json.dumps({'meta_step_ratio': round(lab['meta_step_ms'] / plain['meta_step_ms'], 3), 'build_ratio': round(lab['build_ms'] / plain['build_ms'], 3),
                      'finalize_span_ratio': round(lab['finalize_span_ms'] / max(plain['finalize_span_ms'], 1e-9), 3)}), flush=True)


if __name__ == '__main__':
    main()
