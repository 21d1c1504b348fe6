"""Timing of adaptation and prediction (Meta.adapt / Adapted.predict / Meta.predict) on the synthetic shapes:

  * adapt on the 100 evaluation tasks of the arxiv and FirstMM shapes at K_test = 10;
  * the scoring kernel k_head_predict on >= 100k query subgraphs of one task: its per-launch time comes from a kernel trace of this script
    (rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py); printed here: the whole predict call (host read-back included) and,
    for scale, the public unfused forward gm_gcn_forward on the same batch;
  * Meta.predict against finetunning_batch on the same 100 tasks (predict runs one query evaluation, finetunning K + 1).

    python tools/predict_bench.py [--reps 5] [--nq 100000]

Prints one JSON line per measurement.  The scoring kernel's algorithmic bytes per subgraph: nc * Hd floats of H_L read, its head weights and its
set's prototypes (L2-resident, not counted), n_out logits written and read back once, c_task + 1 words written."""
import argparse
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
from gmeta_amd import synth              # noqa: E402


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def _shape(name, n_tasks, K, **over):
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args(name, task_num=n_tasks, update_step_test=K, **over)
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=args.n_way, k_shot=args.k_spt, k_query=args.k_qry, batchsz=n_tasks, args=args,
                             adjs=store, h=args.h, tables=data['tables'], verbose=False)
    config = synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], synth.n_out(cfg), link=bool(cfg.get('link')))
    m = gmeta_amd.Meta(args, config).to('cuda')
    return args, cfg, data, store, db, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--nq', type=int, default=100000)
    ap.add_argument('--tasks', type=int, default=100)
    ap.add_argument('--K', type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    box = torch.cuda.get_device_name(0)
    for name in ('arxiv', 'firstmm'):
        args, cfg, data, store, db, m = _shape(name, a.tasks, a.K)
        b = db.get_batch(list(range(a.tasks)))
        t_adapt = _timed(lambda: m.adapt(b[0], b[1]), a.reps)
        t_pred = _timed(lambda: m.predict(b[0], b[1], b[2]), a.reps)
        t_ft = _timed(lambda: m.finetunning_batch(b[0], b[1], b[2], b[3]), a.reps)
        print(json.dumps({'shape': name, 'tasks': a.tasks, 'K_test': a.K, 'adapt_ms': round(t_adapt, 3), 'predict_ms': round(t_pred, 3),
                          'finetunning_batch_ms': round(t_ft, 3), 'device': box}), flush=True)
        if name != 'arxiv':
            continue
        # the scoring kernel on >= nq query subgraphs of one task (its launch time: kernel trace); the whole call, and the public unfused forward for scale
        # (16 sampled nodes per query subgraph: the activations of 10^5 full-size arxiv subgraphs would not fit in HBM)
        args, cfg, data, store, db, m = _shape(name, a.tasks, a.K, sample_nodes=16)
        b = db.get_batch(list(range(a.tasks)))
        ad = m.adapt(b[0], b[1])
        rng = np.random.default_rng(0)
        n = data['graphs'][0][0]
        QB = db.query_batch([['0_%d' % v for v in rng.integers(0, n, a.nq)]])
        t_call = _timed(lambda: ad.predict(QB, tasks=[0]), a.reps)
        import ctypes as C
        from gmeta_amd import _lib
        lib = _lib.lib()
        model = m.net.model
        ws = torch.empty(int(lib.gm_gcn_ws_bytes(QB.handle, C.byref(model))), dtype=torch.uint8, device='cuda')
        logits = torch.empty(QB.subs, model.n_out, device='cuda')
        fw = ad.fast_weights[:1].contiguous()

        def fwd():
            _lib.check(lib.gm_gcn_forward(QB.handle, C.byref(model), _lib.ptr(fw), 0, None, None, _lib.ptr(logits), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr()), 'gm_gcn_forward')
        t_fwd = _timed(fwd, a.reps)
        hd, nc, c_task = model.dims[model.n_gcn], QB.centres, ad.prototypes.shape[1]
        by = QB.subs * 4 * (nc * hd + 2 * model.n_out + c_task + 1)
        print(json.dumps({'what': 'predict call on one task (host read-back included)', 'subgraphs': QB.subs, 'rows': QB.rows,
                          'predict_call_ms': round(t_call, 3), 'query_forward_ms': round(t_fwd, 3),
                          'algorithmic_bytes_scoring': by, 'device': box,
                          'note': 'per-launch time of k_head_predict: rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py'}), flush=True)


if __name__ == '__main__':
    main()
