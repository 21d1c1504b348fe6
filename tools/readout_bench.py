"""Cost of the mean readout (gm_set_readout; config entry ('Readout', ['mean'])), reported with no target: an arxiv-shaped node meta-batch
(synth.CONFIGS['arxiv'] at --tasks tasks) and a FirstMM-shaped pair meta-batch (synth.CONFIGS['firstmm']) stepped with the centre readout and
with the mean readout, same process, same batches.

    python tools/readout_bench.py [--reps 10] [--tasks 8] [--configs arxiv,firstmm]

Per config and readout, one JSON line: the meta-step (Meta.forward's gm_meta_step + Adam, median wall time with a synchronise, ms), rows and subgraphs
of both batches.  Under the mean readout also the two pooling kernels, from one more step on ONE stream (gm_hparams_t.serialize, so that no other
kernel shares the chip with them) with the library's launch profile on (gm_profile_read categories 16 / 17): per launch of the support and of the
query batch, time, algorithmic bytes computed HERE from the batch (forward 4 rows Hd + 4 subs Hd, k_readout_mean together with k_readout_mean_fin;
backward 8 rows Hd + 4 subs Hd, k_readout_mean_bwd) -- checked against what the library accounted -- and the share of the box's HBM copy rate
(bench.py's box_calibration: a 1 GiB device copy, bytes read + written per second)."""
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


def _launches(cat, cap=256):
    ms, wk = (C.c_double * cap)(), (C.c_int64 * cap)()
    n = _lib.lib().gm_profile_read_launches(cat, ms, wk, cap)
    if n < 0:
        _lib.check(n, 'gm_profile_read_launches')
    return [(ms[k], wk[k]) for k in range(n)]


def _time_steps(m, b, feats, reps):
    theta = [p.detach().clone() for p in m.net.parameters()]
    ts = []
    for k in range(reps + 2):
        with torch.no_grad():
            for p, v in zip(m.net.parameters(), theta):
                p.copy_(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m(b[0], b[1], b[2], b[3], None, None, None, None, None, None, feats)
        torch.cuda.synchronize()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def measure(name, tasks, reps, copy_gbps):
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args(name, **({'task_num': tasks} if tasks else {}))
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=args.n_way, k_shot=args.k_spt, k_query=args.k_qry, batchsz=args.task_num, args=args,
                             adjs=store, h=args.h, tables=data['tables'], verbose=False)
    b = db.get_batch(list(range(args.task_num)))
    S, Q = b[0][0].view_of, b[2][0].view_of
    link, Hd = bool(cfg.get('link')), cfg['hidden']
    base = synth.make_config(cfg['F0'], Hd, cfg['h'], synth.n_out(cfg))
    out = []
    for readout in ('centre', 'mean'):
        config = base + ([('Readout', ['mean'])] if readout == 'mean' else []) + ([('LinkPred', [True])] if link else [])
        m = gmeta_amd.Meta(args, config).to('cuda')
        r = {'config': name, 'readout': readout, 'tasks': args.task_num, 'K': args.update_step, 'hidden': Hd, 'meta_step_ms': round(_time_steps(m, b, data['feats'], reps), 3),
             'spt_rows': S.rows, 'spt_subs': S.subs, 'qry_rows': Q.rows, 'qry_subs': Q.subs, 'device': torch.cuda.get_device_name(0)}
        if readout == 'mean':
            lib = _lib.lib()
            m.serialize = 1
            m(b[0], b[1], b[2], b[3], None, None, None, None, None, None, data['feats'])      # (the one-stream schedule, warm)
            torch.cuda.synchronize()
            lib.gm_profile_enable(1)
            m(b[0], b[1], b[2], b[3], None, None, None, None, None, None, data['feats'])
            torch.cuda.synchronize()
            for key, cat, per_row in (('k_readout_mean', 16, 4), ('k_readout_mean_bwd', 17, 8)):
                for batch, B in (('spt', S), ('qry', Q)):
                    want = per_row * B.rows * Hd + 4 * B.subs * Hd                        # algorithmic bytes of one launch over this batch
                    mine = [ms for ms, wk in _launches(cat) if wk == want]
                    assert mine, (key, batch, want, sorted({wk for _, wk in _launches(cat)}))
                    ms = float(np.median(mine))
                    gbps = want / (ms * 1e-3) / 1e9
                    r['%s_%s' % (key, batch)] = {'launches': len(mine), 'ms': round(ms, 4), 'bytes': want, 'GBps': round(gbps, 1), 'share_of_hbm_copy': round(gbps / copy_gbps, 3)}
            lib.gm_profile_enable(0)
        print(json.dumps(r), flush=True)
        out.append(r)
    print(json.dumps({'config': name, 'meta_step_ratio_mean_over_centre': round(out[1]['meta_step_ms'] / out[0]['meta_step_ms'], 3)}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--tasks', type=int, default=8, help='tasks of the arxiv-shaped meta-batch (the FirstMM shape keeps its 8)')
    ap.add_argument('--configs', default='arxiv,firstmm')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    import bench
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    box = bench.box_calibration(_lib.lib(), _lib, argparse.Namespace(rows=0))       # (rows = 0: the copy only, not the GEMM calibration)
    print(json.dumps({'box': box}), flush=True)
    copy_gbps = float(box['hbm_copy']['GBps'])
    for name in a.configs.split(','):
        measure(name, a.tasks if name == 'arxiv' else None, a.reps, copy_gbps)


if __name__ == '__main__':
    main()
