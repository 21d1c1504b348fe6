"""Time and memory of the BUDDY pair predictor on the device (gm_prop_pair_mlp_forward / gm_prop_pair_mlp_step) beside the path a user had without it, reported
with no target.  Case: the arxiv-shaped synthetic graph of the other pair benchmarks (synth.CONFIGS['arxiv'], 128 feature columns), hops 2, hidden 256, 16
structure columns (the width sketch_profile_features gives at hops 2; their values do not matter to the time: random here).

    python tools/pair_mlp_bench.py [--reps 5] [--warmup 2] [--section all|kernels|fit] [--out profiles/pair_mlp.txt]

batches        10,000 pairs, 262,144 pairs (half edges, half negatives from GraphStore.negative_pairs), and all directed edges plus as many negatives.
fused          forward (scoring) and step (forward, loss, all gradients): HIP events around the C call, median (min - max) of --reps after --warmup.
unfused        the same model with what the package had before, on the same device in the same process: pair_features(as_torch=True) (its device call) -> torch.cat with the
               structure columns -> torch.addmm / relu / binary_cross_entropy_with_logits -> .backward() for the weights only, in chunks of 262,144 pairs where
               the batch is larger (the materialised [n, K] matrix of a chunk is 0.42 GB).  Its logits and gradients are compared with the fused ones.
memory         unfused: torch's peak allocation above the resident inputs; fused: its scratch by the formula of pair_mlp.hip (dh rows + range partials + tile
               partials of one chunk of pair_mlp_rows), and the drop of free device memory across the first call (the stream-ordered pool keeps what it took).
rates          2 n K Hd FLOP for a forward, 4 n K Hd for a step (the weight gradient; the hidden layer's input needs no gradient), over the time: fp32-equivalent
               TFLOP/s, beside torch's fp32 GEMM [262144, K] @ [K, 256] and the HBM copy rate (bench.py's box_calibration), both measured in this process.
fit            (--section fit, or all) one PairPredictor.fit epoch over 262,144 pairs (batch 4,096) with REAL structure columns, host clock: the columns built up
               front on the host (sketch_profile_features(link_sketch_profiles(...)): pair_counts, read-back, float64 numpy) and passed as extra=, against the same
               epoch with sketches=, which builds them per minibatch on the device (gm_sketch_pair_features).  Both start from the same seed; their losses are printed.
One JSON line per measurement; --out appends a plain-text table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gmeta_amd                         # noqa: E402
from gmeta_amd import _lib, synth        # noqa: E402
from pair_distance_bench import timed    # noqa: E402

HOPS, HD, S, CHUNK = 2, 256, 16, 262144
LIB_ROWS, RANGE, MAX_RANGES, TILE = 65536, 1024, 256, 128          # pair_mlp.hip: PM_ROWS, PM_RANGE, PM_MAX_RANGES, PM_T


def fused_scratch_bytes(n, K, Hd):
    rows = min(LIB_ROWS, n)
    tiles = -(-rows // TILE)
    pad = tiles * TILE
    HP = -(-Hd // 64) * 64
    rr = max(RANGE, -(-(-(-pad // MAX_RANGES)) // 32) * 32)
    ranges = -(-pad // rr)
    return 4 * (pad * HP + tiles * (2 * HP + 4) + ranges * K * Hd)


def fit_section(store, N, src, dst, F, a, lines):
    """one fit epoch over CHUNK pairs: host-built columns as extra= against sketches="""
    rng = np.random.default_rng(7)
    edges = np.stack([src, dst], 1).astype(np.int64)
    pos = edges[rng.choice(len(edges), CHUNK // 2, replace=False)]
    pairs = np.concatenate([pos, store.negative_pairs(0, CHUNK - len(pos), seed=222)]).astype(np.int64)
    labels = np.concatenate([np.ones(len(pos), np.float32), np.zeros(CHUNK - len(pos), np.float32)])
    names = ['0_%d_%d' % (x, y) for x, y in pairs.tolist()]

    def clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = call()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    with store.propagated_features(0, hops=HOPS) as props, store.sketches(0, hops=HOPS) as sk:
        res = {}
        for k in range(a.warmup + a.reps):
            x, t_cols = clock(lambda: gmeta_amd.sketch_profile_features(gmeta_amd.link_sketch_profiles([sk], names)))
            model = gmeta_amd.PairPredictor(F, HOPS, hidden=HD, extra_dim=S, seed=0)
            curve_h, t_host = clock(lambda: model.fit([props], names, labels, extra=x, epochs=1))
            model = gmeta_amd.PairPredictor(F, HOPS, hidden=HD, extra_dim=S, seed=0)
            curve_d, t_dev = clock(lambda: model.fit([props], names, labels, epochs=1, sketches=[sk]))
            if k >= a.warmup:
                for key, v in (('columns', t_cols), ('fit_extra', t_host), ('fit_sketches', t_dev)):
                    res.setdefault(key, []).append(v)
    stat = {key: (float(np.median(v)), float(min(v)), float(max(v))) for key, v in res.items()}
    host_total = stat['columns'][0] + stat['fit_extra'][0]
    rec = {'what': 'fit epoch', 'n': CHUNK, 'batch': 4096, 'host_columns_ms': [round(t, 1) for t in stat['columns']], 'fit_extra_ms': [round(t, 1) for t in stat['fit_extra']],
           'fit_sketches_ms': [round(t, 1) for t in stat['fit_sketches']], 'host_total_over_device': round(host_total / stat['fit_sketches'][0], 2), 'loss_extra': curve_h[0],
           'loss_sketches': curve_d[0]}
    print(json.dumps(rec), flush=True)
    lines.append('fit, one epoch over %d pairs in minibatches of 4096, %d structure columns from the sketches (hops %d, p 8, K 128), host clock, median (min - max) of %d after %d:'
                 % (CHUNK, S, HOPS, a.reps, a.warmup))
    lines.append('  host-built extra=:  columns up front %9.1f ms (%.1f - %.1f)  +  epoch %8.1f ms (%.1f - %.1f)  =  %9.1f ms      sketches=:  epoch %8.1f ms (%.1f - %.1f)      '
                 'host route / device route %.2f      loss %.7f vs %.7f' % (stat['columns'] + stat['fit_extra'] + (host_total,) + stat['fit_sketches'] + (host_total / stat['fit_sketches'][0],
                                                                                                                                                    curve_h[0], curve_d[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--section', default='all', choices=['all', 'kernels', 'fit'])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    import bench
    lib = _lib.lib()
    box = bench.box_calibration(lib, _lib, argparse.Namespace(rows=0))       # (rows = 0: the copy only)
    copy_gbps = float(box['hbm_copy']['GBps'])
    cfg = synth.CONFIGS['arxiv']
    d = synth.node_dataset(cfg['n'], cfg['m'], cfg['F0'], cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    F = store.feat_dim
    K = (HOPS + 1) * F + S
    props = store.propagated_features(0, hops=HOPS)
    model = gmeta_amd.PairPredictor(F, HOPS, hidden=HD, extra_dim=S, seed=0)
    st = _lib.stream_ptr()
    # the box's plain fp32 GEMM: torch.mm at the shape of one chunk's hidden layer
    xa = torch.empty(CHUNK, K, dtype=torch.float32, device='cuda').normal_(); wb = torch.empty(K, HD, dtype=torch.float32, device='cuda').normal_()
    med, _, _ = timed(lambda: [torch.mm(xa, wb) for _ in range(10)], a.reps, a.warmup)
    gemm_tf = 10 * 2.0 * CHUNK * K * HD / (med * 1e-3) / 1e12
    del xa, wb
    rng = np.random.default_rng(5)
    edges = np.stack([src, dst], 1).astype(np.int64)
    lines = ['arxiv (m = %d): %d nodes, %d directed edges, F = %d, hops %d: K = %d, hidden %d, %d structure columns; %s'
             % (cfg['m'], N, len(src), F, HOPS, K, HD, S, torch.cuda.get_device_name(0)),
             'box: HBM copy rate %.0f GB/s (1 GiB device copy, read + written), torch fp32 GEMM [%d, %d] @ [%d, %d] %.1f TFLOP/s; HIP events around the call, median (min - max) of %d '
             'after %d warm-up(s)' % (copy_gbps, CHUNK, K, K, HD, gemm_tf, a.reps, a.warmup),
             'unfused = pair_features(as_torch=True) -> cat -> addmm / relu / BCE-with-logits -> backward for the weights, chunks of %d pairs; memory: MB above the resident inputs' % CHUNK]
    for n in (10000, CHUNK, 2 * len(edges)) if a.section != 'fit' else ():
        pos = edges if n == 2 * len(edges) else edges[rng.choice(len(edges), n // 2, replace=False)]
        pairs = np.concatenate([pos, store.negative_pairs(0, n - len(pos), seed=222)]).astype(np.int64)
        labels = np.concatenate([np.ones(len(pos), np.float32), np.zeros(n - len(pos), np.float32)])
        perm = rng.permutation(n)
        pairs, labels = pairs[perm], labels[perm]
        d_p = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).cuda()
        d_y = torch.from_numpy(labels).cuda()
        d_e = torch.empty(n, S, dtype=torch.float32, device='cuda').uniform_(0, 3)
        logits = torch.empty(n, dtype=torch.float32, device='cuda')
        grad = torch.empty_like(model.params.data)
        loss = torch.empty(1, dtype=torch.float32, device='cuda')
        W = model.params.data
        fwd = lambda: _lib.check(lib.gm_prop_pair_mlp_forward(props.handle, _lib.ptr(d_p), n, 0, _lib.ptr(d_e), S, _lib.ptr(W), HD, _lib.ptr(logits), st), 'forward')      # noqa: E731
        step = lambda: _lib.check(lib.gm_prop_pair_mlp_step(props.handle, _lib.ptr(d_p), n, 0, _lib.ptr(d_e), S, _lib.ptr(d_y), _lib.ptr(W), HD, _lib.ptr(logits), _lib.ptr(loss),      # noqa: E731
                                                            _lib.ptr(grad), st), 'step')
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        step()
        torch.cuda.synchronize()
        pool_mb = (free0 - torch.cuda.mem_get_info()[0]) / 1e6

        w = model.params.data.clone().requires_grad_(True)
        W1, b1, w2, b2 = w[:K * HD].view(K, HD), w[K * HD:K * HD + HD], w[K * HD + HD:K * HD + 2 * HD], w[-1]

        def pair_feats(dp):                 # what pair_features(as_torch=True) runs on the device (without its host-side id check and upload: in the unfused path's favour)
            out = torch.empty((len(dp), HOPS + 1, F), dtype=torch.float32, device='cuda')
            _lib.check(lib.gm_prop_pair_features(props.handle, _lib.ptr(dp), len(dp), 0, _lib.ptr(out), st), 'gm_prop_pair_features')
            return out

        def torch_forward(out):
            with torch.no_grad():
                for i in range(0, n, CHUNK):
                    z = torch.cat([pair_feats(d_p[i:i + CHUNK]).view(-1, K - S), d_e[i:i + CHUNK]], dim=1)
                    out[i:i + CHUNK] = torch.relu(torch.addmm(b1, z, W1)) @ w2 + b2

        def torch_step(out):
            w.grad = None
            total = 0.0
            for i in range(0, n, CHUNK):
                z = torch.cat([pair_feats(d_p[i:i + CHUNK]).view(-1, K - S), d_e[i:i + CHUNK]], dim=1)
                lg = torch.relu(torch.addmm(b1, z, W1)) @ w2 + b2
                part = torch.nn.functional.binary_cross_entropy_with_logits(lg, d_y[i:i + CHUNK], reduction='sum') / n
                part.backward()
                out[i:i + CHUNK] = lg.detach()
                total = total + part.detach()
            return total

        ref_logits = torch.empty_like(logits)
        res = {}
        for what, mine, theirs, flop in (('forward', fwd, lambda: torch_forward(ref_logits), 2.0 * n * K * HD), ('step', step, lambda: torch_step(ref_logits), 4.0 * n * K * HD)):
            m_med, m_lo, m_hi = timed(mine, a.reps, a.warmup)
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
            t_med, t_lo, t_hi = timed(theirs, a.reps, a.warmup)
            peak_mb = (torch.cuda.max_memory_allocated() - base) / 1e6
            res[what] = (m_med, t_med)
            scratch_mb = fused_scratch_bytes(n, K, HD) / 1e6 if what == 'step' else 0.0
            rec = {'what': what, 'n': n, 'fused_ms': round(m_med, 3), 'fused_min_ms': round(m_lo, 3), 'fused_max_ms': round(m_hi, 3), 'unfused_ms': round(t_med, 3),
                   'unfused_min_ms': round(t_lo, 3), 'unfused_max_ms': round(t_hi, 3), 'fused_tflops': round(flop / (m_med * 1e-3) / 1e12, 2),
                   'unfused_tflops': round(flop / (t_med * 1e-3) / 1e12, 2), 'torch_gemm_tflops': round(gemm_tf, 1), 'fused_scratch_MB': round(scratch_mb, 1),
                   'fused_first_call_free_memory_drop_MB': round(pool_mb, 1), 'unfused_peak_MB': round(peak_mb, 1), 'speedup': round(t_med / m_med, 3)}
            print(json.dumps(rec), flush=True)
            lines.append('  n %8d  %-7s  fused %9.3f ms (%.3f - %.3f)  %6.2f TFLOP/s = %.3f of torch GEMM, scratch %7.1f MB   unfused %9.3f ms (%.3f - %.3f)  %6.2f TFLOP/s, '
                         'peak %7.1f MB   unfused / fused %.3f' % (n, what, m_med, m_lo, m_hi, rec['fused_tflops'], rec['fused_tflops'] / gemm_tf, scratch_mb, t_med, t_lo, t_hi,
                                                                   rec['unfused_tflops'], peak_mb, t_med / m_med))
        # the two paths compute the same model
        step(); total = torch_step(ref_logits); torch.cuda.synchronize()
        dl = float((logits - ref_logits).abs().max()); dg = float((grad - w.grad).abs().max()); gs = float(w.grad.abs().max())
        lines.append('  n %8d  agreement: largest |logit difference| %.3g, largest |gradient difference| %.3g (largest |gradient| %.3g), loss %.7f vs %.7f; first step took %.1f MB '
                     'of free device memory' % (n, dl, dg, gs, float(loss.item()), float(total), pool_mb))
        print(json.dumps({'what': 'agreement', 'n': n, 'max_logit_diff': dl, 'max_grad_diff': dg, 'max_grad': gs, 'loss': float(loss.item()), 'loss_unfused': float(total)}), flush=True)
        del d_p, d_y, d_e, logits, grad, ref_logits, w
    props.close()
    if a.section != 'kernels':
        fit_section(store, N, src, dst, F, a, lines)
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
