"""Time and accuracy of the node sketches on the device (gm_store_sketch_build, gm_sketch_pair_counts), reported with no target.  Case: the arxiv-shaped
synthetic graph of the other pair benchmarks (synth.CONFIGS['arxiv']).

    python tools/sketch_bench.py [--reps 5] [--warmup 2] [--section all|sketches|features] [--out profiles/sketches.txt]

build        (p, K) = (8, 128) and (6, 64) at H = 2 and 3: HIP events around the C call (the allocation and the final synchronisation included), median (min -
             max) of --reps after --warmup; per level one more build under GM_TIMING, where the library synchronises the stream behind every level (host
             clock).  A level gathers nnz x record bytes (every index entry reads one record of the level before): that figure per second of the level against
             the box's HBM copy rate (bench.py's box_calibration, measured in this process).
sketch_chunk the library's choice and two others, with the hub rows and segments each cuts.
pair_counts  10,000 pairs (half edges, half negatives) and all |E| edges as pairs, against gm_store_pair_distance_profile on the same 10,000 pairs at max_dist = H,
             measured in the same run.
accuracy     the estimated table (gmeta_amd.sketch_distance_profile) against the exact one over those 10,000 pairs: per cell the mean absolute error and its
             quantiles.
features     (--section features, or all) gm_sketch_pair_features at (p 8, K 128), H = 2 and 3, over the 10,000 pairs and over all edges, the result left on the
             device; gm_sketch_pair_counts alone on the same pairs in the same run; and the full host route to the same columns: NodeSketches.pair_counts (kernel
             + read-back) -> sketch_distance_profile -> sketch_profile_features -> float32 -> upload, on the host clock.  The records' bytes per second against the
             copy rate as in the pair_counts rows.
One JSON line per measurement; --out appends a plain-text table."""
import argparse
import ctypes as C
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
from pair_distance_bench import timed    # noqa: E402

SHAPES = ((8, 128), (6, 64))
HOPS = (2, 3)


def build(store, H, p, K):
    h = C.c_void_p()
    _lib.check(_lib.lib().gm_store_sketch_build(store.handle, 0, H, p, K, 222, _lib.stream_ptr(), C.byref(h)), 'gm_store_sketch_build')
    return h


def level_ms(store, H, p, K):
    """ms of level 0 (the init kernel) and of every propagation level of one build under GM_TIMING: the lines the library prints to stderr."""
    lib = _lib.lib()
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as f:
        os.dup2(f.fileno(), 2)
        try:
            assert lib.gm_set_tuning(b'GM_TIMING', 1) == 0
            lib.gm_sketch_destroy(build(store, H, p, K))
        finally:
            lib.gm_set_tuning(b'GM_TIMING', 0)
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode('utf-8', 'replace')
    ms = [float(x) / 1e3 for x in re.findall(r'gm_store_sketch_build/level(?: 0)? ([\d.]+) us', text)]
    assert len(ms) == H + 1, text
    return ms


def host_clock(call, reps, warmup):
    """ms on the host clock, the device idle before and after: median, min, max"""
    ms = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def features_section(store, N, batches, copy_gbps, a, lines):
    """gm_sketch_pair_features beside gm_sketch_pair_counts and beside the host route to the same columns"""
    lib = _lib.lib()
    lines.append('pair_features (p 8 K 128; the columns left on the device) against pair_counts alone on the same pairs, and against the host route to the same columns '
                 '(pair_counts + read-back + hll_cardinality / sketch_intersections / sketch_distance_profile / sketch_profile_features in float64 numpy + cast + upload; host clock):')
    for H in HOPS:
        L, S = H + 1, (H + 2) ** 2
        with store.sketches(0, hops=H, p=8, k=128, seed=222) as sk:
            for what, pp in batches:
                n = len(pp)
                d_p = torch.from_numpy(np.ascontiguousarray(pp, np.int32)).cuda()
                out = torch.empty((n, L, L, 3), dtype=torch.int64, device='cuda')
                balls = torch.empty((n, 2, L, 2), dtype=torch.int64, device='cuda')
                cols = torch.empty((n, S), dtype=torch.float32, device='cuda')
                counts_call = lambda: _lib.check(lib.gm_sketch_pair_counts(sk.handle, _lib.ptr(d_p), n, _lib.ptr(out), _lib.ptr(balls), _lib.stream_ptr()), 'gm_sketch_pair_counts')      # noqa: E731
                feat_call = lambda: _lib.check(lib.gm_sketch_pair_features(sk.handle, _lib.ptr(d_p), n, 1, _lib.ptr(cols), S, _lib.stream_ptr()), 'gm_sketch_pair_features')      # noqa: E731
                c_med, c_lo, c_hi = timed(counts_call, a.reps, a.warmup)
                f_med, f_lo, f_hi = timed(feat_call, a.reps, a.warmup)

                def host_route():
                    counts, bl = sk.pair_counts(pp)
                    x = gmeta_amd.sketch_profile_features(gmeta_amd.sketch_distance_profile(counts, bl, N, sk.p, sk.k))
                    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()

                h_reps, h_warm = (a.reps, 1) if n <= 100000 else (1, 0)
                h_med, h_lo, h_hi = host_clock(host_route, h_reps, h_warm)
                diff = float((host_route() - cols).abs().max())
                read = 2.0 * L * (256 + 512) * n
                rec = {'what': 'pair_features ' + what, 'hops': H, 'n': n, 'ms': round(f_med, 3), 'min_ms': round(f_lo, 3), 'max_ms': round(f_hi, 3), 'pair_counts_ms': round(c_med, 3),
                       'pair_counts_min_ms': round(c_lo, 3), 'pair_counts_max_ms': round(c_hi, 3), 'record_GBps': round(read / (f_med * 1e-3) / 1e9, 1),
                       'stored_bytes_per_pair': 4 * S, 'pair_counts_stored_bytes_per_pair': 8 * (3 * L * L + 4 * L), 'host_route_ms': round(h_med, 1), 'host_route_min_ms': round(h_lo, 1),
                       'host_route_max_ms': round(h_hi, 1), 'host_route_reps': h_reps, 'max_abs_diff_to_host': diff}
                print(json.dumps(rec), flush=True)
                lines.append('  H %d  %-18s pair_features %9.3f ms (%.3f - %.3f)   pair_counts %9.3f ms (%.3f - %.3f)   features / counts %.3f   stores %d vs %d B per pair   '
                             'records read %7.1f GB/s = %.3f of the copy rate   host route %10.1f ms (%.1f - %.1f, %d run(s)): %.0f x   largest |device - host| %.3g'
                             % (H, what, f_med, f_lo, f_hi, c_med, c_lo, c_hi, f_med / c_med, 4 * S, rec['pair_counts_stored_bytes_per_pair'], rec['record_GBps'],
                                rec['record_GBps'] / copy_gbps, h_med, h_lo, h_hi, h_reps, h_med / f_med, diff))
                del d_p, out, balls, cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--section', default='all', choices=['all', 'sketches', 'features'])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    import bench
    lib = _lib.lib()
    box = bench.box_calibration(lib, _lib, argparse.Namespace(rows=0))       # (rows = 0: the copy only)
    copy_gbps = float(box['hbm_copy']['GBps'])
    cfg = synth.CONFIGS['arxiv']
    d = synth.node_dataset(cfg['n'], cfg['m'], 4, cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    deg = store.neighbour_degrees(0).astype(np.int64)
    nnz = int(deg.sum())
    lines = ['arxiv (m = %d): %d nodes, %d directed edges, %d index entries (mean distinct degree %.2f, longest row %d, %d rows above 256); %s'
             % (cfg['m'], N, len(src), nnz, deg.mean(), deg.max(), int((deg > 256).sum()), torch.cuda.get_device_name(0)),
             'box: HBM copy rate %.0f GB/s (1 GiB device copy, bytes read + written per second); end to end: HIP events around the C call, median (min - max) of %d after %d warm-up(s);'
             % (copy_gbps, a.reps, a.warmup),
             'levels: one build under GM_TIMING, the stream synchronised behind every level (host clock); gathered bytes of a level = index entries x record bytes',
             ]
    rng = np.random.default_rng(5)
    half = len(src) // 2
    n = 10000
    pos = np.stack([src[:half], dst[:half]], 1)[rng.choice(half, n // 2, replace=False)]
    pairs = np.concatenate([pos, store.negative_pairs(0, n - n // 2, seed=222)]).astype(np.int64)
    every = np.stack([src, dst], 1).astype(np.int64)
    if a.section != 'features':
        sketch_sections(store, N, src, deg, nnz, pairs, every, copy_gbps, a, lines)
    if a.section != 'sketches':
        features_section(store, N, (('10,000 pairs', pairs), ('all %d edges' % len(every), every)), copy_gbps, a, lines)
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


def sketch_sections(store, N, src, deg, nnz, pairs, every, copy_gbps, a, lines):
    """the build, sketch_chunk, pair_counts and accuracy sections"""
    lib = _lib.lib()
    n = len(pairs)
    lines.append('build (allocation and final synchronisation included):')
    for p, K in SHAPES:
        rec_bytes = (1 << p) + 4 * K
        for H in HOPS:
            med, lo, hi = timed(lambda: lib.gm_sketch_destroy(build(store, H, p, K)), a.reps, a.warmup)
            lv = level_ms(store, H, p, K)
            gath = nnz * rec_bytes
            rates = [gath / (t * 1e-3) / 1e9 for t in lv[1:]]
            rec = {'what': 'build', 'hops': H, 'p': p, 'k': K, 'record_bytes': rec_bytes, 'sketch_MB': round(N * (H + 1) * rec_bytes / 1e6, 1), 'ms': round(med, 3), 'min_ms': round(lo, 3),
                   'max_ms': round(hi, 3), 'level_ms': [round(t, 3) for t in lv], 'gathered_MB_per_level': round(gath / 1e6, 1), 'level_GBps': [round(r, 1) for r in rates],
                   'hbm_copy_GBps': round(copy_gbps, 1)}
            print(json.dumps(rec), flush=True)
            lines.append('  H %d p %2d K %3d  record %4d B  sketch %7.1f MB  %9.3f ms (%.3f - %.3f)   level 0 %7.3f ms, levels %s ms   gathered %7.1f MB per level: %s GB/s = %s of the copy rate'
                         % (H, p, K, rec_bytes, rec['sketch_MB'], med, lo, hi, lv[0], ' / '.join('%.3f' % t for t in lv[1:]), gath / 1e6, ' / '.join('%.0f' % r for r in rates),
                            ' / '.join('%.3f' % (r / copy_gbps) for r in rates)))
    lines.append('sketch_chunk at H 2 p 8 K 128 (0: the library\'s choice, 256):')
    for chunk in (0, 64, 2 ** 30):
        C_ = chunk if chunk else 256
        hubs = deg[deg > C_]
        assert lib.gm_set_tuning(b'sketch_chunk', chunk) == 0
        try:
            med, lo, hi = timed(lambda: lib.gm_sketch_destroy(build(store, 2, 8, 128)), a.reps, a.warmup)
            lv = level_ms(store, 2, 8, 128)
        finally:
            lib.gm_set_tuning(b'sketch_chunk', 0)
        rec = {'what': 'sketch_chunk', 'chunk': chunk, 'hub_rows': int(len(hubs)), 'segments': int(((hubs + C_ - 1) // C_).sum()), 'ms': round(med, 3), 'min_ms': round(lo, 3),
               'max_ms': round(hi, 3), 'level_ms': [round(t, 3) for t in lv]}
        print(json.dumps(rec), flush=True)
        lines.append('  sketch_chunk %10d  %5d hub rows in %6d segments  %9.3f ms (%.3f - %.3f)   levels %s ms'
                     % (chunk, rec['hub_rows'], rec['segments'], med, lo, hi, ' / '.join('%.3f' % t for t in lv[1:])))
    lines.append('pair_counts (p 8 K 128) against gm_store_pair_distance_profile on the same 10,000 pairs, unmasked, max_dist = H, in the same run:')
    errs = []
    for H in HOPS:
        L = H + 1
        h = build(store, H, 8, 128)
        try:
            for what, pp in (('10,000 pairs', pairs), ('all %d edges' % len(every), every)):
                d_p = torch.from_numpy(np.ascontiguousarray(pp, np.int32)).cuda()
                out = torch.empty((len(pp), L, L, 3), dtype=torch.int64, device='cuda')
                balls = torch.empty((len(pp), 2, L, 2), dtype=torch.int64, device='cuda')
                call = lambda: _lib.check(lib.gm_sketch_pair_counts(h, _lib.ptr(d_p), len(pp), _lib.ptr(out), _lib.ptr(balls), _lib.stream_ptr()), 'gm_sketch_pair_counts')      # noqa: E731
                med, lo, hi = timed(call, a.reps, a.warmup)
                read = 2.0 * L * (256 + 512) * len(pp)
                rec = {'what': 'pair_counts ' + what, 'hops': H, 'ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'us_per_pair': round(med * 1e3 / len(pp), 4),
                       'record_GBps': round(read / (med * 1e-3) / 1e9, 1)}
                line = '  H %d  %-18s %9.3f ms (%.3f - %.3f)   %.4f us per pair   records read %7.1f GB/s = %.3f of the copy rate' % (H, what, med, lo, hi, rec['us_per_pair'], rec['record_GBps'],
                                                                                                                                      rec['record_GBps'] / copy_gbps)
                if len(pp) == n:
                    counts, bl = out.cpu().numpy(), balls.cpu().numpy()
                    ex = torch.empty((n, H + 2, H + 2), dtype=torch.int32, device='cuda')
                    exact_call = lambda: _lib.check(lib.gm_store_pair_distance_profile(store.handle, 0, _lib.ptr(d_p), n, 0, H, _lib.ptr(ex), _lib.stream_ptr()), 'pair_distance_profile')      # noqa: E731
                    e_med, e_lo, e_hi = timed(exact_call, a.reps, a.warmup)
                    exact = ex.cpu().numpy().astype(np.float64)
                    rec.update({'pair_distance_profile_ms': round(e_med, 3), 'ratio': round(e_med / med, 1)})
                    line += '   exact profile %9.3f ms (%.3f - %.3f): %.1f x' % (e_med, e_lo, e_hi, e_med / med)
                    est = gmeta_amd.sketch_distance_profile(counts, bl, N, 8, 128)
                    errs.append((H, np.abs(est - exact), exact))
                print(json.dumps(rec), flush=True)
                lines.append(line)
        finally:
            lib.gm_sketch_destroy(h)
    lines.append('accuracy over the 10,000 pairs (p 8 K 128): |estimated - exact| per cell [a][b] of the table, mean / median / 90 % / 99 % / max (mean exact count):')
    for H, err, exact in errs:
        for i in range(H + 2):
            for j in range(H + 2):
                e = err[:, i, j]
                q = np.quantile(e, (0.5, 0.9, 0.99))
                print(json.dumps({'what': 'error', 'hops': H, 'cell': [i, j], 'mean': round(float(e.mean()), 3), 'q50': round(float(q[0]), 3), 'q90': round(float(q[1]), 3),
                                  'q99': round(float(q[2]), 3), 'max': round(float(e.max()), 3), 'mean_exact': round(float(exact[:, i, j].mean()), 3)}), flush=True)
                lines.append('  H %d [%d][%d]  %10.3f / %10.3f / %10.3f / %10.3f / %10.3f   (%.3f)' % (H, i, j, e.mean(), q[0], q[1], q[2], e.max(), exact[:, i, j].mean()))


if __name__ == '__main__':
    main()
