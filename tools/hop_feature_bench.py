"""Time of the hop-propagated node features on the device (gm_store_propagate_build, gm_prop_pair_features), reported with no target.  Case: the arxiv-shaped
synthetic graph of the other pair benchmarks (synth.CONFIGS['arxiv']) with its 128 feature columns.

    python tools/hop_feature_bench.py [--reps 5] [--warmup 2] [--out profiles/hop_features.txt]

build          hops = 2 and 3, with the self loops: HIP events around the C call (the allocation, the level-0 copy and the final synchronisation included), median
               (min - max) of --reps after --warmup; per phase one more build under GM_TIMING, where the library synchronises the stream behind the norms and
               behind every level (host clock).  A level gathers entries x row bytes (every entry of every extended row reads one row of the level before):
               that figure per second of the level against the box's HBM copy rate (bench.py's box_calibration, measured in this process).
prop_chunk     the library's choice and two others, with the hub rows and segments each cuts.
pair_features  10,000 pairs (half edges, half negatives) and all |E| edges as pairs, both operations; bytes read + written per second.
comparators    torch.sparse.mm with the same operator as a CSR tensor on the same device (if it runs there), and scipy.sparse on the host (if installed): the
               same levels, the largest difference from the device's printed beside the time.
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

HOPS = (2, 3)
LIB_CHUNK = 256


def build(store, hops, flags=1):
    h = C.c_void_p()
    _lib.check(_lib.lib().gm_store_propagate_build(store.handle, 0, hops, flags, _lib.stream_ptr(), C.byref(h)), 'gm_store_propagate_build')
    return h


def phase_ms(store, hops):
    """ms of the norm phase and of every level of one build under GM_TIMING: the lines the library prints to stderr."""
    lib = _lib.lib()
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as f:
        os.dup2(f.fileno(), 2)
        try:
            assert lib.gm_set_tuning(b'GM_TIMING', 1) == 0
            lib.gm_prop_destroy(build(store, hops))
        finally:
            lib.gm_set_tuning(b'GM_TIMING', 0)
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode('utf-8', 'replace')
    norm = [float(x) / 1e3 for x in re.findall(r'gm_store_propagate_build/norm ([\d.]+) us', text)]
    lv = [float(x) / 1e3 for x in re.findall(r'gm_store_propagate_build/level ([\d.]+) us', text)]
    assert len(norm) == 1 and len(lv) == hops, text
    return norm[0], lv


def operator(ptr, idx, N):
    """(row, col, value) of A^ = D~^-1/2 (A + I) D~^-1/2 in float64 over the in-edge CSR, one value per entry (parallel edges stay separate entries)."""
    row = np.concatenate([np.arange(N), np.repeat(np.arange(N), np.diff(ptr))])
    col = np.concatenate([np.arange(N), idx.astype(np.int64)])
    d = np.bincount(row, minlength=N).astype(np.float64)
    nm = 1.0 / np.sqrt(np.where(d > 0, d, 1.0))
    return row, col, nm[row] * nm[col]


def all_levels(h, N, hops, F):
    out = torch.empty((hops + 1, N, F), dtype=torch.float32, device='cuda')
    nodes = torch.arange(N, dtype=torch.int32, device='cuda')
    for t in range(hops + 1):
        _lib.check(_lib.lib().gm_prop_rows(h, t, _lib.ptr(nodes), N, _lib.ptr(out[t]), _lib.stream_ptr()), 'gm_prop_rows')
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    import bench
    lib = _lib.lib()
    box = bench.box_calibration(lib, _lib, argparse.Namespace(rows=0))       # (rows = 0: the copy only)
    copy_gbps = float(box['hbm_copy']['GBps'])
    cfg = synth.CONFIGS['arxiv']
    d = synth.node_dataset(cfg['n'], cfg['m'], cfg['F0'], cfg['classes'])
    N, src, dst = d['graphs'][0]
    store = gmeta_amd.GraphStore(d['graphs'], d['feats'])
    F = store.feat_dim
    ptr, idx = store.host_csr[0]
    length = np.diff(ptr) + 1                                                 # the extended rows: the self loop counts
    entries = int(length.sum())
    row_bytes = 4 * F
    lines = ['arxiv (m = %d): %d nodes, %d directed edges, F = %d (a level is %.1f MB), extended rows: %d entries, mean %.2f, longest %d, %d rows above %d; %s'
             % (cfg['m'], N, len(src), F, N * row_bytes / 1e6, entries, length.mean(), length.max(), int((length > LIB_CHUNK).sum()), LIB_CHUNK, torch.cuda.get_device_name(0)),
             'box: HBM copy rate %.0f GB/s (1 GiB device copy, bytes read + written per second); end to end: HIP events around the C call, median (min - max) of %d after %d warm-up(s);'
             % (copy_gbps, a.reps, a.warmup),
             'phases: one build under GM_TIMING, the stream synchronised behind the norms and behind every level (host clock); gathered bytes of a level = entries x row bytes',
             'build with self loops (allocation, level-0 copy and final synchronisation included):']
    gath = entries * row_bytes
    for hops in HOPS:
        med, lo, hi = timed(lambda: lib.gm_prop_destroy(build(store, hops)), a.reps, a.warmup)
        nm, lv = phase_ms(store, hops)
        rates = [gath / (t * 1e-3) / 1e9 for t in lv]
        rec = {'what': 'build', 'hops': hops, 'F': F, 'MB': round((hops + 1) * N * row_bytes / 1e6, 1), 'ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3),
               'norm_ms': round(nm, 3), 'level_ms': [round(t, 3) for t in lv], 'gathered_MB_per_level': round(gath / 1e6, 1), 'level_GBps': [round(r, 1) for r in rates],
               'hbm_copy_GBps': round(copy_gbps, 1)}
        print(json.dumps(rec), flush=True)
        lines.append('  hops %d  %7.1f MB  %9.3f ms (%.3f - %.3f)   norms + coefficients %7.3f ms, levels %s ms   gathered %7.1f MB per level: %s GB/s = %s of the copy rate'
                     % (hops, rec['MB'], med, lo, hi, nm, ' / '.join('%.3f' % t for t in lv), gath / 1e6, ' / '.join('%.0f' % r for r in rates),
                        ' / '.join('%.3f' % (r / copy_gbps) for r in rates)))
    lines.append('prop_chunk at hops 2 (0: the library\'s choice, %d):' % LIB_CHUNK)
    for chunk in (0, 64, 2 ** 30):
        C_ = chunk if chunk else LIB_CHUNK
        hubs = length[length > C_]
        assert lib.gm_set_tuning(b'prop_chunk', chunk) == 0
        try:
            med, lo, hi = timed(lambda: lib.gm_prop_destroy(build(store, 2)), a.reps, a.warmup)
            nm, lv = phase_ms(store, 2)
        finally:
            lib.gm_set_tuning(b'prop_chunk', 0)
        rec = {'what': 'prop_chunk', 'chunk': chunk, 'hub_rows': int(len(hubs)), 'segments': int(((hubs + C_ - 1) // C_).sum()), 'ms': round(med, 3), 'min_ms': round(lo, 3),
               'max_ms': round(hi, 3), 'norm_ms': round(nm, 3), 'level_ms': [round(t, 3) for t in lv]}
        print(json.dumps(rec), flush=True)
        lines.append('  prop_chunk %10d  %5d hub rows in %6d segments  %9.3f ms (%.3f - %.3f)   norms %7.3f ms, levels %s ms'
                     % (chunk, rec['hub_rows'], rec['segments'], med, lo, hi, nm, ' / '.join('%.3f' % t for t in lv)))
    rng = np.random.default_rng(5)
    half = len(src) // 2
    n = 10000
    pos = np.stack([src[:half], dst[:half]], 1)[rng.choice(half, n // 2, replace=False)]
    pairs = np.concatenate([pos, store.negative_pairs(0, n - n // 2, seed=222)]).astype(np.int64)
    every = np.stack([src, dst], 1).astype(np.int64)
    lines.append('pair_features (bytes = two rows read and one written per pair and level):')
    for hops in HOPS:
        h = build(store, hops)
        try:
            for what, pp in (('10,000 pairs', pairs), ('all %d edges' % len(every), every)):
                d_p = torch.from_numpy(np.ascontiguousarray(pp, np.int32)).cuda()
                out = torch.empty((len(pp), hops + 1, F), dtype=torch.float32, device='cuda')
                for op, code in sorted(_lib.PROP_OPS.items(), key=lambda kv: kv[1]):
                    call = lambda: _lib.check(lib.gm_prop_pair_features(h, _lib.ptr(d_p), len(pp), code, _lib.ptr(out), _lib.stream_ptr()), 'gm_prop_pair_features')      # noqa: E731
                    med, lo, hi = timed(call, a.reps, a.warmup)
                    moved = 3.0 * (hops + 1) * row_bytes * len(pp)
                    rec = {'what': 'pair_features ' + what, 'op': op, 'hops': hops, 'out_MB': round(out.numel() * 4 / 1e6, 1), 'ms': round(med, 3), 'min_ms': round(lo, 3),
                           'max_ms': round(hi, 3), 'us_per_pair': round(med * 1e3 / len(pp), 4), 'GBps': round(moved / (med * 1e-3) / 1e9, 1)}
                    print(json.dumps(rec), flush=True)
                    lines.append('  hops %d  %-18s %-8s  out %7.1f MB  %9.3f ms (%.3f - %.3f)   %.4f us per pair   %7.1f GB/s = %.3f of the copy rate'
                                 % (hops, what, op, rec['out_MB'], med, lo, hi, rec['us_per_pair'], rec['GBps'], rec['GBps'] / copy_gbps))
                del out, d_p
        finally:
            lib.gm_prop_destroy(h)
    lines.append('comparators at hops 3 (the same operator, one value per CSR entry; the build above: norms, coefficients and levels):')
    hops = 3
    h = build(store, hops)
    try:
        mine = all_levels(h, N, hops, F)
    finally:
        lib.gm_prop_destroy(h)
    row, col, val = operator(ptr, idx, N)
    X = torch.from_numpy(np.ascontiguousarray(d['feats'][0], np.float32)).cuda()
    try:
        crow = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(row, minlength=N))]).astype(np.int64)).cuda()
        order = np.argsort(row, kind='stable')
        A = torch.sparse_csr_tensor(crow, torch.from_numpy(col[order]).cuda(), torch.from_numpy(val[order].astype(np.float32)).cuda(), size=(N, N))

        def levels_torch():
            x = [X]
            for _ in range(hops):
                x.append(torch.sparse.mm(A, x[-1]))
            return x
        med, lo, hi = timed(levels_torch, a.reps, a.warmup)
        diff = max(float((t - mine[k]).abs().max()) for k, t in enumerate(levels_torch()))
        print(json.dumps({'what': 'torch.sparse.mm', 'hops': hops, 'ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3), 'max_abs_diff': diff}), flush=True)
        lines.append('  torch.sparse.mm (CSR, same device; the operator given, %d products)  %9.3f ms (%.3f - %.3f)   largest |difference| from the build %.3g' % (hops, med, lo, hi, diff))
    except Exception as e:                                                     # the comparator does not run here: say so, measure the rest
        lines.append('  torch.sparse.mm: did not run on this device (%s: %s)' % (type(e).__name__, str(e).splitlines()[0][:120] if str(e) else ''))
    try:
        import scipy.sparse as sp
        A = sp.csr_matrix((val, (row, col)), shape=(N, N))
        Xh = d['feats'][0].astype(np.float64)
        t0 = time.perf_counter()
        x = [Xh]
        for _ in range(hops):
            x.append(A @ x[-1])
        host_ms = (time.perf_counter() - t0) * 1e3
        diff = max(float(np.abs(t - mine[k].cpu().numpy()).max()) for k, t in enumerate(x))
        print(json.dumps({'what': 'scipy.sparse', 'hops': hops, 'ms': round(host_ms, 1), 'max_abs_diff': diff}), flush=True)
        lines.append('  scipy.sparse csr @ dense, float64, host (the operator given, %d products, once)  %9.1f ms   largest |difference| from the build %.3g' % (hops, host_ms, diff))
    except ImportError:
        lines.append('  scipy.sparse: not installed')
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
