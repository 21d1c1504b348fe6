"""Time of the ranking metrics on the device (gmeta_amd.rank_metrics -> gm_rank_summary), reported with no target, against two routes timed in the same process
that must give the same integers: torch.sort + torch.searchsorted on the device, and what a user does today -- the scores read back to the host and ranked in
numpy (link_auc for the shared mode's AUC; a sort and two searches, or a [P, n] comparison, for the counts).

    python tools/ranking_bench.py [--reps 10] [--warmup 2] [--base_reps 2] [--shared 100000,1000000,10000000] [--positives 100000] [--per 1000] [--out profiles/ranking.txt]

Cases: shared mode, --positives scores against N = each of --shared; ranged mode, --positives scores with --per negatives each.  Score kinds: `continuous`
(standard normals) and `ties` (small integers 0 .. 20, as common neighbours gives).  Per case, medians (min - max) of --reps after --warmup: the end-to-end wall time of
gm_rank_summary with the counts kept (perf_counter around the C call, which returns after its one read-back), under the library's own choice of path and, in
the shared mode, with each path forced (gm_set_tuning("rank_sort_min", 1 | INT32_MAX)); and the time per phase from the library's phase timer (GM_TIMING through
gm_set_tuning in separate calls: the stream is then synchronised behind every phase).  The bytes the chosen path must move at least are held against the
device-to-device copy rate measured in the same process.  One JSON line per measurement; --out appends a plain-text table."""
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
from gmeta_amd import _lib               # noqa: E402

KS = (20, 50, 100)
INT32_MAX = 2 ** 31 - 1
PHASES = ('keys', 'sort', 'search', 'sweep', 'summary')


class Call:
    """gm_rank_summary on device-resident scores, the counts kept"""

    def __init__(self, pos, neg, ranges=None):
        self.pos, self.neg, self.ranges = pos, neg, ranges
        self.counts = torch.empty((len(pos), 2), dtype=torch.int64, device='cuda')
        self.ks = (C.c_int64 * len(KS))(*KS)
        self.s = _lib.RankSummary()

    def __call__(self):
        _lib.check(_lib.lib().gm_rank_summary(_lib.ptr(self.pos), len(self.pos), _lib.ptr(self.neg), len(self.neg), _lib.ptr(self.ranges), self.ks, len(KS),
                                              _lib.ptr(self.counts), C.byref(self.s), _lib.stream_ptr()), 'gm_rank_summary')

    def summary(self):
        s = self.s
        return {'n_pairs': int(s.n_pairs), 'auc2': int(s.auc2), 'hits': [int(s.hits[j]) for j in range(len(KS))], 'rr_sum': float(s.rr_sum)}


def wall_ms(fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def phase_ms(call, reps):
    lib = _lib.lib()
    out = {p: [] for p in PHASES}
    for _ in range(reps):
        torch.cuda.synchronize()
        sys.stderr.flush()
        with tempfile.TemporaryFile(mode='w+') as tmp:
            keep = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                assert lib.gm_set_tuning(b'GM_TIMING', 1) == 0
                call()
            finally:
                lib.gm_set_tuning(b'GM_TIMING', 0)
                os.dup2(keep, 2); os.close(keep)
            tmp.seek(0)
            text = tmp.read()
        laps = re.findall(r'\[gm timing\] rank/(\w+) ([0-9.]+) us', text)
        assert laps, text
        for p in PHASES:
            out[p].append(sum(float(us) for name, us in laps if name == p) / 1e3)
    return {p: med(v) for p, v in out.items() if max(v) > 0.0}


def med(x):
    return float(np.median(x)), float(min(x)), float(max(x))


def fmt(m):
    return '%9.3f (%.3f - %.3f)' % m


def copy_rate():
    """Device-to-device copy rate, bytes read + written per second: the box's own HBM rate for a plain stream."""
    a = torch.empty(1 << 28, dtype=torch.float32, device='cuda'); b = torch.empty_like(a)      # 1 GiB each: beyond the Infinity Cache
    a.zero_()
    ms = wall_ms(lambda: b.copy_(a), 10, 3)
    return 2 * a.numel() * 4 / (np.median(ms) * 1e-3)


def reduce_torch(gt, eq, n_i):
    """the summary of device counts in torch; what comes back is a few numbers"""
    hits = [int((gt + eq < k).sum()) for k in KS]
    rr = float((1.0 / (1.0 + gt.double() + eq.double() / 2.0)).sum())
    return {'n_pairs': int(n_i.sum()) if torch.is_tensor(n_i) else int(n_i) * len(gt), 'auc2': int((2 * (n_i - gt - eq) + eq).sum()), 'hits': hits, 'rr_sum': rr}


def torch_shared(pos, neg):
    s, _ = torch.sort(neg)
    lb, ub = torch.searchsorted(s, pos, right=False), torch.searchsorted(s, pos, right=True)
    gt, eq = len(neg) - ub, ub - lb
    return torch.stack([gt, eq], 1), reduce_torch(gt, eq, len(neg))


def torch_ranged(pos, neg, per):
    s, _ = torch.sort(neg.view(len(pos), per), dim=1)
    p = pos.view(-1, 1).contiguous()
    lb, ub = torch.searchsorted(s, p, right=False).view(-1), torch.searchsorted(s, p, right=True).view(-1)
    gt, eq = per - ub, ub - lb
    return torch.stack([gt, eq], 1), reduce_torch(gt, eq, per)


def reduce_numpy(gt, eq, n_i):
    return {'n_pairs': int(n_i) * len(gt), 'auc2': int((2 * (n_i - gt - eq) + eq).sum()), 'hits': [int((gt + eq < k).sum()) for k in KS],
            'rr_sum': float((1.0 / (1.0 + gt + eq / 2.0)).sum())}


def numpy_shared(pos, neg):
    """the read-back and the numpy route: link_auc as it stands for the AUC (what a user computes today), then the counts by a sort and two searches"""
    t0 = time.perf_counter()
    p, n = pos.cpu().numpy(), neg.cpu().numpy()
    t1 = time.perf_counter()
    auc = gmeta_amd.link_auc(np.concatenate([p, n]), np.concatenate([np.ones(len(p), np.int64), np.zeros(len(n), np.int64)]))
    t2 = time.perf_counter()
    s = np.sort(n)
    lb, ub = np.searchsorted(s, p, 'left'), np.searchsorted(s, p, 'right')
    gt, eq = len(n) - ub, ub - lb
    red = reduce_numpy(gt, eq, len(n))
    t3 = time.perf_counter()
    return np.stack([gt, eq], 1), red, auc, ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)


def numpy_ranged(pos, neg, per):
    """the read-back and the numpy route: a [rows, per] comparison per block of positives"""
    t0 = time.perf_counter()
    p, n = pos.cpu().numpy(), neg.cpu().numpy().reshape(len(pos), per)
    t1 = time.perf_counter()
    gt, eq = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
    for i in range(0, len(p), 4096):
        gt[i:i + 4096] = (n[i:i + 4096] > p[i:i + 4096, None]).sum(1); eq[i:i + 4096] = (n[i:i + 4096] == p[i:i + 4096, None]).sum(1)
    red = reduce_numpy(gt, eq, per)
    t2 = time.perf_counter()
    return np.stack([gt, eq], 1), red, None, ((t1 - t0) * 1e3, 0.0, (t2 - t1) * 1e3)


def same_summary(a, b):
    return all(a[k] == b[k] for k in ('n_pairs', 'auc2', 'hits')) and abs(a['rr_sum'] - b['rr_sum']) <= 1e-9 * abs(b['rr_sum'])


def scores(kind, n, gen):
    if kind == 'ties':
        return torch.randint(0, 21, (n,), generator=gen, device='cuda').to(torch.float32)
    return torch.randn(n, generator=gen, device='cuda', dtype=torch.float32)


def path_grid(gen, reps, lines):
    """The two shared-mode paths forced over a grid of (P, N) around their crossover, and the path the library takes by itself: what its choice is read from."""
    lib = _lib.lib()
    lines.append('shared mode, both paths forced (continuous scores), wall ms median of %d; rows = P rounded up to 256; * = the library\'s own choice' % reps)
    for P in (1, 256, 4096, 65536):
        for N in (4096, 65536, 1048576):
            call = Call(scores('continuous', P, gen), scores('continuous', N, gen))
            t = {}
            for path, v in (('sorted', 1), ('brute', INT32_MAX)):
                assert lib.gm_set_tuning(b'rank_sort_min', v) == 0
                try:
                    call()
                    t[path] = med(wall_ms(call, reps, 2))[0]
                finally:
                    lib.gm_set_tuning(b'rank_sort_min', 0)
            own = 'sorted' if 'sort' in phase_ms(call, 1) else 'brute'
            rows = (P + 255) // 256 * 256
            print(json.dumps({'grid': True, 'P': P, 'N': N, 'rows_x_N': rows * N, 'sorted_ms': round(t['sorted'], 3), 'brute_ms': round(t['brute'], 3), 'library': own}), flush=True)
            lines.append('  P %6d  N %8d  rows x N 2^%4.1f   sorted %7.3f%s   brute %7.3f%s' % (P, N, np.log2(rows * N), t['sorted'], '*' if own == 'sorted' else ' ', t['brute'],
                                                                                               '*' if own == 'brute' else ' '))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--base_reps', type=int, default=2)
    ap.add_argument('--shared', default='100000,1000000,10000000')
    ap.add_argument('--positives', type=int, default=100000)
    ap.add_argument('--per', type=int, default=1000)
    ap.add_argument('--brute_max', type=float, default=2e12, help='largest P * N at which the forced brute-force path is timed')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(222)
    rate = copy_rate()
    P = a.positives
    lines = ['ranking metrics, %d positives, K = %s; %s' % (P, ', '.join(map(str, KS)), torch.cuda.get_device_name(0)),
             'ms, median (min - max) of %d after %d warm-ups (numpy route: %d after 1); wall = perf_counter around the call and a device synchronise; phases = the '
             'library\'s phase timer in separate calls (stream synchronised behind every phase)' % (a.reps, a.warmup, a.base_reps),
             'device-to-device copy of 1 GiB in this process: %.2f TB/s read + written' % (rate / 1e12)]
    ok = True
    cases = [('shared', int(n)) for n in a.shared.split(',') if n] + [('ranged', a.per)]
    for mode, n in cases:
        for kind in ('continuous', 'ties'):
            pos = scores(kind, P, gen)
            N = n if mode == 'shared' else P * n
            neg = scores(kind, N, gen)
            ranges = None if mode == 'shared' else (torch.arange(P, device='cuda', dtype=torch.int64).view(-1, 1) * n + torch.tensor([[0, n]], device='cuda', dtype=torch.int64)).contiguous()
            call = Call(pos, neg, ranges)
            call()
            w = med(wall_ms(call, a.reps, a.warmup))
            ph = phase_ms(call, min(a.reps, 5))
            got_counts, got = call.counts.cpu().numpy(), call.summary()
            forced = {}
            if mode == 'shared':
                for path, v in (('sorted', 1), ('brute', INT32_MAX)):
                    if path == 'brute' and float(P) * N > a.brute_max:
                        continue
                    assert lib.gm_set_tuning(b'rank_sort_min', v) == 0
                    try:
                        call()
                        forced[path] = med(wall_ms(call, max(3, a.reps // 2), 1))
                        ok = ok and bool(np.array_equal(call.counts.cpu().numpy(), got_counts)) and call.summary() == got
                    finally:
                        lib.gm_set_tuning(b'rank_sort_min', 0)
                sorts = 'sorted' if 'sort' in ph else 'brute'                              # the library's own choice, read off its phases
                swept = 8 * (P + N) + (48 * N if sorts == 'sorted' else 4 * N * ((P + 255) // 256)) + 32 * P
            else:
                sorts = 'wave sweep'
                swept = 8 * (P + N) + 4 * N + 16 * P + 32 * P
            troute = (lambda: torch_shared(pos, neg)) if mode == 'shared' else (lambda: torch_ranged(pos, neg, n))
            t_counts, t_red = troute()
            tw = med(wall_ms(troute, a.reps, a.warmup))
            same_t = bool(np.array_equal(t_counts.cpu().numpy(), got_counts)) and same_summary(t_red, got)
            del t_counts
            nb = []
            for r in range(1 + a.base_reps):
                torch.cuda.synchronize()
                n_counts, n_red, auc, parts = numpy_shared(pos, neg) if mode == 'shared' else numpy_ranged(pos, neg, n)
                if r:
                    nb.append(parts)
            same_n = bool(np.array_equal(n_counts, got_counts)) and same_summary(n_red, got)
            our_auc = (got['auc2'] / 2.0) / float(got['n_pairs'])
            same_auc = auc is None or auc == our_auc
            ok = ok and same_t and same_n and same_auc
            back, auc_ms, cnt_ms = (med([x[i] for x in nb]) for i in range(3))
            today = back[0] + (auc_ms[0] if mode == 'shared' else cnt_ms[0])             # what a user does today: read back + link_auc (shared) / the comparison (ranged)
            r = {'mode': mode, 'kind': kind, 'P': P, 'N': N, 'per_positive': n if mode == 'ranged' else N, 'path': sorts, 'wall_ms': round(w[0], 3), 'wall_min_ms': round(w[1], 3),
                 'wall_max_ms': round(w[2], 3), 'swept_mb_at_least': round(swept / 1e6, 1), 'swept_at_copy_rate_ms': round(swept / rate * 1e3, 3),
                 'fraction_of_copy_rate': round(swept / rate * 1e3 / w[0], 3), 'torch_ms': round(tw[0], 3), 'torch_over_call': round(tw[0] / w[0], 2),
                 'readback_ms': round(back[0], 3), 'numpy_link_auc_ms': round(auc_ms[0], 3), 'numpy_counts_ms': round(cnt_ms[0], 3), 'today_over_call': round(today / w[0], 2),
                 'equal_to_torch': same_t, 'equal_to_numpy': same_n, 'auc_equals_link_auc': bool(same_auc), 'hits': got['hits'], 'mrr': got['rr_sum'] / P, 'auc': our_auc}
            r.update({'forced_%s_ms' % k: round(v[0], 3) for k, v in forced.items()})
            r.update({p + '_ms': round(v[0], 3) for p, v in ph.items()})
            print(json.dumps(r), flush=True)
            lines.append('%s, %s: P = %d, N = %d%s; path %s; Hits@%s = %s, MRR %.4f, AUC %.4f' % (mode, kind, P, N, '' if mode == 'shared' else ' (%d per positive)' % n, sorts,
                                                                                               '/'.join(map(str, KS)), '/'.join('%.4f' % (h / P) for h in got['hits']), got['rr_sum'] / P, our_auc))
            lines.append('  call      wall ' + fmt(w) + '   ' + '   '.join('%s %s' % (p, fmt(v)) for p, v in ph.items()))
            if forced:
                lines.append('            forced ' + '   '.join('%s %s' % (k, fmt(v)) for k, v in forced.items()))
            lines.append('            at least %.1f MB moved: %.3f ms at the copy rate = %.3f of the call' % (swept / 1e6, swept / rate * 1e3, swept / rate * 1e3 / w[0]))
            lines.append('  torch     sort + searchsorted + reductions on the device ' + fmt(tw) + ' = %.2f x the call; equal integers: %s' % (tw[0] / w[0], same_t))
            lines.append('  today     read-back ' + fmt(back) + ('   link_auc ' + fmt(auc_ms) if mode == 'shared' else '') + '   numpy counts ' + fmt(cnt_ms)
                         + '   read-back + %s = %.3f = %.2f x the call; equal integers: %s%s' % ('link_auc' if mode == 'shared' else 'counts', today, today / w[0], same_n,
                                                                                                 '' if auc is None else '; AUC equal bit for bit: %s' % same_auc))
            del pos, neg, ranges, call
            torch.cuda.empty_cache()
    path_grid(gen, a.reps, lines)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    assert ok, 'a route disagrees with the device call'


if __name__ == '__main__':
    main()
