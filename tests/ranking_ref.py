"""The definition of gm_rank_counts / gm_rank_summary (include/gmeta_hip.h), restated in numpy: counts by direct comparison of float32 VALUES, chunked over the
positives; rr_sum by math.fsum; the integers as Python ints.  No sort, no key: the device's route is checked against this one, and the key map is restated
separately (key) so that its order can be checked against numpy's own."""
import math

import numpy as np

f32 = np.float32
MAX_K = 8
FLT_MAX = np.finfo(f32).max
DENORM = np.float32(np.finfo(f32).smallest_subnormal)
SPECIAL = np.array([np.inf, -np.inf, 0.0, -0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX, 1.0, -1.0, 1.5, np.nextafter(f32(1.0), f32(2.0)), 3.0e-39, -3.0e-39, 2.0 ** -126,
                    -2.0 ** -126], f32)      # the pool of special values: +-inf, +-0, +- the smallest denormal, +-FLT_MAX, denormals, the smallest normal, ordinary values


def key(x):
    """uint32: the order-preserving key of the definition: -0.0 -> +0.0, then u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000)."""
    u = np.ascontiguousarray(x, f32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def counts(pos, neg, ranges=None, chunk=256):
    """int64 [P, 2]: (gt, eq) per positive against all of neg (ranges None) or neg[b_i : e_i]."""
    pos, neg = np.asarray(pos, f32).reshape(-1), np.asarray(neg, f32).reshape(-1)
    assert not np.isnan(pos).any() and not np.isnan(neg).any()
    out = np.zeros((len(pos), 2), np.int64)
    with np.errstate(invalid='ignore'):
        if ranges is None:
            for i0 in range(0, len(pos), chunk):
                p = pos[i0:i0 + chunk, None]
                out[i0:i0 + chunk, 0] = (neg[None, :] > p).sum(1)
                out[i0:i0 + chunk, 1] = (neg[None, :] == p).sum(1)
        else:
            r = np.asarray(ranges, np.int64).reshape(-1, 2)
            assert len(r) == len(pos) and (r[:, 0] >= 0).all() and (r[:, 0] <= r[:, 1]).all() and (r[:, 1] <= len(neg)).all()
            for i, (b, e) in enumerate(r.tolist()):
                out[i] = ((neg[b:e] > pos[i]).sum(), (neg[b:e] == pos[i]).sum())
    return out


def summary(cnt, n_neg, ks, ranges=None):
    """{'n_pos', 'n_pairs', 'auc2', 'rr_sum', 'hits': [..]} of the [P, 2] counts, by the definition: integers exact, rr_sum the correctly rounded sum (fsum)."""
    cnt = np.asarray(cnt, np.int64).reshape(-1, 2)
    ks = [int(k) for k in ks]
    assert len(ks) <= MAX_K and all(k >= 1 for k in ks)
    P = len(cnt)
    Ni = np.full(P, int(n_neg), np.int64) if ranges is None else np.diff(np.asarray(ranges, np.int64).reshape(-1, 2), axis=1).reshape(-1)
    gt, eq = cnt[:, 0], cnt[:, 1]
    return {'n_pos': P, 'n_pairs': int(Ni.sum()), 'auc2': int((2 * (Ni - gt - eq) + eq).sum()),
            'rr_sum': math.fsum((1.0 / (1.0 + g + e / 2.0)) for g, e in zip(gt.tolist(), eq.tolist())),
            'hits': [int((gt + eq < k).sum()) for k in ks]}


def metrics(pos, neg, ks=(20, 50, 100), ranges=None):
    """The dictionary gmeta_amd.rank_metrics returns, by the definition."""
    s = summary(counts(pos, neg, ranges), len(np.asarray(neg).reshape(-1)), ks, ranges)
    out = {'hits@%d' % k: s['hits'][j] / float(s['n_pos']) for j, k in enumerate(ks)}
    out.update({'mrr': s['rr_sum'] / float(s['n_pos']), 'auc': (s['auc2'] / 2.0) / float(s['n_pairs']), 'n_pos': s['n_pos'], 'n_pairs': s['n_pairs']})
    return out


def group_ranges(groups, labels):
    """link_ranking's grouping: -> (rows of the positives, rows of the negatives in their stable group order, int64 [P, 2] ranges into the latter)."""
    g, y = np.asarray(groups, np.int64).reshape(-1), np.asarray(labels).reshape(-1).astype(np.int64)
    at_pos, at_neg = np.nonzero(y == 1)[0], np.nonzero(y == 0)[0]
    at_neg = at_neg[np.argsort(g[at_neg], kind='stable')]
    r = np.array([[int((g[at_neg] < v).sum()), int((g[at_neg] <= v).sum())] for v in g[at_pos].tolist()], np.int64).reshape(-1, 2)
    return at_pos, at_neg, r


def scores(kind, n, seed):
    """float32 [n] of one of the score kinds of the tests."""
    rng = np.random.default_rng(seed)
    if kind == 'ties':
        return rng.integers(-3, 4, n).astype(f32)                 # small integers, as common neighbours gives: heavy ties
    if kind == 'special':
        return SPECIAL[rng.integers(0, len(SPECIAL), n)]
    if kind == 'normal':
        return rng.standard_normal(n).astype(f32)
    if kind == 'equal':
        return np.full(n, 0.25, f32)
    raise ValueError(kind)
