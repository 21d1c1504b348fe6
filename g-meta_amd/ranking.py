"""Ranking metrics of link-prediction scores, formed on the device (gm_rank_counts / gm_rank_summary; the definition is in include/gmeta_hip.h,
tests/ranking_ref.py restates it): for every positive score the exact numbers of negatives above it and equal to it, and their reduction to

    hits@K = the share of positives with fewer than K negatives at or above them          (OGB's Hits@K: ogbl-collab, -ppa, -ddi)
    mrr    = the mean of 1 / (1 + gt + eq / 2)                                             (OGB's MRR: ogbl-citation2), a tie counting one half
    auc    = the probability that a positive outranks a negative, a tie counting one half   (link_auc's number, from the same counts)

against ONE shared set of negatives, or against a range of the negatives per positive.  Scores that already live on the device (PairPredictor.scores(...,
as_torch=True)) never leave it: a few integers and one double come back.  Scores are compared as float32 values."""
import ctypes as C

import numpy as np

from . import _lib

MAX_KS = _lib.RANK_MAX_K


def _scores(x, what, name):
    """-> a contiguous 1-D CUDA float32 tensor: a CUDA float32 tensor as it is, a numpy float32 / float64 array uploaded (float64 is cast to float32 ONCE, here)."""
    import torch
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError('%s: %s is a %s tensor on %s; a CUDA float32 tensor or a numpy array' % (what, name, x.dtype, x.device))
        return x.detach().reshape(-1).contiguous()
    a = np.asarray(x)
    if a.dtype not in (np.float32, np.float64):
        raise ValueError('%s: %s of dtype %s; float32 or float64' % (what, name, a.dtype))
    return torch.from_numpy(np.array(a.reshape(-1), np.float32)).cuda()      # (a copy: a read-only array is welcome)


def _ranges(r, n_pos, what):
    """-> None, or a contiguous CUDA int64 tensor [n_pos, 2]."""
    import torch
    if r is None:
        return None
    if isinstance(r, torch.Tensor):
        if r.dtype != torch.int64 or not r.is_cuda:
            raise ValueError('%s: ranges is a %s tensor on %s; a CUDA int64 tensor or a numpy array' % (what, r.dtype, r.device))
        d = r.contiguous()
    else:
        a = np.asarray(r)
        if a.dtype.kind not in 'iu':
            raise ValueError('%s: ranges of dtype %s; integers' % (what, a.dtype))
        d = torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()
    if tuple(d.shape) != (n_pos, 2):
        raise ValueError('%s: ranges of shape %s; [%d, 2]' % (what, tuple(d.shape), n_pos))
    return d


def rank_counts(pos, neg, ranges=None, as_torch=False):
    """int64 [P, 2]: per positive score (gt, eq) -- the negatives strictly greater than it and those equal to it (gm_rank_counts).  `pos` [P], `neg` [N]: numpy
    (float64 is cast to float32 once) or CUDA float32 tensors.  `ranges`: None = every positive against all of `neg`; else int [P, 2], positive i against
    neg[b_i : e_i] -- ranges may be empty, overlap and repeat.  A positive's counts do not depend on the other positives or on the order of the negatives.
    as_torch=True leaves the result on the device.  ValueError on a NaN in either array and on a range outside [0, N]."""
    import torch
    _lib.require_gpu()
    p, n = _scores(pos, 'rank_counts', 'pos'), _scores(neg, 'rank_counts', 'neg')
    r = _ranges(ranges, len(p), 'rank_counts')
    out = torch.empty((len(p), 2), dtype=torch.int64, device='cuda')
    _lib.check(_lib.lib().gm_rank_counts(_lib.ptr(p), len(p), _lib.ptr(n), len(n), _lib.ptr(r), _lib.ptr(out), _lib.stream_ptr()), 'gm_rank_counts')
    return out if as_torch else out.cpu().numpy()


def _check_ks(ks, what):
    ks = [int(k) for k in ks]
    if len(ks) > MAX_KS:
        raise ValueError('%s: %d values of K; at most %d' % (what, len(ks), MAX_KS))
    if any(k < 1 for k in ks):
        raise ValueError('%s: K = %d; a K is at least 1' % (what, min(ks)))
    return ks


def rank_metrics(pos, neg, ks=(20, 50, 100), ranges=None):
    """{'hits@K' for every K of `ks`, 'mrr', 'auc', 'n_pos', 'n_pairs'} of the positive scores against the negative ones (gm_rank_summary): the counts of
    rank_counts reduced on the device; only the summary comes back.  Arguments as in rank_counts.  ValueError unless there is a positive and a (positive,
    negative) pair to compare, on more than 8 values of K, on a K below 1 and on a NaN."""
    _lib.require_gpu()
    ks = _check_ks(ks, 'rank_metrics')
    p, n = _scores(pos, 'rank_metrics', 'pos'), _scores(neg, 'rank_metrics', 'neg')
    r = _ranges(ranges, len(p), 'rank_metrics')
    if len(p) == 0 or (r is None and len(n) == 0):
        raise ValueError('rank_metrics needs positives and negatives: %d positive(s), %d negative(s)' % (len(p), len(n)))
    h_ks = (C.c_int64 * max(len(ks), 1))(*ks)
    s = _lib.RankSummary()
    _lib.check(_lib.lib().gm_rank_summary(_lib.ptr(p), len(p), _lib.ptr(n), len(n), _lib.ptr(r), h_ks, len(ks), None, C.byref(s), _lib.stream_ptr()), 'gm_rank_summary')
    if s.n_pairs == 0:
        raise ValueError('rank_metrics needs positives and negatives: every one of the %d range(s) is empty' % len(p))
    out = {'hits@%d' % k: s.hits[j] / float(s.n_pos) for j, k in enumerate(ks)}
    out.update({'mrr': s.rr_sum / float(s.n_pos), 'auc': (s.auc2 / 2.0) / float(s.n_pairs), 'n_pos': int(s.n_pos), 'n_pairs': int(s.n_pairs)})
    return out


def link_ranking(scores, labels, ks=(20, 50, 100), groups=None):
    """rank_metrics of one score per named pair against the 0 / 1 `labels` (numbers or the tables' strings): the twin of link_auc.  The rows are split by
    label.  groups=None: every positive against all negatives (the Hits@K protocol; 'auc' is link_auc's number).  `groups`: one integer per row, such as the
    pair's source node -- every positive is ranked against the negatives of ITS group (the MRR protocol): the negatives are grouped by a stable sort of their
    group ids and every positive gets its group's range, empty where the group has no negative.  `scores`: numpy, or a CUDA float32 tensor that then never
    leaves the device.  ValueError unless both labels occur, on any other label, and on a NaN."""
    import torch
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    n = int(scores.numel()) if isinstance(scores, torch.Tensor) else int(np.asarray(scores).size)
    if n != len(y):
        raise ValueError('link_ranking: %d scores, %d labels' % (n, len(y)))
    if not np.isin(y, (0, 1)).all():
        raise ValueError('link_ranking: labels must be 0 or 1')
    at_pos, at_neg = np.nonzero(y == 1)[0], np.nonzero(y == 0)[0]
    if len(at_pos) == 0 or len(at_neg) == 0:
        raise ValueError('link_ranking needs both labels: %d positive(s), %d negative(s)' % (len(at_pos), len(at_neg)))
    ks = _check_ks(ks, 'link_ranking')
    ranges = None
    if groups is not None:
        g = np.asarray(groups).reshape(-1)
        if len(g) != len(y) or g.dtype.kind not in 'iu':
            raise ValueError('link_ranking: groups of %d %s value(s); one integer per row (%d)' % (len(g), g.dtype, len(y)))
        g = g.astype(np.int64)
        order = np.argsort(g[at_neg], kind='stable')
        at_neg = at_neg[order]
        g_neg = g[at_neg]
        ranges = np.stack([np.searchsorted(g_neg, g[at_pos], 'left'), np.searchsorted(g_neg, g[at_pos], 'right')], axis=1).astype(np.int64)
    s = _scores(scores, 'link_ranking', 'scores')
    take = lambda at: s[torch.from_numpy(at).cuda()]      # noqa: E731
    return rank_metrics(take(at_pos), take(at_neg), ks, ranges)
