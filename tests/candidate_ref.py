"""Restatement of the candidate-partner definition of include/gmeta_hip.h (gm_store_pair_candidates), literally: Python sets for the candidate sets, built on
pair_score_ref.neighbourhoods, and the ranking as the descending order of the integer key the definition names.  The scores are NOT restated here: the
definition makes them the bits of gm_store_pair_scores, so `rank` takes them as given fp32 values (the GPU tests feed it the device's own pair scores
under the same lanes-per-pair configuration).  Pure numpy."""
import numpy as np

import pair_score_ref

MAX_K = 1024


def candidates(N, src, dst, a, nb=None):
    """C(a) = { w : w != a, w not in Gamma(a), Gamma(a) & Gamma(w) not empty } as an ascending list; empty for a source outside [0, N)."""
    nb = pair_score_ref.neighbourhoods(N, src, dst) if nb is None else nb
    a = int(a)
    if not 0 <= a < N:
        return []
    reach = set()
    for z in nb[a]:
        reach |= nb[z]                                                          # w shares the neighbour z with a
    return sorted(reach - nb[a] - {a})


def keys(cands, scores):
    """(uint64(score bits) << 32) | (0xFFFFFFFF - w), as uint64."""
    bits = np.ascontiguousarray(scores, np.float32).view(np.uint32).astype(np.uint64)
    w = np.asarray(cands, np.int64)
    assert len(bits) == len(w) and (w >= 0).all() and (w <= 0xFFFFFFFF).all()
    return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - w.astype(np.uint64))


def rank(cands, scores, k):
    """The first min(k, len) candidates in descending key order, padded to k: (nodes int64 [k], -1 behind the last; scores float32 [k], 0.0 behind it)."""
    assert 1 <= k <= MAX_K
    key = keys(cands, scores)
    assert len(np.unique(key)) == len(key)                                      # distinct w: the keys are unique, the ranking has no ties
    order = np.argsort(key, kind='stable')[::-1][:k]
    nodes = np.full(k, -1, np.int64); sc = np.zeros(k, np.float32)
    nodes[:len(order)] = np.asarray(cands, np.int64)[order]
    sc[:len(order)] = np.ascontiguousarray(scores, np.float32)[order]
    return nodes, sc


def pairs_of(sources, sets):
    """[(a, w)] over the sources' candidate sets, concatenated: int64 [sum |C|, 2]."""
    rows = [np.stack([np.full(len(c), a, np.int64), np.asarray(c, np.int64)], 1) for a, c in zip(sources, sets) if len(c)]
    return np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)


def top_k(sources, sets, scores, k):
    """sources [m], sets = their candidate lists, scores = one fp32 per pair of pairs_of(sources, sets), in its order
    -> (nodes int64 [m, k], scores float32 [m, k], totals int64 [m])."""
    m = len(sources)
    nodes = np.full((m, k), -1, np.int64); sc = np.zeros((m, k), np.float32); tot = np.zeros(m, np.int64)
    at = 0
    for r, c in enumerate(sets):
        tot[r] = len(c)
        if len(c):
            nodes[r], sc[r] = rank(c, scores[at:at + len(c)], k)
        at += len(c)
    assert at == len(scores)
    return nodes, sc, tot


def word_boundary_case():
    """70 nodes (no multiple of 32).  Node 10 joins the ids around every word boundary -- 0, 31, 32, 63, 64, 69 = N - 1 -- and node 5, so each of them is
    a candidate of the others; 5 is also adjacent to 31 and 64 (blocked there), 0 to 63, and 69 to 32; a second hub 40 shares 0, 32 and 69."""
    N = 70
    e = [(10, w) for w in (0, 31, 32, 63, 64, 69, 5)] + [(5, 31), (64, 5), (0, 63), (69, 32), (40, 0), (32, 40), (40, 69), (40, 41), (41, 42)]
    e = np.asarray(e, np.int64)
    return N, e[:, 0].copy(), e[:, 1].copy()
