"""CPU restatement of the hop-distance node labels (include/gmeta_hip.h, gm_set_hop_labels) on top of the oracle: the reference has no
labelling step, so the yardstick is this file (validated by tests/test_hop_label_restatement.py) plus the oracle's own forward / backward /
inner loop, which take the feature rows explicitly.

    labels(batch, D)            int8 [rows, centres]: per subgraph and centre c, BFS from c along the in-edges of the batch's induced CSR;
                                label = the least number of edges of a directed path v -> ... -> c inside the subgraph where that is <= D,
                                else D + 1 (farther, or unreachable)
    features(batch, feats, D)   [rows, F0 + centres * (D + 2)]: hstack([batch.features(feats), one-hot blocks])
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import gmeta_oracle as orc      # noqa: E402

f32 = np.float32


def width(D, link_pred):
    return (D + 2) * (2 if link_pred else 1) if D else 0


def labels(batch, D):
    """batch: an oracle Batch (or anything with sub_off, indptr, indices, centre_rows in batch-global row numbers)."""
    assert 1 <= D <= 7
    nc = batch.centre_rows.shape[1]
    out = np.full((batch.n, nc), D + 1, np.int8)
    for s in range(batch.S):
        r0, r1 = int(batch.sub_off[s]), int(batch.sub_off[s + 1])
        for c in range(nc):
            root = int(batch.centre_rows[s, c])
            assert r0 <= root < r1
            out[root, c] = 0
            frontier = [root]
            for level in range(1, D + 1):
                nxt = []
                for v in frontier:
                    for u in batch.indices[batch.indptr[v]:batch.indptr[v + 1]]:      # sources of the edges u -> v
                        u = int(u)
                        assert r0 <= u < r1
                        if out[u, c] == D + 1:
                            out[u, c] = level
                            nxt.append(u)
                frontier = nxt
    return out


def onehots(lab, D):
    n, nc = lab.shape
    Lw = D + 2
    oh = np.zeros((n, nc * Lw), f32)
    for c in range(nc):
        oh[np.arange(n), c * Lw + lab[:, c].astype(np.int64)] = 1.0
    return oh


def features(batch, feats, D):
    return np.hstack([batch.features(feats), onehots(labels(batch, D), D)]).astype(f32)


def meta_step(feats, spt, qry, y_spt, y_qry, theta, config, k_spt, update_lr, K, D, need_meta_grad=True):
    """orc.meta_step without the Adam step, on the labelled rows: (mean accs [K+1], mean meta-gradient list or None, mean losses_q [K+1])."""
    T = len(spt)
    lq_sum, aq_sum = np.zeros(K + 1, np.float64), np.zeros(K + 1, np.float64)
    gsum = [np.zeros_like(v) for v in theta]
    for t in range(T):
        lq, aq, mg = orc.task_inner_loop(spt[t], qry[t], features(spt[t], feats, D), features(qry[t], feats, D), y_spt[t], y_qry[t], theta, config,
                                         k_spt, update_lr, K, need_meta_grad)
        lq_sum += lq; aq_sum += aq
        if need_meta_grad:
            gsum = [a + b for a, b in zip(gsum, mg)]
    grad = [(g / f32(T)).astype(f32) for g in gsum] if need_meta_grad else None
    return aq_sum / T, grad, lq_sum / T
