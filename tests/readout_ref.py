"""CPU restatement of the mean readout (include/gmeta_hip.h, gm_set_readout(GM_READOUT_MEAN)) on top of the oracle: the reference left the
line commented out (`#h = dgl.mean_nodes(g, 'h')`, learner.py:160), so the yardstick is this file (held to fp64 torch autograd by
tests/test_readout_restatement.py) plus the oracle's own GraphConv stack, losses and inner loop.

    p_s      = (sum over the rows r of subgraph s of H_L[r, :]) / n_s      fp32, rows in ascending order
    logits_s = p_s @ Wl.T + bl                                             Wl [n_out, H], for pairs too
    dH_L[r]  = (dlogits_s @ Wl) / n_s for every row r of s                 (then the oracle's relu' and layer loop)

oracle.task_inner_loop calls classifier_forward / classifier_backward by their module-level names, so `patched()` swaps them (and restores
them): the oracle's inner loop, meta-gradient included, then runs a pooled model without a line of oracle/ changing -- the mechanism of
tests/ragged_ref.py, and the two compose.  orc.parse_config tolerates the ('Readout', ['mean']) entry."""
import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import gmeta_oracle as orc      # noqa: E402

f32 = np.float32
_forward, _backward = orc.classifier_forward, orc.classifier_backward      # the oracle's own, whatever is patched in


def mean_config(config):
    """The fixture's config with the Readout entry, before a trailing LinkPred entry."""
    body = [(n, p) for n, p in config if n not in ('LinkPred', 'Readout')]
    return body + [('Readout', ['mean'])] + [(n, p) for n, p in config if n == 'LinkPred']


def mean_vars(vars_, config):
    """The fixture's weights for the pooled model: a pair model's Wl [C, 2H] cut to its first H columns."""
    gcn, lin, link = orc.parse_config(config)
    out = [v.copy() for v in vars_]
    out[2 * len(gcn)] = np.ascontiguousarray(out[2 * len(gcn)][:, :lin[0]])
    return out


def pool(h, sub_off, reverse=False, dtype=f32):
    """[S, H] means of the rows of every subgraph: one running sum per subgraph, rows added one at a time in ascending (reverse: descending)
    order in `dtype`, then divided by the row count."""
    sub_off = np.asarray(sub_off, np.int64)
    n = np.diff(sub_off)
    assert (n >= 1).all()
    acc = np.zeros((len(n), h.shape[1]), dtype)
    for k in range(int(n.max())):
        live = np.nonzero(n > k)[0]
        rows = sub_off[live + 1] - 1 - k if reverse else sub_off[live] + k
        acc[live] += h[rows].astype(dtype)
    return (acc / n[:, None].astype(dtype)).astype(f32)


def make(reverse=False, dtype=f32):
    def forward(batch, x0, vars_, config):
        gcn, lin, link = orc.parse_config(config)
        L = len(gcn)
        Wl, bl = vars_[2 * L], vars_[2 * L + 1]
        assert Wl.shape == (lin[1], lin[0]), 'the pooled head is [n_out, H], for pairs too'
        stack = list(vars_)
        stack[2 * L] = np.zeros((lin[1], lin[0] * (2 if link else 1)), f32)          # (the oracle's own head, evaluated and dropped)
        _, (cache, _, hshape) = _forward(batch, x0, stack, config)
        p = pool(cache[-1][2], batch.sub_off, reverse, dtype)
        logits = p @ Wl.T + bl
        return logits.astype(f32), (cache, p, hshape)

    def backward(batch, vars_, config, fcache, dlogits):
        """classifier_backward with the pooled head: the oracle's layer loop, line for line, below a dense dH_L."""
        gcn, lin, link = orc.parse_config(config)
        cache, p, hshape = fcache
        L = len(gcn)
        grads = [None] * len(vars_)
        Wl = vars_[2 * L]
        dlogits = np.asarray(dlogits, f32)
        grads[2 * L] = dlogits.T @ p
        grads[2 * L + 1] = dlogits.sum(0)
        n = np.diff(np.asarray(batch.sub_off, np.int64))
        dp = (dlogits @ Wl) / n[:, None].astype(f32)
        dh = np.repeat(dp, n, axis=0).astype(f32)
        norm = batch.norm[:, None]
        for l in range(L - 1, -1, -1):
            W = vars_[2 * l]
            xs, z, hn, mm_first = cache[l]
            dq = dh * (hn > 0)
            grads[2 * l + 1] = dq.sum(0)
            dpre = dq * norm
            if mm_first:
                dy = orc.agg_t(batch, dpre)
                grads[2 * l] = xs.T @ dy
                dxs = dy @ W.T if l > 0 else None
            else:
                grads[2 * l] = z.T @ dpre
                dxs = orc.agg_t(batch, dpre @ W.T) if l > 0 else None
            dh = dxs * norm if l > 0 else None
        return [g.astype(f32) for g in grads]

    return forward, backward


@contextlib.contextmanager
def patched(reverse=False, dtype=f32):
    """The oracle's classifier_forward / classifier_backward replaced by the pooled ones; restored on exit."""
    saved = (orc.classifier_forward, orc.classifier_backward)
    orc.classifier_forward, orc.classifier_backward = make(reverse, dtype)
    try:
        yield
    finally:
        orc.classifier_forward, orc.classifier_backward = saved


# ---------------------------------------------------------------------------------------------------- the golden fixtures under the pooled model
def fixture_batches(fx, t):
    graphs = fx.graphs()
    return [orc.extract_batch(graphs, fx.z[tag + '_seeds'][t], fx.args['h'], fx.args['sample_nodes'], 222, fx.link, replay_nodes=fx.replay_lists(tag, t))
            for tag in ('spt', 'qry')]


def run_tasks(fx, K, need_meta_grad, margins=None, theta=None, **how):
    """task_inner_loop of the pooled model on every task of the fixture: [(losses_q, accs_q, meta-grad list)].  margins: a list that receives, per
    query scoring (K + 1 per task, in step order), the gap between the two largest log-probabilities of every query row (tests/ragged_ref.py: on
    a balanced task its losses perform the oracle's own operations in the oracle's own order)."""
    import ragged_ref as rr
    theta = mean_vars(fx.vars0, fx.config) if theta is None else theta
    cfg = mean_config(fx.config)
    res = []
    for t in range(fx.T):
        sb, qb = fixture_batches(fx, t)
        ys, yq = fx.z['y_spt'][t], fx.z['y_qry'][t]
        with patched(**how), (rr.patched(ys, margins) if margins is not None else contextlib.nullcontext()):
            res.append(orc.task_inner_loop(sb, qb, sb.features(fx.feats), qb.features(fx.feats), ys, yq, theta, cfg, fx.args['k_spt'],
                                           fx.args['update_lr'], K, need_meta_grad))
    return res


def meta_step(fx, theta=None, **how):
    """Meta.forward of the pooled model without the Adam step: task-mean losses_q [K+1], accs [K+1], mean meta-gradient (flat)."""
    res = run_tasks(fx, fx.K, True, theta=theta, **how)
    T = len(res)
    lq = sum(r[0].astype(np.float64) for r in res) / T
    aq = sum(r[1].astype(np.float64) for r in res) / T
    gsum = [np.zeros_like(g) for g in res[0][2]]
    for r in res:
        gsum = [a + b for a, b in zip(gsum, r[2])]
    return lq, aq, np.concatenate([(g / f32(T)).astype(f32).reshape(-1) for g in gsum])
