"""CPU restatement of ragged-task mode (include/gmeta_hip.h, gm_set_ragged_classes): numpy versions of the oracle's proto_loss_spt,
proto_loss_qry and protos_to_dlogits for classes with unequal row counts, and the fixed rule the tests use to cut ragged tasks out of the
balanced golden fixtures.

oracle.task_inner_loop calls those three functions by their module-level names, so `patched(y_spt)` swaps them in (and restores them): the
oracle's inner loop, meta-gradient included, then runs a ragged task without a line of oracle/ changing.  On a balanced task the three
functions perform the oracle's own operations in the oracle's own order (tests/test_ragged_restatement.py holds them to bitwise equality on
all ten fixtures, and to fp64 autograd of a literal statement of the loss on a ragged task)."""
import contextlib

import numpy as np

import gmeta_oracle as orc

f32 = np.float32


def class_rows(y, classes, limit=None):
    """Rows of every class in `classes` (sorted), in batch order; the first `limit` of them when given.  A class may have none."""
    rows = []
    for c in classes:
        r = np.nonzero(y == c)[0]
        rows.append(r[:limit] if limit is not None else r)
    return rows


def loss_core(logits, rows, protos):
    """Sample-mean loss and accuracy of the rows (visited class by class) against the prototypes; G = dL/d(-dist)."""
    idx = np.concatenate(rows)
    tgt = np.concatenate([np.full(len(r), c) for c, r in enumerate(rows)]).astype(np.int64)
    q = logits[idx]
    d = ((q[:, None, :] - protos[None, :, :]) ** 2).sum(2)
    logp = orc._log_softmax(-d)
    Q = len(idx)
    loss = -logp[np.arange(Q), tgt].mean()
    acc = (logp.argmax(1) == tgt).astype(f32).mean()              # first maximum of the fp32 log-probabilities
    G = np.exp(logp); G[np.arange(Q), tgt] -= 1; G /= f32(Q)
    return f32(loss), f32(acc), G.astype(f32), q, idx, logp, tgt


def make(y_spt, margins=None):
    """(proto_loss_spt, proto_loss_qry, protos_to_dlogits) for the task whose support labels are y_spt.  margins: a list that receives, per
    query scoring, the gap between the two largest log-probabilities of every row (inf with one class)."""
    spt_classes = np.unique(y_spt)

    def spt(logits, y, n_support, need_grad=True):
        classes = np.unique(y)
        rows = class_rows(y, classes, n_support)
        protos = np.stack([logits[r].mean(0) for r in rows]).astype(f32)
        loss, acc, G, q, idx, _, _ = loss_core(logits, rows, protos)
        dl = None
        if need_grad:
            dl = np.zeros_like(logits)
            diff = q[:, None, :] - protos[None, :, :]
            np.add.at(dl, idx, (G[:, :, None] * (-2 * diff)).sum(1))      # query role
            dp = (G[:, :, None] * (2 * diff)).sum(0)                      # prototype role
            for c, r in enumerate(rows):
                dl[r] += dp[c] / f32(len(r))
        return loss, acc, protos, dl

    def qry(logits, y, protos, need_grad=False):
        if len(y) == 0:
            raise ValueError('task without query rows')
        if not np.isin(y, spt_classes).all():
            raise ValueError('query label outside the support classes')
        rows = class_rows(y, spt_classes)
        loss, acc, G, q, idx, logp, tgt = loss_core(logits, rows, protos)
        if margins is not None:
            s = np.sort(logp, 1)
            margins.append(s[:, -1] - s[:, -2] if logp.shape[1] > 1 else np.full(len(logp), np.inf))
        if not need_grad:
            return loss, acc, None, None
        diff = q[:, None, :] - protos[None, :, :]
        dl = np.zeros_like(logits)
        np.add.at(dl, idx, (G[:, :, None] * (-2 * diff)).sum(1))
        dp = (G[:, :, None] * (2 * diff)).sum(0)
        return loss, acc, dl.astype(f32), dp.astype(f32)

    def p2d(y, n_support, dprotos, shape):
        rows = class_rows(y, np.unique(y), n_support)
        dl = np.zeros(shape, f32)
        for c, r in enumerate(rows):
            dl[r] += dprotos[c] / f32(len(r))
        return dl

    return spt, qry, p2d


@contextlib.contextmanager
def patched(y_spt, margins=None):
    """The oracle's three loss functions replaced by the ragged ones of the task with support labels y_spt; restored on exit."""
    saved = (orc.proto_loss_spt, orc.proto_loss_qry, orc.protos_to_dlogits)
    orc.proto_loss_spt, orc.proto_loss_qry, orc.protos_to_dlogits = make(y_spt, margins)
    try:
        yield
    finally:
        orc.proto_loss_spt, orc.proto_loss_qry, orc.protos_to_dlogits = saved


# ---------------------------------------------------------------------------------------------------- ragged tasks cut out of the fixtures
def keep_masks(fx, t):
    """The fixed drop rule (classes sorted): if k_spt >= 2 the last support row of the first class goes; the first query row of the first
    class goes; the first t + 1 query rows of the last class go -- in the last task all of them."""
    ys, yq = fx.z['y_spt'][t], fx.z['y_qry'][t]
    cl = np.unique(ys)
    ks, kq = np.ones(len(ys), bool), np.ones(len(yq), bool)
    if fx.args['k_spt'] >= 2:
        ks[np.nonzero(ys == cl[0])[0][-1]] = False
    r = np.nonzero(yq == cl[-1])[0]
    if t == fx.T - 1:
        kq[r] = False
    else:
        kq[r[:t + 1]] = False
    kq[np.nonzero(yq == cl[0])[0][0]] = False
    return ks, kq


def all_masks(fx, ragged=True):
    if ragged:
        return [keep_masks(fx, t) for t in range(fx.T)]
    return [(np.ones(len(fx.z['y_spt'][t]), bool), np.ones(len(fx.z['y_qry'][t]), bool)) for t in range(fx.T)]


def oracle_batches(fx, t, ks, kq):
    graphs = fx.graphs()
    out = []
    for tag, keep in (('spt', ks), ('qry', kq)):
        lists = [l for l, k in zip(fx.replay_lists(tag, t), keep) if k]
        out.append(orc.extract_batch(graphs, fx.z[tag + '_seeds'][t][keep], fx.args['h'], fx.args['sample_nodes'], 222, fx.link, replay_nodes=lists))
    return out


def run_tasks(fx, masks, patch, K, need_meta_grad, margins=None):
    """task_inner_loop on every task of the fixture restricted to `masks`: [(losses_q, accs_q, meta-grad list)] per task."""
    res = []
    for t, (ks, kq) in enumerate(masks):
        sb, qb = oracle_batches(fx, t, ks, kq)
        ys, yq = fx.z['y_spt'][t][ks], fx.z['y_qry'][t][kq]
        ctx = patched(ys, margins) if patch else contextlib.nullcontext()
        with ctx:
            res.append(orc.task_inner_loop(sb, qb, sb.features(fx.feats), qb.features(fx.feats), ys, yq, fx.vars0, fx.config, fx.args['k_spt'],
                                           fx.args['update_lr'], K, need_meta_grad))
    return res


def meta_step(fx, masks):
    """Meta.forward on the restricted tasks: task-mean losses_q [K+1], accs [K+1], mean meta-gradient (flat), post-Adam parameters."""
    res = run_tasks(fx, masks, True, fx.K, True)
    T = len(res)
    lq = sum(r[0].astype(np.float64) for r in res) / T
    aq = sum(r[1].astype(np.float64) for r in res) / T
    gsum = [np.zeros_like(v) for v in fx.vars0]
    for r in res:
        gsum = [a + b for a, b in zip(gsum, r[2])]
    grad = [(g / f32(T)).astype(f32) for g in gsum]
    new = fx.vars0 if np.isnan(lq[-1]) else orc.adam_step(fx.vars0, grad, {}, fx.args['meta_lr'])
    return lq, aq, grad, new


def support_chain(fx, sb, ys, K):
    """fw_K and the prototypes of the support pass at fw_{max(K-1, 0)} (what Meta.adapt returns) of one restricted task."""
    xs = sb.features(fx.feats)
    fw = [v.copy() for v in fx.vars0]
    spt, _, _ = make(ys)
    protos = None
    for _ in range(max(K, 1)):
        logit_s, cs = orc.classifier_forward(sb, xs, fw, fx.config)
        _, _, protos, dls = spt(logit_s, ys, fx.args['k_spt'], need_grad=K > 0)
        if K > 0:
            g = orc.classifier_backward(sb, fw, fx.config, cs, dls)
            fw = [w - f32(fx.args['update_lr']) * gg for w, gg in zip(fw, g)]
    return fw, protos
