"""TEST INFRASTRUCTURE ONLY -- the fp64 reference of a whole meta-step, its fp32 yardstick and the bar, for tests/test_step_ref.py (CPU),
tests/test_hip_step_numerics.py and tests/test_hip_fuzz.py (GPU).  The arithmetic is the oracle's (oracle/gmeta_oracle.py with dtype=float64 / float32);
nothing of it is restated here.

The bar.  For a tensor X with fp64 reference R, err(A) = max|A - R|.  The yardstick is Y = max(err(oracle at float32), err(the reference's golden
gradient) where the fixture carries one, u/2 * max|R|) with u = 2^-24: what honest fp32 implementations of the same step miss fp64 by, and never less
than the error of storing R in fp32.  A device result passes when err <= 4 Y (FACTOR: the project's factor for nonlinear quantities).  The head
bias's gradient is mathematically zero (prototype distances are shift invariant): its floor is u/2 * sum|dlogits| of the fp64
reference (mean over the tasks, like the gradient) in place of u/2 * max|R|.  A GraphConv bias's gradient is a column sum of dq over the rows, and the same
section names the case where it is noise too (every centre unit active: the last layer's is W^T sum_s dlogits_s = 0).  Its floor is never below the error of
STORING what it sums, u/2 * max_col sum_rows |dq| of the fp64 reference -- the head bias's reasoning, per column; where the sum does not cancel that is within a
small factor of u/2 * max|R| and changes nothing (fuzz world 12, the last layer's bias: the device at 3.9 u of max|R|, the oracle at 0.95 u, of a sum whose
terms are 2.6 times its size: 1.3 u of max|R| is the floor there).  The head bias's fast weight, theta - lr * (K such sums), gets
u/2 * (max|theta| + lr * sum over the K support steps of sum|dlogits|) likewise.

Decided rows.  A scored query row is decided when the fp64 gap between its two smallest squared distances (= between its two best log-probabilities)
exceeds 2^-10 * max_c dist(q, c): a condition on the inputs, three orders of magnitude above the logit errors, not a tolerance.  One more condition
comes from the number format: the reference, the oracle and the kernels all take the argmax of log-probabilities STORED in fp32, whose spacing is up to
2u |logp| each, so a gap of at most 4u * max_c |logp_c| cannot be ordered by any of them (golden case g8_wide_scales: distances of 1e-10 under
log-probabilities of -0.69; there the reference's own accuracies differ from fp64's).  Such a row is undecided too.  Accuracies must equal
the fp64 reference's on decided rows; undecided rows are left out on both sides (a device count may lie anywhere between the decided correct rows and
those plus the undecided ones)."""
import numpy as np

import gmeta_oracle as orc

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
FACTOR = 4.0
DECIDED = 2.0 ** -10
LOGP_SPACING = 4 * U
MAX_UNDECIDED = 1.0 / 50
# Scored rows (over tasks and k) of the golden fixtures whose two nearest prototypes are within 2^-10 of the farthest distance: g2_shared task 0, k 2, row 6
# (0.407545 / 0.407587); g7_wide_h2 task 0, k 0, row 2 (0.034992 / 0.035012 / 0.0974) and k 1, row 5 (1.35569 / 1.35646 / 1.9087).  g8_wide_scales (feature scales
# down to 2^-20): 55 of its 150 rows have distances so small under log-probabilities of -0.69 that fp32 log-probabilities tie.  Every other case: none.
GOLDEN_UNDECIDED = {'g2_shared': 1, 'g7_wide_h2': 2, 'g8_wide_scales': 55}


class RefBatch:
    """What the oracle's step functions read of a batch (indptr, indices, norm, centre_rows, n, dst, features()), for one set of rows that is already
    extracted: the norms and feature rows are the fp32 arrays the device gets."""

    def __init__(self, indptr, indices, norm, centre_rows, x):
        self.indptr, self.indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
        self.n = len(self.indptr) - 1
        self.norm = np.asarray(norm, f32)
        self.centre_rows = np.asarray(centre_rows, np.int64)
        self.dst = np.repeat(np.arange(self.n), np.diff(self.indptr))
        self.x = np.asarray(x, f32)

    def features(self, feats):
        return self.x


def device_sets(B, feats=None):
    """One RefBatch per set of a device SubgraphBatch: its in-edge CSR, centre rows and norms (GM_F_NORM) as the kernels read them, and its feature rows --
    gathered on the host from `feats` (the store's per-graph matrices) by the batch's parent ids, or, without them, by gm_gather_features (a pure copy).
    tests/test_hip_parity.py and tests/test_hip_fuzz.py hold the extraction itself bit-exact."""
    import torch
    from gmeta_amd import _lib
    ip, ix = B.csr()
    ip, ix = ip.astype(np.int64), ix.astype(np.int64)
    norm = B._read(_lib.F_NORM, B.rows, f32)
    sub_off = B.sub_off.astype(np.int64)
    cen = sub_off[:-1, None] + B._read(_lib.F_CENTRE, B.subs * B.centres, np.int32).reshape(B.subs, B.centres)
    if feats is not None:
        gid = np.repeat(B._read(_lib.F_GRAPH, B.subs, np.int32), np.diff(sub_off))
        par = B.parent().astype(np.int64)
        x = np.empty((B.rows, np.asarray(feats[0]).shape[1]), f32)
        for g in np.unique(gid):
            x[gid == g] = np.asarray(feats[g], f32)[par[gid == g]]
    else:
        x = torch.empty(B.rows, B.feat_dim, device='cuda')
        _lib.check(_lib.lib().gm_gather_features(B.handle, _lib.ptr(x), _lib.stream_ptr()), 'gm_gather_features')
        torch.cuda.synchronize()
        x = x.cpu().numpy()
    out = []
    sso = B.set_sub_off
    for t in range(B.sets):
        s0, s1 = int(sso[t]), int(sso[t + 1])
        r0, r1 = int(sub_off[s0]), int(sub_off[s1])
        e0, e1 = int(ip[r0]), int(ip[r1])
        out.append(RefBatch(ip[r0:r1 + 1] - e0, ix[e0:e1] - r0, norm[r0:r1], cen[s0:s1] - r0, x[r0:r1]))
    return out


def decided_rows(logits, y, protos):
    """(decided [Q], correct [Q], pred [Q]) of one scored query set in fp64; class c of `protos` is the c-th smallest label."""
    logits, protos = np.asarray(logits, f64), np.asarray(protos, f64)
    classes = np.unique(y)
    tgt = np.searchsorted(classes, np.asarray(y))
    d = ((logits[:, None, :] - protos[None, :, :]) ** 2).sum(2)
    pred = d.argmin(1)
    if d.shape[1] < 2:
        return np.ones(len(d), bool), pred == tgt, pred
    s = np.sort(d, 1)
    gap = s[:, 1] - s[:, 0]
    m = (-d).max(1, keepdims=True)
    logp = -d - m - np.log(np.exp(-d - m).sum(1, keepdims=True))
    return (gap > DECIDED * s[:, -1]) & (gap > LOGP_SPACING * np.abs(logp).max(1)), pred == tgt, pred


def reference(spt, qry, ys, yq, theta, config, k_spt, update_lr, K, golden_grad=None, feats=None, sequential=False):
    """The step in fp64 and in fp32 (the yardstick) on per-task batches (oracle Batch objects with their `feats`, or RefBatch objects).  Returns a dict:
      q[name] = (R, [fp32 results that make the yardstick], floor or None) for name in 'grad/<i>' (mean over tasks), 'losses_q', and per task t
                'fw/<t>/<i>' (fw_K), 'protos/<t>' (step K-1), 'logits_q/<t>' (last pass), 'g_q/<t>/<i>', 'g_p/<t>/<i>' and their sum 'g/<t>/<i>';
      accs[t][k] = (decided-and-correct count, undecided count, rows); rows_total / undecided_total over every scored row;
      pred[t] = (decided, fp64 prediction) of the last pass; det64 / det32 = the oracle's per-task detail.
    sequential: the fp32 oracle with its matrix products as fmaf chains over the contraction index (orc.sequential_products: the arithmetic of k_gemm_nn and k_wgrad, which serve the
    small worlds) is one more fp32 implementation in every yardstick.  Callers switch it on only for a path that those kernels serve (asserted through the
    launch accounting) and on which numpy's order alone left a tensor above the bar; each such path is named where it is switched on."""
    T = len(spt)
    res = {}
    for dt in (f64, f32):
        det = []
        with np.errstate(all='ignore'):
            accs, grad, _, lq = orc.meta_step(None, feats, spt, qry, ys, yq, theta, config, k_spt, update_lr, 1e-3, K, adam_state={}, dtype=dt, detail=det)
        res[dt] = (grad, lq, det)
    g64, l64, d64 = res[f64]
    g32, l32, d32 = res[f32]
    n = len(theta)
    q = {}
    seqs = []
    if sequential:
        det = []
        with np.errstate(all='ignore'), orc.sequential_products():
            _, gs, _, ls = orc.meta_step(None, feats, spt, qry, ys, yq, theta, config, k_spt, update_lr, 1e-3, K, adam_state={}, dtype=f32, detail=det)
        seqs.append((gs, ls, det))
    bias_abs = {i: float(np.mean([d['bias_abs'][i] for d in d64])) for i in d64[0]['bias_abs']}      # (the gradient is the mean over the tasks)
    for i in range(n):
        extra = [g32[i]] + ([np.asarray(golden_grad[i])] if golden_grad is not None else []) + [sq[0][i] for sq in seqs]
        q['grad/%d' % i] = (g64[i], extra, U / 2 * bias_abs[i] if i in bias_abs else None)
    q['losses_q'] = (np.asarray(l64, f64), [np.asarray(l32, f64)] + [np.asarray(sq[1], f64) for sq in seqs], None)
    lr = float(f32(update_lr))
    accs_t, pred = [], []
    rows_total = undecided_total = 0
    for t in range(T):
        a = d64[t]
        bs = [d32[t]] + [sq[2][t] for sq in seqs]
        for i in range(n):
            # the head bias's fast weight is theta - lr * (K column sums that are mathematically zero): the floor of its gradient, once per inner step
            ffw = U / 2 * (float(np.abs(theta[i]).max()) + lr * sum(a['dls_abs'])) if i == n - 1 else None
            q['fw/%d/%d' % (t, i)] = (a['fw'][K][i], [b['fw'][K][i] for b in bs], ffw)
            floor = U / 2 * a['bias_abs'][i] if i in a['bias_abs'] else None
            q['g_q/%d/%d' % (t, i)] = (a['g_q'][i], [b['g_q'][i] for b in bs], floor)
            q['g_p/%d/%d' % (t, i)] = (a['g_p'][i], [b['g_p'][i] for b in bs], floor)
            q['g/%d/%d' % (t, i)] = (a['g_q'][i] + a['g_p'][i], [b['g_q'][i] + b['g_p'][i] for b in bs], floor)
        q['protos/%d' % t] = (a['protos'][K - 1], [b['protos'][K - 1] for b in bs], None)
        q['logits_q/%d' % t] = (a['scored'][K][0], [b['scored'][K][0] for b in bs], None)
        per_k = []
        for k in range(K + 1):
            dec, ok, p = decided_rows(a['scored'][k][0], yq[t], a['scored'][k][1])
            per_k.append((int((dec & ok).sum()), int((~dec).sum()), len(dec)))
            rows_total += len(dec); undecided_total += int((~dec).sum())
        accs_t.append(per_k)
        pred.append((dec, p))
    return dict(q=q, accs=accs_t, pred=pred, rows_total=rows_total, undecided_total=undecided_total, det64=d64, det32=d32, T=T, K=K)


def yardstick(R, others, floor=None):
    """(Y, scale): Y as in the module docstring; scale = what one u of error is measured against (max|R|, or the floor's own sum for the head bias)."""
    R = np.asarray(R, f64)
    scale = float(np.abs(R).max()) if floor is None else max(float(np.abs(R).max()), 2 * floor / U)
    fl = U / 2 * scale
    return max([fl] + [float(np.abs(np.asarray(o, f64) - R).max()) for o in others]), scale


class Report:
    """Collects one line per (path, tensor): the device's error in u, the yardstick in u, their ratio; check() returns the line's failure, if any."""

    def __init__(self):
        self.lines, self.bad = [], []

    @staticmethod
    def measure(X, entry):
        """(error in u, yardstick in u, ratio) of a device result against q's entry; u is taken of the entry's scale."""
        R, others, floor = entry
        X = np.asarray(X, f64).reshape(np.shape(R))
        Y, scale = yardstick(R, others, floor)
        err = float(np.abs(X - np.asarray(R, f64)).max()) if np.isfinite(X).all() else float('inf')
        unit = U * scale if scale > 0 else 1.0
        ratio = err / Y if Y > 0 else (0.0 if err == 0 else float('inf'))
        return err / unit, Y / unit, ratio

    def _line(self, path, name, m):
        line = '%-40s %-18s err %10.3f u  yardstick %10.3f u  ratio %7.3f' % (path, name, m[0], m[1], m[2])
        self.lines.append(line)
        if not m[2] <= FACTOR:
            self.bad.append(line)
        return m[2]

    def check(self, path, name, X, entry):
        return self._line(path, name, self.measure(X, entry))

    def worst(self, path, name, values_entries):
        """Several tensors of one kind (one per task): every one is held to its own bar; the line shows the one with the worst ratio."""
        ms = [self.measure(X, entry) for X, entry in values_entries]
        return self._line(path, name, max(ms, key=lambda m: m[2]))

    def text(self):
        return '\n'.join(self.lines)

    def assert_ok(self):
        print(self.text())
        assert not self.bad, 'above %g x the fp32 yardstick:\n%s' % (FACTOR, '\n'.join(self.bad))


def check_counts(counts, device_acc, what):
    """A device accuracy (fraction of `rows`) against the fp64 count on decided rows: every decided row must agree."""
    ok, und, rows = counts
    got = device_acc * rows
    assert abs(got - round(got)) < 1e-3, (what, device_acc, rows)
    assert ok <= int(round(got)) <= ok + und, (what, 'device %d correct rows; fp64: %d decided and correct, %d undecided, of %d' % (round(got), ok, und, rows))


def split_params(flat, theta):
    out, p = [], 0
    for v in theta:
        out.append(np.asarray(flat[p:p + v.size]).reshape(v.shape)); p += v.size
    assert p == len(flat)
    return out


def golden_batches(fx):
    """The oracle's own batches of a golden fixture, on the reference's node lists (CPU tests)."""
    graphs = fx.graphs()
    mk = lambda tag, t: orc.extract_batch(graphs, fx.z[tag + '_seeds'][t], fx.args['h'], fx.args['sample_nodes'], 222, fx.link,      # noqa: E731
                                          replay_nodes=fx.replay_lists(tag, t))
    return [mk('spt', t) for t in range(fx.T)], [mk('qry', t) for t in range(fx.T)]


def golden_reference(fx, spt=None, qry=None, sequential=False):
    """reference() of a golden fixture's meta-step, with the reference's golden gradient as a second fp32 implementation in the yardstick; on the
    oracle's batches, or on the device's (device_sets) when given."""
    feats = None
    if spt is None:
        spt, qry = golden_batches(fx)
        feats = fx.feats
    return reference(spt, qry, list(fx.z['y_spt']), list(fx.z['y_qry']), fx.vars0, fx.config, fx.args['k_spt'], fx.args['update_lr'], fx.K,
                     golden_grad=fx.grad, feats=feats, sequential=sequential)


# ---------------------------------------------------------------------------------------------------------------- the device side
def hold_step(rep, path, ref, theta, grad_flat, losses):
    """The meta-gradient that reached Adam, per parameter tensor, and losses_q[0..K] of one Meta.forward against `ref`."""
    for i, g in enumerate(split_params(grad_flat, theta)):
        rep.check(path, 'grad/%d' % i, g, ref['q']['grad/%d' % i])
    rep.check(path, 'losses_q', losses, ref['q']['losses_q'])


def hold_accs(ref, accs_task, what):
    """Per-task accuracies [T, K+1] of a step against the fp64 counts on decided rows."""
    accs_task = np.asarray(accs_task)
    assert accs_task.shape == (ref['T'], ref['K'] + 1), (what, accs_task.shape)
    for t in range(ref['T']):
        for k in range(ref['K'] + 1):
            check_counts(ref['accs'][t][k], float(accs_task[t, k]), (what, t, k))


def hold_adapt(rep, path, ref, theta, fw, protos, logits, pred):
    """Meta.adapt's fast weights [T, P] and prototypes [T, C, n_out] and predict's query logits / predictions (lists per task), per task and tensor."""
    T, n = ref['T'], len(theta)
    per_task = [split_params(fw[t], theta) for t in range(T)]
    for i in range(n):
        rep.worst(path, 'fw_K/%d' % i, [(per_task[t][i], ref['q']['fw/%d/%d' % (t, i)]) for t in range(T)])
    rep.worst(path, 'protos', [(protos[t][:len(ref['q']['protos/%d' % t][0])], ref['q']['protos/%d' % t]) for t in range(T)])
    rep.worst(path, 'logits_q', [(logits[t], ref['q']['logits_q/%d' % t]) for t in range(T)])
    for t in range(T):
        dec, want = ref['pred'][t]
        got = np.asarray(pred[t])
        assert np.array_equal(got[dec], want[dec]), (path, t, np.nonzero(dec & (got != want))[0])


def run_device(m, batch, K, feat=None):
    """On one Meta `m` (theta is changed by the last call only): adapt with K steps and predict with logits; the step's per-task accuracies from its output
    block; then Meta.forward with the launch accounting on.  Returns what hold_step / hold_accs / hold_adapt take, and launches[category] / work[category] of the forward (gm_profile_read)."""
    import ctypes as C
    import torch
    from gmeta_amd import _lib
    lib = _lib.lib()
    xs, ys, xq, yq = batch[0], batch[1], batch[2], batch[3]
    assert m.update_step == K
    ad = m.adapt(xs, ys, K=K)
    p = ad.predict(xq, logits=True)
    out, P, T = m._run(xs, ys, xq, yq, K, True)
    K1 = K + 1
    tail = out[P + 2 * K1 + 1:].cpu().numpy().astype(f64)
    accs_task = tail[:T * K1].reshape(T, K1)
    launches, work = {}, {}
    lib.gm_profile_enable(1)
    try:
        accs = np.asarray(m(xs, ys, xq, yq, None, None, None, None, None, None, feat)).copy()
        torch.cuda.synchronize()
        ms, n, wk = C.c_double(), C.c_int64(), C.c_int64()
        for cat in (0, 1, 2, 4, 5, 6, 7, 14):      # (14: the weight gradients' accounted bytes, the A and G rows they read)
            lib.gm_profile_read(cat, C.byref(ms), C.byref(n), C.byref(wk))
            launches[cat], work[cat] = int(n.value), int(wk.value)
    finally:
        lib.gm_profile_enable(0)
    grad = torch.cat([q.grad.reshape(-1) for q in m.net.parameters()]).cpu().numpy().copy()
    np.testing.assert_allclose(accs, accs_task.mean(0), atol=1e-6)
    return dict(grad=grad, losses=np.asarray(m.last_stats['losses_q']).copy(), accs_task=accs_task, fw=ad.fast_weights.cpu().numpy(),
                protos=ad.prototypes.cpu().numpy(), logits=p.logits, pred=p.pred, launches=launches, work=work)


def hold_all(rep, path, ref, theta, dev):
    hold_step(rep, path, ref, theta, dev['grad'], dev['losses'])
    hold_adapt(rep, path, ref, theta, dev['fw'], dev['protos'], dev['logits'], dev['pred'])
    hold_accs(ref, dev['accs_task'], path)
