"""numpy statement of one head-and-loss launch (gm_dense_head_loss; model.hip: k_head_loss and the unfused k_head_fwd / k_proto / k_head_bwd), and the cases
tests/test_hip_head_numerics.py runs.  Two statements on identical inputs:

  * fp64, stage by stage -- logits64 (the linear head), class_tables (which rows score, by the rules of class_tables / class_tables_ragged in model.hip),
    loss64 (prototypes, log-softmax, loss, first-maximum accuracy, dlogits with the prototype path of mode 0, dprotos), bwd64 (dWl, dbl and the head's input
    gradient at the centres with relu'(H)) -- and whole64, the stages chained;
  * loss32, the nonlinear stage restated in fp32 in the kernel's operation order (proto_set): the yardstick of the GPU test, never its subject.

tests/test_head_ref.py holds the fp64 statement against the oracle, tests/ragged_ref.py and finite differences."""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- class tables
def class_tables(y, set_off, mode, n_support=0, ragged=False, spt_classes=None):
    """Per set (classes, rows): the sorted class labels and, per class, the scored subgraph ids (global, batch order).  mode 0: the first n_support rows of a
    class (ragged: min(n_support, count)); mode 1: all rows.  Balanced mode refuses what the library refuses (ValueError).  spt_classes (ragged, mode 1): per set
    the support side's classes, under which the rows are filed -- a class may then have no rows."""
    out = []
    for t in range(len(set_off) - 1):
        a, b = int(set_off[t]), int(set_off[t + 1])
        yt = np.asarray(y[a:b])
        if spt_classes is not None:
            classes = np.asarray(sorted(spt_classes[t]))
            if not np.isin(yt, classes).all():
                raise ValueError('query label outside the support classes')
        else:
            classes = np.unique(yt)
        rows = []
        for c in classes:
            r = a + np.nonzero(yt == c)[0]
            if mode == 0:
                if not ragged and len(r) < n_support:
                    raise ValueError('class with fewer than n_support rows')
                r = r[:n_support]
            rows.append(r)
        if not ragged and len({len(r) for r in rows}) != 1:
            raise ValueError('classes with unequal row counts')
        out.append((classes, rows))
    return out


def is_ragged(tables):
    """The launch holds a set whose classes score unequal row counts (the RGK instantiations run)."""
    return any(len({len(r) for r in rows}) != 1 for _, rows in tables)


# ---------------------------------------------------------------------------------------------------- fp64 stages
def cat_rows(H, crow):
    """cat(h[c0], h[c1]) per subgraph: [subs, nc * Hd]."""
    return np.concatenate([H[crow[:, w]] for w in range(crow.shape[1])], 1)


def logits64(H, crow, sub_set, Wl, bl):
    """logits [subs, C] in fp64 and the bar's scale, sum |x||w| + |b|.  Wl [sets, C, hc], bl [sets, C] (one entry: shared by every set)."""
    x = cat_rows(H.astype(f64), crow)
    W = Wl.astype(f64)[sub_set if len(Wl) > 1 else np.zeros(len(sub_set), int)]
    b = bl.astype(f64)[sub_set if len(bl) > 1 else np.zeros(len(sub_set), int)]
    return np.einsum('sh,sch->sc', x, W) + b, np.einsum('sh,sch->sc', np.abs(x), np.abs(W)) + np.abs(b)


def set_loss64(z, rows, protos):
    """One set in fp64.  z [subs, D] (global ids index it), rows per class, protos [>= Ct, D] or None (mode 0: the class means).  Returns a dict; dlogits covers
    all of z (zero outside the set's rows)."""
    z = z.astype(f64)
    mode0 = protos is None
    Ct = len(rows)
    P = np.stack([z[r].mean(0) for r in rows]) if mode0 else protos[:Ct].astype(f64)
    idx = np.concatenate(rows); tgt = np.concatenate([np.full(len(r), c) for c, r in enumerate(rows)]).astype(np.int64)
    q = z[idx]; Q = len(idx)
    diff = q[:, None, :] - P[None]
    d = (diff ** 2).sum(2)
    a = -d
    mx = a.max(1, keepdims=True)
    logp = a - mx - np.log(np.exp(a - mx).sum(1, keepdims=True))
    pred = logp.argmax(1)                                       # first maximum
    G = np.exp(logp); G[np.arange(Q), tgt] -= 1; G /= Q
    dl = np.zeros_like(z)
    dl[idx] = (G[:, :, None] * (-2 * diff)).sum(1)              # a row scores once
    dp = (G[:, :, None] * (2 * diff)).sum(0)
    if mode0:
        for c, r in enumerate(rows):
            dl[r] += dp[c] / len(r)
    s = np.sort(logp, 1)
    return dict(protos=P, loss=-logp[np.arange(Q), tgt].mean(), acc=(pred == tgt).mean(), correct=int((pred == tgt).sum()), Q=Q, dlogits=dl, dprotos=dp,
                gap=(s[:, -1] - s[:, -2]) if Ct > 1 else np.full(Q, np.inf), dmax=d.max(1), pred=pred, tgt=tgt)


def undecided(r):
    """Scored rows of a set_loss64 result whose two best fp64 log-probabilities are closer than 64 u max_c dist(q, c) (see test_hip_head_numerics.py)."""
    return int(np.count_nonzero(~(r['gap'] > 64 * U * r['dmax'])))


def loss64(z, tables, protos=None):
    return [set_loss64(z, rows, None if protos is None else protos[t]) for t, (_, rows) in enumerate(tables)]


def bwd64(H, crow, set_off, Wl, dlogits):
    """dWl [sets, C, hc], dbl [sets, C], G [subs, nc, Hd] = relu'(H[centre]) * (dlogits @ Wl)[:, centre block], each with the bar's scale (sum of |products|)."""
    Hd = H.shape[1]; nc = crow.shape[1]; sets = len(set_off) - 1
    x = cat_rows(H.astype(f64), crow); dl = dlogits.astype(f64)
    C = dl.shape[1]
    dW = np.zeros((sets, C, nc * Hd)); dWs = np.zeros_like(dW); db = np.zeros((sets, C)); dbs = np.zeros_like(db)
    G = np.zeros((len(crow), nc, Hd)); Gs = np.zeros_like(G)
    for t in range(sets):
        a, b = int(set_off[t]), int(set_off[t + 1])
        W = Wl.astype(f64)[t if len(Wl) > 1 else 0]
        dW[t] = dl[a:b].T @ x[a:b]; dWs[t] = np.abs(dl[a:b]).T @ np.abs(x[a:b])
        db[t] = dl[a:b].sum(0); dbs[t] = np.abs(dl[a:b]).sum(0)
        g = (dl[a:b] @ W).reshape(b - a, nc, Hd); gs = (np.abs(dl[a:b]) @ np.abs(W)).reshape(b - a, nc, Hd)
        keep = np.stack([H[crow[a:b, w]] > 0 for w in range(nc)], 1)          # decided on the input: a masked element is exactly 0
        G[a:b] = np.where(keep, g, 0.0); Gs[a:b] = np.where(keep, gs, 0.0)
    return dW, dWs, db, dbs, G, Gs


def scatter_dq(G, Gs, crow, rows):
    """dQ [rows, Hd] from the compact gradient: the index_select backward -- both centres of a pair may be one row.  Returns dQ, its scale and the written-row mask."""
    dQ = np.zeros((rows, G.shape[2])); sc = np.zeros_like(dQ); hit = np.zeros(rows, bool)
    for w in range(crow.shape[1]):
        np.add.at(dQ, crow[:, w], G[:, w]); np.add.at(sc, crow[:, w], Gs[:, w]); hit[crow[:, w]] = True
    return dQ, sc, hit


def whole64(H, crow, set_off, Wl, bl, tables, protos=None):
    """The launch in fp64 end to end (the GPU test references stage by stage instead, each from the kernel's own fp32 inputs to that stage)."""
    sub_set = np.repeat(np.arange(len(set_off) - 1), np.diff(set_off))
    z, _ = logits64(H, crow, sub_set, Wl, bl)
    res = loss64(z, tables, protos)
    dl = sum(r['dlogits'] for r in res)
    dW, _, db, _, G, Gs = bwd64(H, crow, set_off, Wl, dl)
    dQ, _, hit = scatter_dq(G, Gs, crow, H.shape[0])
    return dict(logits=z, sets=res, dlogits=dl, dWl=dW, dbl=db, G=G, dQ=dQ, hit=hit, loss=np.array([r['loss'] for r in res]))


# ---------------------------------------------------------------------------------------------------- fp32 restatement of the nonlinear stage
def _butterfly(v):
    """wave_sumf: v += shfl_xor(v, o) for o = 32 .. 1 over 64 lanes; lane 0's value."""
    v = np.asarray(v, f32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


def set_loss32(z, rows, protos):
    """proto_set's operations in fp32, in its order: a class mean is a running sum over the class's rows divided by their count; a squared distance a running
    sum over the columns; the softmax sum, a row's gradient and a prototype's gradient running sums over the classes / the scored rows in table order.  (A
    compiler may contract a multiply-add, and expf / logf are the device's own: this is a yardstick for the size of fp32 error, not a bitwise model.)"""
    z = z.astype(f32)
    mode0 = protos is None
    Ct, D = len(rows), z.shape[1]
    if mode0:
        P = np.zeros((Ct, D), f32)
        for c, r in enumerate(rows):
            p = np.zeros(D, f32)
            for i in r:
                p = p + z[i]
            P[c] = p / f32(len(r))
    else:
        P = protos[:Ct].astype(f32)
    idx = np.concatenate(rows); tgt = np.concatenate([np.full(len(r), c) for c, r in enumerate(rows)]).astype(np.int64)
    X = z[idx]; Q = len(idx)
    d = np.zeros((Q, Ct), f32)
    for k in range(D):
        t = X[:, k, None] - P[None, :, k]
        d = d + t * t
    a = -d
    m = a.max(1)
    se = np.zeros(Q, f32)
    for c in range(Ct):
        se = se + np.exp(a[:, c] - m)
    lg = np.log(se); lse = m + lg
    lp = (a - m[:, None]) - lg[:, None]
    terms = -((a[np.arange(Q), tgt] - m) - lg)
    # the block sum of the default launch (1024 threads): thread q % 1024 adds its rows in order, a wave's 64 partials meet in an xor butterfly, the 16 wave
    # sums (padded with zeros to one wave) in another
    part = np.zeros(1024, f32)
    for q0 in range(0, Q, 1024):
        part[:min(1024, Q - q0)] += terms[q0:q0 + 1024]
    waves = np.zeros(64, f32)
    waves[:16] = [_butterfly(part[w * 64:(w + 1) * 64]) for w in range(16)]
    loss = _butterfly(waves) / f32(Q)
    acc = f32(np.count_nonzero(lp.argmax(1) == tgt)) / f32(Q)
    onehot = np.zeros((Q, Ct), f32); onehot[np.arange(Q), tgt] = 1
    G = (np.exp(a - lse[:, None]) - onehot) * (f32(1) / f32(Q))
    dq = np.zeros((Q, D), f32)
    for c in range(Ct):
        dq = dq + G[:, c, None] * f32(-2) * (X - P[None, c])
    dp = np.zeros((Ct, D), f32)
    for q in range(Q):
        dp = dp + G[q, :, None] * f32(2) * (X[q][None] - P)
    dl = np.zeros_like(z)
    dl[idx] = dq
    if mode0:
        for c, r in enumerate(rows):
            dl[r] += dp[c] / f32(len(r))
    return dict(protos=P, loss=loss, acc=acc, dlogits=dl, dprotos=dp)


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test
def _case(name, Hd, pair, C, sets, mode, out, n_support=0, grad=True, ragged=False, spt_extra=None, sgd=False, amax=False, compact_nc=0, shared_params=False,
          tie=False, max_nodes=3, staged=1):
    """pair: '1' node seeds, '2' pairs, '2s' pairs with one subgraph per set whose two centres are the same row (centre_local override).  sets: per set a list of
    (rows of a class); mode 0 scores the first n_support of each.  out: 'dQ', 'Gc' (compact gradient over the full H), 'Gcc' (over a compact H), 'none' (bwd = 0).
    grad: dlogits (and dprotos in mode 1) are asked for.  spt_extra (ragged mode 1): {set: number of support classes without query rows}.  compact_nc: 1 = a
    compact H of ONE row per subgraph whatever the batch (pooled rows).  staged: what a launch with GM_HEAD_STAGE = 1 must report."""
    return dict(name=name, Hd=Hd, pair=pair, C=C, sets=sets, mode=mode, out=out, n_support=n_support, grad=grad, ragged=ragged, spt_extra=spt_extra or {}, sgd=sgd,
                amax=amax, compact_nc=compact_nc, shared_params=shared_params, tie=tie, max_nodes=max_nodes, staged=staged)


EQ = [[4, 4, 4]] * 3                        # three sets of equal subgraph counts and one class layout: subs_per_set, uniform
UNEQ0 = [[4, 4, 4], [6, 6], [3, 3, 3, 3]]   # mode 0: unequal subgraph counts, class counts and rows per class: set_sub_off, tab
UNEQ1 = [[4, 4, 4], [2, 2, 2], [5, 5, 5]]   # mode 1 keeps one class count (the prototypes' stride)
RAG = [[1, 17, 6], [2, 2, 2], [3, 1]]       # a balanced set among ragged ones
CASES = [
    # Hd 8: 16-byte staging, the fast dQ loop at every workgroup size
    _case('hd8_c3_fast_sgd', 8, '1', 3, EQ, 0, 'dQ', n_support=2, sgd=True),
    _case('hd8_pair_shared_fast_amax', 8, '2s', 5, EQ, 0, 'dQ', n_support=3, amax=True),
    _case('hd8_c1', 8, '1', 1, EQ, 0, 'dQ', n_support=4, amax=True),
    _case('hd8_grad_only', 8, '1', 3, UNEQ0, 0, 'none', n_support=2),
    _case('hd8_tie', 8, '1', 3, EQ, 0, 'dQ', n_support=4, tie=True),
    # Hd 6: scalar staging, general dQ loop
    _case('hd6_c2_uneq_sgd', 6, '1', 2, UNEQ0, 0, 'dQ', n_support=2, sgd=True),
    _case('hd6_pair_c1_qry_gc', 6, '2', 1, UNEQ1, 1, 'Gc'),
    _case('hd6_pair_shared_ragged_amax', 6, '2s', 2, RAG, 0, 'dQ', n_support=3, ragged=True, amax=True),
    _case('hd6_pair_compact_sgd', 6, '2', 5, EQ, 0, 'Gcc', n_support=3, sgd=True),
    # Hd 20: 16-byte staging, general dQ loop (1024 % 20 != 0)
    _case('hd20_c8_qry_amax', 20, '1', 8, EQ, 1, 'dQ', amax=True),
    _case('hd20_pair_shared_c9', 20, '2s', 9, UNEQ0, 0, 'dQ', n_support=2),
    _case('hd20_pair_c64_qry_gc', 20, '2', 64, UNEQ1, 1, 'Gc'),
    _case('hd20_qry_no_grad', 20, '1', 2, EQ, 1, 'none', grad=False, shared_params=True),
    _case('hd20_pair_pooled_compact', 20, '2', 2, UNEQ1, 1, 'Gcc', compact_nc=1),
    _case('hd20_pair_ragged_qry_empty_class', 20, '2', 5, RAG, 1, 'Gc', ragged=True, spt_extra={0: 1, 2: 2}),
    # Hd 96: hc = 96 (tail columns) with one centre, 192 (unrolled dot) with two
    _case('hd96_pair_c3_sgd', 96, '2', 3, EQ, 0, 'dQ', n_support=2, sgd=True),
    _case('hd96_c5_qry_fwd_only', 96, '1', 5, UNEQ1, 1, 'none', grad=False),
    _case('hd96_c9_ragged_qry', 96, '1', 9, RAG, 1, 'none', ragged=True),
    _case('hd96_pair_shared_c2_amax', 96, '2s', 2, UNEQ1, 1, 'dQ', amax=True),
    # Hd 256: every column in the unrolled dot; the fast dQ loop with C <= 8
    _case('hd256_c64', 256, '1', 64, [[3, 3]] * 3, 0, 'dQ', n_support=2),
    _case('hd256_pair_c2_qry_amax', 256, '2', 2, [[2, 2]] * 3, 1, 'dQ', amax=True),
    _case('hd256_pair_shared_c8', 256, '2s', 8, EQ, 0, 'dQ', n_support=3, sgd=True),
    _case('hd256_c9_gc', 256, '1', 9, UNEQ0, 0, 'Gc', n_support=3),
    _case('hd256_compact_c3', 256, '1', 3, EQ, 0, 'Gcc', n_support=2),
    # ragged support side: every row counts (n_support above every class), the RGK kernels with SGD
    _case('hd8_ragged_spt_sgd', 8, '1', 3, RAG, 0, 'dQ', n_support=40, ragged=True, sgd=True),
    # distance table: Ct n Ct = 9216 > 8192 recomputes every term; Ct D = 576 preloads the prototypes at 1024 threads only.  8192 exactly keeps the table
    _case('table_off_ct24_n16', 8, '1', 24, [[16] * 24] * 2, 1, 'Gc'),
    _case('table_edge_ct16_n32', 8, '1', 4, [[32] * 16], 1, 'dQ'),
    # 160 single-node subgraphs of 256 columns: above 150 KB of LDS, the host launches unstaged whatever GM_HEAD_STAGE says
    _case('size_unstaged', 256, '1', 3, [[40] * 4], 0, 'dQ', n_support=5, max_nodes=1, staged=0, amax=True),
]
N_NODES = 48


def build(case):
    """Every input of a case, as numpy arrays; deterministic in the case's name.  Geometry first (what SubgraphBatch.from_nodes is given and what it must hand
    back: sub_off, centres), then H, parameters, labels, prototypes."""
    rng = np.random.default_rng(sum(ord(ch) * (k + 1) for k, ch in enumerate(case['name'])))
    nc_b = 1 if case['pair'] == '1' else 2
    sets = case['sets']
    set_off = np.concatenate([[0], np.cumsum([sum(s) for s in sets])]).astype(np.int32)
    subs = int(set_off[-1])
    src, dst = rng.integers(0, N_NODES, 4 * N_NODES), rng.integers(0, N_NODES, 4 * N_NODES)
    seeds, lists, centre = [], [], []
    for s in range(subs):
        size = int(rng.integers(nc_b, max(case['max_nodes'], nc_b) + 1))
        nodes = np.sort(rng.choice(N_NODES, size=size, replace=False)).astype(np.int32)
        pick = rng.choice(size, size=nc_b, replace=False)
        seeds.append((0, int(nodes[pick[0]]), int(nodes[pick[1]]) if nc_b == 2 else -1))
        lists.append(nodes); centre.append([int(p) for p in pick])
    sub_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    centre = np.asarray(centre, np.int32).reshape(subs, nc_b)
    centre_local = None
    if case['pair'] == '2s':                                    # one subgraph per set (its second) scores one row twice
        centre_local = centre.copy()
        for t in range(len(sets)):
            centre_local[set_off[t] + 1, 1] = centre_local[set_off[t] + 1, 0]
    rows = int(sub_off[-1])
    compact = case['out'] == 'Gcc'
    nc = case['compact_nc'] or nc_b
    cen = centre_local if centre_local is not None else centre
    crow = (np.arange(subs * nc).reshape(subs, nc) if compact else sub_off[:-1, None] + cen).astype(np.int64)
    Hd, C = case['Hd'], case['C']
    H = rng.standard_normal((subs * nc if compact else rows, Hd)).astype(f32)
    H[rng.random(H.shape) < 0.15] = 0.0                         # relu' is decided on the input: exact zeros of both signs, and negative entries
    H[rng.random(H.shape) < 0.10] = -0.0
    if case['tie']:
        H[:] = 0.0
    hc = nc * Hd
    n_par = 1 if case['shared_params'] else len(sets)
    Wl = (rng.standard_normal((n_par, C, hc)) / np.sqrt(hc)).astype(f32)
    bl = (0.1 * rng.standard_normal((n_par, C))).astype(f32)
    # labels: arbitrary ints, shuffled inside a set.  Support classes without query rows (ragged, mode 1) get labels of their own
    y = np.zeros(subs, np.int32); spt_classes = []
    for t, s in enumerate(sets):
        labs = rng.choice(1000, size=len(s) + case['spt_extra'].get(t, 0), replace=False)
        yt = np.concatenate([np.full(n, labs[c]) for c, n in enumerate(s)])
        y[set_off[t]:set_off[t + 1]] = yt[rng.permutation(len(yt))]
        spt_classes.append(sorted(int(l) for l in labs))
    spt_classes = spt_classes if case['spt_extra'] else None
    tables = class_tables(y, set_off, case['mode'], case['n_support'], case['ragged'], spt_classes)
    c_task = max(len(cl) for cl, _ in tables)
    protos = rng.standard_normal((len(sets), c_task, C)).astype(f32) if case['mode'] == 1 else None
    return dict(case=case, src=src, dst=dst, seeds=np.asarray(seeds, np.int32), lists=lists, set_off=set_off, sub_off=sub_off, centre=centre, centre_local=centre_local,
                rows=rows, subs=subs, nc=nc, nc_batch=nc_b, compact=compact, crow=crow, H=H, Wl=Wl, bl=bl, y=y, spt_classes=spt_classes, tables=tables, c_task=c_task,
                protos=protos, sub_set=np.repeat(np.arange(len(sets)), np.diff(set_off)), feats=rng.standard_normal((N_NODES, 8)).astype(f32))
