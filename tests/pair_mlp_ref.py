"""Restatement of the BUDDY pair predictor (gm_prop_pair_mlp_forward / gm_prop_pair_mlp_step; THE definition is in include/gmeta_hip.h) in float64 numpy, the
derived tolerance of an fp32 evaluation of it, and the cases the tests share.  Nothing here looks at the device.

    z_k  = [ op(x_0[a], x_0[b]) | ... | op(x_hops[a], x_hops[b]) | s_k ]     K = (hops + 1) F + S
    h_k  = relu(z_k W1 + b1),   l_k = h_k . w2 + b2
    loss = (1/n) sum_k max(l_k, 0) - l_k y_k + log1p(exp(-|l_k|)),   dl_k = (sigmoid(l_k) - y_k) / n
    dw2 = sum dl_k h_k,  db2 = sum dl_k,  dh_k = dl_k w2 [h_k > 0],  dW1 = sum z_k (x) dh_k,  db1 = sum dh_k
    params / gradient: one flat buffer [W1 row-major [K, Hd] | b1 | w2 | b2]

The levels come from hop_feature_ref.levels (float64, exact by the definition) with their bound hop_feature_ref.bound.  The tolerance (bound) is derived, with ONE
assumed figure: the device's expf and log1pf are allowed 4 ulp each (ULP_EXP, ULP_LOG1P) -- the ROCm install at hand carries no HIP math accuracy table to take
their errors from, so this figure is assumed, not derived."""
import numpy as np

import hop_feature_ref as hop

f32, f64 = np.float32, np.float64
U = hop.U
gamma = hop.gamma
ULP_EXP = 4.0       # ulp error allowed to the device's expf and log1pf.  ASSUMED, not derived: the ROCm install at hand carries no HIP math accuracy table
ULP_LOG1P = 4.0


def split(params, K, Hd):
    """-> W1 [K, Hd], b1 [Hd], w2 [Hd], b2 (scalar) as float64 views of the values of the flat fp32 buffer"""
    p = np.asarray(params, f32).astype(f64).reshape(-1)
    assert len(p) == K * Hd + 2 * Hd + 1
    return p[:K * Hd].reshape(K, Hd), p[K * Hd:K * Hd + Hd], p[K * Hd + Hd:K * Hd + 2 * Hd], p[-1]


def inputs(x, pairs, op, extra):
    """float64 [n, K]: z by the definition from the float64 levels x [hops + 1, N, F]"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    a, b = x[:, p[:, 0]], x[:, p[:, 1]]                                        # [L1, n, F]
    assert op in hop.OPS
    z = a * b if op == 'hadamard' else np.abs(a - b)
    z = np.transpose(z, (1, 0, 2)).reshape(len(p), x.shape[0] * x.shape[2])
    if extra is not None and np.asarray(extra).shape[-1]:
        z = np.concatenate([z, np.asarray(extra, f32).astype(f64).reshape(len(p), np.asarray(extra).shape[-1])], axis=1)
    return z


def sigmoid(l):
    e = np.exp(-np.abs(l))
    return np.where(l >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def evaluate(x, pairs, op, extra, params, Hd, labels=None):
    """-> dict: z, pre, h, logits and, with labels, loss, dl, dh and grad (flat float64, the layout of the parameters)"""
    z = inputs(x, pairs, op, extra)
    n, K = z.shape
    W1, b1, w2, b2 = split(params, K, Hd)
    pre = z @ W1 + b1
    h = np.maximum(pre, 0.0)
    l = h @ w2 + b2
    out = dict(z=z, pre=pre, h=h, logits=l)
    if labels is None:
        return out
    y = np.asarray(labels, f32).astype(f64).reshape(-1)
    if n == 0:
        out.update(loss=0.0, dl=np.zeros(0), dh=np.zeros((0, Hd)), grad=np.zeros(K * Hd + 2 * Hd + 1))
        return out
    terms = np.maximum(l, 0.0) - l * y + np.log1p(np.exp(-np.abs(l)))
    dl = (sigmoid(l) - y) / n
    dh = dl[:, None] * w2[None, :] * (h > 0)
    grad = np.concatenate([(z.T @ dh).reshape(-1), dh.sum(0), dl @ h, [dl.sum()]])
    out.update(loss=terms.sum() / n, terms=terms, dl=dl, dh=dh, grad=grad)
    return out


def bound(x, E, pairs, op, extra, params, Hd, labels=None):
    """The tolerance of an fp32 evaluation of the definition in ANY order of every sum -- derived, not measured -> dict logits [n] and, with labels, loss
    (scalar) and grad (flat), plus near [n, Hd]: the near-kink entries.  u = 2^-24, gamma_k = k u / (1 - k u).
      z          the levels carry the error E of hop_feature_ref.bound: |x^a x^b - xa xb| <= |xa| Eb + |xb| Ea + Ea Eb, ||x^a - x^b| - |xa - xb|| <= Ea + Eb; one
                 rounding for op on top: Ez.  The structure columns are exact.  |z^| <= Za = |z| + Ez.
      pre        K products and the bias, K + 1 terms in any order:  Ep = Ez |W1| + gamma_{K+1} (Za |W1| + |b1|).
      h          relu is 1-Lipschitz: Eh = Ep, |h^| <= Ha = h + Ep.
      logit      Hd products and the bias:  El = Eh |w2| + gamma_{Hd+1} (Ha |w2| + |b2|).
      loss term  t(l) has |t'| = |sigmoid - y| <= 1: El; its evaluation: expf to ULP_EXP ulp (1 ulp <= 2 u relative) and log1pf to ULP_LOG1P ulp, both values at
                 most 1, a product and two sums (4 roundings on at most |l^| + log 2); the factor 1/n: float(n), the reciprocal and the product, gamma_3.
                 The n-term sum: gamma_n.
      dl         |sigmoid'| <= 1/4: El / 4; expf, 1 + e and the division: (2 ULP_EXP + 2) u on a value of at most 1; the difference and 1/n: gamma_4 on |dl|.
      dw2, db2   sums of n terms dl^ h^ / dl^: the terms' errors Edl Ha + |dl| Eh / Edl, and gamma_n on the terms' magnitudes.
      dh         Edl |w2| and one product rounding.  A NEAR-KINK entry (|pre| <= Ep: its mask may legitimately flip) gains (|dl| + Edl) |w2|.
      db1, dW1   sums of n terms dh^ / z^ dh^: Edh / (Ez Da + |z| Edh), Da = |dh| + Edh, and gamma_n on Da / Za Da."""
    ref = evaluate(x, pairs, op, extra, params, Hd, labels)
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    xa, xb, Ea, Eb = np.abs(x[:, p[:, 0]]), np.abs(x[:, p[:, 1]]), E[:, p[:, 0]], E[:, p[:, 1]]
    if op == 'hadamard':
        Ez = xa * Eb + xb * Ea + Ea * Eb
        Ez = Ez + U * (xa * xb + Ez)
    else:
        Ez = Ea + Eb
        Ez = Ez + U * (np.abs(x[:, p[:, 0]] - x[:, p[:, 1]]) + Ez)
    n = len(p)
    Ez = np.transpose(Ez, (1, 0, 2)).reshape(n, x.shape[0] * x.shape[2])
    z = ref['z']
    K = z.shape[1]
    Ez = np.concatenate([Ez, np.zeros((n, K - Ez.shape[1]))], axis=1)
    W1, b1, w2, b2 = split(params, K, Hd)
    Za = np.abs(z) + Ez
    Ep = Ez @ np.abs(W1) + gamma(K + 1) * (Za @ np.abs(W1) + np.abs(b1))
    Ha = ref['h'] + Ep
    El = Ep @ np.abs(w2) + gamma(Hd + 1) * (Ha @ np.abs(w2) + abs(b2))
    near = np.abs(ref['pre']) <= Ep
    out = dict(logits=El, near=near, pre=Ep)
    if labels is None or n == 0:
        if labels is not None:
            out.update(loss=0.0, grad=np.zeros(K * Hd + 2 * Hd + 1))
        return out
    l, dl, dh = ref['logits'], ref['dl'], ref['dh']
    g3, g4, gn = gamma(3), gamma(4), gamma(n)
    Et = El + 4 * U * (np.abs(l) + El + np.log(2.0)) + 2 * U * (ULP_EXP + ULP_LOG1P)
    Eterm = Et * (1 + g3) / n + g3 * ref['terms'] / n
    loss = Eterm.sum() + gn * (ref['terms'] / n + Eterm).sum()
    Edl = (El / 4 + (2 * ULP_EXP + 2) * U) * (1 + g4) / n + g4 * np.abs(dl)
    Dla = np.abs(dl) + Edl
    Edw2 = Edl @ Ha + np.abs(dl) @ Ep + gn * (Dla @ Ha)
    Edb2 = Edl.sum() + gn * Dla.sum()
    Edh = Edl[:, None] * np.abs(w2)[None, :] + U * Dla[:, None] * np.abs(w2)[None, :]
    Edh = np.where(ref['h'] > 0, Edh, 0.0) + np.where(near, Dla[:, None] * np.abs(w2)[None, :] + Edh, 0.0)
    Da = np.abs(dh) + Edh
    Edb1 = Edh.sum(0) + gn * Da.sum(0)
    EdW1 = Ez.T @ Da + np.abs(z).T @ Edh + gn * (Za.T @ Da)
    out.update(loss=loss, grad=np.concatenate([EdW1.reshape(-1), Edb1, Edw2, [Edb2]]))
    return out


# ---------------------------------------------------------------------------------------------------- the cases the CPU and the GPU tests share
# (graph, F, hops, S, Hd, n in units of the pair tile: (multiples, offset), op, weighted, self_loops).  A pruned cross product: every F of {5, 64, 100, 300},
# hops of {1, 3}, S of {0, 1, 25}, Hd of {1, 8, 100, 256}, n of {0, 1, T - 1, T, T + 1, 3 T + 7}, both ops, weighted and not, with and without self loops, and the
# corners (F 5, Hd 1, S 0, n 1) and (F 300, Hd 256, S 25, n 3 T + 7).
CASES = (
    ('multigraph', 5, 1, 0, 1, (0, 1), 'hadamard', False, True),
    ('hub', 300, 3, 25, 256, (3, 7), 'hadamard', True, True),
    ('chain', 64, 1, 1, 8, (1, -1), 'abs_diff', False, False),
    ('hub', 100, 3, 25, 100, (1, 0), 'abs_diff', True, False),
    ('multigraph', 64, 3, 0, 256, (1, 1), 'hadamard', True, True),
    ('chain', 100, 1, 1, 100, (3, 7), 'hadamard', False, True),
    ('multigraph', 300, 1, 25, 8, (1, 1), 'abs_diff', False, False),
    ('hub', 5, 3, 1, 1, (1, 0), 'abs_diff', True, True),
    ('chain', 5, 1, 0, 8, (0, 0), 'hadamard', False, True),
)
CASE_IDS = ['%s-F%d-h%d-S%d-Hd%d-n%dT%+d-%s-%s-%s' % (c[0], c[1], c[2], c[3], c[4], c[5][0], c[5][1], c[6], 'w' if c[7] else 'u', 'sl' if c[8] else 'nosl') for c in CASES]


def graph(which):
    """-> N, src, dst, w: the small graphs of the hop-feature tests (fp32 weights in [0.25, 4) for the weighted stores)"""
    import distance_ref
    import negative_ref
    if which == 'hub':
        return hop.hub_case()
    N, src, dst = negative_ref.multigraph_case() if which == 'multigraph' else distance_ref.chain_case()[:3]
    w = np.exp2(np.random.default_rng(41).uniform(-2, 2, len(src))).astype(f32)
    return N, src, dst, w


def init_params(K, Hd, seed):
    """flat fp32 parameters with the ranges of torch.nn.Linear's initialisation: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for a layer's weights and bias"""
    rng = np.random.default_rng(seed)
    k1, k2 = 1.0 / np.sqrt(K), 1.0 / np.sqrt(Hd)
    return np.concatenate([rng.uniform(-k1, k1, K * Hd), rng.uniform(-k1, k1, Hd), rng.uniform(-k2, k2, Hd), rng.uniform(-k2, k2, 1)]).astype(f32)


def case_pairs(N, n, seed):
    """int64 [n, 2]: random pairs with, where n allows, a == b (row 0), a duplicate (rows 1, 2) and both orientations of one pair (rows 3, 4)"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, N, (n, 2)).astype(np.int64)
    if n >= 1:
        p[0, 1] = p[0, 0]
    if n >= 3:
        p[2] = p[1]
    if n >= 5:
        p[4] = p[3][::-1]
    return p


def case_inputs(case, T):
    """-> dict of the seeded inputs of one case for the pair tile T: N, csr (ptr, idx, w), X, pairs, extra (float32 [n, S] or None), labels, params, K, n"""
    which, F, hops, S, Hd, (mul, off), op, weighted, self_loops = case
    N, src, dst, w = graph(which)
    n = mul * T + off
    seed = 1000 + F + 7 * hops + 13 * S + Hd
    rng = np.random.default_rng(seed)
    K = (hops + 1) * F + S
    X = hop.features(N, F, 100 + F)
    extra = rng.integers(0, 6, (n, S)).astype(f32) if S else None            # small counts, as the sketch and distance profiles give
    labels = (rng.random(n) < 0.5).astype(f32)
    if n >= 2:
        labels[1] = 0.25                                                        # a soft label
    return dict(N=N, csr=hop.csr(N, src, dst, w if weighted else None), src=src, dst=dst, w=w if weighted else None, X=X, pairs=case_pairs(N, n, seed + 1), extra=extra,
                labels=labels, params=init_params(K, Hd, seed + 2), K=K, n=n, F=F, hops=hops, S=S, Hd=Hd, op=op, self_loops=self_loops, weighted=weighted)
