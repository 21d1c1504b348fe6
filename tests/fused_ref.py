"""Restatement of what the fused aggregate + GEMM kernels (k_gemm_split_p<true, ...>, gemm_split.h) and the table-fed weight gradient
(k_wgrad_split<., ., 3, true, .>, gemm.hip) compute, for test_fused_ref.py (CPU) and test_hip_fused_numerics.py (GPU).  No GPU and no library needed here.

(a) The per-row source tables of a batch, in numpy, as k_row_tables / k_centre_rows (extract.hip) define them -- one entry {u0, u1, w0, w1} of four int32 per row,
    w the bit pattern of an fp32 -- from the batch's in-edge CSR, its fp32 norm, its feature rows and (weighted batches) its edge weights.  Row r of in-degree d:
        d = 0               {ZERO, ZERO, 1, 0}
        d = 1               {u0, u0, w0, 0}
        d = 2               {u0, u1, w0, w1}
        d > MAXDEG          {r | SELF, r | SELF, 1, 0}
    with u the sources in CSR order and w = norm[u], on weighted batches fl(ew * norm[u]) (one fp32 product).  The feature-row table has feat_row[u] in place
    of u (and the same flags); the dQ table holds {r | SELF, ZERO, 1, 0} on the centre rows and {ZERO, ZERO, 0, 0} elsewhere.  The two counts are the rows of
    more than MAXDEG sources and their in-edges.
(b) In fp64 (torch, on whatever device the operands live):  Z[r] = w0 X[u0] + w1 X[u1]  with a SELF source read from `zside` and a ZERO source 0, and
    C[r] = epi(s[r] (Z[r] @ W_set(r)) + b_set(r)),  epi = ReLU.  Beside every value its condition scale: the same expression over magnitudes.
(c) The weight and bias gradients over the same Z:  dW_t = sum_r (s[r] Z[r])^T G0[r],  db_t = sum_r G0[r]  over the rows of set t, G0 = G with the rows a
    keep flag drops taken as zeros.

The graphs (build_sets): one parent graph whose nodes ARE the batch's rows -- set t is one subgraph of the consecutive nodes [off_t, off_t + n_t), every edge
stays inside its set, so the induced edges are exactly the edges made here and every row's in-degree is the one chosen for it: 0, 1, 2 and >= 3 in fixed shares,
and in turn at the first row of every 128-row tile, the last row of every full tile and the last row of every short tile (degree_mix checks that)."""
import numpy as np
import torch

SELF, ZERO, MAXDEG = 0x40000000, 0x20000000, 2
ONE = int(np.float32(1.0).view(np.int32))
TILE = 128                                               # GM_GEMM_BM: rows of a GEMM tile; tiles never straddle two sets


# ---------------------------------------------------------------------------------------------------- graphs
def tile_spans(set_rows):
    """(first row, rows) of every GEMM tile of a batch with these set sizes"""
    out, r0 = [], 0
    for n in set_rows:
        for k in range(0, n, TILE):
            out.append((r0 + k, min(TILE, n - k)))
        r0 += n
    return out


def build_sets(set_rows, seed, weighted=False, shares=(0.15, 0.3, 0.3, 0.25)):
    """(nodes, src, dst, w or None): the graph of the module docstring.  Sources are distinct per row while the set has enough rows, parallel edges (and
    self-loops) otherwise; weights are fractional, 0.25 .. 1.75."""
    rng = np.random.default_rng(seed)
    rows = int(sum(set_rows))
    big = np.array([3, 4, 4, 4, 5, 8])
    cls = rng.choice(4, rows, p=shares)
    at = [0, 0, 0]
    for r0, n in tile_spans(set_rows):
        cls[r0] = at[0] % 4; at[0] += 1
    for r0, n in tile_spans(set_rows):                   # last rows after first rows: a one-row tile counts as a short tile's last row
        k = 1 if n == TILE else 2
        cls[r0 + n - 1] = at[k] % 4; at[k] += 1
    deg = np.where(cls < 3, cls, big[rng.integers(0, len(big), rows)])
    # sources of row r: d consecutive entries (from a random start, wrapping) of a random permutation of the set's rows
    n_set = np.asarray(set_rows, np.int64)
    set_idx = np.repeat(np.arange(len(set_rows)), n_set)
    r0_row, n_row = (np.cumsum(n_set) - n_set)[set_idx], n_set[set_idx]
    shuffled = np.argsort(set_idx + rng.random(rows), kind='stable')
    start = rng.integers(0, 1 << 30, rows) % n_row
    dst = np.repeat(np.arange(rows), deg)
    j = np.arange(len(dst)) - np.repeat(np.cumsum(deg) - deg, deg)
    src = shuffled[r0_row[dst] + (start[dst] + j) % n_row[dst]]
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    w = (0.25 + 1.5 * rng.random(len(src))).astype(np.float32) if weighted else None
    return rows, src, dst, w


def csr_of(rows, src, dst, w=None):
    """in-edge CSR (indptr, indices, weights) of an edge list, edges of a row in edge-id order"""
    order = np.argsort(dst, kind='stable')
    indptr = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=rows), out=indptr[1:])
    return indptr.astype(np.int32), src[order].astype(np.int32), None if w is None else w[order]


def norm_of(indptr, ew=None):
    """in_degree.clamp(1)^-0.5 in fp32 (weighted: the weighted in-degree) -- for the CPU tests; the GPU tests take the batch's own"""
    if ew is None:
        d = np.diff(indptr).astype(np.float64)
    else:
        d = np.add.reduceat(np.concatenate([ew.astype(np.float64), [0.0]]), indptr[:-1].astype(np.int64))
        d[np.diff(indptr) == 0] = 0.0
    return (1.0 / np.sqrt(np.maximum(d, 1.0))).astype(np.float32)


def degree_mix(indptr, set_rows):
    """{position: set of degree classes present} over the first row of every tile, the last row of every full tile and the last row of every short tile;
    classes 0, 1, 2 and 3 (three sources or more)"""
    d = np.minimum(np.diff(indptr), 3)
    out = {'first': set(), 'last_full': set(), 'last_short': set()}
    for r0, n in tile_spans(set_rows):
        out['first'].add(int(d[r0]))
        out['last_full' if n == TILE else 'last_short'].add(int(d[r0 + n - 1]))
    return out


def assert_degree_mix(indptr, set_rows):
    mix = degree_mix(indptr, set_rows)
    assert all(v == {0, 1, 2, 3} for v in mix.values()), mix


# ---------------------------------------------------------------------------------------------------- (a) tables
def tables(indptr, indices, norm, feat_row, ew=None):
    """(d_fuse2, d_fuse2_feat) as int32 [rows, 4] and (unfused_rows, unfused_edges)"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    norm, feat_row = np.asarray(norm, np.float32), np.asarray(feat_row, np.int64)
    rows = len(indptr) - 1
    d, p = np.diff(indptr), indptr[:-1]
    wt = norm[indices] if ew is None else np.asarray(ew, np.float32) * norm[indices]       # one fp32 product per edge
    assert wt.dtype == np.float32
    wt = wt.view(np.int32).astype(np.int64)
    E = max(len(indices), 1)
    ix = np.concatenate([indices, [0]]) if len(indices) == 0 else indices
    wx = np.concatenate([wt, [0]]) if len(wt) == 0 else wt
    p0, p1 = np.minimum(p, E - 1), np.minimum(p + 1, E - 1)
    one, two, many = d == 1, d == 2, d > MAXDEG
    r = np.arange(rows, dtype=np.int64)
    t = np.empty((rows, 4), np.int64)
    t[:] = [ZERO, ZERO, ONE, 0]                                                             # d == 0
    fused = one | two
    u0 = ix[p0]
    u1 = np.where(two, ix[p1], u0)
    t[fused, 0], t[fused, 1] = u0[fused], u1[fused]
    t[fused, 2] = wx[p0][fused]
    t[fused, 3] = np.where(two, wx[p1], 0)[fused]
    t[many, 0] = t[many, 1] = r[many] | SELF
    t[many, 2], t[many, 3] = ONE, 0
    tf = t.copy()
    tf[fused, 0], tf[fused, 1] = feat_row[u0[fused]], feat_row[u1[fused]]
    return t.astype(np.int32), tf.astype(np.int32), (int(many.sum()), int(d[many].sum()))


def dq_table(rows, centre_rows):
    """d_dq_tab as int32 [rows, 4]"""
    t = np.empty((rows, 4), np.int64)
    t[:] = [ZERO, ZERO, 0, 0]
    c = np.asarray(centre_rows, np.int64)
    t[c, 0], t[c, 1], t[c, 2], t[c, 3] = c | SELF, ZERO, ONE, 0
    return t.astype(np.int32)


def table_sources(tab):
    """rows of X that a table reads (bool over the largest index + 1 is the caller's business: returns the sorted unique indices) and the bool [rows] of
    the rows that read their own row of zside"""
    t = np.asarray(tab, np.int64)
    u = t[:, :2]
    plain = (u & (SELF | ZERO)) == 0
    return np.unique(u[plain]), ((u & SELF) != 0).any(1)


# ---------------------------------------------------------------------------------------------------- (b) rows, product
def form_rows(tab, x, zside):
    """fp64 Z [rows, K] and its condition scale |w0||X[u0]| + |w1||X[u1]| from a table (int32 [rows, 4], numpy or torch), X = x [*, >= K] and zside
    [rows, K].  Rows of x / zside the table does not name are never looked at (they may hold NaN)."""
    dev = zside.device
    t = torch.as_tensor(np.asarray(tab) if not torch.is_tensor(tab) else tab).to(dev)
    K = zside.shape[1]
    w = t[:, 2:].to(torch.int32).contiguous().view(torch.float32).double()
    z = torch.zeros(t.shape[0], K, dtype=torch.float64, device=dev)
    za = torch.zeros_like(z)
    for j in (0, 1):
        u = t[:, j].long()
        zero, own = (u & ZERO) != 0, (u & SELF) != 0
        idx = u & ~(SELF | ZERO)
        v = torch.zeros_like(z)
        plain = ~zero & ~own
        v[plain] = x[idx[plain], :K].double()
        v[own] = zside[idx[own], :K].double()
        z += w[:, j:j + 1] * v
        za += w[:, j:j + 1].abs() * v.abs()
    return z, za


def set_index(set_rows, device):
    return torch.repeat_interleave(torch.arange(len(set_rows), device=device), torch.tensor(list(set_rows), device=device))


def gemm(z, za, set_rows, W, s=None, bias=None, relu=False):
    """fp64 C = epi(s (Z @ W_set) + b_set) and its condition scale |s| (|Z| @ |W|) + |b|.  W: [T, K, N] or [1, K, N] (shared); bias: [T, N] or None"""
    dev = z.device
    Wd = W.double()
    if Wd.shape[0] == 1:
        c, sc = z @ Wd[0], za @ Wd[0].abs()
    else:
        c = torch.empty(z.shape[0], Wd.shape[2], dtype=torch.float64, device=dev)
        sc = torch.empty_like(c)
        r0 = 0
        for t, n in enumerate(set_rows):
            c[r0:r0 + n] = z[r0:r0 + n] @ Wd[t]
            sc[r0:r0 + n] = za[r0:r0 + n] @ Wd[t].abs()
            r0 += n
    if s is not None:
        c, sc = c * s.double()[:, None], sc * s.double().abs()[:, None]
    if bias is not None:
        b = bias.double()[set_index(set_rows, dev)]
        c, sc = c + b, sc + b.abs()
    if relu:
        c = c.clamp_min(0)
    return c, sc


# ---------------------------------------------------------------------------------------------------- (c) weight gradient
def wgrad(z, za, set_rows, G, s=None, keep=None):
    """fp64 dW [T, K, N], db [T, N] and their condition scales sum |s Z|^T |G0|, sum |G0|.  keep: bool [rows] (False: the row of G enters as zeros, whatever
    it holds) or None"""
    g = G.double()
    if keep is not None:
        g = torch.where(keep[:, None], g, torch.zeros_like(g))
    if s is not None:
        z, za = z * s.double()[:, None], za * s.double().abs()[:, None]
    dW, sW, db, sb = [], [], [], []
    r0 = 0
    for n in set_rows:
        zz, gg = z[r0:r0 + n], g[r0:r0 + n]
        dW.append(zz.T @ gg); sW.append(za[r0:r0 + n].T @ gg.abs())
        db.append(gg.sum(0)); sb.append(gg.abs().sum(0))
        r0 += n
    return torch.stack(dW), torch.stack(sW), torch.stack(db), torch.stack(sb)
