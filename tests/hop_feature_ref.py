"""Restatement of the hop-propagated node features (gm_store_propagate_build; THE definition is in include/gmeta_hip.h): the levels x_0 = X,
x_{t+1} = A^ x_t in float64 over a graph's in-edge CSR as the store holds it, the derived tolerance of an fp32 evaluation, the fp32 pair operations, and the
cases the tests share.  Nothing here looks at the device.

A graph is (ptr int64 [N + 1], idx int [nnz], w float32 [nnz] or None): row v lists the sources u of its in-edges in stored order (GraphStore.host_csr /
host_weights)."""
import numpy as np

f32, f64 = np.float32, np.float64
OPS = ('hadamard', 'abs_diff')
U = 2.0 ** -24                                                                 # unit roundoff of fp32


def entries(ptr, idx, w, self_loops):
    """(row, col, weight) of every entry of every EXTENDED row, rows ascending and each in row order: under `self_loops` the entry (v, 1.0) stands in front of
    row v.  Weights are the exact float64 values of the fp32 weights (1.0 on unweighted graphs)."""
    ptr = np.asarray(ptr, np.int64)
    N = len(ptr) - 1
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(ptr))
    col = np.asarray(idx, np.int64).reshape(-1)
    wt = np.ones(len(col), f64) if w is None else np.asarray(w, f32).astype(f64).reshape(-1)
    if self_loops:
        at = ptr[:-1] + np.arange(N)                                           # where row v's extra entry goes in the extended list
        row = np.insert(row, ptr[:-1], np.arange(N))
        col = np.insert(col, ptr[:-1], np.arange(N))
        wt = np.insert(wt, ptr[:-1], 1.0)
        assert (row[at] == np.arange(N)).all() and (col[at] == np.arange(N)).all()
    return N, row, col, wt


def norms(N, row, wt):
    d = np.bincount(row, weights=wt, minlength=N)
    return 1.0 / np.sqrt(np.where(d > 0, d, 1.0))


def row_sums(N, row, vals):
    """float64 [N, F]: vals [entries, F] summed per row (`row` ascending, as `entries` returns it); rows without entries give zeros."""
    out = np.zeros((N, vals.shape[1]), f64)
    n = np.bincount(row, minlength=N)
    if len(row):
        first = (np.cumsum(n) - n)[n > 0]
        out[n > 0] = np.add.reduceat(vals, first, axis=0)
    return out


def coefficients(ptr, idx, w, self_loops):
    """-> N, row, col, c: c = norm(v) * w_uv * norm(u) of every entry, exact float64"""
    N, row, col, wt = entries(ptr, idx, w, self_loops)
    nm = norms(N, row, wt)
    return N, row, col, nm[row] * wt * nm[col]


def levels(ptr, idx, w, X, hops, self_loops):
    """float64 [hops + 1, N, F]: the levels by the definition."""
    N, row, col, c = coefficients(ptr, idx, w, self_loops)
    x = np.asarray(X, f32).astype(f64)
    assert x.shape[0] == N
    out = [x]
    for _ in range(hops):
        out.append(row_sums(N, row, c[:, None] * out[-1][col]))
    return np.stack(out)


def dense_operator(ptr, idx, w, self_loops):
    """float64 [N, N]: A^ = diag(norm) (A + I) diag(norm) as a dense matrix, A[v, u] = the summed weight of the edges u -> v (a multigraph's copies add up)."""
    ptr = np.asarray(ptr, np.int64)
    N = len(ptr) - 1
    A = np.zeros((N, N), f64)
    wt = np.ones(len(idx), f64) if w is None else np.asarray(w, f32).astype(f64)
    np.add.at(A, (np.repeat(np.arange(N), np.diff(ptr)), np.asarray(idx, np.int64)), wt)
    if self_loops:
        A += np.eye(N)
    d = A.sum(1)
    nm = 1.0 / np.sqrt(np.where(d > 0, d, 1.0))
    return nm[:, None] * A * nm[None, :]


def gamma(k):
    return k * U / (1.0 - k * U)


def bound(ptr, idx, w, X, hops, self_loops):
    """float64 [hops + 1, N, F]: the tolerance of an fp32 evaluation of the definition in ANY order of a row's sum -- derived, not measured.  A running-error
    recursion: E_0 = 0 (level 0 is stored), E_{t+1}[v] = sum over the row's entries of |c_uv| (E_t[u] (1 + gamma) + gamma |x_t[u]|), c_uv the exact float64
    coefficient and gamma = gamma_k = k u / (1 - k u) with u = 2^-24 and k = 2 len(row v) + max row length + 8: the row's sum (len), the degree sum behind
    norm(v) (len) and behind norm(u) (at most the longest row), the three products w norm(u), c x, norm(v) S, and an inverse square root (a division and a
    root) in each of the two norms, with one to spare."""
    N, row, col, c = coefficients(ptr, idx, w, self_loops)
    length = np.bincount(row, minlength=N)
    g = gamma(2.0 * length + (length.max() if N else 0) + 8.0)[row][:, None]
    x = levels(ptr, idx, w, X, hops, self_loops)
    E = [np.zeros_like(x[0])]
    for t in range(hops):
        E.append(row_sums(N, row, np.abs(c)[:, None] * (E[-1][col] * (1.0 + g) + g * np.abs(x[t][col]))))
    return np.stack(E)


def levels_fp32(ptr, idx, w, X, hops, self_loops, order='forward', seed=0):
    """float32 [hops + 1, N, F]: a plain fp32 evaluation (degree sums, norms, one product per coefficient, multiply then add) with every row summed in
    forward, reversed or shuffled order -- what `bound` has to cover."""
    N, row, col, wt = entries(ptr, idx, w, self_loops)
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=N))])
    perm = []
    for v in range(N):
        e = np.arange(start[v], start[v + 1])
        perm.append(e if order == 'forward' else e[::-1] if order == 'reversed' else rng.permutation(e))
    wt32 = wt.astype(f32)
    d = np.zeros(N, f32)
    for v in range(N):
        for e in perm[v]:
            d[v] = f32(d[v] + wt32[e])
    nm = (f32(1.0) / np.sqrt(np.where(d > 0, d, f32(1.0)).astype(f32))).astype(f32)
    x = [np.asarray(X, f32)]
    for _ in range(hops):
        nxt = np.zeros_like(x[0])
        for v in range(N):
            acc = np.zeros(x[0].shape[1], f32)
            for e in perm[v]:
                acc = (acc + f32(wt32[e] * nm[col[e]]) * x[-1][col[e]]).astype(f32)
            nxt[v] = nm[v] * acc
        x.append(nxt)
    return np.stack(x)


def pair_features(rows_a, rows_b, op):
    """float32: the pair operation on two arrays of fp32 rows, ONE fp32 operation per entry: a * b ('hadamard') or |a - b| ('abs_diff')."""
    a, b = np.asarray(rows_a, f32), np.asarray(rows_b, f32)
    assert op in OPS
    return (a * b).astype(f32) if op == 'hadamard' else np.abs((a - b).astype(f32))


def csr(N, src, dst, w=None):
    """(ptr, idx, w) as GraphStore stores an edge list: by destination, a stable sort keeps the edge order inside a row."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.argsort(dst, kind='stable')
    ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int64)
    return ptr, src[order].astype(np.int32), None if w is None else np.asarray(w, f32)[order]


def small_case():
    """9 nodes: parallel edges (0 -> 1 three times), self loops (2, 5 twice), an isolated node (8), a node with out-edges only (7), weights that are small
    integers -> (N, src, dst, w)."""
    src = np.array([0, 0, 0, 1, 2, 2, 3, 4, 5, 5, 5, 6, 7, 7, 7, 3, 1, 6], np.int64)
    dst = np.array([1, 1, 1, 2, 2, 3, 4, 0, 5, 5, 6, 0, 0, 3, 6, 1, 4, 2], np.int64)
    w = np.array([1, 2, 1, 3, 1, 1, 2, 1, 1, 2, 1, 3, 1, 1, 2, 1, 1, 1], f32)
    return 9, src, dst, w


def hub_case():
    """401 nodes, directed: rows 0 and 1 with 600 in-entries each drawn with repetition (parallel copies inside a hub row), rows 2 .. 6 of exactly 0, 1, 7, 8, 9
    in-entries, a self loop on 9 (and whatever the hubs draw), node 400 isolated, a random body over 10 .. 399 -> (N, src, dst, w) with fp32 weights in
    [0.25, 4)."""
    rng = np.random.default_rng(77)
    N = 401
    bs, bd = rng.integers(7, 400, 1500), rng.integers(10, 400, 1500)
    s = [bs, rng.integers(0, 400, 600), rng.integers(0, 400, 600), [9]]
    d = [bd, np.zeros(600, np.int64), np.ones(600, np.int64), [9]]
    for v, n in ((3, 1), (4, 7), (5, 8), (6, 9)):
        s.append(rng.integers(7, 400, n)); d.append(np.full(n, v, np.int64))
    s, d = np.concatenate(s).astype(np.int64), np.concatenate(d).astype(np.int64)
    order = rng.permutation(len(s))
    s, d = s[order], d[order]
    w = np.exp2(rng.uniform(-2, 2, len(s))).astype(f32)
    indeg = np.bincount(d, minlength=N)
    assert indeg[:7].tolist() == [600, 600, 0, 1, 7, 8, 9] and indeg[400] == 0 and not (s == 400).any() and ((s == 9) & (d == 9)).any()
    assert len(set(s[d == 0].tolist())) < 600
    return N, s, d, w


def features(N, F, seed):
    """signed fp32 features [N, F] whose magnitudes span a few binades"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, F)) * np.exp2(rng.integers(-3, 4, (N, 1)))).astype(f32)
