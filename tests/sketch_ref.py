"""Restatement of the node-sketch definition of include/gmeta_hip.h (gm_store_sketch_build, gm_sketch_registers, gm_sketch_pair_counts), twice: by the
DEFINITION (the ball of every node by a plain breadth-first search, every node of the ball inserted) and by the RECURRENCE (element-wise max / min over the
node's own record of the level before and those of its neighbours).  Everything is an integer, so the GPU tests ask for equality.  The estimators' error
bounds of the tests are here too, so that the CPU and the GPU tests hold the same ones."""
import numpy as np

import distance_ref
import gmeta_oracle as orc

SALT_HLL, SALT_MH = 0x534B4831, 0x534B4D31
GOLDEN = 0x9E3779B9


def salts(seed, g):
    return int(orc.sample_salt(int(seed), int(g), SALT_HLL, 0)), int(orc.sample_salt(int(seed), int(g), SALT_MH, 0))


def hll_insert(nodes, s_h, p):
    """-> (register j, rho) of every node: h = lowbias32(z ^ s_h), j = h >> (32 - p), w = h << p, rho = clz32(w) + 1 or 33 - p for w == 0."""
    h = orc.lowbias32(np.asarray(nodes, np.uint32) ^ np.uint32(s_h)).astype(np.uint64)
    j = (h >> np.uint64(32 - p)).astype(np.int64)
    w = (h << np.uint64(p)) & np.uint64(0xFFFFFFFF)
    rho = np.array([33 - p if x == 0 else 32 - int(x).bit_length() + 1 for x in w.tolist()], np.uint8)
    return j, rho


def minhash(nodes, s_m, K):
    """uint32 [n, K]: mh_k(z) = lowbias32(lowbias32(z ^ s_m) + (k + 1) * 0x9E3779B9), wrap-around."""
    q = orc.lowbias32(np.asarray(nodes, np.uint32) ^ np.uint32(s_m)).astype(np.uint64)
    step = (np.arange(1, K + 1, dtype=np.uint64) * np.uint64(GOLDEN)) & np.uint64(0xFFFFFFFF)
    return orc.lowbias32(((q[:, None] + step[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32))


def level0(N, p, K, seed, g=0):
    """-> (R uint8 [N, 2^p], M uint32 [N, K]) of the balls {x}"""
    s_h, s_m = salts(seed, g)
    j, rho = hll_insert(np.arange(N), s_h, p)
    R = np.zeros((N, 1 << p), np.uint8)
    R[np.arange(N), j] = rho
    return R, minhash(np.arange(N), s_m, K)


def ball_distances(N, nb, nodes, H):
    """uint8 [len(nodes), N]: distance_ref.column of every node, searched to H: B_d(x) = { z : row[z] <= d }."""
    return np.stack([distance_ref.column(N, nb, int(x), -1, H) for x in nodes]) if len(nodes) else np.zeros((0, N), np.uint8)


def by_definition(N, nb, H, p, K, seed, g=0):
    """-> (R uint8 [H + 1, N, 2^p], M uint32 [H + 1, N, K]): for every node and level the ball by breadth-first search, every node of it inserted."""
    R0, M0 = level0(N, p, K, seed, g)
    R = np.zeros((H + 1, N, 1 << p), np.uint8)
    M = np.zeros((H + 1, N, K), np.uint32)
    for x in range(N):
        dist = distance_ref.column(N, nb, x, -1, H)
        for d in range(H + 1):
            ball = np.nonzero(dist <= d)[0]
            R[d, x] = R0[ball].max(0)
            M[d, x] = M0[ball].min(0)
    return R, M


def by_recurrence(N, nb, H, p, K, seed, g=0):
    """The same arrays level by level: the element-wise max / min over x's own record of the level before and those of G(x)."""
    R0, M0 = level0(N, p, K, seed, g)
    R, M = [R0], [M0]
    for d in range(1, H + 1):
        Rn, Mn = R[-1].copy(), M[-1].copy()
        for x in range(N):
            if nb[x]:
                z = np.fromiter(nb[x], np.int64, len(nb[x]))
                Rn[x] = np.maximum(Rn[x], R[-1][z].max(0))
                Mn[x] = np.minimum(Mn[x], M[-1][z].min(0))
        R.append(Rn); M.append(Mn)
    return np.stack(R), np.stack(M)


def zeros_zsum(reg):
    """(zero registers, sum of 2^(32 - register)) over the last axis of a register array, int64"""
    reg = np.asarray(reg, np.uint8)
    return (reg == 0).sum(-1).astype(np.int64), (np.int64(1) << (32 - reg.astype(np.int64))).sum(-1)


def pair_counts(R, M, pairs):
    """-> (counts int64 [n, H + 1, H + 1, 3], balls int64 [n, 2, H + 1, 2]) of the canonical pairs (u, v) = (min, max); a node outside the graph: zeros."""
    L, N = R.shape[0], R.shape[1]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    counts = np.zeros((len(pairs), L, L, 3), np.int64)
    balls = np.zeros((len(pairs), 2, L, 2), np.int64)
    for i, (a, b) in enumerate(pairs.tolist()):
        if not (0 <= a < N and 0 <= b < N):
            continue
        u, v = min(a, b), max(a, b)
        counts[i, :, :, 0] = (M[:, None, u, :] == M[None, :, v, :]).sum(-1)
        counts[i, :, :, 1], counts[i, :, :, 2] = zeros_zsum(np.maximum(R[:, None, u, :], R[None, :, v, :]))
        for side, x in enumerate((u, v)):
            balls[i, side, :, 0], balls[i, side, :, 1] = zeros_zsum(R[:, x, :])
    return counts, balls


def pair_counts_all(R, M):
    """pair_counts of EVERY pair of nodes at once -> (counts int64 [N, N, H + 1, H + 1, 3], balls int64 [N, H + 1, 2]): entry [x, y] is the row of the
    pair (x, y) in either orientation, balls[x] the ball entries of x.  The same numbers by other means, for the tests that take every ordered pair: the
    matches row by row; the histogram of U = max(R_a(u), R_b(v)) from products of indicator matrices -- |{ j : U[j] <= t }| = (R_a(u) <= t) . (R_b(v) <= t),
    0 / 1 sums of at most 2^10 terms, exact in float32 -- and zsum = sum over t of 2^(32 - t) |{ j : U[j] == t }|.  test_sketch_restatement.py holds it
    to pair_counts."""
    L, N, m = R.shape
    K = M.shape[2]
    lo = np.minimum.outer(np.arange(N), np.arange(N))
    hi = np.maximum.outer(np.arange(N), np.arange(N))
    canon = np.zeros((L, L, N, N, 3), np.int64)                                # [a, b, u, v]: level a of u against level b of v
    for a in range(L):
        for b in range(L):
            for u in range(N):
                canon[a, b, u, :, 0] = (M[a, u][None, :] == M[b]).sum(1)
    flat = R.reshape(L * N, m)
    below = np.zeros((L * N, L * N), np.int64)                                 # |{ j : U[j] <= t - 1 }|
    for t in range(int(R.max()) + 1):
        le = (flat <= t).astype(np.float32)
        upto = np.rint(le @ le.T).astype(np.int64)
        if t == 0:
            zeros = upto
            zsum = upto << 32
        else:
            zsum = zsum + ((upto - below) << (32 - t))
        below = upto
    assert (below == m).all()
    for a in range(L):
        for b in range(L):
            canon[a, b, :, :, 1] = zeros[a * N:(a + 1) * N, b * N:(b + 1) * N]
            canon[a, b, :, :, 2] = zsum[a * N:(a + 1) * N, b * N:(b + 1) * N]
    counts = np.ascontiguousarray(canon[:, :, lo, hi, :].transpose(2, 3, 0, 1, 4))
    balls = np.stack(zeros_zsum(R), -1).transpose(1, 0, 2)
    return counts, np.ascontiguousarray(balls)


# ---------------------------------------------------------------------------------------------------- the estimators' bounds (theory, not measurement)
def sigma(p):
    """the relative standard error of a HyperLogLog of 2^p registers"""
    return 1.04 / np.sqrt(float(1 << p))


def ball_bound(size, p):
    """|estimate - |B|| <= 5 sigma |B| + 1  (the + 1: two nodes colliding in one register of a three-node ball)"""
    return 5.0 * sigma(p) * np.asarray(size, np.float64) + 1.0


def intersection_bound(inter, union, p, K):
    """|estimate - I| <= 5 U sqrt(J (1 - J) / K + J^2 sigma^2) + 1, J = I / U: the MinHash's binomial deviation and the HyperLogLog's, five of them"""
    I, U = np.asarray(inter, np.float64), np.asarray(union, np.float64)
    J = I / U
    return 5.0 * U * np.sqrt(J * (1.0 - J) / float(K) + J * J * sigma(p) ** 2) + 1.0


def exact_cumulative(dist_u, dist_v, H):
    """From the two distance rows of a pair: (I [H + 1, H + 1] = |B_a(u) & B_b(v)|, U = the unions, su [H + 1] = |B_a(u)|, sv), int64"""
    bu = np.stack([dist_u <= a for a in range(H + 1)])
    bv = np.stack([dist_v <= b for b in range(H + 1)])
    inter = (bu[:, None, :] & bv[None, :, :]).sum(-1).astype(np.int64)
    su, sv = bu.sum(-1).astype(np.int64), bv.sum(-1).astype(np.int64)
    return inter, su[:, None] + sv[None, :] - inter, su, sv


def cumulate(P):
    """The tables [n, H + 2, H + 2] of the profile layout -> (C [n, H + 1, H + 1] cumulative intersections, su [n, H + 1], sv [n, H + 1] ball sizes)"""
    P = np.asarray(P)
    L = P.shape[1] - 1
    return P[:, :L, :L].cumsum(1).cumsum(2), P[:, :L, :].sum(2).cumsum(1), P[:, :, :L].sum(1).cumsum(1)


def random_case():
    """The fixed random graph of the accuracy checks: N = 2,000, 6,000 random edges (mean degree about 6), seed 222; 200 random pairs and 100 adjacent ones.
    -> (N, src, dst, pairs)"""
    N = 2000
    rng = np.random.default_rng(222)
    src, dst = rng.integers(0, N, 3 * N).astype(np.int64), rng.integers(0, N, 3 * N).astype(np.int64)
    some = rng.integers(0, N, (200, 2))
    e = rng.choice(np.nonzero(src != dst)[0], 100, replace=False)
    return N, src, dst, np.concatenate([some, np.stack([src[e], dst[e]], 1)])
