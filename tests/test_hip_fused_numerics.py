"""GPU (-m gpu): the fused aggregate + GEMM feeders k_gemm_split_p<true, ...> (gemm_split.h) and the weight gradient that forms its A operand from the per-row
source table, k_wgrad_split<., ., 3, true, .> (gemm.hip), each launched on its own through the test-only exports gm_dense_fused_gemm / gm_dense_wgrad_fused and
held against the fp64 restatement of fused_ref.py on the same fp32 inputs:

    Z[r] = w0 X[u0] + w1 X[u1]   ({u0, u1, w0, w1} = the batch's table entry of row r; a SELF source is the row's own row of zside, a ZERO source 0)
    C[r] = relu(s[r] (Z[r] @ W_set(r)) + b_set(r)),      dW_t = sum_r (s[r] Z[r])^T G0[r],   db_t = sum_r G0[r].

(a) test_tables: gm_batch::d_fuse2, d_fuse2_feat, d_dq_tab and the two counts, bitwise fused_ref.tables / dq_table from the batch's own CSR, fp32 norm,
    feature rows and edge weights (w0 / w1 as bit patterns), on every batch.
(b) test_fused_gemm, against fp64.  Three-piece kernels, per element, derived, not fitted:   |C - ref| <= (C_DET + LAMBDA sqrt(K)) u scale,   u = 2^-24, LAMBDA = 8,
    C_DET = 12: the 10 of test_hip_gemm_epilogue.py (two epilogue roundings, the three dropped products of bf16 pieces) plus the two roundings of
    fmaf(x1, w1, fmaf(x0, w0, 0)), each below u (|w0 x0| + |w1 x1|) and passed through the product linearly;  scale = |s| sum_k (|w0||x0_k| + |w1||x1_k|)|W_k|
    + |b|, with |zside_k| in place of the formed row on SELF rows.  The reference takes the table's own fp32 w0 / w1, which (a) pins.  Two-piece kernels: the
    worst normalised error is at most 2 max(exact-fp32 kernel, torch fp32) + 2^-22, both measured in the same test over the stored Z.
(c) the same test: every output of the fused launch -- C, relu' bits, zero fill, amax slots -- equals, bit for bit, gm_dense_aggregate into a stored Z followed
    by gm_dense_gemm with the same number of pieces.  On `short` the unfused launch walks 64-row half tiles (ids 32 / 33) and the fused one whole tiles: an
    element's k-order is the same.
(d) the same test: zside is NaN on every row of at most two sources, x (or the store's feature table) NaN on every row that is no source of such a row; C and
    zero_out are pre-filled with NaN, relu' bits with 0xA5, amax padding with 0x5A5A5A5A.  Every stored output is finite; sentinels survive on the rows s_keep
    flags (gm_batch::d_norm_c, d_norm_src), in columns >= N and in the amax padding, and nowhere else.  A relu' bit is C > 0 of the kernel's own value and the
    sign of the reference wherever |ref| exceeds the bar (at most 0.1 % of the elements fall under it: asserted from the reference).
(e) test_exact_answers: integer x (|x| <= 8, zero at the rows whose norm is no power of two), small integer W, s and b powers of two: every partial sum is
    exact, every kernel returns the fp64 answer bitwise.  A dropped source, swapped w0 / w1 or another row's entry is an error of at least 1/2.
(f) test_table_wgrad: (K, N) in {128, 256}^2, with and without g_keep, against fp64 with the bar of test_hip_wgrad_numerics.py plus the same two roundings
    (c_t = 12 + 8 sqrt(n_t + 8) on every set, n_t the rows of the set that enter its sums -- with g_keep the rows it keeps; the comparative bar
    2 max(exact, torch) + 2^-23 on sums of more than 257 terms too), and bitwise against gm_dense_wgrad
    mode 1 (g_keep: gm_dense_wgrad_centre) over the stored Z.  A is NaN on every row the table forms, gx on every non-source row, and with g_keep G on every
    row it flags.  `chunks` has 160-row chunks and last chunks of 1, 15, 16, 17 and 129 rows, `short` 128-row chunks and last chunks of 1 .. 127 rows.
(g) test_refusals: GM_EINVAL with the outputs untouched.

Batches (fused_ref.build_sets; thresholds from the CU count, 256 on the MI355X); every one has rows of 0, 1, 2 and >= 3 sources at the first row of a tile, the
last row of a full tile and the last row of a short tile (asserted from the batch's CSR before anything is launched):
    short    sets of 1 .. 1000 rows, 21 tiles: the grid is the tile count, one tile per workgroup; short_w the same sets with edge weights
    capped   ~4.5 tiles per CU in sets of 1 .. 2 tiles: the grid is 3 x the capped grid, about half of the workgroups walk two tiles of different sets
    deep     ~9.4 tiles per CU, one small tile per set: every workgroup walks three or four tiles
    wide     ~16.3 tiles per CU in sets of a few rows (and eight of one or two full tiles): the mult_f = 2 grid, eight or nine tiles per workgroup
    chunks   116 sets of two 160-row weight-gradient chunks
Instantiations (GM_GEMM_ID_SPLIT(1, MI, WC, NP); 42 / 43, fused half tiles, do not exist and are never reported):
    40 split_p<true,2,4,3>   short K 64 / 256 (shared W, ldx > K, ldz > K), short_w K 128, table 1 F 64 / 128 / 62, capped K 64, deep K 64, wide K 64
    41 split_p<true,2,4,2>   short K 128, table 1 F 64, capped K 128, deep K 256 (shared W), wide K 128 (shared W)
    44 split_p<true,1,2,3>   short K 256, table 1 F 64, capped K 256 (shared W), wide K 64
    45 split_p<true,1,2,2>   short K 64, short_w K 64, table 1 F 128 / 62, capped K 128, deep K 128
    wgrad_split<KT,NT,3,true,DR>   every (KT, NT, DR) on `chunks`; <1,2,.,0> <2,1,.,1> short, <2,2,.,0> short_w, <1,1,.,1> <1,2,.,0> table 1
Measured on an MI355X (pytest -s prints every case's figures).  Two-piece comparison, worst over the 33 runs: fused 2.72e-07 against exact-fp32 3.57e-07 and torch
fp32 3.24e-07 (capped, K 128, N 256, every row stored); closest to its bar: fused 1.22e-07 against max(exact, torch) 9.48e-08, i.e. 1.29 x where the bar allows
2 x + 2^-22 (short, K 64, N 128, centre rows).  Three-piece kernels: at most 4.7 u of the 76 .. 140 u the bar allows; table-fed weight gradient: at most 9.0 u.
(c) held everywhere, half tiles included: no fused output differs from the unfused pass in a single bit.  A reference with w0 / w1 swapped fails 50 of the 60
tests of this file; one in which a single row of each batch, the first of a tile, takes its neighbour's table entry fails 40."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fused_ref as R
from hip_util import Batch, n_cus

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_DET, LAMBDA = 12, 8
GM_EINVAL = -1
BOUND_PAD = 64
SHORT_SETS = [1, 15, 16, 17, 127, 128, 129, 255, 257, 1000]
CAPPED_PATTERN = [100, 129, 256, 37, 200, 1, 128]        # 10 tiles
DEEP_PATTERN = [3, 20, 1, 64, 9, 128, 31, 16]            # one tile each
WIDE_PATTERN = [3, 7, 1, 12, 5, 9, 2, 16]
CHUNK_SETS = [289] * 100 + [161, 175, 176, 177] * 4      # 160-row chunks: last chunks of 129, 1, 15, 16, 17 rows
FUSED_IDS = {40: 'split_p<true,2,4,3>', 41: 'split_p<true,2,4,2>', 44: 'split_p<true,1,2,3>', 45: 'split_p<true,1,2,2>'}
NAN_BITS = 0x7FC00000


def _L():
    from gmeta_amd import _lib as L
    return L


def chunk_rows(set_rows, n_cu):
    """gm_wgrad_chunk_rows (gm_internal.h): rows per weight-gradient chunk"""
    total, mx = sum(set_rows), max(1, max(set_rows))

    def chunks_at(cr):
        return sum((n + cr - 1) // cr for n in set_rows)
    best, best_eff = 128, -1.0
    for rounds in (1, 2, 3, 4, 6, 8):
        cap = n_cu * rounds
        lo, hi = 1, (mx + 31) // 32
        if chunks_at(32 * hi) > cap:
            continue
        while lo < hi:
            mid = (lo + hi) // 2
            if chunks_at(32 * mid) <= cap:
                hi = mid
            else:
                lo = mid + 1
        cr = max(128, 32 * lo)
        c = chunks_at(cr)
        eff = total / (((c + n_cu - 1) // n_cu) * n_cu * cr)
        if eff > best_eff + 0.25:
            best_eff, best = eff, cr
    return best


def set_sizes(name):
    cus = n_cus()
    if name in ('short', 'short_w'):
        return list(SHORT_SETS)
    if name == 'capped':
        assert cus >= 128                                # the split grid is capped only on parts of at least 128 CUs
        return CAPPED_PATTERN * ((9 * cus) // 20)
    if name == 'deep':
        return DEEP_PATTERN * ((75 * cus) // 64)         # 9.4 tiles per CU
    if name == 'wide':
        return WIDE_PATTERN * (2 * cus + 8) + [128, 129] * 4
    assert name == 'chunks'
    return list(CHUNK_SETS)


# ---------------------------------------------------------------------------------------------------- batches
class Env:
    def __hash__(self):
        return id(self)

    def __eq__(self, other):
        return self is other


@functools.lru_cache(maxsize=None)
def env(name, F=8):
    """the batch `name` over a store whose features are F wide: built once per module.  Row r of set t is node r + 3 + 2 t of the one parent graph, so the
    feature-row table differs from the batch-row table.  The store's features are NaN on every node that is no source of a row of at most two sources."""
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    L = _L()
    e = Env()
    e.name, e.F, e.weighted = name, F, name.endswith('_w')
    set_rows = set_sizes(name)
    T = len(set_rows)
    rows, src, dst, w = R.build_sets(set_rows, 17 + len(name), e.weighted)
    set_idx = np.repeat(np.arange(T), set_rows)
    node = np.arange(rows) + 3 + 2 * set_idx
    n_nodes = rows + 3 + 2 * T
    deg = np.bincount(dst, minlength=rows)
    few = deg <= R.MAXDEG
    is_src = np.zeros(rows, bool)
    is_src[src[few[dst]]] = True                         # sources of the rows the fused kernels form themselves
    rng = np.random.default_rng(7)
    clean = (rng.standard_normal((n_nodes, F)) * np.logspace(-1, 1, n_nodes)[rng.permutation(n_nodes)][:, None]).astype(np.float32)
    poison = np.full_like(clean, np.nan)
    poison[node[is_src]] = clean[node[is_src]]
    graph = (n_nodes, node[src], node[dst]) + ((w,) if e.weighted else ())
    e.store = gmeta_amd.GraphStore([graph], [poison])
    so = np.concatenate([[0], np.cumsum(set_rows)])
    lists = [node[so[t]:so[t + 1]].astype(np.int32) for t in range(T)]
    seeds = np.array([(0, int(l[0]), -1) for l in lists], np.int32)
    e.B = SubgraphBatch.from_nodes(e.store, seeds, np.arange(T + 1), lists, False)
    b = e.b = Batch(e.B)
    assert b.set_rows == list(set_rows) and e.B.edges == len(src)
    e.rows, e.T, e.set_rows = rows, T, list(set_rows)
    # what the batch itself says: CSR, norm, feature rows, weights
    ip, ix = e.B.csr()
    assert np.array_equal(np.diff(ip), deg)
    R.assert_degree_mix(ip, set_rows)                    # the precondition of every test below
    feat_row = e.B._read(L.F_FEAT_ROW, rows, np.int32)
    assert np.array_equal(feat_row, node)
    norm = e.B._read(L.F_NORM, rows, np.float32)
    ew = e.B.edge_weights() if e.weighted else None
    e.t0, e.t1, e.counts = R.tables(ip, ix, norm, feat_row, ew)
    e.dq = R.dq_table(rows, so[:-1])                     # the centres: the first row of every set
    assert np.array_equal(R.table_sources(e.t0)[0], np.nonzero(is_src)[0])
    info = (C.c_int64 * 16)()
    L.check(L.lib().gm_dense_agg_info(e.B.handle, 0, info), 'gm_dense_agg_info')
    counts = (C.c_int64 * 2)()
    L.check(L.lib().gm_dense_fuse_counts(e.B.handle, counts), 'gm_dense_fuse_counts')
    e.got_counts = tuple(counts)
    e.feat_ld = int(info[14])
    assert int(info[13]) == F and e.feat_ld == (F if F % 4 == 0 else (F + 63) // 64 * 64)

    def pad(a):                                          # the store's table: feat_ld columns, the extra ones zero
        return torch.from_numpy(np.concatenate([a, np.zeros((n_nodes, e.feat_ld - F), np.float32)], 1)).cuda()
    e.feats_clean, e.feats_poison = pad(clean), pad(poison)
    e.feat_row = torch.from_numpy(node).cuda()
    e.few = torch.from_numpy(few).cuda()
    e.src_rows = torch.from_numpy(np.nonzero(is_src)[0]).cuda()
    e.keep = {}
    for key, field in (('c', L.F_NORM_CENTRE), ('src', L.F_NORM_SRC)):
        v = e.B._read(field, rows, np.float32)
        assert np.array_equal(np.abs(v), norm)
        e.keep[key] = (e.B.device_ptr(field), torch.from_numpy(~np.signbit(v)).cuda())
    centre = np.zeros(rows, bool)
    centre[so[:-1]] = True
    assert np.array_equal(e.keep['c'][1].cpu().numpy(), centre)
    assert np.array_equal(e.keep['src'][1].cpu().numpy(), np.bincount(src, minlength=rows) > 0)
    e.set_of = R.set_index(set_rows, 'cuda')
    return e


def test_batch_shapes():
    """the launch shapes the docstring names, from the launcher's own rules (gemm.hip, launch_gemm_nn)"""
    cus = n_cus()
    nt = {k: env(k).b.n_tiles for k in ('short', 'capped', 'deep', 'wide')}

    def cap(n):                                          # (two CUs per XCD, eight XCDs)
        return cus - 16 if 2 * cus < n <= 6 * cus and cus >= 128 else cus
    grid = {k: min(n, (2 if n >= 16 * cap(n) else 3) * cap(n)) for k, n in nt.items()}
    assert grid['short'] == nt['short'] == 21
    assert 4 * cus < nt['capped'] <= 6 * cus and grid['capped'] == 3 * (cus - 16) and grid['capped'] < nt['capped'] < 2 * grid['capped']
    assert nt['deep'] > 7 * cus and grid['deep'] == 3 * cus and nt['deep'] >= 3 * grid['deep']
    assert nt['wide'] >= 16 * cus and grid['wide'] == 2 * cus
    cr = chunk_rows(CHUNK_SETS, cus)
    assert cr == 160 and {n % cr for n in CHUNK_SETS} == {129, 1, 15, 16, 17}
    assert chunk_rows(SHORT_SETS, cus) == 128


# ---------------------------------------------------------------------------------------------------- (a) tables
def read_table(e, which):
    L = _L()
    t = torch.empty(e.rows, 4, dtype=torch.int32, device='cuda')
    L.check(L.lib().gm_dense_agg_table(e.B.handle, which, 0, L.ptr(t), e.rows, L.stream_ptr()), 'gm_dense_agg_table')
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize('name,F', [('short', 64), ('short', 62), ('short_w', 64), ('capped', 64), ('deep', 8), ('wide', 8), ('chunks', 8)])
def test_tables(name, F):
    e = env(name, F)
    for which, want in ((4, e.t0), (5, e.t1), (6, e.dq)):
        got = read_table(e, which)
        bad = np.nonzero((got != want).any(1))[0]
        assert len(bad) == 0, (name, which, bad[:5], got[bad[:5]], want[bad[:5]])
    assert e.got_counts == e.counts, (e.got_counts, e.counts)
    assert not np.array_equal(e.t0, e.t1)                # (feature rows are not batch rows here)
    # rows + 1 entries: refused
    L = _L()
    t = torch.empty(e.rows + 1, 4, dtype=torch.int32, device='cuda')
    assert L.lib().gm_dense_agg_table(e.B.handle, 4, 0, L.ptr(t), e.rows + 1, L.stream_ptr()) == GM_EINVAL


# ---------------------------------------------------------------------------------------------------- launches
def aggregate(e, x, ldx, K):
    """the unfused pass's Z: gm_dense_aggregate over the batch's per-edge norm table (gcn_forward's launch), every row stored"""
    L = _L()
    out = torch.full((e.rows, K), float('nan'), device='cuda')
    L.check(L.lib().gm_dense_aggregate(e.B.handle, 0, 0, L.ptr(x), ldx, K, 2, None, None, 0, None, 0, 0, None, None, None, 2, None, 0, 0, 0, 1, 0, 0,
                                       L.ptr(out), None, L.stream_ptr()), 'gm_dense_aggregate')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return out


class Run:
    pass


def _outputs(e, ldc, bits, zero, amax):
    r = Run()
    r.ldc = ldc
    r.out = torch.full((e.rows, ldc), float('nan'), device='cuda')
    r.bits = torch.full((e.rows * ldc // 4,), 0xA5, dtype=torch.uint8, device='cuda') if bits else None
    r.zero = torch.full((e.rows, ldc), float('nan'), device='cuda') if zero else None
    r.slots = None
    if amax:
        r.slots = torch.full((e.T * BOUND_PAD,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        r.slots[::BOUND_PAD] = 0
    return r


def _untouched(r):
    ok = bool((r.out.view(torch.int32) == NAN_BITS).all()) and (r.bits is None or bool((r.bits == 0xA5).all()))
    ok = ok and (r.zero is None or bool((r.zero.view(torch.int32) == NAN_BITS).all()))
    if r.slots is not None:
        sl = r.slots.view(-1, BOUND_PAD)
        ok = ok and bool((sl[:, 1:] == 0x5A5A5A5A).all()) and bool((sl[:, 0] == 0).all())
    return ok


def _profile(lib, L, cats):
    ran = {}
    for cat in cats:
        ms, n, w = C.c_double(), C.c_int64(), C.c_int64()
        L.check(lib.gm_profile_read(cat, C.byref(ms), C.byref(n), C.byref(w)), 'gm_profile_read')
        if n.value:
            ran[cat] = int(n.value)
    return ran


def run_gemm(e, cs, mode, fused, keep=None, relu=True, bits=True, zero=True, amax=None, ldc=None, expect_rc=0, zside=None, ldz=None, K=None):
    """gm_dense_fused_gemm (fused) or gm_dense_gemm over the stored Z, into sentinel-filled outputs, with s = the batch's norm"""
    L = _L()
    lib = L.lib()
    K, N = K or cs.K, cs.N
    ldc = ldc or N
    amax = (mode == 2) if amax is None else amax
    r = _outputs(e, ldc, bits, zero and ldc == N, amax)
    launched = C.c_int32(-1)
    w_stride = 0 if cs.shared_w else K * N
    s_keep = e.keep[keep][0] if keep else None
    lib.gm_profile_enable(1)
    try:
        if fused:
            zs = cs.zside if zside is None else zside
            rc = lib.gm_dense_fused_gemm(e.B.handle, cs.table, L.ptr(cs.x_poison) if cs.table == 0 else None, cs.ldx, K, L.ptr(zs), ldz or cs.ldz,
                                         L.ptr(cs.zfull), K, L.ptr(cs.W), w_stride, N, L.ptr(r.out), ldc, e.b.norm_ptr, s_keep, L.ptr(cs.bias),
                                         cs.bias_stride, 1 if relu else 0, L.ptr(r.bits), L.ptr(r.zero), L.ptr(r.slots), mode, C.byref(launched),
                                         L.stream_ptr())
        else:
            rc = lib.gm_dense_gemm(e.B.handle, L.ptr(cs.zfull), K, K, L.ptr(cs.W), w_stride, 0, N, L.ptr(r.out), ldc, e.b.norm_ptr, s_keep, L.ptr(cs.bias),
                                   cs.bias_stride, 1 if relu else 0, L.ptr(r.bits), None, None, L.ptr(r.zero), L.ptr(r.slots), mode, C.byref(launched),
                                   L.stream_ptr())
        torch.cuda.synchronize()
        if expect_rc:
            assert rc == expect_rc and launched.value == -1, (rc, launched.value)
            assert _untouched(r)
            return None
        L.check(rc, 'gm_dense_fused_gemm' if fused else 'gm_dense_gemm')
        ran = _profile(lib, L, (1, 4, 6))
    finally:
        lib.gm_profile_enable(0)
    r.kid = launched.value
    assert ran == {(1 if mode == 0 else 4 if mode == 1 else 6): 1}, (r.kid, ran)
    if fused:
        assert r.kid in FUSED_IDS and r.kid == 40 + (0 if N == 256 else 4) + (mode == 2), r.kid
    else:
        assert (30 <= r.kid <= 35 and r.kid % 2 == (mode == 2)) if mode else r.kid < 30, r.kid
    return r


def unpack_bits(bits, rows, ldc):
    """packed relu' bits -> [rows, ldc] bool: byte (row ldc + col) / 4, bit col % 4"""
    by = bits.view(rows, ldc // 4).to(torch.int32)
    return torch.stack([(by >> k) & 1 for k in range(4)], 2).reshape(rows, ldc).bool()


# ---------------------------------------------------------------------------------------------------- inputs
class Case:
    """operands of one fused product.  table 0: x [rows, ldx], rows over two decades, NaN (x_poison) on every row that is no source of a row of at most two
    sources; table 1: the store's feature table (NaN there since the store was made).  zfull: the stored Z of the unfused pass, from the clean operands;
    zside: its rows of three or more sources, NaN elsewhere and in the columns [K, ldz).  W per set (or shared), a bias per set."""

    def __init__(self, e, table, K, N, seed, shared_w=False, ldx=None, ldz=None, exact=False):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        self.e, self.table, self.K, self.N, self.shared_w = e, table, K, N, shared_w
        rows, T = e.rows, e.T
        if table == 0:
            self.ldx = ldx or K
            if exact:
                xc = torch.randint(-8, 9, (rows, self.ldx), device='cuda', generator=gen).float()
                pow2 = torch.from_numpy(np.frexp(e.b.norm.cpu().numpy())[0] == 0.5).cuda()
                xc[~pow2] = 0.0
            else:
                perm = torch.randperm(rows, device='cuda', generator=gen)
                xc = torch.randn(rows, self.ldx, device='cuda', generator=gen) * torch.logspace(-1, 1, rows, device='cuda')[perm][:, None]
            self.x_clean = xc
            self.x_poison = torch.full_like(xc, float('nan'))
            self.x_poison[e.src_rows] = xc[e.src_rows]
            self.tab = e.t0
            self.zfull = aggregate(e, xc, self.ldx, K)
        else:
            assert K == e.feat_ld and not exact
            self.ldx = K
            self.x_clean, self.x_poison = e.feats_clean, e.feats_poison
            self.tab = e.t1
            self.zfull = aggregate(e, e.feats_clean[e.feat_row].contiguous(), K, K)
        self.ldz = ldz or K
        self.zside = torch.full((rows, self.ldz), float('nan'), device='cuda')
        self.zside[~e.few, :K] = self.zfull[~e.few]
        Tw = 1 if shared_w else T
        self.bias_stride = N + 4
        if exact:
            self.W = torch.randint(-2, 3, (Tw, K, N), device='cuda', generator=gen).float()
            self.s_set = torch.exp2((torch.arange(T, device='cuda') % 5 - 2).float())
            self.bias = torch.zeros(T, self.bias_stride, device='cuda')
            self.bias[:, :N] = (4 * self.s_set)[:, None]
        else:
            self.W = torch.randn(Tw, K, N, device='cuda', generator=gen) * (0.3 / K ** 0.5) * torch.logspace(-0.5, 0.5, Tw, device='cuda')[:, None, None]
            self.bias = torch.randn(T, self.bias_stride, device='cuda', generator=gen)
        self._ref = {}

    def rows64(self):
        """fp64 Z and its condition scale from the table and the POISONED operands (finite: the table names no poisoned row)"""
        if 'z' not in self._ref:
            z, za = R.form_rows(self.tab, self.x_poison, self.zside[:, :self.K])
            assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(za).all())
            self._ref['z'] = (z, za)
        return self._ref['z']

    def reference(self, relu, s=None):
        key = ('c', relu, s is None)
        if key not in self._ref:
            z, za = self.rows64()
            self._ref[key] = R.gemm(z, za, self.e.set_rows, self.W, self.e.b.norm if s is None else s, self.bias[:, :self.N], relu)
        return self._ref[key]

    def torch32(self, relu):
        e = self.e
        W = self.W[0].expand(e.T, -1, -1) if self.shared_w else self.W
        out = torch.empty(e.rows, self.N, device='cuda')
        r0 = 0
        for t, n in enumerate(e.set_rows):
            out[r0:r0 + n] = (self.zfull[r0:r0 + n] @ W[t]) * e.b.norm[r0:r0 + n, None] + self.bias[t, :self.N]
            r0 += n
        return out.clamp_min(0) if relu else out


def bar(K):
    return (C_DET + LAMBDA * K ** 0.5) * U


def nerr(out, ref, scale):
    """|out - ref| / scale; elements of zero scale must be exact (NaN fails every bar)"""
    e = (out.double() - ref).abs()
    return torch.where(scale > 0, e / scale.clamp_min(1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float('inf'))))


def note(key, v):
    print('worst normalised error', key, '%.3g' % v, '(%.2f u)' % (v / U))


def check_fused(cs, r, mode, relu, stored=None, exact_out=None, what=''):
    """checks (b) and (d) of one fused run.  stored: bool [rows] of the rows the kernel stores (None: all)"""
    e, K, N, ldc = cs.e, cs.K, cs.N, r.ldc
    what = (what, e.name, FUSED_IDS[r.kid], K, N, ldc)
    stored = torch.ones(e.rows, dtype=torch.bool, device='cuda') if stored is None else stored
    if ldc > N:
        ok = bool((r.out[:, N:].view(torch.int32) == NAN_BITS).all())
        assert ok, ('columns >= N written',) + what
    ok = bool((r.out[~stored, :N].contiguous().view(torch.int32) == NAN_BITS).all())
    assert ok, ('unstored rows were written',) + what
    C32 = r.out[:, :N]
    ok = bool(torch.isfinite(C32[stored]).all())
    assert ok, ('a stored element is not finite',) + what
    ref, scale = cs.reference(relu)
    e_ = nerr(C32[stored], ref[stored], scale[stored])
    worst = float(e_.max()) if e_.numel() else 0.0
    if mode == 2:
        ex = float(nerr(exact_out[stored], ref[stored], scale[stored]).max())
        et = float(nerr(cs.torch32(relu)[stored], ref[stored], scale[stored]).max())
        print('two-piece comparison', what, 'fused %.3g exact %.3g torch %.3g' % (worst, ex, et))
        assert worst <= 2.0 * max(ex, et) + 2.0 ** -22, what + (worst, ex, et)
    else:
        assert worst <= bar(K), what + (worst / U, bar(K) / U)
    note(what, worst)
    if r.bits is not None:
        by = r.bits.view(e.rows, ldc // 4)
        if ldc > N:
            ok = bool((by[:, N // 4:] == 0xA5).all())
            assert ok, ('relu bits written past N',) + what
        bits = unpack_bits(r.bits, e.rows, ldc)[:, :N]
        ok = torch.equal(bits[stored], C32[stored] > 0)
        assert ok, ('relu bits != C > 0',) + what
        tol = (bar(K) if mode == 1 else 2.0 ** -20) * scale
        sure = ref.abs() > tol
        if mode == 1:                                    # how many elements the bits are not held to: from the reference alone (pre-activation)
            pre, _ = cs.reference(False)
            share = float((pre.abs() <= tol).double().mean())
            assert share <= 1e-3, ('elements under the bar',) + what + (share,)
            sure = pre.abs() > tol
            ok = torch.equal(bits[sure], (pre > 0)[sure])
        else:
            ok = torch.equal(bits[sure], (ref > 0)[sure])
        assert ok, ('relu bits disagree with the reference',) + what
    if r.zero is not None:
        ok = bool((r.zero.view(torch.int32) == 0).all())
        assert ok, ('zero_out not filled',) + what
    if r.slots is not None:
        sl = r.slots.view(e.T, BOUND_PAD)
        ok = bool((sl[:, 1:] == 0x5A5A5A5A).all())
        assert ok, ('amax padding written',) + what
        got = sl[:, 0].contiguous().view(torch.float32)
        neg = torch.full((e.rows,), -1.0, device='cuda')
        rowmax = torch.where(stored, C32.abs().amax(1), neg)
        m = torch.full((e.T,), -1.0, device='cuda').scatter_reduce(0, e.set_of, rowmax, 'amax').clamp_min(0)
        # rows computed and not stored may count too: at most the largest |C| of any row of the set
        hi = torch.zeros(e.T, dtype=torch.float64, device='cuda').scatter_reduce(0, e.set_of, (ref.abs() + 2.0 ** -18 * scale).amax(1), 'amax')
        allst = torch.ones(e.T, dtype=torch.int32, device='cuda').scatter_reduce(0, e.set_of, stored.int(), 'amin').bool()
        ok = bool(((got == m) | (~allst & (got >= m) & (got.double() <= torch.maximum(hi, m.double())))).all())
        assert ok, ('amax slots',) + what
    return worst


def same_bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---------------------------------------------------------------------------------------------------- (b) (c) (d) the fused GEMM
# (id, batch, F, table, K, N, shared W, ldx - K, ldz - K, ldc - N)
FUSED_CASES = [
    (40, 'short', 64, 0, 64, 256, False, 0, 0, 0),
    (40, 'short', 64, 0, 256, 256, True, 4, 8, 4),
    (41, 'short', 64, 0, 128, 256, False, 0, 0, 0),
    (44, 'short', 64, 0, 256, 128, False, 0, 4, 0),
    (45, 'short', 64, 0, 64, 128, False, 8, 0, 4),
    (40, 'short_w', 64, 0, 128, 256, False, 0, 0, 0),
    (45, 'short_w', 64, 0, 64, 128, False, 0, 0, 0),
    (40, 'short_w', 64, 1, 64, 256, False, 0, 0, 0),
    (41, 'short', 64, 1, 64, 256, False, 0, 0, 0),
    (44, 'short', 64, 1, 64, 128, True, 0, 0, 0),
    (40, 'short', 128, 1, 128, 256, False, 0, 0, 0),
    (45, 'short', 128, 1, 128, 128, False, 0, 0, 0),
    (40, 'short', 62, 1, 64, 256, False, 0, 0, 0),       # feat_ld 64 > feat_dim 62: the padded model's K
    (45, 'short', 62, 1, 64, 128, False, 0, 0, 0),
    (40, 'capped', 64, 0, 64, 256, False, 0, 0, 0),
    (41, 'capped', 64, 0, 128, 256, False, 0, 0, 0),
    (44, 'capped', 64, 0, 256, 128, True, 0, 0, 0),
    (45, 'capped', 64, 0, 128, 128, False, 0, 0, 0),
    (40, 'capped', 64, 1, 64, 256, False, 0, 0, 0),
    (40, 'deep', 8, 0, 64, 256, False, 0, 0, 0),
    (45, 'deep', 8, 0, 128, 128, False, 0, 0, 0),
    (41, 'deep', 8, 0, 256, 256, True, 0, 0, 0),
    (44, 'wide', 8, 0, 64, 128, False, 0, 0, 0),
    (41, 'wide', 8, 0, 128, 256, True, 0, 0, 0),
    (40, 'wide', 8, 0, 64, 256, True, 0, 0, 0),
]


def _cid(c):
    return '%d-%s-F%d-t%d-K%d-N%d%s%s' % (c[:6] + ('-shared' if c[6] else '', '-ld' if any(c[7:]) else ''))


@pytest.mark.parametrize('case', FUSED_CASES, ids=[_cid(c) for c in FUSED_CASES])
def test_fused_gemm(case):
    """checks (b), (c), (d) of the module docstring with the three epilogues production launches: s_keep = d_norm_c with relu' bits, zero fill and amax (the
    last layer of a differentiated pass), s_keep = d_norm_src with bits (a layer below it), every row stored without bits or ReLU"""
    kid, name, F, table, K, N, shared, dx, dz, dc = case
    e = env(name, F)
    mode = 2 if kid % 2 else 1
    cs = Case(e, table, K, N, 1000 + kid + 7 * K + N, shared_w=shared, ldx=K + dx, ldz=K + dz)
    exact = {}
    if mode == 2:
        for relu in (True, False):
            exact[relu] = run_gemm(e, cs, 0, False, relu=relu, bits=False, zero=False).out
    for what, kw, relu in (('keep c', dict(keep='c', ldc=N + dc), True), ('keep src', dict(keep='src', zero=False, ldc=N + dc), True),
                           ('all rows', dict(bits=False, zero=False), False)):
        r = run_gemm(e, cs, mode, True, relu=relu, **kw)
        assert r.kid == kid, (r.kid, kid)
        stored = e.keep[kw['keep']][1] if 'keep' in kw else None
        check_fused(cs, r, mode, relu, stored=stored, exact_out=exact.get(relu), what=what)
        # (c) bit for bit the unfused pass over the stored Z
        u = run_gemm(e, cs, mode, False, relu=relu, **kw)
        if name.startswith('short') and N == 256:        # the unfused launch of so few tiles walks half tiles: another tile shape, the same bits
            assert u.kid in (32, 33), u.kid
        for k in ('out', 'bits', 'zero', 'slots'):
            ok = same_bits(getattr(r, k), getattr(u, k))
            assert ok, ('fused != unfused', k, what, _cid(case), FUSED_IDS[r.kid], u.kid)
    r2 = run_gemm(e, cs, mode, True, relu=False, bits=False, zero=False)
    ok = same_bits(r2.out, r.out) and same_bits(r2.slots, r.slots)
    assert ok, ('second run differs', _cid(case))


# ---------------------------------------------------------------------------------------------------- (e) exact answers
EXACT_CASES = [(40, 'short', 64, 256), (41, 'short', 128, 256), (44, 'short', 256, 128), (45, 'short', 64, 128),
               (40, 'capped', 128, 256), (41, 'capped', 64, 256), (44, 'capped', 64, 128), (45, 'capped', 256, 128),
               (40, 'deep', 64, 256), (45, 'deep', 64, 128), (41, 'wide', 64, 256), (44, 'wide', 64, 128)]


@pytest.mark.parametrize('case', EXACT_CASES, ids=['%d-%s-K%d-N%d' % c for c in EXACT_CASES])
def test_exact_answers(case):
    """integer operands, power-of-two scales: the fp64 answer, bitwise.  (The batches are unweighted: a table weight is a norm, a power of two where the
    source has 0, 1 or 4 in-edges; x is zero at every other row.)"""
    kid, name, K, N = case
    e = env(name, 64 if name in ('short', 'capped') else 8)
    mode = 2 if kid % 2 else 1
    cs = Case(e, 0, K, N, 5000 + kid + K, shared_w=name in ('deep', 'wide'), exact=True)
    used = R.form_rows(e.t0, cs.x_poison, cs.zside)[1].abs().sum(1) > 0
    assert float(used.double().mean()) > 0.3             # (the zeros at the other norms leave most rows something to get wrong)
    s = cs.s_set[e.set_of].contiguous()
    L = _L()
    r = _outputs(e, N, False, False, mode == 2)
    launched = C.c_int32(-1)
    L.check(L.lib().gm_dense_fused_gemm(e.B.handle, 0, L.ptr(cs.x_poison), K, K, L.ptr(cs.zside), K, L.ptr(cs.zfull), K, L.ptr(cs.W),
                                        0 if cs.shared_w else K * N, N, L.ptr(r.out), N, L.ptr(s), None, L.ptr(cs.bias), cs.bias_stride, 1, None, None,
                                        L.ptr(r.slots), mode, C.byref(launched), L.stream_ptr()), 'gm_dense_fused_gemm')
    torch.cuda.synchronize()
    assert launched.value == kid
    ref, _ = cs.reference(True, s=s)
    want = ref.float()
    assert torch.equal(want.double(), ref)               # the answer is an fp32 number
    bad = r.out != want
    ok = not bool(bad.any())
    assert ok, (FUSED_IDS[kid], name, int(bad.sum()), float((r.out.double() - ref).abs().max()))


# ---------------------------------------------------------------------------------------------------- (f) the table-fed weight gradient
FAMILY = {2: 'exact', 5: 'split', 7: 'split16'}
# (batch, F, table, K, N, g_keep) -> k_wgrad_split<K / 128, N / 128, 3, true, g_keep>
WGRAD_CASES = [('chunks', 8, 0, K, N, keep) for K in (128, 256) for N in (128, 256) for keep in (False, True)] + [
    ('short', 64, 0, 128, 256, False), ('short', 64, 0, 256, 128, True), ('short_w', 64, 0, 256, 256, False),
    ('short', 128, 1, 128, 128, True), ('short', 128, 1, 128, 256, False)]


def run_wgrad(e, cs, G, which, keep, expect_rc=0, mode=1):
    """which: 'fused' gm_dense_wgrad_fused over the table, 'stored' gm_dense_wgrad mode 1 / gm_dense_wgrad_centre over the stored Z, 'exact' gm_dense_wgrad
    mode 0 over the stored Z.  NaN-filled outputs"""
    L = _L()
    lib = L.lib()
    K, N, T = cs.K, cs.N, e.T
    dW = torch.full((T, K, N), float('nan'), device='cuda')
    db = torch.full((T, N), float('nan'), device='cuda')
    lib.gm_profile_enable(1)
    try:
        if which == 'fused':
            rc = lib.gm_dense_wgrad_fused(e.B.handle, cs.table, L.ptr(cs.zside), cs.ldz, K, L.ptr(cs.x_poison) if cs.table == 0 else None, cs.ldx, L.ptr(G),
                                          N, N, e.b.norm_ptr, e.keep['c'][0] if keep else None, L.ptr(dW), K * N, L.ptr(db), N, mode, L.stream_ptr())
        elif which == 'stored' and keep:
            rc = lib.gm_dense_wgrad_centre(e.B.handle, L.ptr(cs.zfull), K, L.ptr(G), N, L.ptr(dW), K * N, L.ptr(db), N, L.stream_ptr())
        else:
            rc = lib.gm_dense_wgrad(e.B.handle, L.ptr(cs.zfull), K, K, L.ptr(G), N, N, e.b.norm_ptr, None, N, L.ptr(dW), K * N, L.ptr(db), N,
                                    1 if which == 'stored' else 0, None, None, 0, 0.0, None, None, None, L.stream_ptr())
        torch.cuda.synchronize()
        if expect_rc:
            assert rc == expect_rc, rc
            ok = bool((dW.view(torch.int32) == NAN_BITS).all()) and bool((db.view(torch.int32) == NAN_BITS).all())
            assert ok, 'a refused call wrote its outputs'
            return None
        L.check(rc, 'wgrad ' + which)
        ran = {FAMILY[c]: n for c, n in _profile(lib, L, FAMILY).items()}
    finally:
        lib.gm_profile_enable(0)
    assert ran == {('exact' if which == 'exact' else 'split'): 1}, (which, ran)
    return dW, db


@pytest.mark.parametrize('case', WGRAD_CASES, ids=['%s-F%d-t%d-K%d-N%d-%s' % (c[:5] + ('keep' if c[5] else 'all',)) for c in WGRAD_CASES])
def test_table_wgrad(case):
    name, F, table, K, N, keep = case
    e = env(name, F)
    cs = Case(e, table, K, N, 9000 + K + 3 * N + keep)
    gen = torch.Generator(device='cuda').manual_seed(77 + K + N)
    perm = torch.randperm(e.rows, device='cuda', generator=gen)
    G = torch.randn(e.rows, N, device='cuda', generator=gen) * torch.logspace(-1, 1, e.rows, device='cuda')[perm][:, None]
    kept = e.keep['c'][1] if keep else None
    G0 = G
    if keep:
        G0 = torch.where(kept[:, None], G, torch.zeros_like(G))
        G = torch.where(kept[:, None], G, torch.full_like(G, float('nan')))         # the rows nobody wrote
    dW, db = run_wgrad(e, cs, G, 'fused', keep)
    ok = bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    assert ok, case
    # against fp64: every set
    z, za = cs.rows64()
    rW, sW, rb, sb = R.wgrad(z, za, e.set_rows, G, e.b.norm, kept)
    # terms of a set's sums: its rows, with g_keep the rows it keeps (the others enter as exact zeros: adding them rounds nothing)
    terms = torch.zeros(e.T, dtype=torch.float64, device='cuda').index_add_(0, e.set_of, (kept if keep else torch.ones_like(e.few)).double())
    c_t = (C_DET + LAMBDA * (terms + 8).sqrt()) * U
    eW, eb = nerr(dW, rW, sW).amax((1, 2)), nerr(db, rb, sb).amax(1)
    ok = bool((eW <= c_t).all()) and bool((eb <= c_t).all())
    assert ok, (case, float((eW / c_t).max()), float((eb / c_t).max()))
    worst = float(eW.max())
    note(('wgrad',) + case, worst)
    # the comparative bar on the long sums (more than 257 terms: with g_keep a set's sum has one term, its centre row's, and the bar above is the test)
    big = [t for t in range(e.T) if float(terms[t]) > 257]
    xW, xb = run_wgrad(e, cs, G0, 'exact', False)
    tW = torch.stack([(cs.zfull[r0:r0 + n] * e.b.norm[r0:r0 + n, None]).T @ G0[r0:r0 + n] for r0, n in zip(e.b.so, e.set_rows)])
    if big:
        n_out, n_x, n_t = (float(nerr(v[big], rW[big], sW[big]).max()) for v in (dW, xW, tW))
        assert n_out <= 2.0 * max(n_x, n_t) + 2.0 ** -23, (case, n_out, n_x, n_t)
    # bitwise the split kernel over the stored Z
    uW, ub = run_wgrad(e, cs, G, 'stored', keep)
    ok = same_bits(dW, uW) and same_bits(db, ub)
    assert ok, ('table-fed != stored Z', case, float((dW - uW).abs().max()))
    d2, b2 = run_wgrad(e, cs, G, 'fused', keep)
    ok = same_bits(dW, d2) and same_bits(db, b2)
    assert ok, ('second run differs', case)


# ---------------------------------------------------------------------------------------------------- (g) refusals, coverage
def test_refusals():
    e = env('short', 64)
    cs = Case(e, 0, 128, 128, 3)
    G = torch.randn(e.rows, 128, device='cuda')
    run_wgrad(e, cs, G, 'fused', False, expect_rc=GM_EINVAL, mode=0)       # the exact kernels take no table
    run_wgrad(e, cs, G, 'fused', False, expect_rc=GM_EINVAL, mode=2)       # two-piece operands
    run_wgrad(e, cs, G, 'fused', True, expect_rc=GM_EINVAL, mode=2)
    for mode in (1, 2):
        run_gemm(e, cs, mode, True, K=32, expect_rc=GM_EINVAL)             # fewer chunks than the feeders' prefetch depth
        run_gemm(e, cs, mode, True, K=48, expect_rc=GM_EINVAL)
        zs = torch.full((e.rows * 128 + 4,), float('nan'), device='cuda')
        run_gemm(e, cs, mode, True, zside=zs[1:1 + e.rows * 128].view(e.rows, 128), expect_rc=GM_EINVAL)
        run_gemm(e, cs, mode, True, zside=torch.full((e.rows, 130), float('nan'), device='cuda'), ldz=130, expect_rc=GM_EINVAL)
    # mode 0 / -1: not a fused launch
    L = _L()
    r = _outputs(e, 128, False, False, False)
    for mode in (0, -1, 3):
        rc = L.lib().gm_dense_fused_gemm(e.B.handle, 0, L.ptr(cs.x_poison), 128, 128, L.ptr(cs.zside), 128, L.ptr(cs.zfull), 128, L.ptr(cs.W), 128 * 128, 128,
                                         L.ptr(r.out), 128, None, None, None, 0, 0, None, None, None, mode, None, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == GM_EINVAL and _untouched(r)


def test_every_instantiation_is_asserted():
    """the cases above name every fused GEMM id and every (KT, NT, DR) of the table-fed weight gradient (each of them asserts what ran)"""
    assert {c[0] for c in FUSED_CASES} == {c[0] for c in EXACT_CASES} == set(FUSED_IDS)
    assert {(c[3], c[4], c[5]) for c in WGRAD_CASES} == {(K, N, k) for K in (128, 256) for N in (128, 256) for k in (False, True)}
    for name in ('short', 'capped', 'deep', 'wide'):
        assert {c[0] for c in FUSED_CASES if c[1] == name} >= ({40, 41, 44, 45} if name in ('short', 'capped') else {40} if name == 'deep' else {41, 44})
