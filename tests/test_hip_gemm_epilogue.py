"""GPU (-m gpu): every kernel instantiation of the update GEMM (gm_launch_gemm_nn: the GraphConv forward of learner.py:36,47 and the backward's
dZ = norm (dQ W^T)) and every epilogue option it supports, against an fp64 reference on the same fp32 inputs, through the test-only export
gm_dense_gemm:

    C[r] = epi(s[r] (x[r] @ W_set(r)) + b_set(r)),   epi = ReLU (NaN kept), then the relu' mask (mask_h <= 0 or a clear mask_b bit: 0).

Every case asserts which instantiation ran (gm_dense_gemm's `launched`, KERNELS below) and that the profile category agrees with it (1 exact,
4 three-piece split, 6 two-piece split).  Outputs are pre-filled with sentinels (C and zero_out NaN, relu' bits 0xA5, amax padding words
0x5A5A5A5A): an element no kernel writes fails, and so does a write outside [0, N) of a row, outside the tile rows or to another set's slot.

Per-element bar of the exact-fp32 and three-piece kernels, derived, not fitted:  |C - ref| <= (C_DET + LAMBDA sqrt(K)) u scale,  u = 2^-24,
scale = |s| sum_k |x_k||w_k| + |b|.
  - C_DET = 10, the rounding that does not depend on K.  The epilogue forms v s + b in fp32: at most two roundings, each below u scale.  The
    three-piece kernel cuts each fp32 operand a into bf16 pieces by truncation, a = a_h + a_m + a_l exactly, |a_m| < 2^-7 |a|, |a_l| < 2^-15 |a|;
    the products of pieces are exact in fp32, and the three it drops (m l, l m, l l) are below (2^-22 + 2^-22 + 2^-30) |a||b| < 8u |a||b|.
  - the fp32 accumulation: the exact kernels' f32 MFMA is an fmaf chain, one rounding per k; the split kernels round at most six times per
    16-k chunk.  Every rounding is below u |partial sum| <= u sum |x||w|.  The worst case, K u, is far from what independent roundings make: by
    the probabilistic bound of Higham and Mary (SIAM J. Sci. Comput. 41, 2019) the error of a K-term sum stays below lambda sqrt(K) u sum|.|
    except with probability ~2K exp(-lambda^2 / 2); LAMBDA = 8 puts that below 10^-8 per element.
ReLU and the masks do not widen the bar: |relu(a) - relu(b)| <= |a - b|, and a masked element must be exactly 0 on both sides.
The two-piece kernel takes the comparative bars of test_hip_gemm_numerics.py instead (worst normalised error at most 2 max(exact kernel,
torch fp32) + 2^-22) and, with every other kernel, the exact-answer cases: every operand 1 + 2^-8 (bf16 pieces 1 and 2^-8, exact in fp16),
K in {32, 64}, s a power of two per set and b = -s K, so that C = s K (2^-7 + 2^-16) and every partial sum are exact in fp32 -- every kernel
must return it bitwise, and a dropped cross product shows as an error of at least 2^8 u of C.

Batches (thresholds from the device's CU count): `short`, sets of 1 .. 1000 rows (23 tiles: the half-tile split kernel, glds_small, WC = 1);
`capped`, ~4.5 tiles per CU in sets of 1 .. 2 tiles, so that the persistent split grid takes its capped size and every workgroup walks tiles
of several sets (glds<2>, glds<1>, WC = 2); the 286k-row arxiv batch (glds<4>, WC = 4), referenced on every 37th row of each set."""
import ctypes as C
import zlib

import pytest
import torch

from hip_util import arxiv_query_batch, Batch, n_cus, synthetic_batch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_DET, LAMBDA = 10, 8
GM_EINVAL = -1
BOUND_PAD = 64                                           # GM_BOUND_PAD: words between two sets' amax slots
SHORT_SETS = [1, 15, 16, 17, 31, 33, 127, 128, 129, 255, 257, 1000]
CAPPED_PATTERN = [100, 129, 256, 37, 200, 1, 128]        # 10 tiles

# the instantiations gm_dense_gemm can reach, by GM_GEMM_ID_* (gm_internal.h).  The fused feeders k_gemm_split_p<true, ...> (ids 40 .. 45)
# need the batch's aggregate tables: test_hip_fused_numerics.py launches them (gm_dense_fused_gemm) against fp64 and bitwise against this pass.
KERNELS = {1: 'glds<4>', 2: 'glds<2>', 3: 'glds<1>', 4: 'glds_small'}
for _wi, _wc in enumerate((1, 2, 4)):
    for _vec in (0, 1):
        for _tb in (0, 1):
            KERNELS[10 + 4 * _wi + 2 * _vec + _tb] = 'nn<%d,%d,%d>' % (_wc, _vec, _tb)
KERNELS.update({30: 'split<2,4,3>', 31: 'split<2,4,2>', 32: 'split<1,4,3>', 33: 'split<1,4,2>', 34: 'split<1,2,3>', 35: 'split<1,2,2>'})
ID = {v: k for k, v in KERNELS.items()}


def family(kid):
    return 'exact' if kid < 30 else ('split16' if kid % 2 else 'split')


CATEGORY = {'exact': 1, 'split': 4, 'split16': 6}


def _lib():
    from gmeta_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------------------- batches
@pytest.fixture(scope='module')
def short():
    b = synthetic_batch(SHORT_SETS, 5)
    assert 2 * b.n_tiles <= n_cus() and b.n_tiles < n_cus() // 4
    return b


@pytest.fixture(scope='module')
def capped():
    cus = n_cus()
    assert cus >= 128                                    # the split grid is capped only on parts of at least 128 CUs
    b = synthetic_batch(CAPPED_PATTERN * ((9 * cus) // 20), 8)
    assert 4 * cus < b.n_tiles <= 6 * cus and b.n_tiles < 1536
    return b


@pytest.fixture(scope='module')
def arxiv():
    Q, store = arxiv_query_batch(8)
    b = Batch(Q)
    b.store = store
    assert b.n_tiles >= max(1536, 6 * n_cus() + 1)
    return b


def ref_rows(b):
    """rows referenced in fp64: every 37th row of each set of the arxiv batch, every row of the others"""
    if b.rows < 200000:
        return torch.arange(b.rows, device='cuda')
    return torch.cat([torch.arange(b.so[t], b.so[t + 1], 37) for t in range(b.T)]).cuda()


# ---------------------------------------------------------------------------------------------------- the call
class Run:
    pass


def run(b, x, ldx, K, W, N, mode, trans=False, shared_w=False, ldc=None, s=None, s_keep=None, bias=None, bias_stride=0, relu=False,
        bits=False, mask_h=None, mask_b=None, zero=False, amax=False, expect_rc=0):
    """gm_dense_gemm into sentinel-filled outputs; returns them with the instantiation that ran"""
    L = _lib()
    lib = L.lib()
    ldc = ldc or N
    r = Run()
    r.ldc = ldc
    r.out = torch.full((b.rows, ldc), float('nan'), device='cuda')
    r.bits = torch.full((b.rows * ldc // 4,), 0xA5, dtype=torch.uint8, device='cuda') if bits else None
    r.zero = torch.full((b.rows, ldc), float('nan'), device='cuda') if zero else None
    r.slots = None
    if amax:
        r.slots = torch.full((b.T * BOUND_PAD,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        r.slots[::BOUND_PAD] = 0
    launched = C.c_int32(-1)
    w_stride = 0 if shared_w else K * N
    lib.gm_profile_enable(1)
    try:
        rc = lib.gm_dense_gemm(b.B.handle, L.ptr(x), ldx, K, L.ptr(W), w_stride, 1 if trans else 0, N, L.ptr(r.out), ldc, L.ptr(s), L.ptr(s_keep),
                               L.ptr(bias), bias_stride, 1 if relu else 0, L.ptr(r.bits), L.ptr(mask_h), L.ptr(mask_b), L.ptr(r.zero),
                               L.ptr(r.slots), mode, C.byref(launched), L.stream_ptr())
        torch.cuda.synchronize()
        if expect_rc:
            assert rc == expect_rc and launched.value == -1, (rc, launched.value)
            return None
        L.check(rc, 'gm_dense_gemm')
        ran = {}
        for name, cat in CATEGORY.items():
            ms, n, w = C.c_double(), C.c_int64(), C.c_int64()
            L.check(lib.gm_profile_read(cat, C.byref(ms), C.byref(n), C.byref(w)), 'gm_profile_read')
            if n.value:
                ran[name] = int(n.value)
    finally:
        lib.gm_profile_enable(0)
    r.kid = launched.value
    assert r.kid in KERNELS, r.kid
    r.kernel = KERNELS[r.kid]
    assert ran == {family(r.kid): 1}, (r.kernel, ran)
    return r


def unpack_bits(bits, rows, ldc):
    """packed relu' bits -> [rows, ldc] bool: byte (row ldc + col) / 4, bit col % 4"""
    by = bits.view(rows, ldc // 4).to(torch.int32)
    return torch.stack([(by >> k) & 1 for k in range(4)], 2).reshape(rows, ldc).bool()


# ---------------------------------------------------------------------------------------------------- inputs and reference
class Case:
    """inputs of one product: x (optionally one float past a 16-byte boundary), W per set ([K, N], or [N, K] when trans), a bias per set
    (optionally misaligned), a positive row scale over four octaves"""

    def __init__(self, b, K, N, seed, trans=False, shared_w=False, xoff=False, bias_off=False, ldx=None):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        self.b, self.K, self.N, self.trans, self.shared_w = b, K, N, trans, shared_w
        self.ldx = ldx or K
        perm = torch.randperm(b.rows, device='cuda', generator=gen)
        xs = torch.randn(b.rows * self.ldx + 4, device='cuda', generator=gen)
        self.x = xs[(1 if xoff else 0):(1 if xoff else 0) + b.rows * self.ldx].view(b.rows, self.ldx)
        self.x *= torch.logspace(-1, 1, b.rows, device='cuda')[perm][:, None]
        Tw = 1 if shared_w else b.T
        shape = (Tw, N, K) if trans else (Tw, K, N)
        self.W = torch.randn(shape, device='cuda', generator=gen) * (0.3 / K ** 0.5) * torch.logspace(-0.5, 0.5, Tw, device='cuda')[:, None, None]
        self.bias_stride = N + (0 if bias_off else 4)
        bb = torch.randn(b.T * self.bias_stride + 4, device='cuda', generator=gen)
        self.bias = bb[(1 if bias_off else 0):(1 if bias_off else 0) + b.T * self.bias_stride]
        self.s = torch.exp2(torch.rand(b.rows, device='cuda', generator=gen) * 4 - 2)
        keep = torch.ones(b.rows, dtype=torch.bool, device='cuda')
        keep[3::7] = False
        self.keep = keep
        self.s_keep = torch.where(keep, self.s, -self.s)
        m = torch.randn(b.rows * 300 + 4, device='cuda', generator=gen)
        self.mask_store = m

    def mask_h(self, ldc):
        """[rows, ldc] with exact +0.0, -0.0 and +- denormal entries"""
        m = self.mask_store[:self.b.rows * ldc].view(self.b.rows, ldc).clone()
        f = m.view(-1)
        f[::11] = 0.0
        f[5::11] = -0.0
        f[7::13] = 1e-40
        f[9::13] = -1e-40
        return m

    def w_of(self, t):
        W = self.W[0 if self.shared_w else t]
        return W.T if self.trans else W

    def args(self):
        return dict(trans=self.trans, shared_w=self.shared_w)

    def reference(self, rows, relu=False, bias=True, s=True):
        """fp64 pre-activation (s x W + b, then ReLU if asked), the condition scale and torch's fp32 value, on `rows` (sorted)"""
        b, K, N = self.b, self.K, self.N
        ref = torch.empty(len(rows), N, dtype=torch.float64, device='cuda')
        scale = torch.empty_like(ref)
        t32 = torch.empty(len(rows), N, device='cuda')
        so = torch.tensor(b.so, device='cuda')
        cut = torch.searchsorted(rows, so).tolist()
        for t in range(b.T):
            i0, i1 = cut[t], cut[t + 1]
            if i0 == i1:
                continue
            rr = rows[i0:i1]
            xr, W = self.x[rr, :K], self.w_of(t)
            sv = self.s[rr][:, None] if s else torch.ones(len(rr), 1, device='cuda')
            bv = self.bias[t * self.bias_stride:t * self.bias_stride + N] if bias else torch.zeros(N, device='cuda')
            ref[i0:i1] = (xr.double() @ W.double()) * sv.double() + bv.double()
            scale[i0:i1] = (xr.double().abs() @ W.double().abs()) * sv.double() + bv.double().abs()
            t32[i0:i1] = (xr @ W) * sv + bv
        if relu:
            ref = torch.where(ref < 0, torch.zeros_like(ref), ref)
            t32 = torch.where(t32 < 0, torch.zeros_like(t32), t32)
        return ref, scale, t32


def bar(K):
    return (C_DET + LAMBDA * K ** 0.5) * U


def nerr(out, ref, scale):
    """|out - ref| / scale; elements of zero scale must be exact (NaN fails every bar)"""
    e = (out.double() - ref).abs()
    return torch.where(scale > 0, e / scale.clamp_min(1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float('inf'))))


def note(key, v):
    print('worst normalised error', key, '%.3g' % v, '(%.2f u)' % (v / U))


def check_run(case, r, rows, relu, mask=None, stored=None, exact_out=None, what=''):
    """the epilogue checks of one run.  mask: [rows, ldc] bool of the relu' mask (None: no mask); stored: [rows] bool of the rows the kernel
    must store (None: all); exact_out: the exact kernel's C of the same case (two-piece kernels: the comparative bar)"""
    b, K, N, ldc = case.b, case.K, case.N, r.ldc
    what = (what, r.kernel, K, N, ldc)
    allrows = torch.ones(b.rows, dtype=torch.bool, device='cuda')
    stored = allrows if stored is None else stored
    # sentinels: columns [N, ldc) of every row, and every column of the rows not stored
    if ldc > N:
        ok = bool(torch.isnan(r.out[:, N:]).all())
        assert ok, what
    ok = bool(torch.isnan(r.out[~stored, :N]).all())
    assert ok, ('unstored rows were written',) + what
    C32 = r.out[:, :N]
    ok = not bool(torch.isnan(C32[stored]).any())
    assert ok, ('a stored element is NaN',) + what
    if mask is not None:
        ok = bool((C32[stored][~mask[stored][:, :N]] == 0).all())
        assert ok, ('masked element not zero',) + what
    # values
    ref, scale, t32 = case.reference(rows, relu=relu)
    if mask is not None:
        mk = mask[rows][:, :N]
        ref = torch.where(mk, ref, torch.zeros_like(ref)); t32 = torch.where(mk, t32, torch.zeros_like(t32))
    st = stored[rows]
    e = nerr(C32[rows][st], ref[st], scale[st])
    worst = float(e.max()) if e.numel() else 0.0
    if family(r.kid) == 'split16':
        ex = nerr(exact_out[rows][st, :N], ref[st], scale[st])
        et = nerr(t32[st], ref[st], scale[st])
        assert worst <= 2.0 * max(float(ex.max()), float(et.max())) + 2.0 ** -22, what + (worst, float(ex.max()), float(et.max()))
    else:
        assert worst <= bar(K), what + (worst / U, bar(K) / U)
    note(what, worst)
    # relu' bits: C > 0 of the kernel's own C on stored rows, the fp64 reference where |ref| exceeds the bar on every row, sentinels elsewhere
    if r.bits is not None:
        by = r.bits.view(b.rows, ldc // 4)
        if ldc > N:
            ok = bool((by[:, N // 4:] == 0xA5).all())
            assert ok, ('relu bits written past N',) + what
        bits = unpack_bits(r.bits, b.rows, ldc)[:, :N]
        ok = torch.equal(bits[stored], C32[stored] > 0)
        assert ok, ('relu bits != C > 0',) + what
        tol = bar(K) * scale if family(r.kid) != 'split16' else 2.0 ** -20 * scale
        sure = (ref.abs() > tol)
        ok = torch.equal(bits[rows][sure], (ref > 0)[sure])
        assert ok, ('relu bits disagree with the reference',) + what
    # zero fill: the whole [rows, ldc] buffer, +0.0
    if r.zero is not None:
        ok = bool((r.zero.view(torch.int32) == 0).all())
        assert ok, ('zero_out not filled',) + what
    # bounds: at least the largest |C| stored for the set, equal when every row is stored; padding and other slots untouched
    if r.slots is not None:
        sl = r.slots.view(b.T, BOUND_PAD)
        ok = bool((sl[:, 1:] == 0x5A5A5A5A).all())
        assert ok, ('amax padding written',) + what
        got = sl[:, 0].view(torch.float32).cpu()
        cut = torch.searchsorted(rows, torch.tensor(b.so, device='cuda')).tolist()
        tol = bar(K) if family(r.kid) != 'split16' else 2.0 ** -18
        for t in range(b.T):
            r0, r1 = b.so[t], b.so[t + 1]
            blk = C32[r0:r1][stored[r0:r1]]
            m = float(blk.abs().max()) if blk.numel() else 0.0
            if bool(stored[r0:r1].all()):
                assert float(got[t]) == m, ('amax slot', t) + what + (float(got[t]), m)
            else:
                # rows computed and not stored may count too: at most the largest |C| of any row of the set
                hi = float((ref[cut[t]:cut[t + 1]].abs() + tol * scale[cut[t]:cut[t + 1]]).max()) if cut[t + 1] > cut[t] else 0.0
                assert m <= float(got[t]) <= max(hi, m), ('amax slot', t) + what + (float(got[t]), m, hi)
    return worst


# ---------------------------------------------------------------------------------------------------- (1) exact kernels
# (kernel, batch, K, N, Case options, run options).  The DMA kernels need K % 16 == 0, 16-byte aligned x / W / bias and N a multiple of the
# column tile; anything else, a transposed W or mask_b takes k_gemm_nn<WC, VEC, TB>.  WC follows from the tile count and N (256 / 128 / 64-wide
# column tiles), VEC from the alignment of x and W and K, N >= 4.
# The DMA pipeline has three regimes, each run on every DMA instantiation: K = 32 (two chunks, no refill), K = 48 (three chunks, each LDS stage
# used once), K >= 64 (stages reused); one row per instantiation has ldc > N (zero_out by memset instead of in the epilogue).
EXACT_CASES = [
    ('glds<4>', 'arxiv', 64, 256, {}, {}),
    ('glds<4>', 'arxiv', 32, 256, {}, {'ldc': 260}),                       # zero_out by memset
    ('glds<4>', 'arxiv', 48, 256, {}, {}),
    ('glds<2>', 'capped', 128, 256, {}, {}),
    ('glds<2>', 'capped', 48, 128, {'shared_w': True}, {'ldc': 132}),
    ('glds<2>', 'capped', 32, 128, {}, {}),
    ('glds<2>', 'capped', 64, 128, {}, {}),
    ('glds<1>', 'capped', 64, 64, {}, {}),
    ('glds<1>', 'capped', 32, 64, {}, {'ldc': 68}),
    ('glds<1>', 'capped', 48, 64, {'shared_w': True}, {}),
    ('glds_small', 'short', 256, 256, {}, {}),
    ('glds_small', 'short', 32, 64, {}, {'ldc': 68}),
    ('glds_small', 'short', 48, 64, {}, {}),
    ('glds_small', 'short', 64, 64, {'shared_w': True}, {}),
    ('nn<4,1,0>', 'arxiv', 64, 256, {'bias_off': True}, {}),
    ('nn<4,1,1>', 'arxiv', 64, 256, {'trans': True}, {}),
    ('nn<4,0,0>', 'arxiv', 64, 256, {'xoff': True}, {}),
    ('nn<4,0,1>', 'arxiv', 50, 130, {'trans': True}, {}),
    ('nn<2,1,0>', 'capped', 20, 128, {}, {}),
    ('nn<2,1,1>', 'capped', 64, 256, {'trans': True, 'shared_w': True}, {'ldc': 260}),
    ('nn<2,0,0>', 'capped', 5, 130, {}, {}),
    ('nn<2,0,1>', 'capped', 50, 130, {'trans': True}, {}),
    ('nn<1,1,0>', 'short', 24, 24, {}, {}),
    ('nn<1,1,0>', 'short', 64, 64, {'bias_off': True}, {'ldc': 72}),
    ('nn<1,1,1>', 'short', 32, 64, {'trans': True}, {}),
    ('nn<1,0,0>', 'short', 1, 1, {}, {}),
    ('nn<1,0,0>', 'short', 5, 130, {}, {'ldc': 131}),
    ('nn<1,0,1>', 'short', 50, 24, {'trans': True}, {}),
    ('nn<1,0,1>', 'short', 64, 64, {'trans': True, 'xoff': True}, {}),
]


def _id(c):
    return '%s-%s-K%d-N%d%s' % (c[0], c[1], c[2], c[3], ''.join('-%s' % k for k in sorted(list(c[4]) + list(c[5]))))


@pytest.mark.parametrize('case', EXACT_CASES, ids=[_id(c) for c in EXACT_CASES])
def test_exact_kernels(request, case):
    """mode 0 with every option the kernel supports: s, a per-set bias, ReLU, relu' bits, mask_h (and, on k_gemm_nn's vector stores, a
    second run with mask_b taken from the first run's bits), zero_out.  The exact kernels store every row (they read s, not s_keep)."""
    kname, bname, K, N, copt, ropt = case
    b = request.getfixturevalue(bname)
    cs = Case(b, K, N, zlib.crc32(_id(case).encode()) % 10007, **copt)
    ldc = ropt.get('ldc', N)
    vec_c = N % 4 == 0 and ldc % 4 == 0
    rows = ref_rows(b)
    mh = cs.mask_h(ldc)
    r = run(b, cs.x, cs.ldx, K, cs.W, N, 0, ldc=ldc, s=cs.s, s_keep=cs.s_keep, bias=cs.bias, bias_stride=cs.bias_stride, relu=True, bits=vec_c,
            mask_h=mh, zero=True, **cs.args())
    assert r.kernel == kname, (r.kernel, kname)
    check_run(cs, r, rows, True, mask=mh.view(torch.int32) > 0, what='mask_h')
    if vec_c and kname.startswith('nn'):
        mb = r.bits.clone()
        r2 = run(b, cs.x, cs.ldx, K, cs.W, N, 0, ldc=ldc, s=cs.s, bias=cs.bias, bias_stride=cs.bias_stride, relu=True, bits=True, mask_b=mb,
                 **cs.args())
        assert r2.kernel == kname, (r2.kernel, kname)
        check_run(cs, r2, rows, True, mask=unpack_bits(mb, b.rows, ldc), what='mask_b')
    # no row scale (1), no ReLU, no outputs besides C
    r3 = run(b, cs.x, cs.ldx, K, cs.W, N, 0, ldc=ldc, bias=cs.bias, bias_stride=cs.bias_stride, **cs.args())
    assert r3.kernel == kname
    ref, scale, _ = cs.reference(rows, s=False)
    e = float(nerr(r3.out[rows][:, :N], ref, scale).max())
    assert e <= bar(K), (kname, e / U)
    if ldc > N:
        ok = bool(torch.isnan(r3.out[:, N:]).all())
        assert ok, kname


# ---------------------------------------------------------------------------------------------------- (2) split kernels
# (kernel, batch, K, N, Case options, ldc).  K = 32, 48: fewer chunks than the A feeders' prefetch depth, the tile constants go through
# stage_tile_consts; K >= 64: they ride with the A loads.
SPLIT_CASES = [
    ('split<1,4,3>', 'short', 32, 256, {}, 256),
    ('split<1,4,3>', 'short', 256, 256, {'trans': True}, 256),
    ('split<1,4,2>', 'short', 64, 256, {}, 256),
    ('split<1,4,2>', 'short', 48, 256, {'trans': True, 'shared_w': True}, 260),
    ('split<1,2,3>', 'short', 48, 128, {'trans': True}, 128),
    ('split<1,2,3>', 'capped', 32, 128, {}, 132),
    ('split<1,2,3>', 'capped', 256, 128, {'shared_w': True}, 128),
    ('split<1,2,2>', 'capped', 64, 128, {}, 128),
    ('split<1,2,2>', 'short', 32, 128, {'trans': True}, 128),
    ('split<2,4,3>', 'capped', 64, 256, {'trans': True}, 256),
    ('split<2,4,3>', 'capped', 48, 256, {}, 260),
    ('split<2,4,3>', 'arxiv', 256, 256, {'shared_w': True}, 256),
    ('split<2,4,2>', 'capped', 32, 256, {}, 256),
    ('split<2,4,2>', 'arxiv', 128, 256, {'trans': True}, 256),
]


@pytest.mark.parametrize('case', SPLIT_CASES, ids=['%s-%s-K%d-N%d-ldc%d%s' % (c[0], c[1], c[2], c[3], c[5], ''.join('-' + k for k in sorted(c[4])))
                                                   for c in SPLIT_CASES])
def test_split_kernels(request, case):
    """modes 1 / 2 with s, s_keep, a per-set bias, ReLU, relu' bits, zero_out (ldc == N only), amax_out (two-piece): the rows whose s_keep sign
    bit is set stay NaN, their relu' bits are still written; then the keep-only epilogue (no bits, no zero fill); a second run is bitwise
    identical."""
    kname, bname, K, N, copt, ldc = case
    b = request.getfixturevalue(bname)
    mode = 2 if kname.endswith(',2>') else 1
    cs = Case(b, K, N, zlib.crc32((kname + bname).encode()) % 10007 + K, **copt)
    rows = ref_rows(b)
    exact = None
    if mode == 2:
        exact = run(b, cs.x, cs.ldx, K, cs.W, N, 0, ldc=ldc, s=cs.s, bias=cs.bias, bias_stride=cs.bias_stride, relu=True, **cs.args()).out
    kw = dict(ldc=ldc, s=cs.s, s_keep=cs.s_keep, bias=cs.bias, bias_stride=cs.bias_stride, relu=True, bits=True, zero=ldc == N, amax=mode == 2)
    r = run(b, cs.x, cs.ldx, K, cs.W, N, mode, **kw, **cs.args())
    assert r.kernel == kname, (r.kernel, kname)
    check_run(cs, r, rows, True, stored=cs.keep, exact_out=exact, what='keep')
    r2 = run(b, cs.x, cs.ldx, K, cs.W, N, mode, **kw, **cs.args())
    ok = torch.equal(r2.out.view(torch.int32), r.out.view(torch.int32)) and torch.equal(r2.bits, r.bits)
    if mode == 2:
        ok = ok and torch.equal(r2.slots, r.slots)
    assert ok, ('second run differs',) + case[:4]
    # keep-only epilogue: unkept rows are neither stored nor counted
    r3 = run(b, cs.x, cs.ldx, K, cs.W, N, mode, ldc=ldc, s=cs.s, s_keep=cs.s_keep, bias=cs.bias, bias_stride=cs.bias_stride, relu=False,
             amax=mode == 2, **cs.args())
    assert r3.kernel == kname
    ex3 = None
    if mode == 2:
        ex3 = run(b, cs.x, cs.ldx, K, cs.W, N, 0, ldc=ldc, s=cs.s, bias=cs.bias, bias_stride=cs.bias_stride, **cs.args()).out
    check_run(cs, r3, rows, False, stored=cs.keep, exact_out=ex3, what='keep-only')
    # s without s_keep: every row stored
    r4 = run(b, cs.x, cs.ldx, K, cs.W, N, mode, ldc=ldc, s=cs.s, bias=cs.bias, bias_stride=cs.bias_stride, relu=True, amax=mode == 2, **cs.args())
    check_run(cs, r4, rows, True, exact_out=exact, what='all rows')


# ---------------------------------------------------------------------------------------------------- (3) exact answers, every kernel
# (kernel, batch, K, N, trans, xoff, bias_off, mode)
EXACT_ANSWER = [
    ('glds<4>', 'arxiv', 64, 256, False, False, False, 0), ('glds<2>', 'capped', 32, 256, False, False, False, 0),
    ('glds<1>', 'capped', 64, 64, False, False, False, 0), ('glds_small', 'short', 32, 64, False, False, False, 0),
] + [('nn<%d,%d,%d>' % (wc, vec, tb), bn, K, 256 if wc > 1 else 64, bool(tb), not vec, bool(vec and not tb), 0)
     for wc, bn, K in ((4, 'arxiv', 32), (2, 'capped', 64), (1, 'short', 32)) for vec in (0, 1) for tb in (0, 1)] + [
    ('split<2,4,3>', 'capped', 64, 256, False, False, False, 1), ('split<2,4,2>', 'capped', 32, 256, True, False, False, 2),
    ('split<1,4,3>', 'short', 32, 256, True, False, False, 1), ('split<1,4,2>', 'short', 64, 256, False, False, False, 2),
    ('split<1,2,3>', 'capped', 32, 128, False, False, False, 1), ('split<1,2,2>', 'short', 64, 128, False, False, False, 2),
]


@pytest.mark.parametrize('case', EXACT_ANSWER, ids=['%s-%s-K%d' % (c[0], c[1], c[2]) for c in EXACT_ANSWER])
def test_exact_answer(request, case):
    """every operand 1 + 2^-8, s = 2^(t % 5 - 2) on set t, b_t = -s_t K:  C = s_t K (2^-7 + 2^-16) bitwise, on every kernel"""
    kname, bname, K, N, trans, xoff, bias_off, mode = case
    b = request.getfixturevalue(bname)
    v = 1.0 + 2.0 ** -8
    xs = torch.full((b.rows * K + 4,), v, device='cuda')
    x = xs[(1 if xoff else 0):(1 if xoff else 0) + b.rows * K].view(b.rows, K)
    W = torch.full((b.T, N, K) if trans else (b.T, K, N), v, device='cuda')
    set_of = torch.repeat_interleave(torch.arange(b.T, device='cuda'), torch.tensor(b.set_rows, device='cuda'))
    st = torch.exp2((torch.arange(b.T, device='cuda') % 5 - 2).float())
    s = st[set_of].contiguous()
    bs = N + (0 if bias_off else 4)
    bb = torch.zeros(b.T * bs + 4, device='cuda')
    bias = bb[(1 if bias_off else 0):(1 if bias_off else 0) + b.T * bs]
    bias.view(b.T, bs)[:, :N] = (-st * K)[:, None]
    r = run(b, x, K, K, W, N, mode, trans=trans, s=s, s_keep=s if mode else None, bias=bias, bias_stride=bs, relu=True, amax=mode == 2)
    assert r.kernel == kname, (r.kernel, kname)
    want = (st * K * (2.0 ** -7 + 2.0 ** -16))[set_of]
    got = r.out
    bad = got != want[:, None]
    ok = not bool(bad.any())
    assert ok, (kname, int(bad.sum()), float((got - want[:, None]).abs().max() / want.min()) / U)


# ---------------------------------------------------------------------------------------------------- (4) NaN rows
NAN_CASES = [('glds_small', 'short', 64, 64, 0, False), ('glds<2>', 'capped', 64, 128, 0, False), ('nn<1,1,1>', 'short', 32, 64, 0, True),
             ('nn<2,0,0>', 'capped', 5, 130, 0, False), ('split<1,4,3>', 'short', 64, 256, 1, False), ('split<2,4,3>', 'capped', 128, 256, 1, True),
             ('split<1,2,3>', 'short', 32, 128, 1, False)]


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('case', NAN_CASES, ids=['%s-%s-K%d' % (c[0], c[1], c[2]) for c in NAN_CASES])
def test_nan_rows(request, case, relu):
    """a NaN in one element of a row of x makes the whole row NaN, with or without ReLU (torch.relu(NaN) is NaN); its relu' bits are 0; the
    other rows of the tile stay within their bar.  (The two-piece kernels send non-finite data to their violation path instead.)"""
    kname, bname, K, N, mode, trans = case
    b = request.getfixturevalue(bname)
    cs = Case(b, K, N, 77 + K + N, trans=trans)
    nan_rows = torch.tensor(sorted({b.so[t] for t in range(b.T)} | {b.so[t] + 5 for t in range(b.T) if b.set_rows[t] > 5}), device='cuda')
    cs.x[nan_rows, K // 2] = float('nan')
    bits = N % 4 == 0
    r = run(b, cs.x, cs.ldx, K, cs.W, N, mode, s=cs.s, s_keep=cs.s if mode else None, bias=cs.bias, bias_stride=cs.bias_stride, relu=relu,
            bits=bits, **cs.args())
    assert r.kernel == kname, (r.kernel, kname)
    ok = bool(torch.isnan(r.out[nan_rows]).all())
    assert ok, kname
    if bits:
        ok = not bool(unpack_bits(r.bits, b.rows, N)[nan_rows].any())
        assert ok, kname
    clean = torch.ones(b.rows, dtype=torch.bool, device='cuda')
    clean[nan_rows] = False
    rows = ref_rows(b)
    rows = rows[clean[rows]]
    ref, scale, _ = cs.reference(rows, relu=relu)
    e = float(nerr(r.out[rows][:, :N], ref, scale).max())
    assert e <= bar(K), (kname, e / U)


# ---------------------------------------------------------------------------------------------------- (5) mode -1, rejections, coverage
def test_library_choice(short, capped):
    """mode -1 takes the exact kernels below a quarter of the CUs' worth of tiles, the split kernel (if gm_set_gemm_mode says so) above; the
    result is bitwise that of the mode it picked"""
    L = _lib()
    for b, split_side in ((short, False), (capped, True)):
        cs = Case(b, 64, 256, 31)
        kw = dict(s=cs.s, bias=cs.bias, bias_stride=cs.bias_stride, relu=True)
        rm = run(b, cs.x, cs.ldx, 64, cs.W, 256, -1, **kw)
        split = split_side and L.lib().gm_get_gemm_mode() == 1
        rx = run(b, cs.x, cs.ldx, 64, cs.W, 256, 1 if split else 0, **kw)
        assert rm.kernel == rx.kernel == ('split<2,4,3>' if split else ('glds_small' if b is short else 'glds<2>')), (rm.kernel, rx.kernel)
        ok = torch.equal(rm.out.view(torch.int32), rx.out.view(torch.int32))
        assert ok, rm.kernel


def test_rejections(short):
    """GM_EINVAL, with no kernel launched: a split mode with mask_h or mask_b, N not 128 / 256, K not a multiple of 16 or below 32, zero_out with
    ldc != N; relu' bits or mask_b where the C stores are not vectorised"""
    b = short
    cs = Case(b, 64, 256, 3)
    mh = cs.mask_h(256)
    mb = torch.zeros(b.rows * 256 // 4, dtype=torch.uint8, device='cuda')
    for mode in (1, 2):
        run(b, cs.x, 64, 64, cs.W, 256, mode, mask_h=mh, expect_rc=GM_EINVAL)
        run(b, cs.x, 64, 64, cs.W, 256, mode, mask_b=mb, expect_rc=GM_EINVAL)
        run(b, cs.x, 64, 64, cs.W, 192, mode, expect_rc=GM_EINVAL)
        run(b, cs.x, 64, 40, cs.W, 256, mode, expect_rc=GM_EINVAL)
        run(b, cs.x, 64, 16, cs.W, 256, mode, expect_rc=GM_EINVAL)
        run(b, cs.x, 64, 64, cs.W, 256, mode, ldc=260, zero=True, expect_rc=GM_EINVAL)
    c2 = Case(b, 16, 130, 4)
    run(b, c2.x, 16, 16, c2.W, 130, 0, bits=False, mask_b=mb, expect_rc=GM_EINVAL)
    run(b, c2.x, 16, 16, c2.W, 128, 0, ldc=130, mask_b=mb, expect_rc=GM_EINVAL)
    L = _lib()
    bits = torch.zeros(b.rows * 130, dtype=torch.uint8, device='cuda')
    out = torch.zeros(b.rows * 130, device='cuda')
    launched = C.c_int32(-1)
    rc = L.lib().gm_dense_gemm(b.B.handle, L.ptr(c2.x), 16, 16, L.ptr(c2.W), 16 * 130, 0, 130, L.ptr(out), 130, None, None, None, 0, 1,
                               L.ptr(bits), None, None, None, None, 0, C.byref(launched), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == GM_EINVAL and launched.value == -1


def test_every_instantiation_is_asserted():
    """the cases above name every instantiation of the table at least once (each of them asserts `launched`)"""
    named = {c[0] for c in EXACT_CASES} | {c[0] for c in SPLIT_CASES} | {c[0] for c in EXACT_ANSWER} | {c[0] for c in NAN_CASES}
    assert named == set(ID), set(ID) ^ named
