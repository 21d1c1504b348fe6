"""GPU (-m gpu): numerics of the weight-gradient kernels (the backward of learner.py:36,47 `torch.matmul(feat, weight)` + bias) against an fp64
reference on the same fp32 inputs, through the test-only export gm_dense_wgrad:  dW_t = sum_{rows r of set t} (s[r] x[r, :])^T g[r, :],
db_t = sum_r gb[r, :], over the batch's weight-gradient row chunks.  Every dispatch path is driven and every test asserts which kernel family ran
(profile categories 2 / 5 / 7: exact fp32 = k_wgrad_fast or k_wgrad, three-piece split-bf16 = k_wgrad_split<., ., 3>, two-piece split-fp16 =
k_wgrad_split<., ., 2>); which of k_wgrad_fast / k_wgrad runs follows from the shape and alignment of each case (gemm.hip, wgrad_fast_ok and the
<TK, TN> table).  Every output is pre-filled with NaN (planes with 0xFFFF), so an element no kernel writes fails.

Per-element bar of the short sets (at most 257 rows), set t of n_t rows:  |dW - ref| <= c_t u sum_r |s x_r| |g_r|  (u = 2^-24, the fp32 unit
roundoff), with c_t = C_DET + LAMBDA sqrt(n_t + 8) derived, not fitted:
  - C_DET = 10, the rounding that does not depend on the row count.  The split kernel cuts each fp32 operand a into bf16 pieces by truncation,
    a = a_h + a_m + a_l exactly, |a_m| < 2^-7 |a|, |a_l| < 2^-15 |a|; the three products it drops (m l, l m, l l) are below
    (2^-22 + 2^-22 + 2^-30) |a||b| < 8u |a||b|, the products of bf16 pieces are exact in fp32.  The operand s x is formed in fp32 (u), and on the
    exact kernels the product (s x) g too (u).
  - the fp32 accumulation: both kernel families round an output's accumulator at most once per row (six MFMAs per 16-row stage on the split
    kernel, one per two rows on the exact ones), the chunk reduction adds at most 8 more roundings; every rounding is below u |partial sum| <=
    u sum |s x||g|.  The worst case, (n + 8) u, is far from what independent roundings produce: by the probabilistic bound of Higham and Mary
    (SIAM J. Sci. Comput. 41, 2019) the error of an n-term sum stays below lambda sqrt(n) u sum|.| except with probability ~2n exp(-lambda^2 / 2).
    LAMBDA = 8 puts that below 10^-5 for all ~10^6 elements of a run.
  A fixed c of 8 - 16 does not hold: these inputs (rows over three decades) let a few rows dominate every sum, so later roundings act at the full
  scale, and the exact fp32 kernels themselves reach ~18u on 200-row sets.  The bar still catches a dropped m m product on the one-row set: that
  error is up to 2^-14 = 1024u there, against c = 34.  The split kernel's results on the short sets must also meet the comparative bar below.
The long sets (the full-size batch, the 1000-row set) take the comparative bars of the forward test (test_hip_gemm_numerics.py): the split kernel's
worst normalised error is at most 2 x max(exact kernel, torch fp32) + 2^-23, its rms error relative to each set's output scale at most 1.25 x the
exact kernel's, and a second run is bitwise identical."""
import ctypes as C

import numpy as np
import pytest
import torch

from hip_util import Batch, n_cus, synthetic_batch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_DET, LAMBDA = 10, 8
GM_EINVAL, GM_ERANGE = -1, -4
FAMILY = {2: 'exact', 5: 'split', 7: 'split16'}
SHORT_SETS = [1, 15, 16, 17, 31, 33, 127, 128, 129, 255, 257, 1000]


def _lib():
    from gmeta_amd import _lib as L
    return L


@pytest.fixture(scope='module')
def arxiv():
    from hip_util import arxiv_query_batch
    Q, store = arxiv_query_batch(8)
    b = Batch(Q)
    b.store = store
    assert b.n_chunks >= n_cus() // 4            # the library's own pick is the split kernel here
    return b


@pytest.fixture(scope='module')
def short():
    """12 sets straddling the 16-row stage and the 128-row chunk: 23 chunks, so k_wgrad_fast splits its tiles over 4 (256 x 256) or 2
    (128 x 256, 256 x 128) workgroups per chunk."""
    b = synthetic_batch(SHORT_SETS, 5)
    assert b.n_chunks < 48
    return b


@pytest.fixture(scope='module')
def many():
    """200 sets of 200 rows: one chunk each, 200 chunks -- k_wgrad_fast without the z-split."""
    b = synthetic_batch([200] * 200, 6)
    assert b.n_chunks >= 192
    return b


def run_wgrad(b, x, K, g, N, mode, s=True, gb=None, ldx=None, ldg=None, sgd=None):
    """gm_dense_wgrad into NaN-filled outputs.  Returns dW [T, K, N], db [T, N] and the kernel family that ran.  s=True: the batch's norm."""
    L = _lib()
    lib = L.lib()
    T = b.T
    dW = torch.full((T, K, N), float('nan'), device='cuda')
    db = torch.full((T, N), float('nan'), device='cuda')
    cur = nxt = wt = plf = pld = None
    pstride, lr = 0, 0.0
    if sgd is not None:
        cur, nxt, wt, plf, pld, pstride, lr = sgd
    lib.gm_profile_enable(1)
    try:
        L.check(lib.gm_dense_wgrad(b.B.handle, L.ptr(x), ldx or K, K, L.ptr(g), ldg or N, N,
                                   b.norm_ptr if s is True else L.ptr(s), L.ptr(gb), N, L.ptr(dW), K * N, L.ptr(db), N, mode,
                                   L.ptr(cur), L.ptr(nxt), pstride, lr, L.ptr(wt), L.ptr(plf), L.ptr(pld), L.stream_ptr()), 'gm_dense_wgrad')
        ran = {}
        for cat, name in FAMILY.items():
            ms, n, w = C.c_double(), C.c_int64(), C.c_int64()
            L.check(lib.gm_profile_read(cat, C.byref(ms), C.byref(n), C.byref(w)), 'gm_profile_read')
            if n.value:
                ran[name] = int(n.value)
    finally:
        lib.gm_profile_enable(0)
    torch.cuda.synchronize()
    assert len(ran) == 1 and list(ran.values()) == [1], ran
    return dW, db, next(iter(ran))


def reference(b, x, K, g, N, s=True, gb=None):
    """fp64 dW, db per set and their condition scales sum |s x| |g|, sum |gb|; plus torch's fp32 product for the comparative bars."""
    sv = b.norm if s is True else (s if s is not None else torch.ones(b.rows, device='cuda'))
    gbv = g if gb is None else gb
    out = {k: [] for k in ('dW', 'sW', 'db', 'sb', 'tW', 'tb')}
    for t in range(b.T):
        r0, r1 = b.so[t], b.so[t + 1]
        a = x[r0:r1, :K].double() * sv[r0:r1, None].double()
        gg = g[r0:r1, :N].double()
        out['dW'].append(a.T @ gg); out['sW'].append(a.abs().T @ gg.abs())
        out['db'].append(gbv[r0:r1, :N].double().sum(0)); out['sb'].append(gbv[r0:r1, :N].double().abs().sum(0))
        af = x[r0:r1, :K] * sv[r0:r1, None]
        out['tW'].append(af.T @ g[r0:r1, :N]); out['tb'].append(gbv[r0:r1, :N].sum(0))
    return {k: torch.stack(v) for k, v in out.items()}


def nerr(out, ref, scale):
    """|out - ref| / scale, elements of zero scale must be exact (NaN stays NaN and fails every bar)."""
    e = (out.double() - ref).abs()
    return torch.where(scale > 0, e / scale.clamp_min(1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float('inf'))))


def rms_rel(out, ref):
    """rms error relative to each set's output scale (rms of the set's reference)."""
    dims = tuple(range(1, ref.dim()))
    rs = ref.pow(2).mean(dims, keepdim=True).sqrt().clamp_min(1e-300)
    return float((((out.double() - ref) / rs) ** 2).mean().sqrt())


def assert_elementwise(out, ref, scale, b, sets, what):
    """the per-element bar of the module docstring on the given sets; returns the worst error in units of u"""
    worst = 0.0
    for t in sets:
        e = float(nerr(out[t], ref[t], scale[t]).max())
        c = C_DET + LAMBDA * (b.set_rows[t] + 8) ** 0.5
        assert e <= c * U, (what, b.set_rows[t], e / U, c)
        worst = max(worst, e)
    return worst


def assert_comparative(out, ref, scale, exact, torch32, what, rms=True):
    """the comparative bars of the full-size launches (module docstring); exact=None: the exact kernel itself, against torch fp32"""
    n_out = float(nerr(out, ref, scale).max())
    n_t = float(nerr(torch32, ref, scale).max())
    n_x = float(nerr(exact, ref, scale).max()) if exact is not None else 0.0
    assert n_out <= 2.0 * max(n_x, n_t) + 2.0 ** -23, (what, n_out, n_x, n_t)
    if exact is not None and rms:
        assert rms_rel(out, ref) <= 1.25 * rms_rel(exact, ref), (what, rms_rel(out, ref), rms_rel(exact, ref))
    return n_out


def inputs(b, K, N, seed, ldx=None, ldg=None):
    """x rows over three decades with exact zeros (as the forward test), g rows over two"""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    ldx, ldg = ldx or K, ldg or N
    perm = torch.randperm(b.rows, device='cuda', generator=gen)
    x = torch.randn(b.rows, ldx, device='cuda', generator=gen) * torch.logspace(-2, 1, b.rows, device='cuda')[perm][:, None]
    x[::97, ::5] = 0.0
    g = torch.randn(b.rows, ldg, device='cuda', generator=gen) * torch.logspace(-1, 1, b.rows, device='cuda')[perm.flip(0)][:, None]
    return x, g


def note(key, v):
    """the worst normalised error of a case, printed (pytest -s): the baseline of the next change to these kernels"""
    print('worst normalised error', key, '%.3g' % v, '(%.2f u)' % (v / U))


# ---------------------------------------------------------------------------------------------------- (a) full size, (f) mode -1 there
@pytest.mark.parametrize('K,N', [(256, 256), (128, 256), (256, 128), (128, 128)])
def test_full_size_split_is_as_accurate_as_fp32(arxiv, K, N):
    """the arxiv query batch (~286k rows, 8 sets): three-piece split against the exact kernel and torch fp32; mode -1 (what gm_meta_step runs,
    with the batch's norm as the row scale) takes the split kernel here and gives the same bits as mode 1."""
    b = arxiv
    x, g = inputs(b, K, N, K + 7 * N)
    dW0, db0, f0 = run_wgrad(b, x, K, g, N, 0)
    dW1, db1, f1 = run_wgrad(b, x, K, g, N, 1)
    assert (f0, f1) == ('exact', 'split')
    r = reference(b, x, K, g, N)
    note(('full', K, N, 0), float(nerr(dW0, r['dW'], r['sW']).max()))
    note(('full', K, N, 1), assert_comparative(dW1, r['dW'], r['sW'], dW0, r['tW'], 'dW'))
    assert_comparative(db1, r['db'], r['sb'], db0, r['tb'], 'db')
    dW2, db2, f2 = run_wgrad(b, x, K, g, N, 1)
    assert f2 == 'split' and torch.equal(dW2, dW1) and torch.equal(db2, db1)
    dWm, dbm, fm = run_wgrad(b, x, K, g, N, -1)
    assert fm == ('split' if _lib().lib().gm_get_gemm_mode() == 1 else 'exact')
    assert torch.equal(dWm, dW1 if fm == 'split' else dW0) and torch.equal(dbm, db1 if fm == 'split' else db0)


# ---------------------------------------------------------------------------------------------------- (b) short sets and tails, (f) there
@pytest.mark.parametrize('K,N', [(256, 256), (128, 256), (256, 128), (128, 128)])
def test_short_sets_and_tails(short, K, N):
    """sets of 1 .. 257 rows (and one of 1000) on the split kernel, forced (the batch has far fewer chunks than the library's threshold), and on
    the exact kernel (k_wgrad_fast: K, N multiples of 32, aligned).  Mode -1 picks the exact kernel at this launch size."""
    b = short
    x, g = inputs(b, K, N, 100 + K + N)
    r = reference(b, x, K, g, N)
    small = [t for t in range(b.T) if b.set_rows[t] <= 257]
    big = [t for t in range(b.T) if b.set_rows[t] > 257]
    dW0, db0, f0 = run_wgrad(b, x, K, g, N, 0)
    dW1, db1, f1 = run_wgrad(b, x, K, g, N, 1)
    assert (f0, f1) == ('exact', 'split')
    for dW, db, m in ((dW0, db0, 0), (dW1, db1, 1)):
        note(('short', K, N, m), assert_elementwise(dW, r['dW'], r['sW'], b, small, ('dW', m)))
        assert_elementwise(db, r['db'], r['sb'], b, small, ('db', m))
    assert_comparative(dW1[small], r['dW'][small], r['sW'][small], dW0[small], r['tW'][small], 'dW short split', rms=False)
    assert_comparative(dW0[big], r['dW'][big], r['sW'][big], None, r['tW'][big], 'dW 1000 exact')
    assert_comparative(dW1[big], r['dW'][big], r['sW'][big], dW0[big], r['tW'][big], 'dW 1000 split')
    assert_comparative(db1[big], r['db'][big], r['sb'][big], db0[big], r['tb'][big], 'db 1000 split')
    dW2, db2, _ = run_wgrad(b, x, K, g, N, 1)
    assert torch.equal(dW2, dW1) and torch.equal(db2, db1)
    dWm, dbm, fm = run_wgrad(b, x, K, g, N, -1)
    assert fm == 'exact' and torch.equal(dWm, dW0) and torch.equal(dbm, db0)


# ---------------------------------------------------------------------------------------------------- (c) exact-fp32 dispatch coverage
FAST_SHAPES = [(32, 32), (64, 128), (128, 64), (256, 256), (32, 256), (128, 128), (256, 128)]          # k_wgrad_fast's <TK, TN> table
GENERIC_SHAPES = [(1, 64), (5, 128), (24, 24), (50, 100), (96, 300), (100, 50), (300, 5), (512, 96), (64, 512), (512, 512), (64, 1)]
WIDE_SHAPES = [(2048, 2048), (2048, 1), (1, 2048), (2048, 64)]       # k_wgrad at its smallest stage (RK = 2), up to 64 z-groups


def _exact_case(b, K, N, seed, **kw):
    x, g = inputs(b, K, N, seed, kw.get('ldx'), kw.get('ldg'))
    gb = kw.get('gb')
    r = reference(b, x, K, g, N, gb=gb)
    dW, db, fam = run_wgrad(b, x, K, g, N, 0, gb=gb, ldx=kw.get('ldx'), ldg=kw.get('ldg'))
    assert fam == 'exact'
    small = [t for t in range(b.T) if b.set_rows[t] <= 257]
    big = [t for t in range(b.T) if b.set_rows[t] > 257]
    worst = assert_elementwise(dW, r['dW'], r['sW'], b, small, ('dW', K, N))
    assert_elementwise(db, r['db'], r['sb'], b, small, ('db', K, N))
    if big:
        assert_comparative(dW[big], r['dW'][big], r['sW'][big], None, r['tW'][big], 'dW 1000')
        assert_comparative(db[big], r['db'][big], r['sb'][big], None, r['tb'][big], 'db 1000')
    return worst


@pytest.mark.parametrize('K,N', FAST_SHAPES + GENERIC_SHAPES)
@pytest.mark.parametrize('which', ['short', 'many'])
def test_exact_kernels(request, which, K, N):
    """k_wgrad_fast (its table) and k_wgrad (every other width, vectorised or not) on a few-chunk batch (z-split 4 / 2 where the tile grid
    allows) and a many-chunk one (no z-split)"""
    b = request.getfixturevalue(which)
    note(('exact', which, K, N), _exact_case(b, K, N, 300 + K * 7 + N))


@pytest.mark.parametrize('K,N', WIDE_SHAPES)
def test_exact_kernels_widest_layers(short, K, N):
    """the widest layers gm_make_layout accepts: k_wgrad with RK = 2 and the bias sums at their 2048-column limit"""
    note(('wide', K, N), _exact_case(short, K, N, 400 + K + N))


def test_exact_kernels_misaligned_and_strided(short):
    """an x that is not 16-byte aligned, an ldx that is not a multiple of 4, a separate gb: each rules out k_wgrad_fast (and the split
    kernel), k_wgrad reads element-wise (not vectorised) / sums gb for db"""
    b = short
    K = N = 128
    # x one float past an aligned allocation
    xs = torch.randn(b.rows * K + 4, device='cuda')
    x = xs[1:1 + b.rows * K].view(b.rows, K)
    assert x.data_ptr() % 16 == 4
    _, g = inputs(b, K, N, 501)
    r = reference(b, x, K, g, N)
    dW, db, fam = run_wgrad(b, x, K, g, N, 0)
    assert fam == 'exact'
    small = [t for t in range(b.T) if b.set_rows[t] <= 257]
    note(('misaligned', K, N), assert_elementwise(dW, r['dW'], r['sW'], b, small, 'misaligned dW'))
    assert_elementwise(db, r['db'], r['sb'], b, small, 'misaligned db')
    assert _lib().lib().gm_dense_wgrad(b.B.handle, _lib().ptr(x), K, K, _lib().ptr(g), N, N, b.norm_ptr, None, N, _lib().ptr(dW), K * N,
                                       _lib().ptr(db), N, 1, None, None, 0, 0.0, None, None, None, _lib().stream_ptr()) == GM_EINVAL
    # ldx = 131
    note(('ldx131', K, N), _exact_case(b, K, N, 502, ldx=131))
    # gb given
    gb = torch.randn(b.rows, N, device='cuda') * 3.0
    note(('gb', K, N), _exact_case(b, K, N, 503, gb=gb))


def test_rejections(short):
    """K or N above 2048: GM_ERANGE (k_wgrad's bias sums would leave columns unwritten); the split modes where the shape cannot take them:
    GM_EINVAL"""
    L = _lib()
    lib = L.lib()
    b = short
    buf = torch.zeros(b.rows * 2049 + 16, device='cuda')
    out = torch.zeros(b.T * 2049 * 8 + 16, device='cuda')

    def call(K, N, mode, gb=None):
        return lib.gm_dense_wgrad(b.B.handle, L.ptr(buf), K, K, L.ptr(buf), N, N, b.norm_ptr, L.ptr(gb), N, L.ptr(out), K * N, L.ptr(out), N,
                                  mode, None, None, 0, 0.0, None, None, None, L.stream_ptr())
    assert call(2049, 8, 0) == GM_ERANGE
    assert call(8, 2049, 0) == GM_ERANGE
    assert call(64, 128, 1) == GM_EINVAL
    assert call(128, 96, 2) == GM_EINVAL
    assert call(128, 128, 1, gb=buf) == GM_EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- (d) two-piece fp16 kernel
@pytest.mark.parametrize('K,N', [(256, 256), (128, 256), (256, 128), (128, 128)])
def test_split_fp16_is_as_accurate_as_fp32(arxiv, K, N):
    """mode 2: two fp16 pieces per operand under per-set power-of-two scales (bounds taken by the call).  Sets four decades apart; column n of g
    sits 2^-(n % 21) below its set's bound, so that every output column is made of values at one depth under the bound -- below ~2^-18 the
    low fp16 piece is subnormal and keeps 2^-24 absolute of the scaled value, i.e. ~2^-(38 - r) of a column at depth r.  Bars as in the forward
    test's fp16 cases: worst normalised error <= 2 max(exact, torch) + 2^-22 (the dropped-product floor) + 2^-(36 - r) (the subnormal floor,
    4x head-room), rms <= 1.25 x the exact kernel's, bitwise repeatable.  A flushed low piece would show as ~2^-11 at r >= 19."""
    b = arxiv
    gen = torch.Generator(device='cuda').manual_seed(900 + K + N)
    set_of = torch.repeat_interleave(torch.arange(b.T, device='cuda'), torch.tensor(b.set_rows, device='cuda'))
    mag = torch.logspace(-2, 2, b.T, device='cuda')
    x = torch.randn(b.rows, K, device='cuda', generator=gen) * mag[set_of][:, None] * (torch.rand(b.rows, 1, device='cuda', generator=gen) + 0.5)
    x[::97, ::5] = 0.0
    depth = (torch.arange(N, device='cuda') % 21).float()
    g = torch.randn(b.rows, N, device='cuda', generator=gen).clamp(-4, 4) * mag.flip(0)[set_of][:, None] * torch.exp2(-depth)[None, :]
    dW0, db0, f0 = run_wgrad(b, x, K, g, N, 0)
    dW2, db2, f2 = run_wgrad(b, x, K, g, N, 2)
    assert (f0, f2) == ('exact', 'split16')
    r = reference(b, x, K, g, N)
    e16, e0, et = (nerr(o, r['dW'], r['sW']) for o in (dW2, dW0, r['tW']))
    floor = 2.0 * max(float(e0.max()), float(et.max())) + 2.0 ** -22 + torch.exp2(-(36 - depth)).double()
    worst = e16.amax((0, 1))
    assert bool((worst <= floor).all()), [(int(n), float(worst[n]), float(floor[n])) for n in range(N) if not worst[n] <= floor[n]][:8]
    assert rms_rel(dW2, r['dW']) <= 1.25 * rms_rel(dW0, r['dW']), (rms_rel(dW2, r['dW']), rms_rel(dW0, r['dW']))
    note(('fp16', K, N, 2), float(e16.max()))
    eb16, eb0, ebt = (nerr(o, r['db'], r['sb']) for o in (db2, db0, r['tb']))
    floor_b = 2.0 * max(float(eb0.max()), float(ebt.max())) + 2.0 ** -22 + torch.exp2(-(36 - depth)).double()
    assert bool((eb16.amax(0) <= floor_b).all()), (float(eb16.max()), float(floor_b.min()))
    dW3, db3, _ = run_wgrad(b, x, K, g, N, 2)
    assert torch.equal(dW3, dW2) and torch.equal(db3, db2)


# ---------------------------------------------------------------------------------------------------- (e) fused SGD outputs
def _decode_planes(pl, T, K, N, layout):
    """[T][3][K/8][N][8] (fwd) or [T][3][N/8][K][8] (dz) bf16 bit patterns -> hi + mid + lo in fp64, [T, K, N]"""
    a = pl.cpu().numpy().view(np.uint16).reshape(T, 3, -1)
    if layout == 'fwd':
        p = a.reshape(T, 3, K // 8, N, 8).transpose(0, 1, 2, 4, 3).reshape(T, 3, K, N)
    else:
        p = a.reshape(T, 3, N // 8, K, 8).transpose(0, 1, 3, 2, 4).reshape(T, 3, K, N)
    f = (p.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return f[:, 0] + f[:, 1] + f[:, 2]


@pytest.mark.parametrize('K,N,mode,use_gb,family', [(256, 128, 1, False, 'split'),        # wgrad_reduce_pl_body
                                                     (128, 128, 0, True, 'exact')])        # wgrad_reduce_body (k_wgrad: gb given)
def test_fused_sgd_outputs(short, K, N, mode, use_gb, family):
    """next = cur - lr (dW, db) within one rounding of the fp64 step from the kernel's own gradient; wt is bitwise next's W transposed; the
    three bf16 planes of both layouts add up to next's W bitwise; dW and db do not depend on the SGD block."""
    b = short
    T = b.T
    x, g = inputs(b, K, N, 700 + K)
    gb = torch.randn(b.rows, N, device='cuda') if use_gb else None
    P = K * N + N
    ps = P + 12                                                           # a parameter stride wider than the vector
    cur = torch.randn(T * ps, device='cuda')
    nxt = torch.full((T * ps,), float('nan'), device='cuda')
    wt = torch.full((T, N, K), float('nan'), device='cuda')
    plf = torch.full((T * 3 * K * N,), -1, dtype=torch.int16, device='cuda')
    pld = torch.full((T * 3 * K * N,), -1, dtype=torch.int16, device='cuda')
    lr = 0.37
    dW, db, fam = run_wgrad(b, x, K, g, N, mode, gb=gb, sgd=(cur, nxt, wt, plf, pld, ps, lr))
    assert fam == family
    dWn, dbn, _ = run_wgrad(b, x, K, g, N, mode, gb=gb)
    assert torch.equal(dW, dWn) and torch.equal(db, dbn)
    cur2, nxt2 = cur.view(T, ps)[:, :P].double(), nxt.view(T, ps)
    assert bool(torch.isnan(nxt2[:, P:]).all())                           # nothing past the vector
    grad = torch.cat([dW.reshape(T, -1), db], 1).double()
    step = lr * grad
    ref = cur2 - float(np.float32(lr)) * grad
    err = (nxt2[:, :P].double() - ref).abs()
    assert bool((err <= U * (ref.abs() + step.abs()) * (1 + 1e-6)).all()), float((err / (ref.abs() + step.abs()).clamp_min(1e-300)).max())
    Wn = nxt2[:, :K * N].reshape(T, K, N)
    assert torch.equal(wt, Wn.transpose(1, 2))
    Wd = Wn.double().cpu().numpy()
    for pl, layout in ((plf, 'fwd'), (pld, 'dz')):
        assert np.array_equal(_decode_planes(pl, T, K, N, layout), Wd), layout
