"""GPU (-m gpu): every kernel instantiation of the aggregate (gm_launch_aggregate: DGL's update_all(copy_src, sum) of learner.py:38-39,44-45 with
GraphConv's normalisations, and its transpose in the backward) and every option its callers set, against an fp64 reference computed from the test's own
edge list (tests/agg_ref.py), through the test-only export gm_dense_aggregate:

    out[v] = epi(|s_out[v]| sum_e w_e X[src_e] + b_set(v)),   epi = ReLU, then the relu' mask (mask_h <= 0 or a clear mask_b bit: 0).

Every case asserts which instantiation ran (`launched`, GM_AGG_ID_* of gm_internal.h, restated in expected_id below).  `out` is pre-filled with NaN and the
relu' bits with 0xA5: the sentinel must survive bitwise exactly where no store is due (sign-flagged rows under keep_signed, rows in the skip range, rows off
the row list) and nowhere else.  Every row of x that no edge reads in the orientation under test is NaN (row 0, the kernels' former padding target, among them;
under x_src 3 every row but the centres'), and every stored output must be finite.

Per-element bar, derived, not fitted:   |out - ref| <= (C_DET + min(2d, LAMBDA sqrt(2d))) u scale,   u = 2^-24, C_DET = 4, LAMBDA = 8,
d = the row's term count, scale = |s_out| sum_e |w_e||x[src_e]| + |b|.
  - each term enters by one fused multiply-add (or an exact-product multiply and an add in the generic kernel's chain: still one rounding of the running sum per
    term): d roundings;
  - combining the two accumulators, the lane groups' partial rows and the hub parts adds at most one rounding per non-zero partial: <= d more;
  - the epilogue adds at most three: the sum of the two accumulators, the scale, the bias -- C_DET = 4 leaves one to spare;
  - every rounding is below u times the running absolute sum <= u scale;
  - the square-root form is the probabilistic bound of Higham and Mary (SIAM J. Sci. Comput. 41, 2019) that test_hip_gemm_epilogue.py uses, same LAMBDA;
  - the reference takes the fp32 values of the batch's own norm and per-edge tables, converted to fp64: forming those tables is not part of this bar
    (test_batch_tables compares them bitwise with norm[src] / feat_row[src]);
  - ReLU and the masks do not widen the bar: |relu(a) - relu(b)| <= |a - b|, a masked element is exactly 0 on both sides.
A packed relu' bit must equal `out > 0` of the GPU's own value wherever that value is stored, and the reference's sign wherever |ref| exceeds the bar.

Exact-answer cases on every family: x holds integers |x| <= 8, scales and biases are powers of two, so every partial sum is exact in fp32 and the result must be
bitwise the integer answer -- a dropped, doubled or misattributed edge is an error of at least 1.  (Under the batch's own norm table x is zero at the
sources whose norm is not a power of two: the terms that remain are exact.)

Graphs (tests/agg_ref.py): `sparse` (hub threshold 32, split hubs in parts of 128 edges), `dense` (threshold 64, 4-row windows, never stream-eligible),
`giant` (parts of 160 edges, a 5,000-edge row in 31 parts), `flat` (no hub), `unsplit` (hubs up to 191 edges: scheduled, not split); 8,192 rows in sets of
2,048 / 4,096 / 2,048.

Which case reaches which id (generic k_agg<VEC, LPR>: 100 + 10 [VEC 4] + log2 LPR; window k_agg_win<LPR, NCH>: 200 / 216 / 232 / 248 for widths 64 / 128 /
256 / 512, + 1 scheduled, + 2 split, + 4 separate k_agg_heavy launch, + 8 row list; stream k_agg_stream<LPR>: 300 / 302 / 304 for widths 64 / 128 / 256, + 1 split):
  test_generic           111 (4, 8), 112 (12, 16), 113 (20, 32), 114 (36), 115 (68), 116 (132, 300, 1024); 101 (1, 2), 102 (3), 103 (5), 104 (9), 105 (17),
                         106 (33, 50, 130); plain and full epilogue each
  test_generic_misaligned 106 (width 64, x one float off), 116 (width 256, bias one float off)
  test_window            base + 3 (sparse, dense, giant: scheduled and split), base + 1 (unsplit), base + 0 (flat; hubs = 0 anywhere)
  test_heavy_launch      base + 4 (sparse, giant: hub list without a schedule)
  test_row_list          base + 8 (no hubs), base + 12 (hubs by the separate launch), base + 11 (the batch's own list and list schedule)
  test_stream            301 / 303 / 305 (sparse, giant), 300 / 302 / 304 (flat, unsplit); dense: the window kernel
  test_weighted          window, generic and stream ids on a weighted sparse batch"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import agg_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_DET, LAMBDA = 4, 8
GM_EINVAL = -1
NAN_BITS = 0x7FC00000
WIN_WIDTHS = (64, 128, 256, 512)
ALL_OPTS = ('s_out', 'keep', 'bias', 'relu', 'bits', 'mask_b')


def _L():
    from gmeta_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------------------- batches
class Env:
    """a ladder graph, its store (features F wide, NaN at the nodes nobody reads in orientation `poison_o`) and the batch of sum(SET_SUBS) whole-graph subgraphs"""

    def __hash__(self):
        return id(self)

    def __eq__(self, other):
        return self is other


@functools.lru_cache(maxsize=None)
def env(variant, F=64, weighted=False, poison_o=0, set_subs=tuple(R.SET_SUBS)):
    import gmeta_amd
    from gmeta_amd.subgraphs import SubgraphBatch
    L = _L()
    e = Env()
    g = e.g = R.build_graph(variant, weighted=weighted)
    subs = sum(set_subs)
    rows = subs * R.N
    e.variant, e.F, e.weighted, e.rows, e.T = variant, F, weighted, rows, len(set_subs)
    din, dout = R.degrees(g)
    rng = np.random.default_rng(7)
    feats = (rng.standard_normal((R.N, F)) * np.logspace(-1, 1, R.N)[rng.permutation(R.N)][:, None]).astype(np.float32)
    feats[(dout if poison_o == 0 else din) == 0] = np.nan
    graph = (R.N, g.src, g.dst, g.w) if weighted else (R.N, g.src, g.dst)
    e.store = gmeta_amd.GraphStore([graph], [feats])
    e.centre_nodes = [50 + 7 * k for k in range(subs)]
    seeds = np.array([(0, c, -1) for c in e.centre_nodes], np.int32)
    nodes = np.arange(R.N, dtype=np.int32)
    e.B = SubgraphBatch.from_nodes(e.store, seeds, np.cumsum([0] + list(set_subs)), [nodes] * subs, False)
    assert (e.B.rows, e.B.sets, e.B.subs) == (rows, e.T, subs) and e.B.edges == len(g.src) * subs      # the induced edges are the edges made here
    assert np.array_equal(e.B._read(L.F_FEAT_ROW, rows, np.int32), np.tile(nodes, subs))
    s, d, w = R.batch_edges(g, subs)
    e.n_edges = len(s)
    es, ed = torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda()
    e.read, e.write = (es, ed), (ed, es)                  # rows of x read / rows of out written per edge, by orientation
    e.e_w = None if w is None else torch.from_numpy(w).cuda()
    e.deg = tuple(torch.bincount(x, minlength=rows) for x in e.write)
    e.unread = tuple(torch.bincount(x, minlength=rows) == 0 for x in e.read)
    e.norm = torch.from_numpy(e.B._read(L.F_NORM, rows, np.float32).copy()).cuda()
    e.set_row = torch.from_numpy(R.set_of_rows(g, list(set_subs))).cuda()
    e.feats = torch.from_numpy(feats).cuda()
    e.feat_row = torch.arange(rows, device='cuda') % R.N
    e.centre_rows = torch.tensor([k * R.N + c for k, c in enumerate(e.centre_nodes)], device='cuda')
    e.info = tuple(batch_info(e, o) for o in (0, 1))
    # the batch's own CSR agrees with the edge list: degrees in both orientations
    for o in (0, 1):
        ip = e.B.csr(transposed=bool(o))[0]
        assert np.array_equal(np.diff(ip), e.deg[o].cpu().numpy())
    return e


def batch_info(e, o):
    L = _L()
    info = (C.c_int64 * 16)()
    L.check(L.lib().gm_dense_agg_info(e.B.handle, o, info), 'gm_dense_agg_info')
    v = list(info)
    return dict(threshold=v[0], n_heavy=v[1], sched_win=v[2], hub_part=v[3], parts=v[4], sched=v[5], n_mid=v[6], mid_win=v[7], sched_mid=v[8], nseg=v[9],
                nwg=v[10], hub_wgs=v[11], weighted=v[12], feat_dim=v[13], feat_ld=v[14])


def batch_table(e, which, o, n, dtype):
    L = _L()
    t = torch.empty(n, dtype=dtype, device='cuda')
    L.check(L.lib().gm_dense_agg_table(e.B.handle, which, o, L.ptr(t), n, L.stream_ptr()), 'gm_dense_agg_table')
    torch.cuda.synchronize()
    return t


@contextlib.contextmanager
def stream_knob():
    """GM_AGG_STREAM_MIN_ROWS = 0 (a batch decides whether it gets stream tables at its first stream-eligible launch), restored afterwards"""
    L = _L()
    was = L.lib().gm_get_tuning(b'GM_AGG_STREAM_MIN_ROWS')
    L.check(L.lib().gm_set_tuning(b'GM_AGG_STREAM_MIN_ROWS', 0))
    try:
        yield
    finally:
        L.check(L.lib().gm_set_tuning(b'GM_AGG_STREAM_MIN_ROWS', was))


# ---------------------------------------------------------------------------------------------------- inputs and reference
class Inputs:
    pass


@functools.lru_cache(maxsize=48)
def inputs(e, o, width, x_src=0, scale=0, exact=False, xoff=False, ldpad=0):
    """x (NaN where nobody reads it), the source scale, and the fp64 sums of the reference; one per (batch, orientation, width, source forms)"""
    gen = torch.Generator(device='cuda').manual_seed(1000 * width + 10 * x_src + 2 * scale + o)
    i = Inputs()
    rows = e.rows
    i.ldx = width + ldpad
    i.s_in = None
    if x_src in (1, 2):
        assert width == e.F and not exact
        i.x, i.ldx = None, 0
        xref = e.feats[e.feat_row]
    else:
        xrows = rows + (1 if x_src == 3 else 0)
        store = torch.empty(xrows * i.ldx + 4, device='cuda')
        x = store[(1 if xoff else 0):(1 if xoff else 0) + xrows * i.ldx].view(xrows, i.ldx)
        if exact:
            x.copy_(torch.randint(-8, 9, (xrows, i.ldx), device='cuda', generator=gen).float())
            if scale == 2:       # the batch's norms: keep the sources whose norm is a power of two
                pow2 = (e.norm.view(torch.int32) & 0x7FFFFF) == 0
                x[:rows][~pow2] = 0.0
        else:
            x.copy_(torch.randn(xrows, i.ldx, device='cuda', generator=gen))
            x[:rows] *= torch.logspace(-1, 1, rows, device='cuda')[torch.randperm(rows, device='cuda', generator=gen)][:, None]
        if x_src == 3:           # read through the centre-edge table: only the centre rows and the zero row behind T are ever read
            keep = torch.zeros(xrows, dtype=torch.bool, device='cuda')
            keep[e.centre_rows] = True
            x[~keep] = float('nan')
            x[rows] = 0.0
            xref = torch.where(keep[:rows, None], x[:rows, :width], torch.zeros_like(x[:rows, :width]))
        else:
            x[e.unread[o]] = float('nan')
            xref = x[:, :width]
        i.x, i.store = x, store
    if scale == 0:
        w = e.e_w
    elif scale == 1:
        if exact:
            i.s_in = torch.randint(0, 2, (rows,), device='cuda', generator=gen).float() + 1.0
        else:
            i.s_in = torch.randn(rows, device='cuda', generator=gen)
        i.s_in[e.unread[o]] = float('nan')
        w = i.s_in[e.read[o]]
    else:
        w = e.norm[e.read[o]]
        if e.e_w is not None:
            w = e.e_w * w          # fp32, as the table was formed (test_batch_tables: bitwise)
    i.acc, i.sab, i.d = R.edge_sums(rows, e.read[o], e.write[o], w, xref)
    assert torch.equal(i.d, e.deg[o])
    return i


@functools.lru_cache(maxsize=48)
def epilogue_inputs(e, width, exact=False):
    gen = torch.Generator(device='cuda').manual_seed(77 + width)
    p = Inputs()
    rows = e.rows
    if exact:
        p.s = torch.exp2(torch.randint(-1, 2, (rows,), device='cuda', generator=gen).float())
    else:
        p.s = torch.exp2(torch.rand(rows, device='cuda', generator=gen) * 4 - 2)
    p.flag = torch.arange(rows, device='cuda') % 7 == 3
    p.s_signed = torch.where(p.flag, -p.s, p.s)
    p.stride = width + (4 if width % 4 == 0 else 3)
    bb = torch.empty(e.T * p.stride + 4, device='cuda')
    if exact:
        bb.copy_(torch.exp2(torch.randint(0, 3, bb.shape, device='cuda', generator=gen).float()) * (torch.randint(0, 2, bb.shape, device='cuda', generator=gen).float() * 2 - 1))
    else:
        bb.copy_(torch.randn(bb.shape, device='cuda', generator=gen))
    p.bias_store = bb
    m = torch.randn(rows * width, device='cuda', generator=gen)
    m[::11] = 0.0
    m[5::11] = -0.0
    m[7::13] = 1e-40
    m[9::13] = -1e-40
    p.mask_h = m.view(rows, width)
    p.mask = p.mask_h > 0
    p.mask_b = None
    if width % 4 == 0:
        q = p.mask.view(rows * width // 4, 4).to(torch.int32)
        p.mask_b = (q[:, 0] | (q[:, 1] << 1) | (q[:, 2] << 2) | (q[:, 3] << 3) | 0xA0).to(torch.uint8)      # (the high nibble is nobody's)
    return p


def unpack_bits(bits, rows, width):
    by = bits.view(rows, width // 4).to(torch.int32)
    return torch.stack([(by >> k) & 1 for k in range(4)], 2).reshape(rows, width).bool()


# ---------------------------------------------------------------------------------------------------- the call
def lpr_code(lpr):
    return {2: 1, 4: 2, 8: 3, 16: 4, 32: 5, 64: 6}[lpr]


def expected_id(family, width, info=None, hubs=2, rowlist=False, list_sched=False):
    """GM_AGG_ID_* (gm_internal.h) of the instantiation a launch must take"""
    if family == 'vec4':
        n4 = width // 4
        lpr = 64 if n4 > 32 else 32 if n4 > 16 else 16 if n4 > 8 else 8 if n4 > 4 else 4 if n4 > 2 else 2
        return 110 + lpr_code(lpr)
    if family == 'vec1':
        lpr = 64 if width > 32 else 32 if width > 16 else 16 if width > 8 else 8 if width > 4 else 4 if width > 2 else 2
        return 100 + lpr_code(lpr)
    idx = WIN_WIDTHS.index(width)
    if family == 'stream':
        return 300 + 2 * idx + (1 if info['hub_part'] else 0)
    assert family == 'win'
    n_heavy = info['n_heavy'] if hubs else 0
    sched = (hubs == 2 and info['sched'] and not rowlist) or list_sched
    kid = 200 + 16 * idx + (8 if rowlist else 0)
    if sched:
        return kid + 1 + (2 if info['hub_part'] else 0)
    return kid + (4 if n_heavy > 0 else 0)


class Run:
    pass


def launch(e, o, width, x=None, ldx=0, x_src=0, scale=0, s_in=None, s_out=None, keep=False, bias=None, bias_stride=0, relu=False, bits=False,
           mask_h=None, mask_b=None, hubs=2, rowlist=None, list_win=0, list_sched=False, skip=None, stream=False, expect_rc=0):
    """gm_dense_aggregate into sentinel-filled outputs"""
    L = _L()
    r = Run()
    r.out_store = torch.full((e.rows * width + 4,), float('nan'), device='cuda')
    r.out = r.out_store[:e.rows * width].view(e.rows, width)
    r.bits = torch.full((e.rows * width // 4 + 4,), 0xA5, dtype=torch.uint8, device='cuda') if bits else None
    launched = C.c_int32(-1)
    lo, hi = skip if skip else (1, 0)
    rc = L.lib().gm_dense_aggregate(e.B.handle, o, x_src, L.ptr(x), ldx, width, scale, L.ptr(s_in), L.ptr(s_out), 1 if keep else 0, L.ptr(bias), bias_stride,
                                    1 if relu else 0, L.ptr(r.bits), L.ptr(mask_h), L.ptr(mask_b), hubs, L.ptr(rowlist), 0 if rowlist is None else len(rowlist),
                                    list_win, 1 if list_sched else 0, lo, hi, 1 if stream else 0, L.ptr(r.out), C.byref(launched), L.stream_ptr())
    torch.cuda.synchronize()
    r.kid = launched.value
    if expect_rc:
        assert rc == expect_rc and r.kid == -1, (rc, r.kid, L.lib().gm_last_error())
        assert (r.out_store.view(torch.int32) == NAN_BITS).all() and (r.bits is None or (r.bits == 0xA5).all())       # a refusal leaves the outputs alone
        return None
    L.check(rc, 'gm_dense_aggregate')
    return r


def check(e, o, width, family, opts=(), x_src=0, scale=0, hubs=2, rowlist=None, list_win=0, list_sched=False, skip=None, stream=False, exact=False, xoff=False,
          bias_off=False, shared_bias=False, ldpad=0):
    """one launch with the options `opts` (of ALL_OPTS + mask_h), checked against the reference, the sentinels and the expected instantiation"""
    opts = set(opts)
    assert opts <= set(ALL_OPTS) | {'mask_h'} and ('keep' not in opts or 's_out' in opts) and ('bits' not in opts or 'relu' in opts)
    i = inputs(e, o, width, x_src, scale, exact, xoff, ldpad)
    p = epilogue_inputs(e, width, exact)
    info = e.info[o]
    kw = dict(x=i.x, ldx=i.ldx, x_src=x_src, scale=scale, s_in=i.s_in, hubs=hubs, rowlist=rowlist, list_win=list_win, list_sched=list_sched, skip=skip, stream=stream)
    s_out = bias_rows = mask = None
    if 's_out' in opts:
        s_out = p.s_signed if 'keep' in opts else p.s
        kw.update(s_out=s_out, keep='keep' in opts)
    if 'bias' in opts:
        b0 = 1 if bias_off else 0
        bias = p.bias_store[b0:b0 + e.T * p.stride]
        kw.update(bias=bias, bias_stride=0 if shared_bias else p.stride)
        bt = bias.view(e.T, p.stride)[:, :width]
        bias_rows = bt[0].expand(e.rows, width) if shared_bias else bt[e.set_row]
    if 'relu' in opts:
        kw.update(relu=True, bits='bits' in opts)
    if 'mask_b' in opts:
        kw.update(mask_b=p.mask_b)
        mask = p.mask
    elif 'mask_h' in opts:
        kw.update(mask_h=p.mask_h)
        mask = p.mask
    r = launch(e, o, width, **kw)
    want = expected_id(family, width, info, hubs, rowlist is not None, list_sched)
    assert r.kid == want, ('launched %d, expected %d' % (r.kid, want), e.variant, o, width, sorted(opts))
    ref, scl = R.epilogue(i.acc, i.sab, s_out, bias_rows, 'relu' in opts, mask)
    # ---- where a store is due
    deg = e.deg[o]
    window = family == 'win'
    written = torch.ones(e.rows, dtype=torch.bool, device='cuda')
    if rowlist is not None:
        written[:] = False
        written[rowlist.long()] = True
        if hubs and info['n_heavy']:
            written |= deg > info['threshold']            # hub rows keep their own workgroups
    if skip and window:
        written &= ~((deg >= skip[0]) & (deg <= skip[1]))
    stored = written & ~p.flag if 'keep' in opts else written
    outb = r.out.view(torch.int32)
    assert (outb[~stored] == NAN_BITS).all(), 'a row that is not due was written'
    assert (r.out_store[e.rows * width:].view(torch.int32) == NAN_BITS).all()
    got = r.out[stored]
    assert torch.isfinite(got).all(), 'sentinel or NaN left in %d stored elements' % int((~torch.isfinite(got)).sum())
    # ---- the bar
    d2 = 2.0 * i.d.double()[:, None]
    tol = (C_DET + torch.minimum(d2, LAMBDA * torch.sqrt(d2))) * U * scl
    err = (r.out.double() - ref).abs()
    bad = stored[:, None] & ~(err <= tol)
    if bad.any():
        k = int(torch.argmax(torch.where(bad, err / tol.clamp_min(1e-300), torch.zeros_like(err))))
        row, col = divmod(k, width)
        pytest.fail('%s o=%d width=%d id=%d %s: %d elements over the bar; worst row %d (degree %d) col %d: got %r ref %r err %.3g bar %.3g' % (
            e.variant, o, width, r.kid, sorted(opts), int(bad.sum()), row, int(deg[row]), col, float(r.out[row, col]), float(ref[row, col]), float(err[row, col]),
            float(tol[row, col])))
    if exact:
        assert torch.equal(got.double(), ref[stored]), 'exact-answer case: %d elements differ' % int((got.double() != ref[stored]).sum())
    # ---- packed relu' bits
    if r.bits is not None:
        by = r.bits[:e.rows * width // 4].view(e.rows, width // 4)
        assert (by[~written] == 0xA5).all() and (r.bits[e.rows * width // 4:] == 0xA5).all()
        assert (by[written] < 16).all()
        ub = unpack_bits(r.bits[:e.rows * width // 4], e.rows, width)
        assert torch.equal(ub[stored], got > 0)
        clear = written[:, None] & (ref.abs() > tol)
        assert torch.equal(ub[clear], (ref > 0)[clear])
    r.stored, r.ref = stored, ref
    return r


# ---------------------------------------------------------------------------------------------------- the batches are what the tests take them for
@pytest.mark.parametrize('variant', sorted(R.VARIANTS))
def test_batch_tables(variant):
    e = env(variant)
    L = _L()
    for o in (0, 1):
        info = e.info[o]
        th, hubs, hp, parts = R.expected_hubs(e.deg[o].cpu().numpy(), e.rows, e.n_edges)
        assert (info['threshold'], info['n_heavy'], info['hub_part']) == (th, len(hubs), hp), (variant, o, info)
        assert info['sched_win'] == R.agg_window(e.rows, e.n_edges) and info['sched'] == (1 if len(hubs) else 0)
        if hp:
            assert info['parts'] == parts
        if len(hubs):
            assert np.array_equal(batch_table(e, 3, o, len(hubs), torch.int32).cpu().numpy(), hubs)
        # the per-edge tables, bitwise: source norm and (by destination) source feature row
        ix = torch.from_numpy(e.B.csr(transposed=bool(o))[1].astype(np.int64)).cuda()
        assert torch.equal(batch_table(e, 0, o, e.n_edges, torch.float32).view(torch.int32), e.norm[ix].view(torch.int32))
        if o == 0:
            assert torch.equal(batch_table(e, 1, 0, e.n_edges, torch.int32).long(), e.feat_row[ix])
    n_mid = int(((e.deg[0] >= 3) & (e.deg[0] <= e.info[0]['threshold'])).sum())
    assert e.info[0]['n_mid'] == n_mid and e.info[0]['sched_mid'] == (1 if e.info[0]['n_heavy'] else 0)
    assert (e.info[0]['feat_dim'], e.info[0]['feat_ld'], e.info[0]['weighted']) == (64, 64, 0)
    assert L.lib().gm_get_tuning(b'GM_AGG_STREAM') == 1


# ---------------------------------------------------------------------------------------------------- generic kernel
FULL = ('s_out', 'keep', 'bias', 'relu', 'bits', 'mask_b')
FULL1 = ('s_out', 'keep', 'bias', 'relu', 'mask_h')
VEC4_WIDTHS = (4, 8, 12, 16, 20, 32, 36, 68, 132, 300, 1024)
VEC1_WIDTHS = (1, 2, 3, 5, 9, 17, 33, 50, 130)


@pytest.mark.parametrize('o', (0, 1))
@pytest.mark.parametrize('width', VEC4_WIDTHS + VEC1_WIDTHS)
def test_generic(width, o):
    e = env('sparse')
    fam = 'vec4' if width % 4 == 0 else 'vec1'
    check(e, o, width, fam)                                               # hub rows are walked by their own lane group here, whatever `hubs` says
    check(e, o, width, fam, FULL if fam == 'vec4' else FULL1, scale=1, hubs=1 + o)
    check(e, o, width, fam, ('s_out', 'bias'), scale=1, exact=True, hubs=0)


@pytest.mark.parametrize('opts', [('s_out',), ('s_out', 'keep'), ('bias',), ('relu',), ('relu', 'bits'), ('mask_h',), ('mask_b',)], ids=lambda o: '+'.join(o))
def test_generic_each_option(opts):
    e = env('sparse')
    check(e, 0, 36, 'vec4', opts, scale=2)
    check(e, 1, 300, 'vec4', opts, shared_bias=True)
    if 'bits' not in opts and 'mask_b' not in opts:
        check(e, 1, 33, 'vec1', opts, scale=2)


def test_generic_misaligned():
    e = env('sparse')
    for o in (0, 1):
        r = check(e, o, 64, 'vec1', xoff=True)                            # x one float past a 16-byte boundary: k_agg<1, 64>
        assert r.kid == 106
        check(e, o, 64, 'vec1', FULL1, xoff=True, scale=1)
        r = check(e, o, 256, 'vec4', ('s_out', 'bias', 'relu', 'bits'), bias_off=True, scale=2)      # a bias that is not 16-byte aligned: k_agg<4, 64>
        assert r.kid == 116
        check(e, o, 128, 'win', ldpad=4)                                  # a caller matrix with its own row stride stays on the window kernel
        check(e, o, 128, 'vec1', ldpad=3)


# ---------------------------------------------------------------------------------------------------- window kernel
FWD = ('s_out', 'bias', 'relu', 'bits')              # gcn_forward's matmul-first layer
BWD = ('s_out', 'keep', 'mask_b')                    # gcn_backward


@pytest.mark.parametrize('o', (0, 1))
@pytest.mark.parametrize('width', WIN_WIDTHS)
@pytest.mark.parametrize('variant', ('sparse', 'dense', 'giant', 'flat', 'unsplit'))
def test_window(variant, width, o):
    e = env(variant)
    info = e.info[o]
    r = check(e, o, width, 'win', scale=2)
    assert (r.kid - 200) % 16 == {'flat': 0, 'unsplit': 1}.get(variant, 3)
    check(e, o, width, 'win', FWD, scale=0)
    check(e, o, width, 'win', BWD, scale=0 if o else 1)
    check(e, o, width, 'win', ('s_out', 'bias'), scale=1, exact=True)
    check(e, o, width, 'win', ('s_out', 'keep', 'relu', 'bits', 'mask_h'), scale=2, exact=True, hubs=0)      # hub rows by the windows' own edge loop
    assert info['sched_win'] == (4 if variant == 'dense' else 2)


@pytest.mark.parametrize('opts', [('s_out',), ('s_out', 'keep'), ('bias',), ('relu',), ('relu', 'bits'), ('mask_h',), ('mask_b',)], ids=lambda o: '+'.join(o))
def test_window_each_option(opts):
    for variant, o, width in (('sparse', 0, 64), ('dense', 1, 128), ('giant', 0, 256), ('sparse', 1, 512)):
        e = env(variant)
        a = check(e, o, width, 'win', opts, scale=2)
        if 'bias' in opts:                                                # one bias for every set against a bias per set
            b = check(e, o, width, 'win', opts, scale=2, shared_bias=True)
            other = e.set_row != 0
            assert torch.equal(a.out[~other], b.out[~other]) and not torch.equal(a.out[other], b.out[other])


@pytest.mark.parametrize('F', (64, 128))
def test_window_source_forms(F):
    """the three sources of x at width == feat_dim: a caller matrix, the store's features per source row and per edge; and the centre-edge table"""
    for variant in ('sparse', 'dense'):
        e = env(variant, F)
        for scale in (0, 2):
            a = check(e, 0, F, 'win', x_src=1, scale=scale)
            b = check(e, 0, F, 'win', x_src=2, scale=scale)
            assert torch.equal(a.out, b.out)
            check(e, 0, F, 'win', FWD, x_src=2, scale=scale)
        check(e, 0, F, 'win', x_src=1, scale=1)
        check(e, 0, F, 'win', BWD, x_src=2, scale=1)
        check(e, 1, F, 'win', BWD, x_src=3, scale=0)                      # gcn_backward's last layer: keep_signed through x_idx
        check(e, 1, F, 'win', x_src=3, scale=2, hubs=1)
        et = env(variant, F, poison_o=1)
        check(et, 1, F, 'win', x_src=1, scale=2)
        check(et, 1, F, 'win', FWD, x_src=1, scale=1)


# ---------------------------------------------------------------------------------------------------- separate heavy launch
@pytest.mark.parametrize('o', (0, 1))
@pytest.mark.parametrize('width', WIN_WIDTHS)
@pytest.mark.parametrize('variant', ('sparse', 'giant'))
def test_heavy_launch(variant, width, o):
    e = env(variant)
    r = check(e, o, width, 'win', scale=2, hubs=1)
    assert (r.kid - 200) % 16 == 4
    check(e, o, width, 'win', FWD, scale=1, hubs=1)
    check(e, o, width, 'win', BWD, scale=0, hubs=1)
    check(e, o, width, 'win', ('s_out', 'bias'), scale=1, exact=True, hubs=1)


# ---------------------------------------------------------------------------------------------------- row list
def row_lists(e, o):
    deg = e.deg[o]
    rows = torch.arange(e.rows, device='cuda', dtype=torch.int32)
    return {'all': rows, 'third': rows[::3].contiguous(), 'mid': rows[(deg >= 3) & (deg <= e.info[o]['threshold'])].contiguous()}


LIST_CASES = []
for _wi, _w in enumerate(WIN_WIDTHS):
    _G = 64 // min(64, _w // 4)
    for _ki, _win in enumerate((2, 4, 8, 16, 32, 64)):
        LIST_CASES.append((_w, _win, 'all', 1, None, 1))
        LIST_CASES.append((_w, _win, 'third', _G - 1 if _G > 1 else 1, (0, 2), 0))
        LIST_CASES.append((_w, _win, 'mid', _G + 1, (0, 2) if (_wi + _ki) % 2 else None, 1))


@pytest.mark.parametrize('width,win,kind,rem,skip,hubs', LIST_CASES)
def test_row_list(width, win, kind, rem, skip, hubs):
    e = env('sparse' if (width // 64 + win) % 3 else 'dense')
    o = (width // 64 + win // 2) % 2
    full = row_lists(e, o)[kind]
    n = (len(full) // win - 1) * win + rem                                # the last window holds rem % win rows (or is full)
    lst = full[:n].contiguous()
    r = check(e, o, width, 'win', scale=2, hubs=hubs, rowlist=lst, list_win=win, skip=skip)
    assert (r.kid - 200) % 16 == (12 if hubs else 8)
    check(e, o, width, 'win', FWD if kind != 'third' else BWD, scale=1, hubs=hubs, rowlist=lst, list_win=win, skip=skip, exact=True)


@pytest.mark.parametrize('variant', ('sparse', 'dense', 'giant', 'unsplit', 'flat'))
def test_row_list_production(variant):
    """the batch's own list of window rows (degree 3 .. threshold) with its window and, where the batch has hub rows, its list schedule: gcn_forward's
    partial launch of a fused pass"""
    e = env(variant)
    info = e.info[0]
    want = row_lists(e, 0)['mid']
    if not info['n_mid']:
        pytest.skip('%s: the batch keeps no list of window rows' % variant)
    mid = batch_table(e, 2, 0, info['n_mid'], torch.int32)
    assert torch.equal(mid, want)
    for width in WIN_WIDTHS:
        if info['sched_mid']:
            r = check(e, 0, width, 'win', scale=2, rowlist=mid, list_win=info['mid_win'], list_sched=True, skip=(0, 2))
            assert (r.kid - 200) % 16 == 9 + (2 if info['hub_part'] else 0)
            check(e, 0, width, 'win', FWD, scale=1, rowlist=mid, list_win=info['mid_win'], list_sched=True, skip=(0, 2), exact=True)
        else:
            assert info['n_heavy'] == 0
            r = check(e, 0, width, 'win', scale=2, rowlist=mid, list_win=info['mid_win'], skip=(0, 2))
            assert (r.kid - 200) % 16 == 8
    if e.F == 64:
        check(e, 0, 64, 'win', scale=2, x_src=2, rowlist=mid, list_win=info['mid_win'], list_sched=bool(info['sched_mid']), skip=(0, 2))


# ---------------------------------------------------------------------------------------------------- stream kernel
@pytest.mark.parametrize('width', (64, 128, 256))
@pytest.mark.parametrize('variant', ('sparse', 'flat', 'giant', 'unsplit'))
def test_stream(variant, width):
    e = env(variant)
    with stream_knob():
        for o in (0, 1):
            a = check(e, o, width, 'stream', scale=2, stream=True)
            assert a.kid == 300 + 2 * WIN_WIDTHS.index(width) + (1 if variant in ('sparse', 'giant') else 0)
            b = check(e, o, width, 'stream', scale=2, stream=True)
            assert torch.equal(a.out.view(torch.int32), b.out.view(torch.int32))                       # two launches, bit for bit
            w = check(e, o, width, 'win', scale=2)
            low = e.deg[o] <= e.info[o]['threshold']
            assert torch.equal(a.out[low].view(torch.int32), w.out[low].view(torch.int32))             # the kernel's contract: the window kernel's rows
            check(e, o, width, 'stream', scale=2, stream=True, exact=True)
            # anything the stream kernel does not do stays on the window kernel
            check(e, o, width, 'win', ('s_out',), scale=2, stream=True)
            check(e, o, width, 'win', scale=1, stream=True)
            info = batch_info(e, o)
            assert info['nseg'] > 0 and info['nwg'] % 8 == 0 and info['hub_wgs'] % 8 == 0 and (info['hub_wgs'] > 0) == (info['n_heavy'] > 0)


def test_stream_feature_gather():
    for variant in ('sparse', 'flat', 'giant'):
        for F in (64, 128):
            e = env(variant, F)
            with stream_knob():
                a = check(e, 0, F, 'stream', x_src=2, scale=2, stream=True)
                w = check(e, 0, F, 'win', x_src=2, scale=2)
                low = e.deg[0] <= e.info[0]['threshold']
                assert torch.equal(a.out[low].view(torch.int32), w.out[low].view(torch.int32))
                check(e, 0, F, 'win', x_src=1, scale=2, stream=True)      # no per-edge feature rows in the launch: not the stream kernel's aggregate


def test_stream_dense_keeps_the_window_kernel():
    e = env('dense')
    with stream_knob():
        for o in (0, 1):
            r = check(e, o, 128, 'win', scale=2, stream=True)
            assert (r.kid - 200) % 16 == 3 and batch_info(e, o)['nseg'] == 0


def test_stream_segments_outnumber_half_the_rows():
    """Most waves of a small launch get an empty or a one-row segment.  A stream launch has max(3 per CU, cost / 384) workgroups of four waves
    (gm_stream_wgs): 768 on a 256-CU part, so at most 3,072 row segments -- fewer than half the rows of the 8,192-row batches (their figures are printed),
    more than half the rows of a batch of two subgraphs (4,096 rows), which is the one held to it here, with and without hub rows"""
    for variant in ('sparse', 'flat'):
        with stream_knob():
            big = env(variant)
            check(big, 0, 64, 'stream', scale=2, stream=True)
            info = batch_info(big, 0)
            print('%s: %d rows: %d segments, %d workgroups (%d for hub parts)' % (variant, big.rows, info['nseg'], info['nwg'], info['hub_wgs']))
            e = env(variant, set_subs=(1, 1))
            for o in (0, 1):
                for width in (64, 128, 256):
                    a = check(e, o, width, 'stream', scale=2, stream=True)
                    w = check(e, o, width, 'win', scale=2)
                    low = e.deg[o] <= e.info[o]['threshold']
                    assert torch.equal(a.out[low].view(torch.int32), w.out[low].view(torch.int32))
                    check(e, o, width, 'stream', scale=2, stream=True, exact=True)
                info = batch_info(e, o)
                print('%s: %d rows, orientation %d: %d segments, %d workgroups (%d for hub parts)' % (variant, e.rows, o, info['nseg'], info['nwg'], info['hub_wgs']))
                assert info['nseg'] > e.rows // 2


# ---------------------------------------------------------------------------------------------------- weighted store
def test_weighted():
    e = env('sparse', weighted=True)
    assert e.info[0]['weighted'] == 1
    L = _L()
    for o in (0, 1):
        ix = torch.from_numpy(e.B.csr(transposed=bool(o))[1].astype(np.int64)).cuda()
        ew = torch.from_numpy(e.B.edge_weights(transposed=bool(o)).copy()).cuda()
        assert (ew != ew.round()).float().mean() > 0.99
        assert torch.equal(batch_table(e, 0, o, e.n_edges, torch.float32).view(torch.int32), (ew * e.norm[ix]).view(torch.int32))
        for scale in (0, 2):                                              # the raw weights, and weight x norm
            for width in (64, 256, 512):
                check(e, o, width, 'win', scale=scale)
                check(e, o, width, 'win', FWD if o == 0 else BWD, scale=scale, hubs=1)
            check(e, o, 36, 'vec4', scale=scale)
            check(e, o, 36, 'vec4', FULL, scale=scale)
            check(e, o, 17, 'vec1', FULL1, scale=scale)
        with stream_knob():
            for width in (64, 128, 256):
                a = check(e, o, width, 'stream', scale=2, stream=True)
                assert a.kid % 2 == 1
                check(e, o, width, 'win', scale=0, stream=True)           # the raw weights are not the stream tables' weights
    check(e, 0, 64, 'win', x_src=2, scale=2)
    # the refusals of gm_aggregate
    i = inputs(e, 0, 64)
    s_in = torch.ones(e.rows, device='cuda')
    launch(e, 0, 64, x=i.x, ldx=64, scale=1, s_in=s_in, expect_rc=GM_EINVAL)
    assert b'weighted' in L.lib().gm_last_error()
    for o in (0, 1):                                                      # a per-source feature gather would drop the weights
        launch(e, o, 64, x_src=1, expect_rc=GM_EINVAL)
        assert b'weighted' in L.lib().gm_last_error()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    e = env('sparse')
    L = _L()
    err = L.lib().gm_last_error
    i = inputs(e, 0, 64)
    p = epilogue_inputs(e, 64)
    lst = torch.arange(0, e.rows, 2, device='cuda', dtype=torch.int32)
    launch(e, 0, 64, x=i.x, ldx=64, mask_h=p.mask_h, mask_b=p.mask_b, expect_rc=GM_EINVAL)
    assert b'mask_h together with mask_b' in err()
    with stream_knob():
        launch(e, 0, 64, x=i.x, ldx=64, scale=2, rowlist=lst, list_win=4, stream=True, expect_rc=GM_EINVAL)
    assert b'row list together with the stream kernel' in err()
    launch(e, 0, 32, x_src=1, expect_rc=GM_EINVAL)
    assert b'width == feat_dim' in err()
    launch(e, 0, 128, x_src=2, expect_rc=GM_EINVAL)
    assert b'width == feat_dim' in err()
    launch(e, 1, 64, x_src=2, expect_rc=GM_EINVAL)
    launch(e, 0, 64, x=i.x, ldx=64, x_src=3, expect_rc=GM_EINVAL)
    # gm_launch_aggregate's own: packed masks where the stores are not 16-byte vectors, a row list off the window kernel
    i6, p6 = inputs(e, 0, 6), epilogue_inputs(e, 8)
    launch(e, 0, 6, x=i6.x, ldx=6, mask_b=p6.mask_b, expect_rc=GM_EINVAL)
    assert b'packed relu masks' in err()
    ioff = inputs(e, 0, 64, xoff=True)
    launch(e, 0, 64, x=ioff.x, ldx=64, relu=True, bits=True, expect_rc=GM_EINVAL)
    assert b'packed relu masks' in err()
    i32 = inputs(e, 0, 32)
    launch(e, 0, 32, x=i32.x, ldx=32, rowlist=lst, list_win=4, expect_rc=GM_EINVAL)
    assert b'a row list needs the window kernel' in err()
    launch(e, 0, 64, x=ioff.x, ldx=64, rowlist=lst, list_win=4, expect_rc=GM_EINVAL)
    assert b'a row list needs the window kernel' in err()
    # the export's checks of a row list: ascending, in range, a window the kernel has, the list schedule only with the batch's own list
    bad = lst.clone()
    bad[5], bad[6] = lst[6], lst[5]
    launch(e, 0, 64, x=i.x, ldx=64, rowlist=bad, list_win=4, expect_rc=GM_EINVAL)
    bad = lst.clone()
    bad[-1] = e.rows
    launch(e, 0, 64, x=i.x, ldx=64, rowlist=bad, list_win=4, expect_rc=GM_EINVAL)
    launch(e, 0, 64, x=i.x, ldx=64, rowlist=lst, list_win=3, expect_rc=GM_EINVAL)
    launch(e, 0, 64, x=i.x, ldx=64, rowlist=lst, list_win=128, expect_rc=GM_EINVAL)
    launch(e, 0, 64, x=i.x, ldx=64, rowlist=lst, list_win=4, list_sched=True, expect_rc=GM_EINVAL)
    launch(e, 0, 64, x=i.x, ldx=64, scale=2, hubs=1, stream=True, expect_rc=GM_EINVAL)
    launch(e, 0, 64, x=i.x, ldx=64, keep=True, expect_rc=GM_EINVAL)
    launch(e, 0, 64, x=i.x, ldx=32, expect_rc=GM_EINVAL)
    launch(e, 0, 64, expect_rc=GM_EINVAL)
