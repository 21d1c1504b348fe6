"""CPU: the restatement of the fused aggregate + GEMM and the table-fed weight gradient (fused_ref.py) against two independent statements of the same
operation on random ragged sets: the plain fp64 aggregate of agg_ref.py (sum_e w_e x[src_e] from the edge list) wherever a row has at most two sources, and a
dense fp64 A_hat X W with A_hat[v, u] = sum of the weights of the edges u -> v."""
import numpy as np
import pytest
import torch

import agg_ref
import fused_ref as F

SETS = [1, 2, 3, 15, 127, 128, 129, 300]


def make(seed, weighted, K=12, N=7):
    set_rows = SETS
    rows, src, dst, w = F.build_sets(set_rows, seed, weighted)
    indptr, indices, ew = F.csr_of(rows, src, dst, w)
    norm = F.norm_of(indptr, ew)
    rng = np.random.default_rng(seed + 1)
    feat_row = rng.permutation(rows + 5)[:rows]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=gen)
    W = torch.randn(len(set_rows), K, N, generator=gen)
    bias = torch.randn(len(set_rows), N, generator=gen)
    s = torch.exp2(torch.rand(rows, generator=gen) * 4 - 2)
    # per-edge weight as the kernels take it: the fp32 product ew * norm[src]
    we = norm[indices] if ew is None else ew * norm[indices]
    es = torch.from_numpy(indices.astype(np.int64))
    ed = torch.from_numpy(np.repeat(np.arange(rows), np.diff(indptr)))
    return dict(set_rows=set_rows, rows=rows, indptr=indptr, indices=indices, ew=ew, norm=norm, feat_row=feat_row, x=x, W=W, bias=bias, s=s,
                we=torch.from_numpy(we), es=es, ed=ed, K=K, N=N)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_graph_has_every_degree_at_every_tile_edge(seed, weighted):
    c = make(seed, weighted)
    F.assert_degree_mix(c['indptr'], c['set_rows'])
    # every edge stays inside its set
    so = np.cumsum([0] + c['set_rows'])
    set_of = np.searchsorted(so, np.arange(c['rows']), side='right') - 1
    assert np.array_equal(set_of[c['indices']], set_of[c['ed'].numpy()])


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_table_layout(seed, weighted):
    """the entries by degree, the feature-row table, the counts"""
    c = make(seed, weighted)
    t, tf, (nr, ne) = F.tables(c['indptr'], c['indices'], c['norm'], c['feat_row'], c['ew'])
    d = np.diff(c['indptr'])
    assert nr == int((d > 2).sum()) and ne == int(d[d > 2].sum())
    wbits = c['we'].numpy().view(np.int32)
    for r in range(c['rows']):
        p = c['indptr'][r]
        if d[r] == 0:
            want = [F.ZERO, F.ZERO, F.ONE, 0]
            wantf = want
        elif d[r] == 1:
            u = c['indices'][p]
            want, wantf = [u, u, wbits[p], 0], [c['feat_row'][u], c['feat_row'][u], wbits[p], 0]
        elif d[r] == 2:
            u0, u1 = c['indices'][p], c['indices'][p + 1]
            want, wantf = [u0, u1, wbits[p], wbits[p + 1]], [c['feat_row'][u0], c['feat_row'][u1], wbits[p], wbits[p + 1]]
        else:
            want = [r | F.SELF, r | F.SELF, F.ONE, 0]
            wantf = want
        assert list(t[r]) == list(want) and list(tf[r]) == list(wantf), r
    centres = np.array([0, 5, c['rows'] - 1])
    dq = F.dq_table(c['rows'], centres)
    other = np.ones(c['rows'], bool)
    other[centres] = False
    assert (dq[other] == [F.ZERO, F.ZERO, 0, 0]).all()
    assert all(list(dq[r]) == [r | F.SELF, F.ZERO, F.ONE, 0] for r in centres)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_rows_product_and_gradients(seed, weighted):
    c = make(seed, weighted)
    rows, K, N = c['rows'], c['K'], c['N']
    t, tf, _ = F.tables(c['indptr'], c['indices'], c['norm'], c['feat_row'], c['ew'])
    agg, _, d = agg_ref.edge_sums(rows, c['es'], c['ed'], c['we'], c['x'])
    few = d <= 2
    # Z from the table alone where a row has at most two sources: zside and every row of x that is no source of such a row are NaN
    src_rows, own = F.table_sources(t)
    assert np.array_equal(own, ~few.numpy())
    xp = torch.full_like(c['x'], float('nan'))
    xp[src_rows] = c['x'][src_rows]
    zside = torch.full((rows, K), float('nan'))
    zside[~few] = agg[~few].float()
    z, za = F.form_rows(t, xp, zside)
    assert torch.isfinite(z).all()
    assert torch.allclose(z[few], agg[few], rtol=1e-13, atol=0)
    assert torch.equal(z[~few], zside[~few].double())
    # the feature-row table over the feature matrix: the same rows
    feats = torch.full((rows + 5, K), float('nan'))
    feats[c['feat_row'][src_rows]] = c['x'][src_rows]
    zf, _ = F.form_rows(tf, feats, zside)
    assert torch.equal(zf, z)
    # C and dW against the dense product, with a fully aggregated fp64 side buffer
    A = torch.zeros(rows, rows, dtype=torch.float64).index_put_((c['ed'], c['es']), c['we'].double(), accumulate=True)
    AX = A @ c['x'].double()
    z64, za64 = F.form_rows(t, c['x'].double(), AX)
    set_of = F.set_index(c['set_rows'], 'cpu')
    Cd = torch.einsum('rk,rkn->rn', AX, c['W'].double()[set_of]) * c['s'].double()[:, None] + c['bias'].double()[set_of]
    Cr, sc = F.gemm(z64, za64, c['set_rows'], c['W'], c['s'], c['bias'], relu=False)
    assert torch.allclose(Cr, Cd, rtol=0, atol=1e-12 * float(sc.max()))
    assert (sc >= Cr.abs() * (1 - 1e-12)).all()
    Crelu, _ = F.gemm(z64, za64, c['set_rows'], c['W'], c['s'], c['bias'], relu=True)
    assert torch.equal(Crelu, Cr.clamp_min(0))
    Cs, _ = F.gemm(z64, za64, c['set_rows'], c['W'][:1], None, None)
    assert torch.allclose(Cs, AX @ c['W'][0].double(), rtol=0, atol=1e-12 * float(sc.max()))
    gen = torch.Generator().manual_seed(seed + 9)
    G = torch.randn(rows, N, generator=gen)
    keep = torch.rand(rows, generator=gen) < 0.3
    Gp = torch.where(keep[:, None], G, torch.full_like(G, float('nan')))
    for kp, g in ((None, G), (keep, Gp)):
        dW, sW, db, sb = F.wgrad(z64, za64, c['set_rows'], g, c['s'], kp)
        g0 = G.double() if kp is None else torch.where(kp[:, None], G.double(), torch.zeros(rows, N, dtype=torch.float64))
        r0 = 0
        for ti, n in enumerate(c['set_rows']):
            want = (AX[r0:r0 + n] * c['s'].double()[r0:r0 + n, None]).T @ g0[r0:r0 + n]
            assert torch.allclose(dW[ti], want, rtol=0, atol=1e-12 * max(1.0, float(sW[ti].max())))
            assert torch.allclose(db[ti], g0[r0:r0 + n].sum(0), rtol=0, atol=1e-12 * max(1.0, float(sb[ti].max())))
            r0 += n
