"""CPU: the degree-ladder graphs and the fp64 reference of tests/agg_ref.py are what test_hip_agg_numerics.py takes them for."""
import numpy as np
import pytest
import torch

import agg_ref as R

ROWS = sum(R.SET_SUBS) * R.N


@pytest.fixture(scope='module', params=sorted(R.VARIANTS))
def graph(request):
    return R.build_graph(request.param)


def test_ladder_degrees_both_orientations(graph):
    g = graph
    din, dout = R.degrees(g)
    L = len(g.lad)
    assert list(din[g.a0:g.a0 + L]) == g.lad and list(dout[g.b0:g.b0 + L]) == g.lad
    assert g.lad == [d for d in R.LADDER if d <= R.VARIANTS[g.variant][0]]
    # node 0 is nobody's source, the last node nobody's destination
    assert dout[0] == 0 and din[0] == 0 and din[R.N - 1] == 0
    # every other row keeps the filler's in-degree
    lo, hi = R.VARIANTS[g.variant][1]
    other = np.ones(R.N, bool)
    other[:L] = False
    other[R.N - 1] = False
    if g.g_in is not None:
        other[g.g_in] = False
        assert din[g.g_in] == R.GIANT and dout[g.g_out] == R.GIANT
        assert ((g.src == g.g_out) == (g.dst == g.g_in)).all()                 # parallel edges of one pair
    assert din[other].min() >= lo and din[other].max() <= hi
    # a batch's rows repeat the graph
    s, d, _ = R.batch_edges(g)
    assert np.array_equal(np.bincount(d, minlength=ROWS), np.tile(din, sum(R.SET_SUBS)))
    assert np.array_equal(np.bincount(s, minlength=ROWS), np.tile(dout, sum(R.SET_SUBS)))
    assert (s // R.N == d // R.N).all()


def test_parallel_edges_and_hub_self_loop(graph):
    g = graph
    key = g.src * R.N + g.dst
    assert len(np.unique(key)) < len(key)                                      # parallel edges
    if R.VARIANTS[g.variant][0] > 32:
        hub = len(g.lad) - 1
        assert ((g.src == hub) & (g.dst == hub)).sum() == 1                    # one self-loop on the largest in-degree hub


def test_density_class_and_hub_tables(graph):
    g = graph
    din, dout = R.degrees(g)
    E = len(g.src) * sum(R.SET_SUBS)
    dense = E > 8 * ROWS
    assert dense == (g.variant == 'dense')
    assert R.agg_window(ROWS, E) == (4 if dense else 2)
    for deg in (din, dout):
        th, hubs, hp, parts = R.expected_hubs(np.tile(deg, sum(R.SET_SUBS)), ROWS, E)
        assert th == (64 if dense else 32)
        if g.variant == 'flat':
            assert len(hubs) == 0 and deg.max() <= 20 and deg.max() <= th     # no row above its threshold: no hub list, no schedule
        elif g.variant == 'unsplit':
            assert len(hubs) > 0 and hp == 0 and parts == len(hubs) and deg.max() == 191
        elif g.variant == 'giant':
            assert hp == 160
        else:
            assert hp == 128
        if hp:
            by_deg = {int(d): R.hub_parts(int(d), hp) for d in deg[deg > th]}
            assert by_deg[1000] == (6 if hp == 160 else 8)
            if hp == 160:
                assert by_deg[R.GIANT] == 31 and by_deg[255] == 2 and by_deg[193] == 1
    assert R.heavy_deg_for(100, 800) == 32 and R.heavy_deg_for(100, 801) == 64


def test_restated_part_rule():
    assert R.hub_part_for(1000) == 128 and R.hub_part_for(4096) == 128 and R.hub_part_for(4097) == 144 and R.hub_part_for(R.GIANT) == 160
    got = [R.hub_parts(d, 128) for d in (191, 192, 319, 320, 1000)]
    assert got == [1, 2, 2, 3, 8]
    assert R.hub_parts(33, 128) == 1 and R.hub_parts(448, 128) == 4
    assert R.agg_window(1 << 21, 1 << 22) == 64 and R.agg_window(1 << 20, 1 << 21) == 32 and R.agg_window(141000, 300000) == 4


def test_poisoned_rows_have_no_reader(graph):
    g = graph
    s, d, _ = R.batch_edges(g)
    for read, name in ((s, 'by destination'), (d, 'by source')):
        unread = np.ones(ROWS, bool)
        unread[read] = False
        assert unread.any(), name
        x = torch.randn(ROWS, 4)
        x[torch.from_numpy(unread)] = float('nan')
        src, dst = (s, d) if read is s else (d, s)
        out, scale, deg = R.reference(ROWS, torch.from_numpy(src), torch.from_numpy(dst), None, x)
        assert torch.isfinite(out).all() and torch.isfinite(scale).all()
    assert not np.isin(0, s) and not np.isin(ROWS - 1, d) and not np.isin(0, d)      # row 0 in both orientations, the last row by source


def test_weighted_graph_has_fractional_weights():
    g = R.build_graph('sparse', weighted=True)
    assert g.w.dtype == np.float32 and len(g.w) == len(g.src) and g.w.min() >= 0.25 and g.w.max() <= 1.75
    assert (g.w != np.round(g.w)).mean() > 0.99
    h = R.build_graph('sparse')
    assert np.array_equal(g.src, h.src) and np.array_equal(g.dst, h.dst)


def test_reference_equals_dense_product_on_a_hand_graph():
    # 6 nodes: parallel edges 1 -> 0 (twice), a self-loop on 2, node 5 without in-edges, node 4 without out-edges
    src = torch.tensor([1, 1, 2, 3, 0, 2, 5, 1])
    dst = torch.tensor([0, 0, 2, 2, 3, 4, 4, 4])
    w = torch.tensor([0.5, 2.0, 1.0, 0.25, 3.0, 1.5, 0.75, 1.25])
    x = torch.randn(6, 3, dtype=torch.float64).float()
    s_out = torch.tensor([0.5, -2.0, 1.0, -0.25, 4.0, 1.0])
    bias_t = torch.randn(2, 3, dtype=torch.float64).float()
    sets = torch.tensor([0, 0, 0, 1, 1, 1])
    mask = torch.rand(6, 3) > 0.4
    for ww in (None, w):
        A = torch.zeros(6, 6, dtype=torch.float64)
        for k in range(len(src)):
            A[dst[k], src[k]] += 1.0 if ww is None else float(ww[k])
        base = A @ x.double()
        out, scale, d = R.reference(6, src, dst, ww, x)
        assert torch.equal(d, torch.tensor([2, 0, 2, 1, 3, 0]))
        assert torch.allclose(out, base, rtol=1e-15, atol=1e-15)
        assert torch.allclose(scale, A.abs() @ x.double().abs(), rtol=1e-15, atol=1e-15)
        # each epilogue option singly, then all together
        so = s_out.double().abs()[:, None]
        bb = bias_t.double()[sets]
        out, scale, _ = R.reference(6, src, dst, ww, x, s_out=s_out)
        assert torch.allclose(out, so * base, rtol=1e-15, atol=1e-15)
        out, scale, _ = R.reference(6, src, dst, ww, x, bias=bias_t[sets])
        assert torch.allclose(out, base + bb, rtol=1e-15, atol=1e-15) and torch.allclose(scale, A.abs() @ x.double().abs() + bb.abs(), rtol=1e-15, atol=1e-15)
        out, _, _ = R.reference(6, src, dst, ww, x, relu=True)
        assert torch.allclose(out, base.clamp_min(0), rtol=1e-15, atol=1e-15) and (out >= 0).all()
        out, _, _ = R.reference(6, src, dst, ww, x, mask=mask)
        assert torch.allclose(out, torch.where(mask, base, torch.zeros_like(base)), rtol=1e-15, atol=1e-15) and (out[~mask] == 0).all()
        out, scale, _ = R.reference(6, src, dst, ww, x, s_out=s_out, bias=bias_t[sets], relu=True, mask=mask)
        want = torch.where(mask, (so * base + bb).clamp_min(0), torch.zeros_like(base))
        assert torch.allclose(out, want, rtol=1e-15, atol=1e-15)
        assert torch.allclose(scale, so * (A.abs() @ x.double().abs()) + bb.abs(), rtol=1e-15, atol=1e-15)
    # the transposed orientation is the same sum with the roles swapped
    out, _, d = R.reference(6, dst, src, w, x)
    A = torch.zeros(6, 6, dtype=torch.float64)
    for k in range(len(src)):
        A[src[k], dst[k]] += float(w[k])
    assert torch.allclose(out, A @ x.double(), rtol=1e-15, atol=1e-15) and torch.equal(d, torch.tensor([1, 3, 2, 1, 0, 1]))
