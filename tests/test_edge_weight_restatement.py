"""CPU: the restatement of edge-weighted parent graphs (tests/edge_weight_ref.py) is validated before the GPU tests trust it -- bitwise against
the pinned oracle with all weights 1 (every golden fixture), against the UNPATCHED oracle on the expanded multigraph with integer weights, and
against fp64 autograd of a literal statement of the weighted GraphConv with fractional weights -- and the host-side plumbing carries weights
(edge list -> CSR order, data directory, synthetic data, declared symbols)."""
import os

import numpy as np
import pytest
import torch

import edge_weight_ref as ew
import gmeta_oracle as orc
from golden_util import CASES, Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
TOL = 1e-4                       # the project's parity tolerance (tests/test_hip_fuzz.py)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _fixture_batches(fx, graphs, make):
    spt = [make(graphs, fx.z['spt_seeds'][t], fx.args['h'], fx.args['sample_nodes'], 222, fx.link, replay_nodes=fx.replay_lists('spt', t)) for t in range(fx.T)]
    qry = [make(graphs, fx.z['qry_seeds'][t], fx.args['h'], fx.args['sample_nodes'], 222, fx.link, replay_nodes=fx.replay_lists('qry', t)) for t in range(fx.T)]
    return spt, qry


def _step(fx, spt, qry, weighted, theta=None):
    a = (fx.feats, spt, qry, fx.z['y_spt'], fx.z['y_qry'], fx.vars0 if theta is None else theta, fx.config, fx.args['k_spt'], fx.args['update_lr'], fx.args['meta_lr'], fx.K)
    if weighted:
        return ew.meta_step(*a)
    accs, grad, _, lq = orc.meta_step(None, *a, adam_state={})
    return accs, grad, lq


@pytest.mark.parametrize('case', CASES)
def test_unit_weights_are_the_oracle_bit_for_bit(case):
    """All weights 1.0: the weighted batch has the oracle's norm, and the patched meta-step returns exactly the unpatched one's arrays (query
    losses, accuracies, every meta-gradient array, NaN positions included).  The patch is undone afterwards."""
    fx = Fixture(case)
    spt, qry = _fixture_batches(fx, fx.graphs(), orc.extract_batch)
    wspt, wqry = _fixture_batches(fx, ew.unit_graphs(fx.edges), ew.extract_batch)
    for a, b in zip(spt + qry, wspt + wqry):
        assert _same(a.indptr, b.indptr) and _same(a.indices, b.indices) and _same(a.norm, b.norm) and (b.ew == 1).all()
    saved = (orc.agg, orc.agg_t)
    want, got = _step(fx, spt, qry, False), _step(fx, wspt, wqry, True)
    assert (orc.agg, orc.agg_t) == saved
    assert _same(want[0], got[0]) and _same(want[2], got[2])
    assert len(want[1]) == len(got[1]) and all(_same(g, h) for g, h in zip(want[1], got[1]))


@pytest.mark.parametrize('case', ['g0_disjoint_h1', 'g1_sampled_h2', 'g2_shared', 'g3_linkpred', 'g5_in_gt_out', 'g7_wide_h2'])
def test_integer_weights_equal_the_expanded_multigraph(case):
    """Weights in {1, 2, 3}: the restatement on the weighted graph against the UNPATCHED oracle on the multigraph in which edge u->v is repeated
    w_uv times.  Same node sets (extraction is topological), same norm bit for bit (an integer degree either way); losses, accuracies and the
    meta-gradient within the parity tolerance (the two sum the same terms in another grouping: w * x once against x added w times).
    The fixtures' biases start at zero (learner.py:96), which puts a centre without in-edges exactly on the relu kink, where rounding noise in a
    mathematically zero bias gradient decides relu' in the later inner steps -- a property of the model, not of either implementation
    (tests/test_hip_fuzz.py conditions its comparison the same way): every bias is moved off the kink first."""
    fx = Fixture(case)
    rng = np.random.default_rng(11)
    theta = [t if t.ndim > 1 else (rng.uniform(0.15, 0.4, size=t.shape) * rng.choice([-1.0, 1.0], size=t.shape)).astype(f32) for t in fx.vars0]
    wts = [rng.integers(1, 4, size=len(s)).astype(f32) for n, s, d in fx.edges]
    wg = [ew.Graph(n, s, d, w) for (n, s, d), w in zip(fx.edges, wts)]
    mg = [orc.Graph(*ew.expand(n, s, d, w)) for (n, s, d), w in zip(fx.edges, wts)]
    wspt, wqry = _fixture_batches(fx, wg, ew.extract_batch)
    mspt, mqry = _fixture_batches(fx, mg, orc.extract_batch)
    for a, b in zip(mspt + mqry, wspt + wqry):
        assert _same(a.parent, b.parent) and _same(a.centre_rows, b.centre_rows) and _same(a.norm, b.norm)
        assert len(a.indices) == int(b.ew.sum()) and _same(a.indices, np.repeat(b.indices, b.ew.astype(np.int64)))
    want, got = _step(fx, mspt, mqry, False, theta), _step(fx, wspt, wqry, True, theta)
    np.testing.assert_allclose(got[2], want[2], atol=TOL, rtol=1e-4)
    gw, gg = np.concatenate([g.reshape(-1) for g in want[1]]), np.concatenate([g.reshape(-1) for g in got[1]])
    np.testing.assert_allclose(gg, gw, atol=TOL * max(1.0, float(np.abs(gw).max())), rtol=1e-3)
    assert np.abs(np.asarray(got[0]) - np.asarray(want[0])).max() <= 1.0 / len(fx.z['y_qry'][0]) + 1e-9


# ---------------------------------------------------------------------------------------------------- fractional weights against fp64 autograd
def _tiny():
    """12 nodes: a self loop, parallel edges, an isolated node (11), a node without in-edges (0), in-degrees 1..5; two subgraphs that overlap."""
    src = np.array([0, 0, 1, 2, 2, 3, 3, 3, 4, 5, 5, 6, 7, 8, 8, 9, 1, 4, 6, 10, 2], np.int64)
    dst = np.array([1, 2, 2, 3, 3, 3, 4, 5, 5, 6, 1, 7, 8, 9, 4, 10, 9, 9, 9, 9, 9], np.int64)
    n = 12
    seeds = np.array([(0, 9, -1), (0, 3, -1), (0, 11, -1), (0, 0, -1)], np.int32)
    lists = [np.array([1, 2, 4, 6, 8, 9, 10]), np.array([0, 1, 2, 3, 5]), np.array([11]), np.array([0, 2])]
    return n, src, dst, seeds, lists


def _literal(n, src, dst, w, seeds, lists, x, theta, config, R):
    """The weighted GraphConv stack, literally, in torch (any dtype): per subgraph a dense adjacency A[v, u] = sum of w over the edges u->v
    inside it, d = A 1, norm = (d > 0 ? d : 1)^-0.5, layers relu(norm * (A (norm * h)) W + b) in either product order; loss = sum(logits * R)."""
    gcn, lin, _ = orc.parse_config(config)
    outs = []
    for (g, i, j), nodes in zip(seeds.tolist(), lists):
        nodes = list(map(int, nodes)); loc = {v: k for k, v in enumerate(nodes)}
        A = torch.zeros((len(nodes), len(nodes)), dtype=x.dtype)
        for u, v, ww in zip(src.tolist(), dst.tolist(), w.tolist()):
            if u in loc and v in loc:
                A[loc[v], loc[u]] += ww
        d = A.sum(1)
        norm = torch.where(d > 0, d, torch.ones_like(d)).pow(-0.5)[:, None]
        h = x[nodes]
        for l, (fi, fo) in enumerate(gcn):
            W, b = theta[2 * l], theta[2 * l + 1]
            xs = h * norm
            pre = A @ (xs @ W) if fi > fo else (A @ xs) @ W
            h = torch.relu(pre * norm + b)
        outs.append(h[loc[i]])
    logits = torch.stack(outs) @ theta[2 * len(gcn)].T + theta[2 * len(gcn) + 1]
    return (logits * R).sum()


def _gap(config, weights, seed, literal_weights=None):
    """max |fp32 restatement gradient - fp64 autograd gradient| / max |fp64 gradient| over every parameter array."""
    n, src, dst, seeds, lists = _tiny()
    rng = np.random.default_rng(seed)
    gcn, lin, _ = orc.parse_config(config)
    x = rng.standard_normal((n, gcn[0][0])).astype(f32)
    theta = []
    for fi, fo in gcn:
        theta += [(rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(f32), rng.uniform(0.1, 0.3, fo).astype(f32)]
    theta += [(rng.standard_normal((lin[1], lin[0])) / np.sqrt(lin[0])).astype(f32), rng.standard_normal(lin[1]).astype(f32)]
    R = rng.standard_normal((len(seeds), lin[1])).astype(f32)
    if weights is None:                                    # the unweighted oracle, unpatched
        b = orc.Batch([orc.Graph(n, src, dst)], seeds, lists)
        logits, cache = orc.classifier_forward(b, x[b.parent], theta, config)
        grads = orc.classifier_backward(b, theta, config, cache, R)
        w = np.ones(len(src))
    else:
        b = ew.Batch([ew.Graph(n, src, dst, weights)], seeds, lists)
        with ew.patched([b]):
            logits, cache = orc.classifier_forward(b, x[b.parent], theta, config)
            grads = orc.classifier_backward(b, theta, config, cache, R)
        w = np.asarray(weights if literal_weights is None else literal_weights, np.float64)
    t64 = [torch.tensor(v.astype(np.float64), requires_grad=True) for v in theta]
    L = _literal(n, src, dst, w, seeds, lists, torch.tensor(x.astype(np.float64)), t64, config, torch.tensor(R.astype(np.float64)))
    g64 = torch.autograd.grad(L, t64)
    if literal_weights is None:
        assert abs(float((logits.astype(np.float64) * R).sum()) - float(L.detach())) <= 1e-4 * max(1.0, abs(float(L.detach())))
    num = max(float(np.abs(g.astype(np.float64) - h.numpy()).max()) for g, h in zip(grads, g64))
    return num / max(float(h.abs().max()) for h in g64)


@pytest.mark.parametrize('config', [[('GraphConv', [6, 10]), ('GraphConv', [10, 10]), ('Linear', [10, 3])],
                                    [('GraphConv', [12, 5]), ('GraphConv', [5, 8]), ('Linear', [8, 3])]], ids=['aggregate_first', 'multiply_first'])
def test_fractional_weight_gradients_match_fp64_autograd(config):
    """Log-uniform weights in [0.25, 4], not symmetric, on the 12-node graph of _tiny(), both branch orders of learner.py:34-47.  The bound is not
    chosen in advance: it is 4x the gap the UNWEIGHTED, unpatched oracle shows against the same literal statement on the same graph, parameters
    and loss (relative to the largest fp64 gradient entry, so that the larger activations weights up to 4 produce do not enter the comparison).
    Measured here -- aggregate_first: unweighted gap 6.60e-08, weighted 8.63e-08; multiply_first: unweighted 8.86e-08, weighted 8.86e-08 (there the
    largest error sits in the head's bias gradient, which no weight reaches)."""
    n, src, dst, _, _ = _tiny()
    w = np.exp(np.random.default_rng(5).uniform(np.log(0.25), np.log(4.0), len(src))).astype(f32)
    base = _gap(config, None, 7)
    got = _gap(config, w, 7)
    print('fp32-vs-fp64 relative gradient gap: unweighted oracle %.3g, weighted restatement %.3g' % (base, got))
    assert 0 < base < 1e-5
    assert got <= 4 * base
    # and the comparison can tell: against the literal statement with the weights dropped the same gradients are off by orders of magnitude
    assert _gap(config, w, 7, literal_weights=np.ones(len(src))) > 1e4 * base


def test_weighted_norm_sums_in_edge_order_and_clamps_only_at_zero():
    indptr = np.array([0, 0, 1, 4, 6])
    w = np.array([0.25, 1e8, 1.0, -0.0 + 1.0, 0.3, 0.2], f32)
    got = ew.weighted_norm(indptr, w)
    d2 = f32(f32(f32(1e8) + f32(1.0)) + f32(1.0))
    want = np.array([1.0, f32(0.25) ** f32(-0.5), d2 ** f32(-0.5), f32(f32(0.3) + f32(0.2)) ** f32(-0.5)], f32)
    assert np.array_equal(got, want)
    assert got[1] == 2.0                                   # a degree below 1 is NOT clamped: clamp(min=1) of the multigraph only ever acts at degree 0


# ---------------------------------------------------------------------------------------------------- host plumbing (no GPU)
def test_edges_to_in_csr_carries_weights_through_its_stable_order():
    from gmeta_amd.graphstore import edges_to_in_csr
    src = np.array([3, 0, 3, 1, 0, 2]); dst = np.array([1, 2, 1, 0, 2, 1]); w = np.array([.5, 2, 3, 4, 5, 6], f32)
    ip, ix, cw = edges_to_in_csr(4, src, dst, w)
    assert ip.tolist() == [0, 1, 4, 6, 6] and ix.tolist() == [1, 3, 3, 2, 0, 0] and cw.tolist() == [4, .5, 3, 6, 2, 5]
    ip2, ix2 = edges_to_in_csr(4, src, dst)
    assert np.array_equal(ip, ip2) and np.array_equal(ix, ix2)
    G = ew.Graph(4, src, dst, w)
    assert np.array_equal(G.w, cw) and np.array_equal(G.indices, ix)
    with pytest.raises(ValueError, match='one weight per edge'):
        edges_to_in_csr(4, src, dst, w[:3])


def test_datadir_round_trips_optional_weights(tmp_path):
    from gmeta_amd import datadir
    g = [(4, np.array([0, 1, 2]), np.array([1, 2, 3])), (3, np.array([0]), np.array([2]))]
    datadir.save_graphs(str(tmp_path), g)
    back = datadir.load_graphs(str(tmp_path))
    assert all(len(b) == 3 for b in back)                  # files without g{g}_w load exactly as before
    gw = [g[0] + (np.array([.5, 1.5, 2.5], f32),), g[1] + (np.array([3.0], f32),)]
    datadir.save_graphs(str(tmp_path), gw)
    back = datadir.load_graphs(str(tmp_path))
    assert all(len(b) == 4 for b in back)
    for a, b in zip(gw, back):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and b[3].dtype == np.float32


def test_synth_emits_weights_on_request():
    from gmeta_amd import synth
    c = dict(synth.CONFIGS['syn0'], n=300)
    plain, wd = synth.make_dataset(c), synth.make_dataset(c, edge_weights=True)
    (n, s, d), (n2, s2, d2, w) = plain['graphs'][0], wd['graphs'][0]
    assert n == n2 and np.array_equal(s, s2) and np.array_equal(d, d2) and w.dtype == np.float32 and len(w) == len(s)
    assert w.min() >= 0.25 and w.max() <= 4.0 and len(np.unique(w)) > len(w) // 4
    rev = {(int(a), int(b)): float(x) for a, b, x in zip(s2, d2, w)}
    assert all(rev[(b, a)] == x for (a, b), x in rev.items())          # an edge and its reverse share a weight: the stored graph stays symmetric
    asym = synth.with_edge_weights(plain['graphs'], symmetric=False)[0][3]
    assert not np.array_equal(asym, w)


def test_new_symbols_are_declared():
    from gmeta_amd import _lib
    for name in ('gm_store_create_weighted', 'gm_store_weighted', 'gm_batch_weighted'):
        assert name in _lib.PROTOTYPES
    assert (_lib.F_EDGE_W, _lib.F_EDGE_W_T) == (13, 14) and _lib.F_NORM_CENTRE == 12          # appended at the end of gm_field
    hdr = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    assert 'int gm_store_create_weighted(' in hdr and 'int32_t gm_store_weighted(const gm_store_t* s);' in hdr and 'int32_t gm_batch_weighted(const gm_batch_t* b);' in hdr
    assert hdr.index('GM_F_NORM_CENTRE,') < hdr.index('GM_F_EDGE_W,') < hdr.index('GM_F_EDGE_W_T ')
    _lib.lib()                                             # (raises AttributeError when a declared symbol is not exported)
