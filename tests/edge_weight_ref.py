"""CPU restatement of edge-weighted parent graphs (include/gmeta_hip.h, gm_store_create_weighted) out of the oracle's own pieces.

    d(v)    = sum of w_uv over the in-edges of v inside its subgraph, fp32, in the row's edge order
    norm(v) = (d(v) > 0 ? d(v) : 1) ** -0.5
    GraphConv: relu(norm(v) * sum_{u->v} w_uv * norm(u) * x[u] W + b); the backward uses the same coefficients by source.

Extraction is topological, so node sets, CSR and centres are the oracle's.  A weighted `Batch` is the oracle's Batch with the induced weights
(`ew`, aligned with `indices`) and the weighted norm.  orc.classifier_forward / classifier_backward call `agg`, `agg_t` and `batch.norm` by
module-level name or attribute, so `patched(...)` swaps weighted versions of the two aggregates in (and restores them): the oracle's inner
loop, meta-gradient included, then runs on weighted batches without a line of oracle/ changing.  The weighted aggregates scale every edge's
source row by its weight and hand the scaled rows to the oracle's OWN aggregate, one row per edge in edge order: with all weights 1 they
perform the oracle's operations in the oracle's order (tests/test_edge_weight_restatement.py holds them to bitwise equality on every
fixture, to the unpatched oracle on the expanded multigraph for integer weights, and to fp64 autograd for fractional ones)."""
import contextlib

import numpy as np

import gmeta_oracle as orc

f32 = np.float32


class Graph(orc.Graph):
    """orc.Graph with one weight per edge, carried through the same stable sort (`w` is aligned with `indices`)."""

    def __init__(self, n, src, dst, w):
        super().__init__(n, src, dst)
        w = np.asarray(w, f32).reshape(-1)
        assert len(w) == len(self.indices)
        self.w = np.ascontiguousarray(w[np.argsort(np.asarray(dst, np.int64), kind='stable')])


def induce_weights(G, nodes):
    """The weights of the edges orc.induce(G, nodes) keeps, in its order."""
    nodes = np.asarray(nodes, np.int64)
    inside = np.zeros(G.n, bool); inside[nodes] = True
    out = []
    for v in nodes:
        a, b = G.indptr[v], G.indptr[v + 1]
        out.append(G.w[a:b][inside[G.indices[a:b]]])
    return np.concatenate(out).astype(f32) if out else np.zeros(0, f32)


def weighted_norm(indptr, ew):
    d = np.zeros(len(indptr) - 1, f32)
    np.add.at(d, np.repeat(np.arange(len(d)), np.diff(indptr)), np.asarray(ew, f32))      # unbuffered: one fp32 add per edge, in edge order
    return np.power(np.where(d > 0, d, f32(1)).astype(f32), f32(-0.5)).astype(f32)


class Batch(orc.Batch):
    def __init__(self, graphs, seeds, node_lists):
        super().__init__(graphs, seeds, node_lists)
        self.ew = np.concatenate([induce_weights(graphs[g], nodes) for (g, i, j), nodes in zip(seeds, node_lists)] + [np.zeros(0, f32)]).astype(f32)
        assert len(self.ew) == len(self.indices)
        self.norm = weighted_norm(self.indptr, self.ew)

    def by_source(self):
        """(indptr_t, destinations, weights) of the same edges grouped by source, destinations in edge order (orc._by_source's order)."""
        ptr, dst = orc._by_source(self)
        return ptr, dst, self.ew[np.argsort(self.indices, kind='stable')]


def extract_batch(graphs, seeds, h, sample_n, rng_seed, link_pred, replay_nodes=None):
    """orc.extract_batch on weighted graphs: the oracle's node sets, a weighted Batch."""
    ob = orc.extract_batch(graphs, seeds, h, sample_n, rng_seed, link_pred, replay_nodes)
    lists = [ob.parent[ob.sub_off[s]:ob.sub_off[s + 1]] for s in range(ob.S)]
    return Batch(graphs, seeds, lists)


_ORIG_AGG = orc.agg


def _edge_rows(w, x, src):
    return (np.asarray(w, f32)[:, None] * np.ascontiguousarray(x, f32)[src]).astype(f32)


def make(batches):
    """(agg, agg_t) for the given weighted batches; agg finds its batch by the identity of the `indices` array it is handed."""
    by_id = {id(b.indices): b for b in batches}

    def agg(indptr, indices, x):
        b = by_id[id(indices)]
        return _ORIG_AGG(indptr, np.arange(len(indices), dtype=np.int64), _edge_rows(b.ew, x, indices))

    def agg_t(batch, g):
        ptr, dst, w = batch.by_source()
        return _ORIG_AGG(ptr, np.arange(len(dst), dtype=np.int64), _edge_rows(w, g, dst))
    return agg, agg_t


@contextlib.contextmanager
def patched(batches):
    saved = (orc.agg, orc.agg_t)
    orc.agg, orc.agg_t = make(batches)
    try:
        yield
    finally:
        orc.agg, orc.agg_t = saved


def unit_graphs(edges):
    return [Graph(n, s, d, np.ones(len(s), f32)) for n, s, d in edges]


def expand(n, src, dst, w):
    """The multigraph in which edge u->v is repeated w_uv times (integer weights), repeats adjacent in edge order."""
    k = np.asarray(w).astype(np.int64)
    assert np.array_equal(k, np.asarray(w)) and (k >= 1).all()
    return n, np.repeat(np.asarray(src, np.int64), k), np.repeat(np.asarray(dst, np.int64), k)


def meta_step(feats, spt, qry, y_spt, y_qry, theta, config, k_spt, update_lr, meta_lr, K):
    """orc.meta_step over weighted batches: accs, grad, losses_q."""
    with patched(list(spt) + list(qry)):
        accs, grad, _, lq = orc.meta_step(None, feats, spt, qry, y_spt, y_qry, theta, config, k_spt, update_lr, meta_lr, K, adam_state={})
    return accs, grad, lq


def finetune(feats, spt, qry, y_spt, y_qry, theta, config, k_spt, update_lr, K_test):
    with patched([spt, qry]):
        return orc.finetune(None, feats, spt, qry, y_spt, y_qry, theta, config, k_spt, update_lr, K_test)
