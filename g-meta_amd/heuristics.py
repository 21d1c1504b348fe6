"""Neighbourhood heuristics as a link-prediction baseline: the scores of GraphStore.pair_scores (gm_store_pair_scores; the definition is in
include/gmeta_hip.h) turned into the ROC AUC a learned link predictor is held against.  The scores come from the device; the AUC is host work over
one number per pair.  The path scores one step further -- the local path index and the truncated Katz index -- are formed here, in float64, from the exact walk
counts of GraphStore.pair_walks (gm_store_pair_walks).  The one global score, rooted PageRank, is the float64 sum of the two columns of
GraphStore.pair_pagerank (gm_store_pair_pagerank).  Graph distance is the negated byte of GraphStore.pair_distance (gm_store_pair_distance).
The joint hop-distance tables of GraphStore.pair_distance_profile (gm_store_pair_distance_profile) are no score: link_distance_profiles orients them by the
pair's name and distance_profile_features turns them into input features.  Their ESTIMATES for every pair come from the node sketches of GraphStore.sketches
(gm_store_sketch_build / gm_sketch_pair_counts): hll_cardinality, sketch_intersections and sketch_distance_profile form them in float64 from the integers,
link_sketch_profiles orients them by the pair's name and sketch_profile_features gives the same feature shape; link_sketch_features is that chain in one call
on the device (gm_sketch_pair_features).  link_propagated_features is their twin for the
hop-propagated node features of GraphStore.propagated_features (gm_store_propagate_build / gm_prop_pair_features): the other input of a BUDDY predictor."""
import numpy as np

from ._lib import DIST_UNREACHED
from .negatives import _pair

PAIR_SCORES = ('cn', 'jaccard', 'adamic_adar', 'resource_allocation', 'pref_attachment')      # the columns of GraphStore.pair_scores, in order
PATH_SCORES = ('local_path', 'katz')                                                          # the scores made of GraphStore.pair_walks' three columns
PAGERANK_SCORES = ('rooted_pagerank',)                                                        # the score made of GraphStore.pair_pagerank's two columns
DISTANCE_SCORES = ('graph_distance',)                                                        # the score made of GraphStore.pair_distance's byte


def link_auc(scores, labels):
    """ROC AUC of `scores` against the 0 / 1 `labels` (numbers or the tables' strings) in the Mann-Whitney form: the positives' rank sum, tied scores
    sharing the average of their ranks -- the probability that a positive outranks a negative, a tie counting one half.  ValueError unless both labels
    occur, on any other label and on a score that is not finite."""
    s = np.asarray(scores, np.float64).reshape(-1)
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    if len(s) != len(y):
        raise ValueError('link_auc: %d scores, %d labels' % (len(s), len(y)))
    if not np.isin(y, (0, 1)).all():
        raise ValueError('link_auc: labels must be 0 or 1')
    n_pos = int(y.sum()); n_neg = len(y) - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError('link_auc needs both labels: %d positive(s), %d negative(s)' % (n_pos, n_neg))
    if not np.isfinite(s).all():
        raise ValueError('link_auc: a score is not finite')
    _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
    rank = (np.cumsum(cnt) - (cnt - 1) / 2.0)[inv]                  # 1-based; a tie group shares the mean of the ranks it spans
    return float((rank[y == 1].sum() - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * n_neg))


def _per_graph(store, names, width, dtype, call):
    """`dtype` [len(names), width]: call(g, pairs) of the pairs named 'g_i_j', one call per graph, rows in the order of `names`."""
    trip = np.asarray([_pair(nm) for nm in names], np.int64).reshape(-1, 3)
    out = np.zeros((len(trip), width), dtype)
    for g in np.unique(trip[:, 0]).tolist():
        at = np.nonzero(trip[:, 0] == g)[0]
        out[at] = call(g, trip[at, 1:])
    return out


def link_heuristic_scores(store, names, mask_target=False):
    """float32 [len(names), 5]: GraphStore.pair_scores of the pairs named 'g_i_j', one call per graph, rows in the order of `names`."""
    return _per_graph(store, names, len(PAIR_SCORES), np.float32, lambda g, p: store.pair_scores(g, p, mask_target=mask_target))


def link_heuristic_auc(store, names, labels, mask_target=False):
    """{score name: ROC AUC} of the five heuristics over the pairs `names` ('g_i_j') with the 0 / 1 `labels` of a link table, all graphs together.
    mask_target as in GraphStore.pair_scores: pass True when the positive pairs are edges of the store's graphs."""
    sc = link_heuristic_scores(store, names, mask_target)
    return {nm: link_auc(sc[:, k], labels) for k, nm in enumerate(PAIR_SCORES)}


def local_path_index(walks, eps=0.01):
    """float64 [m]: w2 + eps * w3 of the int64 [m, 3] walk counts (w1, w2, w3) -- A^2 + eps A^3 at the pair."""
    w = np.asarray(walks, np.int64).reshape(-1, 3).astype(np.float64)
    return w[:, 1] + float(eps) * w[:, 2]


def katz_index(walks, beta=0.005):
    """float64 [m]: beta * w1 + beta^2 * w2 + beta^3 * w3 of the int64 [m, 3] walk counts -- the Katz index truncated after the walks of length three."""
    w = np.asarray(walks, np.int64).reshape(-1, 3).astype(np.float64)
    b = float(beta)
    return b * w[:, 0] + b ** 2 * w[:, 1] + b ** 3 * w[:, 2]


def link_path_scores(store, names, mask_target=False):
    """int64 [len(names), 3]: GraphStore.pair_walks of the pairs named 'g_i_j', one call per graph, rows in the order of `names`."""
    return _per_graph(store, names, 3, np.int64, lambda g, p: store.pair_walks(g, p, mask_target=mask_target))


def link_path_auc(store, names, labels, mask_target=False, eps=0.01, beta=0.005):
    """{score name: ROC AUC} of the two path scores (PATH_SCORES) over the pairs `names` ('g_i_j') with the 0 / 1 `labels` of a link table, all graphs together;
    mask_target as in link_heuristic_auc."""
    w = link_path_scores(store, names, mask_target)
    return {'local_path': link_auc(local_path_index(w, eps), labels), 'katz': link_auc(katz_index(w, beta), labels)}


def rooted_pagerank_index(cols):
    """float64 [m]: pi_u(v) + pi_v(u) of the float32 [m, 2] columns of GraphStore.pair_pagerank -- the symmetric rooted PageRank score of a pair."""
    c = np.asarray(cols, np.float32).reshape(-1, 2).astype(np.float64)
    return c[:, 0] + c[:, 1]


def link_pagerank_scores(store, names, mask_target=False, alpha=0.15, iters=20):
    """float32 [len(names), 2]: GraphStore.pair_pagerank of the pairs named 'g_i_j', one call per graph, rows in the order of `names`."""
    return _per_graph(store, names, 2, np.float32, lambda g, p: store.pair_pagerank(g, p, mask_target=mask_target, alpha=alpha, iters=iters))


def link_pagerank_auc(store, names, labels, mask_target=False, alpha=0.15, iters=20):
    """{'rooted_pagerank': ROC AUC} (PAGERANK_SCORES) over the pairs `names` ('g_i_j') with the 0 / 1 `labels` of a link table, all graphs together;
    mask_target as in link_heuristic_auc."""
    return {'rooted_pagerank': link_auc(rooted_pagerank_index(link_pagerank_scores(store, names, mask_target, alpha, iters)), labels)}


def graph_distance_index(dist, max_dist):
    """float64 [m]: -d of the uint8 [m] distances of GraphStore.pair_distance, an unreached pair (DIST_UNREACHED) at -(max_dist + 1): a closer pair ranks
    higher and an unreached one below everything reached."""
    d = np.asarray(dist, np.uint8).reshape(-1)
    return -np.where(d == DIST_UNREACHED, int(max_dist) + 1, d).astype(np.float64)


def link_distance_scores(store, names, mask_target=False, max_dist=8):
    """uint8 [len(names)]: GraphStore.pair_distance of the pairs named 'g_i_j', one call per graph, in the order of `names`."""
    return _per_graph(store, names, 1, np.uint8, lambda g, p: store.pair_distance(g, p, mask_target=mask_target, max_dist=max_dist).reshape(-1, 1)).reshape(-1)


def link_distance_auc(store, names, labels, mask_target=False, max_dist=8):
    """{'graph_distance': ROC AUC} (DISTANCE_SCORES) over the pairs `names` ('g_i_j') with the 0 / 1 `labels` of a link table, all graphs together; the many
    pairs at one distance tie and count one half each (link_auc).  mask_target as in link_heuristic_auc."""
    return {'graph_distance': link_auc(graph_distance_index(link_distance_scores(store, names, mask_target, max_dist), max_dist), labels)}


def link_distance_profiles(store, names, mask_target=False, max_dist=3):
    """int32 [len(names), D + 2, D + 2], D = max_dist: GraphStore.pair_distance_profile of the pairs named 'g_i_j', one call per graph, rows in the order of
    `names`, each table in the orientation of its name: entry [a][b] counts the nodes a hops from i and b hops from j (the store's table is that of
    (min, max): a name with i > j gets the transpose)."""
    side = int(max_dist) + 2
    flat = _per_graph(store, names, side * side, np.int32,
                      lambda g, p: np.asarray(store.pair_distance_profile(g, p, mask_target=mask_target, max_dist=max_dist), np.int32).reshape(len(p), side * side))
    out = flat.reshape(-1, side, side)
    trip = np.asarray([_pair(nm) for nm in names], np.int64).reshape(-1, 3)
    swap = trip[:, 1] > trip[:, 2]
    out[swap] = out[swap].transpose(0, 2, 1)
    return out


def distance_profile_features(profiles, symmetric=True):
    """float64 [m, (D + 2)^2]: the [m, D + 2, D + 2] tables of link_distance_profiles as input features of a learned link predictor: log1p of the counts,
    row-major.  symmetric=True (default) takes log1p(P + P^T), which does not depend on the orientation of the pair; False log1p(P)."""
    p = np.asarray(profiles, np.int64)
    if p.ndim != 3 or p.shape[1] != p.shape[2]:
        raise ValueError('distance_profile_features: tables of shape %s; [m, D + 2, D + 2]' % (p.shape,))
    if symmetric:
        p = p + p.transpose(0, 2, 1)
    return np.log1p(p.astype(np.float64)).reshape(len(p), p.shape[1] * p.shape[2])


def hll_cardinality(zeros, zsum, p):
    """float64, the shape of `zeros`: the HyperLogLog estimate of a set's size from its m = 2^p registers' two integers -- `zeros` registers equal to 0 and
    `zsum` = the sum of 2^(32 - register), as NodeSketches.pair_counts returns them.  E = alpha_m m^2 / (zsum / 2^32); where E <= 2.5 m and zeros > 0 the
    linear count m ln(m / zeros) takes its place.  alpha = 0.673, 0.697, 0.709 at m = 16, 32, 64, else 0.7213 / (1 + 1.079 / m).  No large-range correction:
    a ball holds fewer than 2^31 nodes.  An all-zero record (zsum == 0: the C call's answer for a node outside the graph) gives 0."""
    p = int(p)
    if not 4 <= p <= 10:
        raise ValueError('hll_cardinality: p = %d; 4 .. 10' % p)
    m = float(1 << p)
    alpha = {16: 0.673, 32: 0.697, 64: 0.709}.get(1 << p, 0.7213 / (1.0 + 1.079 / m))
    z = np.asarray(zeros, np.int64).astype(np.float64)
    s = np.asarray(zsum, np.int64).astype(np.float64) / 4294967296.0
    with np.errstate(divide='ignore', invalid='ignore'):
        est = np.where(s > 0, alpha * m * m / s, 0.0)
        lin = m * np.log(m / np.where(z > 0, z, 1.0))
    return np.where((s > 0) & (est <= 2.5 * m) & (z > 0), lin, est)


def sketch_intersections(counts, p, k):
    """float64 [m, H + 1, H + 1]: the estimate of |B_a(u) & B_b(v)| from the int64 [m, H + 1, H + 1, 3] counts of NodeSketches.pair_counts: the MinHash
    Jaccard match / k times the HyperLogLog cardinality of the union."""
    c = np.asarray(counts, np.int64)
    if c.ndim != 4 or c.shape[1] != c.shape[2] or c.shape[3] != 3:
        raise ValueError('sketch_intersections: counts of shape %s; [m, H + 1, H + 1, 3]' % (c.shape,))
    return c[..., 0].astype(np.float64) / float(int(k)) * hll_cardinality(c[..., 1], c[..., 2], p)


def sketch_distance_profile(counts, balls, n_nodes, p, k):
    """float64 [m, H + 2, H + 2]: the estimate of GraphStore.pair_distance_profile(max_dist=H), unmasked, in its layout, from the two results of
    NodeSketches.pair_counts.  With C = sketch_intersections (cumulative: nodes within a of u AND within b of v), the inner cells are the 2-D difference
    C[a][b] - C[a-1][b] - C[a][b-1] + C[a-1][b-1] (C[-1][.] = C[.][-1] = 0); row and column H + 1 are the differences of the ball sizes (hll_cardinality of
    `balls`) minus the inner row / column sums; the corner is n_nodes minus everything else, so every table sums to n_nodes.  Estimates are NOT clipped: a
    cell may come out slightly negative (sketch_profile_features clips)."""
    c = sketch_intersections(counts, p, k)
    b = np.asarray(balls, np.int64)
    m, L = c.shape[0], c.shape[1]
    if b.shape != (m, 2, L, 2):
        raise ValueError('sketch_distance_profile: balls of shape %s for counts of shape %s; [m, 2, H + 1, 2]' % (b.shape, np.shape(counts)))
    size = hll_cardinality(b[..., 0], b[..., 1], p)                            # [m, 2, L]: |B_a(u)|, |B_a(v)|
    ring = np.diff(size, axis=2, prepend=0.0)
    inner = np.diff(np.diff(c, axis=1, prepend=0.0), axis=2, prepend=0.0)
    out = np.zeros((m, L + 1, L + 1), np.float64)
    out[:, :L, :L] = inner
    out[:, :L, L] = ring[:, 0] - inner.sum(2)
    out[:, L, :L] = ring[:, 1] - inner.sum(1)
    out[:, L, L] = float(n_nodes) - out.reshape(m, -1).sum(1)
    return out


def link_sketch_profiles(sketches_by_graph, names):
    """float64 [len(names), H + 2, H + 2]: sketch_distance_profile of the pairs named 'g_i_j' from sketches_by_graph[g] (a dict or a sequence of
    NodeSketches with one `hops`), one pair_counts call per graph, rows in the order of `names`, each table in the orientation of its name as
    link_distance_profiles orients the exact ones (a name with i > j gets the transpose)."""
    trip = np.asarray([_pair(nm) for nm in names], np.int64).reshape(-1, 3)
    graphs = np.unique(trip[:, 0]).tolist()
    hops = {int(sketches_by_graph[g].hops) for g in graphs}
    if len(hops) > 1:
        raise ValueError('link_sketch_profiles: sketches of different hops %s' % sorted(hops))
    side = (hops.pop() if hops else 0) + 2
    out = np.zeros((len(trip), side, side), np.float64)
    for g in graphs:
        sk = sketches_by_graph[g]
        at = np.nonzero(trip[:, 0] == g)[0]
        counts, balls = sk.pair_counts(trip[at, 1:])
        out[at] = sketch_distance_profile(counts, balls, sk.n_nodes, sk.p, sk.k)
    swap = trip[:, 1] > trip[:, 2]
    out[swap] = out[swap].transpose(0, 2, 1)
    return out


def sketch_profile_features(tables, symmetric=True):
    """float64 [m, (H + 2)^2]: the estimated tables of link_sketch_profiles as input features, in the shape distance_profile_features gives for the exact
    ones (either feeds the same predictor): log1p(max(P, 0)) row-major, P + P^T in place of P when symmetric (default)."""
    t = np.asarray(tables, np.float64)
    if t.ndim != 3 or t.shape[1] != t.shape[2]:
        raise ValueError('sketch_profile_features: tables of shape %s; [m, H + 2, H + 2]' % (t.shape,))
    if symmetric:
        t = t + t.transpose(0, 2, 1)
    return np.log1p(np.maximum(t, 0.0)).reshape(len(t), t.shape[1] * t.shape[2])


def link_sketch_features(sketches_by_graph, names, symmetric=True):
    """float32 [len(names), (H + 2)^2]: NodeSketches.pair_features of the pairs named 'g_i_j' from sketches_by_graph[g] (a dict or a sequence of NodeSketches
    with one `hops`), one call per graph, rows in the order of `names` -- the one-call twin of sketch_profile_features(link_sketch_profiles(...), symmetric),
    formed on the device (gm_sketch_pair_features) and equal to it to float32 rounding.  A pair is passed in its name's order: symmetric=False orients the
    table by the name."""
    trip = np.asarray([_pair(nm) for nm in names], np.int64).reshape(-1, 3)
    graphs = np.unique(trip[:, 0]).tolist()
    hops = {int(sketches_by_graph[g].hops) for g in graphs}
    if len(hops) > 1:
        raise ValueError('link_sketch_features: sketches of different hops %s' % sorted(hops))
    out = np.zeros((len(trip), ((hops.pop() if hops else 0) + 2) ** 2), np.float32)
    for g in graphs:
        at = np.nonzero(trip[:, 0] == g)[0]
        out[at] = sketches_by_graph[g].pair_features(trip[at, 1:], symmetric=symmetric)
    return out


def link_propagated_features(props_by_graph, names, op='hadamard'):
    """float32 [len(names), hops + 1, F]: PropagatedFeatures.pair_features of the pairs named 'g_i_j' from props_by_graph[g] (a dict or a sequence of
    PropagatedFeatures with one `hops` and one `feat_dim`), one call per graph, rows in the order of `names` -- the twin of link_sketch_profiles: the two together
    are the precomputed inputs of a BUDDY predictor.  Both operations ('hadamard', 'abs_diff') are symmetric in the pair: the orientation of a name drops out."""
    from .propagate import check_op
    check_op(op, 'link_propagated_features')
    trip = np.asarray([_pair(nm) for nm in names], np.int64).reshape(-1, 3)
    graphs = np.unique(trip[:, 0]).tolist()
    hops = {int(props_by_graph[g].hops) for g in graphs}
    if len(hops) > 1:
        raise ValueError('link_propagated_features: propagated features of different hops %s' % sorted(hops))
    width = {int(props_by_graph[g].feat_dim) for g in graphs}
    if len(width) > 1:
        raise ValueError('link_propagated_features: propagated features of different feat_dim %s' % sorted(width))
    out = np.zeros((len(trip), (hops.pop() if hops else 0) + 1, width.pop() if width else 0), np.float32)
    for g in graphs:
        at = np.nonzero(trip[:, 0] == g)[0]
        out[at] = props_by_graph[g].pair_features(trip[at, 1:], op)
    return out


def candidate_names(g, nodes, partners):
    """The partners GraphStore.link_candidates (or pagerank_candidates) found for the `nodes` of graph `g`, as pair names: one list of 'g_a_w' per node, in ranking order, the -1
    padding skipped -- the shape Subgraphs.query_batch takes (one set per source), whose batch Adapted.predict scores."""
    a = np.asarray(nodes, np.int64).reshape(-1)
    p = np.asarray(partners, np.int64)
    if p.ndim != 2 or len(p) != len(a):
        raise ValueError('candidate_names: %d nodes, partners of shape %s' % (len(a), p.shape))
    return [['%d_%d_%d' % (int(g), x, w) for w in row.tolist() if w >= 0] for x, row in zip(a.tolist(), p)]
