"""Neighbourhood heuristics as a link-prediction baseline: the scores of GraphStore.pair_scores (gm_store_pair_scores; the definition is in
include/gmeta_hip.h) turned into the ROC AUC a learned link predictor is held against.  The scores come from the device; the AUC is host work over
one number per pair.  The path scores one step further -- the local path index and the truncated Katz index -- are formed here, in float64, from the exact walk
counts of GraphStore.pair_walks (gm_store_pair_walks).  The one global score, rooted PageRank, is the float64 sum of the two columns of
GraphStore.pair_pagerank (gm_store_pair_pagerank).  Graph distance is the negated byte of GraphStore.pair_distance (gm_store_pair_distance).
The joint hop-distance tables of GraphStore.pair_distance_profile (gm_store_pair_distance_profile) are no score: link_distance_profiles orients them by the
pair's name and distance_profile_features turns them into input features."""
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


def candidate_names(g, nodes, partners):
    """The partners GraphStore.link_candidates (or pagerank_candidates) found for the `nodes` of graph `g`, as pair names: one list of 'g_a_w' per node, in ranking order, the -1
    padding skipped -- the shape Subgraphs.query_batch takes (one set per source), whose batch Adapted.predict scores."""
    a = np.asarray(nodes, np.int64).reshape(-1)
    p = np.asarray(partners, np.int64)
    if p.ndim != 2 or len(p) != len(a):
        raise ValueError('candidate_names: %d nodes, partners of shape %s' % (len(a), p.shape))
    return [['%d_%d_%d' % (int(g), x, w) for w in row.tolist() if w >= 0] for x, row in zip(a.tolist(), p)]
