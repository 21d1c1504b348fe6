"""gmeta_amd -- MI355X-native (gfx950) implementation of G-Meta's inner-loop hot path.

Host mirror of the reference's Python surface (same names, argument meaning and error behaviour)
over the C-ABI library libgmeta_hip.so (include/gmeta_hip.h):

    reference (G-Meta/)                          here
    subgraph_data_processing.Subgraphs/collate   gmeta_amd.subgraphs.Subgraphs / collate
    learner.Classifier                           gmeta_amd.learner.Classifier
    meta.Meta (.forward / .finetunning)          gmeta_amd.meta.Meta

There is no CPU fallback: every compute entry point raises if the HIP library or a GPU is missing.
"""
from . import _lib  # noqa: F401
from .graphstore import GraphStore  # noqa: F401
from .subgraphs import Subgraphs, SubgraphBatch, collate, hop_label_width, hop_labels_switch  # noqa: F401
from .learner import Classifier  # noqa: F401
from .meta import Meta  # noqa: F401
from .negatives import link_holdout, link_tables_with_negatives  # noqa: F401
from .heuristics import (DISTANCE_SCORES, DIST_UNREACHED, PAGERANK_SCORES, PAIR_SCORES, PATH_SCORES, candidate_names, distance_profile_features,  # noqa: F401
                         graph_distance_index, hll_cardinality, katz_index, link_distance_profiles, link_sketch_features, link_sketch_profiles,
                         link_auc, link_distance_auc, link_distance_scores, link_heuristic_auc, link_pagerank_auc, link_pagerank_scores, link_path_auc,
                         link_path_scores, link_propagated_features, local_path_index, rooted_pagerank_index, sketch_distance_profile, sketch_intersections, sketch_profile_features)
from .sketches import NodeSketches  # noqa: F401
from .propagate import PropagatedFeatures  # noqa: F401
from .predictor import PairPredictor  # noqa: F401
from .ranking import link_ranking, rank_counts, rank_metrics  # noqa: F401

__all__ = ['GraphStore', 'Subgraphs', 'SubgraphBatch', 'collate', 'Classifier', 'Meta', 'hop_label_width', 'hop_labels_switch', 'link_tables_with_negatives', 'link_holdout',
           'PAIR_SCORES', 'link_auc', 'link_heuristic_auc', 'candidate_names', 'PATH_SCORES', 'local_path_index', 'katz_index', 'link_path_scores',
           'link_path_auc', 'PAGERANK_SCORES', 'rooted_pagerank_index', 'link_pagerank_scores', 'link_pagerank_auc',
           'DISTANCE_SCORES', 'DIST_UNREACHED', 'graph_distance_index', 'link_distance_scores', 'link_distance_auc',
           'link_distance_profiles', 'distance_profile_features',
           'NodeSketches', 'hll_cardinality', 'sketch_intersections', 'sketch_distance_profile', 'link_sketch_profiles', 'sketch_profile_features', 'link_sketch_features',
           'PropagatedFeatures', 'link_propagated_features', 'PairPredictor', 'rank_counts', 'rank_metrics', 'link_ranking']
