"""ctypes binding of libgmeta_hip.so (include/gmeta_hip.h).  Fails loudly if the library is absent."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GMETA_HIP_LIB') or os.path.join(HERE, 'libgmeta_hip.so')      # override: kernel experiments with variant builds

GM_MAX_GCN = 4
(F_SUB_OFF, F_SET_SUB_OFF, F_PARENT, F_GRAPH, F_INDPTR, F_INDICES, F_INDPTR_T, F_INDICES_T, F_CENTRE, F_NORM,
 F_FEAT_ROW, F_NORM_SRC, F_NORM_CENTRE, F_EDGE_W, F_EDGE_W_T, F_HOP, F_NORM_E1, F_EDGE_CENTRE_T, F_OBS_CENTRE, F_OBS_E1) = range(20)
LINK_SYMMETRIC = 2      # GM_LINK_SYMMETRIC: the link_pred mode of gm_extract / gm_extract_pair with h hops around both endpoints
LINK_MASK_TARGET = 4    # GM_LINK_MASK_TARGET: flag OR-ed onto a pair mode -- the subgraph of (i, j) is built without the i-j edges themselves
NEG_MODES = {'uniform': 0, 'two_hop': 1}      # GM_NEG_UNIFORM / GM_NEG_TWO_HOP (gm_store_negative_pairs)
PAIR_MASK_TARGET = 1    # GM_PAIR_MASK_TARGET: flag of gm_store_pair_scores / gm_store_pair_walks / gm_store_pair_pagerank / gm_store_pair_distance / gm_store_pair_distance_profile -- the pair is scored as if no edge joined its two nodes
PROP_SELF_LOOPS = 1     # GM_PROP_SELF_LOOPS: flag of gm_store_propagate_build -- one extra entry (v, 1.0) in front of every row: the A + I of GCN / SIGN / BUDDY
PROP_OPS = {'hadamard': 0, 'abs_diff': 1}      # GM_PROP_HADAMARD / GM_PROP_ABS_DIFF: how gm_prop_pair_features combines the two nodes' rows of a level
DIST_UNREACHED = 255    # GM_DIST_UNREACHED: the byte of gm_store_node_distances / gm_store_pair_distance for a node no path of at most max_dist edges reaches


class Seed(C.Structure):
    _fields_ = [('graph', C.c_int32), ('i', C.c_int32), ('j', C.c_int32)]


class Model(C.Structure):
    _fields_ = [('n_gcn', C.c_int32), ('dims', C.c_int32 * (GM_MAX_GCN + 1)), ('n_out', C.c_int32), ('link_pred', C.c_int32)]


class HParams(C.Structure):
    _fields_ = [('update_lr', C.c_float), ('update_step', C.c_int32), ('k_spt', C.c_int32), ('need_meta_grad', C.c_int32),
                ('hoist_z1', C.c_int32), ('serialize', C.c_int32), ('sparse_bwd', C.c_int32), ('cone', C.c_int32)]


RANK_MAX_K = 8          # GM_RANK_MAX_K: the K values one gm_rank_summary call takes


class RankSummary(C.Structure):
    _fields_ = [('n_pos', C.c_int64), ('n_pairs', C.c_int64), ('auc2', C.c_int64), ('rr_sum', C.c_double), ('hits', C.c_int64 * RANK_MAX_K)]


vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
PROTOTYPES = {
    'gm_last_error': (C.c_char_p, []),
    'gm_version': (C.c_int, []),
    'gm_store_create': (C.c_int, [i32, vp, vp, vp, vp, i32, vp]),
    'gm_store_create_weighted': (C.c_int, [i32, vp, vp, vp, vp, vp, i32, vp]),
    'gm_store_weighted': (i32, [vp]),
    'gm_batch_weighted': (i32, [vp]),
    'gm_store_destroy': (None, [vp]),
    'gm_store_negative_pairs': (i32, [vp, i32, i64, u64, i32, vp, i64, vp, vp, vp]),
    'gm_store_has_edges': (i32, [vp, i32, vp, i64, vp, vp]),
    'gm_store_without_edges': (i32, [vp, vp, vp, vp, vp]),
    'gm_store_split_edges': (i32, [vp, i32, u64, u64, u64, vp, vp, i64, vp, vp]),
    'gm_store_dims': (i32, [vp, i32, vp, vp, vp]),
    'gm_store_read_csr': (i32, [vp, i32, i32, vp, vp, vp]),
    'gm_store_pair_scores': (i32, [vp, i32, vp, i64, i32, vp, vp]),
    'gm_store_pair_walks': (i32, [vp, i32, vp, i64, i32, vp, vp]),
    'gm_store_rooted_pagerank': (i32, [vp, i32, vp, i64, C.c_float, i32, vp, vp]),
    'gm_store_pair_pagerank': (i32, [vp, i32, vp, i64, i32, C.c_float, i32, vp, vp]),
    'gm_store_pagerank_candidates': (i32, [vp, i32, vp, i64, i32, C.c_float, i32, vp, vp, vp, vp]),
    'gm_store_node_distances': (i32, [vp, i32, vp, i64, i32, vp, vp]),
    'gm_store_pair_distance': (i32, [vp, i32, vp, i64, i32, i32, vp, vp]),
    'gm_store_pair_distance_profile': (i32, [vp, i32, vp, i64, i32, i32, vp, vp]),
    'gm_store_sketch_build': (i32, [vp, i32, i32, i32, i32, u64, vp, vp]),
    'gm_sketch_dims': (i32, [vp, vp, vp, vp, vp, vp]),
    'gm_sketch_registers': (i32, [vp, i32, vp, i64, vp, vp, vp]),
    'gm_sketch_pair_counts': (i32, [vp, vp, i64, vp, vp, vp]),
    'gm_sketch_pair_features': (i32, [vp, vp, i64, i32, vp, i64, vp]),
    'gm_sketch_destroy': (None, [vp]),
    'gm_store_propagate_build': (i32, [vp, i32, i32, i32, vp, vp]),
    'gm_prop_dims': (i32, [vp, vp, vp, vp, vp, vp]),
    'gm_prop_rows': (i32, [vp, i32, vp, i64, vp, vp]),
    'gm_prop_pair_features': (i32, [vp, vp, i64, i32, vp, vp]),
    'gm_prop_destroy': (None, [vp]),
    'gm_prop_pair_mlp_dims': (i32, [vp, i32, i32, vp, vp]),
    'gm_prop_pair_mlp_tile': (i32, []),
    'gm_prop_pair_mlp_forward': (i32, [vp, vp, i64, i32, vp, i32, vp, i32, vp, vp]),
    'gm_prop_pair_mlp_step': (i32, [vp, vp, i64, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp]),
    'gm_rank_counts': (i32, [vp, i64, vp, i64, vp, vp, vp]),
    'gm_rank_summary': (i32, [vp, i64, vp, i64, vp, vp, i32, vp, vp, vp]),
    'gm_store_neighbour_degrees': (i32, [vp, i32, vp, vp]),
    'gm_store_pair_candidates': (i32, [vp, i32, vp, i64, i32, i32, vp, vp, vp, vp]),
    'gm_extract': (C.c_int, [vp, vp, i32, vp, i32, i32, i32, u64, i32, vp, vp]),
    'gm_extract_pair': (C.c_int, [vp, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, u64, i32, vp, vp, vp]),
    'gm_batch_from_nodes': (C.c_int, [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp]),
    'gm_set_hop_labels': (None, [i32]),
    'gm_get_hop_labels': (i32, []),
    'gm_batch_hop_labels': (i32, [vp]),
    'gm_batch_mask_target': (i32, [vp]),
    'gm_batch_concat': (C.c_int, [vp, i32, vp, vp]),
    'gm_batch_destroy': (None, [vp]),
    'gm_batch_prepare_cone': (C.c_int, [vp, i32, vp]),
    'gm_batch_prepare_cone_pair': (C.c_int, [vp, vp, i32, vp]),
    'gm_batch_cone_dims': (C.c_int, [vp, i32, vp, vp, vp]),
    'gm_batch_cone_read': (C.c_int, [vp, i32, i32, i32, vp, i64]),
    'gm_batch_dims': (C.c_int, [vp, vp, vp, vp, vp, vp]),
    'gm_batch_read': (C.c_int, [vp, i32, vp, i64]),
    'gm_batch_device_ptr': (C.c_int, [vp, i32, vp]),
    'gm_batch_source_rows': (C.c_int, [vp, vp]),
    'gm_batch_e1_source_rows': (C.c_int, [vp, vp]),
    'gm_gather_features': (C.c_int, [vp, vp, vp]),
    'gm_aggregate': (C.c_int, [vp, i32, i32, vp, i32, vp, vp, vp, vp]),
    'gm_aggregate_bytes': (i64, [vp, i32]),
    'gm_model_param_count': (i64, [vp]),
    'gm_gcn_ws_bytes': (i64, [vp, vp]),
    'gm_gcn_forward': (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]),
    'gm_gcn_backward': (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, i64, vp]),
    'gm_dense_update': (C.c_int, [vp, vp, i32, vp, i64, i32, vp, i32, vp]),
    'gm_dense_gemm': (C.c_int, [vp, vp, i64, i32, vp, i64, i32, i32, vp, i64, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, i32, vp, vp]),
    'gm_dense_fused_gemm': (C.c_int, [vp, i32, vp, i64, i32, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, vp, vp, i64, i32, vp, vp, vp, i32, vp, vp]),
    'gm_dense_fused_gemm_rows': (C.c_int, [vp, i32, i32, i32, i32, i32, vp, i64, i32, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, vp, vp, vp, i32, vp, vp]),
    'gm_dense_fused_gemm_packed': (C.c_int, [vp, i32, i32, i32, vp, i64, i32, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, vp, vp]),
    'gm_dense_wgrad_fused': (C.c_int, [vp, i32, vp, i64, i32, vp, i64, vp, i64, i32, vp, vp, vp, i64, vp, i64, i32, vp]),
    'gm_dense_aggregate': (C.c_int, [vp, i32, i32, vp, i64, i32, i32, vp, vp, i32, vp, i64, i32, vp, vp, vp, i32, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp]),
    'gm_dense_agg_info': (C.c_int, [vp, i32, vp]),
    'gm_dense_obs_lists': (C.c_int, [vp, vp, vp]),
    'gm_dense_fuse_counts': (C.c_int, [vp, vp]),
    'gm_dense_agg_table': (C.c_int, [vp, i32, i32, vp, i64, vp]),
    'gm_dense_dz_centre': (C.c_int, [vp, vp, i32, vp, i64, i32, vp, vp]),
    'gm_dense_dz_centre_rows': (C.c_int, [vp, vp, i32, vp, i64, i32, vp, i32, i32, vp]),
    'gm_dense_wgrad_centre': (C.c_int, [vp, vp, i32, vp, i32, vp, i64, vp, i64, vp]),
    'gm_dense_agg_centre_t': (C.c_int, [vp, vp, i32, vp, vp, i32, vp]),
    'gm_dense_wgrad_e1': (C.c_int, [vp, vp, i32, vp, i32, vp, i64, vp, i64, vp]),
    'gm_dense_wgrad': (C.c_int, [vp, vp, i64, i32, vp, i64, i32, vp, vp, i64, vp, i64, vp, i64, i32, vp, vp, i64, C.c_float, vp, vp, vp, vp]),
    'gm_proto_loss_spt': (C.c_int, [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
    'gm_proto_loss_qry': (C.c_int, [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    'gm_dense_head_loss': (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i64, i64, i64, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp, vp,
                                     vp, vp, i64, C.c_float, vp, i32, vp, vp]),
    'gm_set_ragged_classes': (None, [i32]),
    'gm_get_ragged_classes': (i32, []),
    'gm_set_readout': (None, [i32]),
    'gm_get_readout': (i32, []),
    'gm_meta_ws_bytes': (i64, [vp, vp, vp, vp]),
    'gm_meta_out_floats': (i64, [vp, vp, vp]),
    'gm_meta_step': (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp]),
    'gm_adapt_ws_bytes': (i64, [vp, vp, vp]),
    'gm_meta_adapt': (C.c_int, [vp, vp, vp, vp, vp, vp, i64, vp, i32, vp, i64, vp]),
    'gm_predict_ws_bytes': (i64, [vp, vp, vp]),
    'gm_proto_predict': (C.c_int, [vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp, vp, i64, vp]),
    'gm_meta_finish': (C.c_int, [vp, i64, i32, vp, vp, vp]),
    'gm_meta_finish_adam': (C.c_int, [vp, i64, i32, vp, vp, vp, vp, vp, i32, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, vp]),
    'gm_set_gemm_mode': (None, [i32]),
    'gm_get_gemm_mode': (i32, []),
    'gm_get_split_pieces': (i32, []),
    'gm_set_split_pieces': (None, [i32]),
    'gm_set_tuning': (C.c_int, [C.c_char_p, i32]),
    'gm_get_tuning': (i32, [C.c_char_p]),
    'gm_tuning_epoch': (i32, []),
    'gm_set_fuse_agg': (None, [i32]),
    'gm_get_fuse_agg': (i32, []),
    'gm_profile_enable': (None, [i32]),
    'gm_profile_aggregate': (C.c_int, [vp, vp, vp]),
    'gm_profile_read': (C.c_int, [i32, vp, vp, vp]),
    'gm_profile_read_launches': (C.c_int, [i32, vp, vp, i32]),
}
# include/gmeta_hip_probes.h: exported only by the probe build (build.py --probes -> libgmeta_hip_probes.so, loaded through GMETA_HIP_LIB by tools/)
PROBE_PROTOTYPES = {
    'gm_debug_stamp': (C.c_int, [vp, vp]),
    'gm_stream_debug': (C.c_int, [i32, vp, i32]),
    'gm_head_loss_debug': (C.c_int, [i32, vp]),
}

# test-only exports of PROTOTYPES younger than the rest: a library given through GMETA_HIP_LIB may be an older build without them (the A/B measurements run
# the parent commit's library in this checkout) and still loads; the package's own library must export every one (tests/test_cabi_and_host.py)
LATER_EXPORTS = {'gm_dense_obs_lists', 'gm_dense_fused_gemm_rows', 'gm_dense_fused_gemm_packed', 'gm_dense_dz_centre_rows'}

_lib = None


def lib():
    """The loaded library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('gmeta_amd: %s is missing -- run `python -c "import __graft_entry__ as g; g.build()"` '
                               '(hipcc --offload-arch=gfx950).  There is no CPU fallback.' % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            if name in LATER_EXPORTS and os.environ.get('GMETA_HIP_LIB') and not hasattr(l, name):
                continue
            fn = getattr(l, name)           # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        for name, (res, args) in PROBE_PROTOTYPES.items():
            if hasattr(l, name):            # the probe build only
                fn = getattr(l, name)
                fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().gm_last_error().decode('utf-8', 'replace')
        exc = ValueError if rc == -1 else RuntimeError
        raise exc('%s failed (code %d): %s' % (what or 'libgmeta_hip', rc, msg))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('gmeta_amd needs an AMD GPU (gfx950); torch.cuda.is_available() is False and there is no CPU fallback')


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device/host address of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    if hasattr(t, 'data_ptr'):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


READOUT_CENTRE, READOUT_MEAN = 0, 1      # GM_READOUT_*
READOUTS = {'centre': READOUT_CENTRE, 'mean': READOUT_MEAN}


def config_readout(config):
    """The readout a config asks for: 'centre' (no entry, or ('Readout', ['centre'])) or 'mean' (('Readout', ['mean'])).  At most one entry, after the
    Linear entry's GraphConv stack or anywhere else -- but before a trailing ('LinkPred', [True]), which learner.py:78-79 looks for at config[-1]."""
    ent = [(k, p) for k, (n, p) in enumerate(config) if n == 'Readout']
    if not ent:
        return 'centre'
    if len(ent) > 1:
        raise ValueError("config holds %d 'Readout' entries; at most one" % len(ent))
    k, p = ent[0]
    if not isinstance(p, (list, tuple)) or len(p) != 1 or p[0] not in READOUTS:
        raise ValueError("config entry ('Readout', %r): expected ['centre'] or ['mean']" % (p,))
    if any(n == 'LinkPred' for n, _ in config) and config[-1][0] != 'LinkPred':
        raise ValueError("the ('Readout', ...) entry must come before the trailing ('LinkPred', [True]) entry")
    return p[0]


class readout_switch:
    """The calling thread's readout (gm_set_readout) set for the length of the block; the block restores what it found, after an exception too."""

    def __init__(self, readout):
        self.mode = READOUTS[readout] if isinstance(readout, str) else int(readout)

    def __enter__(self):
        l = lib()
        self.was = int(l.gm_get_readout())
        if self.was != self.mode:
            l.gm_set_readout(self.mode)
        return self

    def __exit__(self, *exc):
        if self.was != self.mode:
            lib().gm_set_readout(self.was)
        return False


def make_model(config):
    """train.py:67-75 config list -> gm_model_t.  Mirrors learner.py:78-97 parsing.  The readout is not part of gm_model_t (a switch of the calling
    thread, gm_set_readout): config_readout(config) names it."""
    unknown = sorted({str(n) for n, _ in config if n not in ('GraphConv', 'Linear', 'LinkPred', 'Readout', 'Attention')})
    if unknown:
        raise ValueError('unknown config entries: %s' % ', '.join(unknown))
    config_readout(config)
    gcn = [p for n, p in config if n == 'GraphConv']
    lin = [p for n, p in config if n == 'Linear']
    if any(n == 'Attention' for n, _ in config):
        raise NotImplementedError("the 'Attention' branch of learner.py:98-131 is dead code in the reference (uses an undefined name)")
    if not gcn or len(lin) != 1 or len(gcn) > GM_MAX_GCN:
        raise ValueError('config must hold 1..%d GraphConv entries and one Linear entry' % GM_MAX_GCN)
    m = Model()
    m.n_gcn = len(gcn)
    for l, (fi, fo) in enumerate(gcn):
        if l and m.dims[l] != fi:
            raise ValueError('GraphConv dims do not chain')
        m.dims[l], m.dims[l + 1] = fi, fo
    if lin[0][0] != m.dims[m.n_gcn]:
        raise ValueError('Linear input dim must equal the last GraphConv output dim')
    m.n_out = lin[0][1]
    m.link_pred = 1 if config[-1][0] == 'LinkPred' else 0
    return m
