"""BUDDY / SIGN hop-propagated node features of a whole parent graph (gm_store_propagate_build, gm_prop_*; the definition is in include/gmeta_hip.h,
tests/hop_feature_ref.py restates it): the levels x_0 = X, x_{t+1} = A^ x_t for t < hops, with the project's GraphConv normalisation over the store's in-edge CSR
(parallel edges, self loops, directions and weights kept) and, by default, one self loop in front of every row -- the A^ = D~^-1/2 (A + I) D~^-1/2 of GCN / SIGN /
BUDDY.  Built once on the device; afterwards the per-pair inputs x_t[u] * x_t[v] of a BUDDY predictor are one gather.  Together with the structural counts of
GraphStore.sketches they are the two precomputed inputs of that predictor.

There is no mask_target: the levels describe the whole graph, as the sketches do, and a pair's own edge cannot be taken out of them."""
import ctypes as C

import numpy as np

from . import _lib

MAX_HOPS = 8


def check_hops(hops, what):
    """`hops` as an int after the range check of gm_store_propagate_build; ValueError names the value."""
    hops = int(hops)
    if not 1 <= hops <= MAX_HOPS:
        raise ValueError('%s: hops = %d; 1 .. %d' % (what, hops, MAX_HOPS))
    return hops


def check_op(op, what):
    """The GM_PROP_* code of the pair operation named `op` ('hadamard' / 'abs_diff'); ValueError names the value."""
    if op not in _lib.PROP_OPS:
        raise ValueError('%s: op = %r; one of %s' % (what, op, sorted(_lib.PROP_OPS)))
    return _lib.PROP_OPS[op]


class PropagatedFeatures:
    """The propagated features of graph `g` of `store` (GraphStore.propagated_features builds one).  Attributes n_nodes, hops, feat_dim, self_loops, nbytes (the
    device memory it owns: (hops + 1) n_nodes ld 4, ld the store's padded feature width).  Level 0 is a copy of the store's features: the object does not
    reference the store afterwards.  A context manager; .close() frees the device memory.  No mask_target: the levels describe the whole graph."""

    def __init__(self, store, g, hops=2, self_loops=True):
        hops = check_hops(hops, 'propagated_features')
        g = int(g)
        if not 0 <= g < store.n_graphs:
            raise ValueError('propagated_features: graph %d of a store with %d graph(s)' % (g, store.n_graphs))
        self.handle = None
        h = C.c_void_p()
        _lib.check(_lib.lib().gm_store_propagate_build(store.handle, g, hops, _lib.PROP_SELF_LOOPS if self_loops else 0, _lib.stream_ptr(), C.byref(h)),
                   'gm_store_propagate_build')
        self.handle = h
        n, hh, f, fl, nb = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().gm_prop_dims(h, C.byref(n), C.byref(hh), C.byref(f), C.byref(fl), C.byref(nb)), 'gm_prop_dims')
        self.n_nodes, self.hops, self.feat_dim, self.self_loops, self.nbytes = n.value, hh.value, f.value, bool(fl.value & _lib.PROP_SELF_LOOPS), nb.value

    def _ids(self, ids, what, shape):
        if not self.handle:
            raise ValueError('%s: the propagated features are closed' % what)
        a = np.asarray(ids, np.int64).reshape(shape)
        if len(a) and (a.min() < 0 or a.max() >= self.n_nodes):
            raise ValueError('%s: node id outside the graph (%d nodes)' % (what, self.n_nodes))
        return a

    def rows(self, nodes, level):
        """float32 [m, feat_dim]: x_level of the `nodes` (level 0 .. hops; 0 is the store's features), as stored (gm_prop_rows).  Duplicates are allowed."""
        import torch
        level = int(level)
        if not 0 <= level <= self.hops:
            raise ValueError('rows: level = %d; 0 .. %d' % (level, self.hops))
        a = self._ids(nodes, 'rows', (-1,))
        out = torch.empty((len(a), self.feat_dim), dtype=torch.float32, device='cuda')
        if len(a):
            d_a = torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
            _lib.check(_lib.lib().gm_prop_rows(self.handle, level, _lib.ptr(d_a), len(a), _lib.ptr(out), _lib.stream_ptr()), 'gm_prop_rows')
        return out.cpu().numpy()

    def pair_features(self, pairs, op='hadamard', as_torch=False):
        """float32 [m, hops + 1, feat_dim] of the [m, 2] node `pairs`: entry [k, t] is x_t[a] * x_t[b] ('hadamard') or |x_t[a] - x_t[b]| ('abs_diff'), one fp32
        operation on the rows .rows returns, the same bits for both orientations of a pair (gm_prop_pair_features).  as_torch=True leaves the result on the
        device as a CUDA tensor: it feeds a predictor."""
        import torch
        code = check_op(op, 'pair_features')
        p = self._ids(pairs, 'pair_features', (-1, 2))
        out = torch.empty((len(p), self.hops + 1, self.feat_dim), dtype=torch.float32, device='cuda')
        if len(p):
            d_p = torch.from_numpy(np.ascontiguousarray(p, np.int32)).cuda()
            _lib.check(_lib.lib().gm_prop_pair_features(self.handle, _lib.ptr(d_p), len(p), code, _lib.ptr(out), _lib.stream_ptr()), 'gm_prop_pair_features')
        return out if as_torch else out.cpu().numpy()

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().gm_prop_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
