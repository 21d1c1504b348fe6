"""ELPH / BUDDY neighbourhood sketches of every node of a parent graph (gm_store_sketch_build, gm_sketch_*; the definition is in include/gmeta_hip.h,
tests/sketch_ref.py restates it): per node and level d = 0 .. hops a HyperLogLog record of 2^p byte registers and a MinHash record of k words of its d-hop
ball, built once on the device; afterwards the integers behind the joint hop-distance table of ANY pair come from 2 (hops + 1) small records, with no search.
The estimators over those integers exist twice: in float64 on the host (gmeta_amd.hll_cardinality, sketch_intersections, sketch_distance_profile), and on the
device in NodeSketches.pair_features (gm_sketch_pair_features), which hands a predictor its structure columns without a read-back.

There is no mask_target: the sketches describe the whole graph and a pair's own edge cannot be taken out of them (ELPH has the same limit).  The exact,
masked table of a shortlist is GraphStore.pair_distance_profile(mask_target=True)."""
import ctypes as C

import numpy as np

from . import _lib


def check_params(hops, p, k, what):
    """(hops, p, k) as ints after the range checks of gm_store_sketch_build; ValueError names the value."""
    hops, p, k = int(hops), int(p), int(k)
    if not 1 <= hops <= 4:
        raise ValueError('%s: hops = %d; 1 .. 4' % (what, hops))
    if not 4 <= p <= 10:
        raise ValueError('%s: p = %d; 4 .. 10' % (what, p))
    if not (32 <= k <= 512 and k % 32 == 0):
        raise ValueError('%s: k = %d; a multiple of 32 in 32 .. 512' % (what, k))
    return hops, p, k


class NodeSketches:
    """The sketches of graph `g` of `store` (GraphStore.sketches builds one).  Attributes n_nodes, hops, p, k, seed, nbytes (the device memory it owns:
    n_nodes (hops + 1) (2^p + 4 k)).  It does not reference the store afterwards.  A context manager; .close() frees the device memory."""

    def __init__(self, store, g, hops=2, p=8, k=128, seed=222):
        hops, p, k = check_params(hops, p, k, 'sketches')
        g = int(g)
        if not 0 <= g < store.n_graphs:
            raise ValueError('sketches: graph %d of a store with %d graph(s)' % (g, store.n_graphs))
        self.handle = None
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        h = C.c_void_p()
        _lib.check(_lib.lib().gm_store_sketch_build(store.handle, g, hops, p, k, self.seed, _lib.stream_ptr(), C.byref(h)), 'gm_store_sketch_build')
        self.handle = h
        n, hh, pp, kk, nb = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().gm_sketch_dims(h, C.byref(n), C.byref(hh), C.byref(pp), C.byref(kk), C.byref(nb)), 'gm_sketch_dims')
        self.n_nodes, self.hops, self.p, self.k, self.nbytes = n.value, hh.value, pp.value, kk.value, nb.value

    def _ids(self, ids, what, shape):
        if not self.handle:
            raise ValueError('%s: the sketches are closed' % what)
        a = np.asarray(ids, np.int64).reshape(shape)
        if len(a) and (a.min() < 0 or a.max() >= self.n_nodes):
            raise ValueError('%s: node id outside the graph (%d nodes)' % (what, self.n_nodes))
        return a

    def pair_counts(self, pairs):
        """(counts int64 [m, hops + 1, hops + 1, 3], balls int64 [m, 2, hops + 1, 2]) of the [m, 2] node `pairs`, canonicalised to (u, v) = (min, max):
        counts[., a, b] = (MinHash matches, zero registers, sum of 2^(32 - register)) of the level-a record of u against the level-b record of v, balls
        the last two of u's and then v's own records (gm_sketch_pair_counts).  Exact integers, the same for both orientations of a pair."""
        import torch
        p = self._ids(pairs, 'pair_counts', (-1, 2))
        L = self.hops + 1
        out = torch.empty((len(p), L, L, 3), dtype=torch.int64, device='cuda')
        balls = torch.empty((len(p), 2, L, 2), dtype=torch.int64, device='cuda')
        if len(p):
            d_p = torch.from_numpy(np.ascontiguousarray(p, np.int32)).cuda()
            _lib.check(_lib.lib().gm_sketch_pair_counts(self.handle, _lib.ptr(d_p), len(p), _lib.ptr(out), _lib.ptr(balls), _lib.stream_ptr()), 'gm_sketch_pair_counts')
        return out.cpu().numpy(), balls.cpu().numpy()

    @property
    def n_columns(self):
        """(hops + 2)^2: the structure columns pair_features gives per pair"""
        return (self.hops + 2) ** 2

    def pair_features(self, pairs, symmetric=True, as_torch=False, out=None):
        """float32 [m, (hops + 2)^2]: the structure columns of a BUDDY predictor for the [m, 2] node `pairs`, formed on the device from the integers of
        pair_counts (gm_sketch_pair_features): log1p(max(T, 0)) row-major of the estimated joint hop-distance table, T = P + P^T when symmetric (default; both
        orientations of a pair give the same bits), else P in the orientation the pair is passed in -- to float32 rounding what
        sketch_profile_features(sketch_distance_profile(*pair_counts(pairs), ...), symmetric) gives on the host.  numpy, or with as_torch=True a CUDA tensor
        that never left the device.  `out`: a CUDA float32 tensor [m, W >= (hops + 2)^2] with contiguous rows; its first (hops + 2)^2 columns are filled in
        place, the others are not touched, and it is what is returned (as_torch) or copied back."""
        import torch
        p = self._ids(pairs, 'pair_features', (-1, 2))
        S = self.n_columns
        if out is None:
            out = torch.empty((len(p), S), dtype=torch.float32, device='cuda')
        else:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_cuda:
                raise ValueError('pair_features: out must be a CUDA float32 tensor')
            if out.dim() != 2 or out.shape[0] != len(p) or out.shape[1] < S:
                raise ValueError('pair_features: out of shape %s; [%d, at least %d]' % (tuple(out.shape), len(p), S))
            if out.shape[1] and out.stride(1) != 1 or len(p) > 1 and out.stride(0) != out.shape[1]:
                raise ValueError('pair_features: out of strides %s; contiguous rows' % (tuple(out.stride()),))
        if len(p):
            self._features_into(torch.from_numpy(np.ascontiguousarray(p, np.int32)).cuda(), len(p), symmetric, out)
        return out if as_torch else out[:, :S].cpu().numpy()

    def _features_into(self, d_pairs, m, symmetric, out):
        """gm_sketch_pair_features of the device int32 [m, 2] `d_pairs` (ids already checked) into the first n_columns columns of the CUDA float32 [m, W]
        `out`, ld = W"""
        if not self.handle:
            raise ValueError('pair_features: the sketches are closed')
        _lib.check(_lib.lib().gm_sketch_pair_features(self.handle, _lib.ptr(d_pairs), m, 1 if symmetric else 0, _lib.ptr(out), out.shape[1], _lib.stream_ptr()),
                   'gm_sketch_pair_features')

    def registers(self, nodes, level):
        """(uint8 [m, 2^p], uint32 [m, k]): the HyperLogLog registers and the MinHash words of the `nodes` at `level` (0 .. hops), as stored
        (gm_sketch_registers)."""
        import torch
        level = int(level)
        if not 0 <= level <= self.hops:
            raise ValueError('registers: level = %d; 0 .. %d' % (level, self.hops))
        a = self._ids(nodes, 'registers', (-1,))
        hll = torch.empty((len(a), 1 << self.p), dtype=torch.uint8, device='cuda')
        mh = torch.empty((len(a), self.k), dtype=torch.int32, device='cuda')
        if len(a):
            d_a = torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
            _lib.check(_lib.lib().gm_sketch_registers(self.handle, level, _lib.ptr(d_a), len(a), _lib.ptr(hll), _lib.ptr(mh), _lib.stream_ptr()), 'gm_sketch_registers')
        return hll.cpu().numpy(), mh.cpu().numpy().view(np.uint32)

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().gm_sketch_destroy(self.handle)
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
