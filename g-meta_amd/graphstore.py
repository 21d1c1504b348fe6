"""GraphStore: parent graphs + node features resident in HBM.  Replaces the pickled list of DGLGraph
objects and the `feat` list that train.py:41-44,63-65 load and hand to Subgraphs / Meta."""
import ctypes as C

import numpy as np

from . import _lib


def edges_to_in_csr(n, src, dst, w=None):
    """Directed multigraph edge list (edge k: src[k] -> dst[k]) -> in-edge CSR.  Within a row the
    parent edge-id order is kept (DGL's in_edges order, sdp.py:301).  With edge weights `w` (one per edge) a third
    array comes back: the weights in the CSR's order (the same stable sort carries them)."""
    src = np.asarray(src, np.int64).reshape(-1); dst = np.asarray(dst, np.int64).reshape(-1)
    if src.shape != dst.shape:
        raise ValueError('src and dst must have the same length')
    if w is not None:
        w = np.asarray(w, np.float32).reshape(-1)
        if w.shape != src.shape:
            raise ValueError('need one weight per edge (%d weights, %d edges)' % (len(w), len(src)))
    if len(src) and (src.min() < 0 or src.max() >= n or dst.min() < 0 or dst.max() >= n):
        raise ValueError('edge endpoint out of range')
    order = np.argsort(dst, kind='stable')
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, dst + 1, 1)
    if w is not None:
        return np.cumsum(indptr), np.ascontiguousarray(src[order].astype(np.int32)), np.ascontiguousarray(w[order])
    return np.cumsum(indptr), np.ascontiguousarray(src[order].astype(np.int32))


class GraphStore:
    """`graphs`: list of (n_nodes, src, dst) edge lists or (indptr, indices) in-CSR pairs;
    `feats`: list of float arrays [n_nodes, F0] (one per graph).
    Edge weights (beyond the reference; include/gmeta_hip.h, gm_store_create_weighted): (n_nodes, src, dst, w) 4-tuples, or `edge_weights` =
    one array per graph aligned with the graph's edge list (3-tuples) or with its `indices` (CSR pairs).  Every graph carries weights or none
    does; they must be finite and > 0.  `.weighted` says which kind the store is, `.host_weights` keeps the weights in `host_csr`'s order."""

    def __init__(self, graphs, feats, edge_weights=None):
        _lib.require_gpu()
        if len(graphs) != len(feats) or not graphs:
            raise ValueError('need one feature matrix per graph')
        if edge_weights is not None and len(edge_weights) != len(graphs):
            raise ValueError('edge_weights needs one array per graph')
        ptrs, idxs, ns, wts = [], [], [], []
        for k, g in enumerate(graphs):
            w = None if edge_weights is None else edge_weights[k]
            if len(g) == 4:
                if w is not None:
                    raise ValueError('graph %d has weights in its tuple and in edge_weights' % k)
                g, w = g[:3], g[3]
            if len(g) == 3:
                n, src, dst = g
                if w is None:
                    ip, ix = edges_to_in_csr(int(n), src, dst)
                else:
                    ip, ix, w = edges_to_in_csr(int(n), src, dst, w)
            else:
                ip, ix = np.ascontiguousarray(g[0], np.int64), np.ascontiguousarray(g[1], np.int32)
                n = len(ip) - 1
                if w is not None:
                    w = np.ascontiguousarray(w, np.float32).reshape(-1)
                    if len(w) != len(ix):
                        raise ValueError('graph %d: %d weights for %d edges' % (k, len(w), len(ix)))
            ptrs.append(ip); idxs.append(ix); ns.append(int(n)); wts.append(w)
        if any(w is None for w in wts) and not all(w is None for w in wts):
            raise ValueError('either every graph carries edge weights or none does')
        self.weighted = wts[0] is not None
        F0 = int(np.asarray(feats[0]).shape[1])
        fl = []
        for n, f in zip(ns, feats):
            f = np.ascontiguousarray(f, np.float32)
            if f.shape != (n, F0):
                raise ValueError('feature matrix shape %s does not match (%d, %d)' % (f.shape, n, F0))
            fl.append(f)
        G = len(ns)
        n_arr = (C.c_int64 * G)(*ns)
        p_arr = (C.c_void_p * G)(*[a.ctypes.data for a in ptrs])
        i_arr = (C.c_void_p * G)(*[a.ctypes.data for a in idxs])
        f_arr = (C.c_void_p * G)(*[a.ctypes.data for a in fl])
        h = C.c_void_p()
        if self.weighted:
            w_arr = (C.c_void_p * G)(*[a.ctypes.data for a in wts])
            _lib.check(_lib.lib().gm_store_create_weighted(G, n_arr, p_arr, i_arr, w_arr, f_arr, F0, C.byref(h)), 'gm_store_create_weighted')
        else:
            _lib.check(_lib.lib().gm_store_create(G, n_arr, p_arr, i_arr, f_arr, F0, C.byref(h)), 'gm_store_create')
        self.handle = h
        self.n_graphs, self.n_nodes, self.feat_dim = G, ns, F0
        self.n_edges = [int(p[-1]) for p in ptrs]
        self._host_csr = list(zip(ptrs, idxs))      # host copy of the in-edge CSR (Subgraphs(sample_mode='reference') walks it like sdp.py:301)
        self._host_weights = wts if self.weighted else None      # per graph: the edge weights aligned with host_csr's indices

    @property
    def host_csr(self):
        """Per graph (indptr int64 [N + 1], indices int32 [E]): the host copy of the in-edge CSR.  A derived store (without_edges) reads it back from the
        device at the first access (gm_store_read_csr), not at construction."""
        if self._host_csr is None:
            self._read_back()
        return self._host_csr

    @host_csr.setter
    def host_csr(self, v):
        self._host_csr = v

    @property
    def host_weights(self):
        """Per graph the edge weights aligned with host_csr's indices (None for a store without weights); read back like host_csr on a derived store."""
        if self.weighted and self._host_weights is None:
            self._read_back()
        return self._host_weights

    @host_weights.setter
    def host_weights(self, v):
        self._host_weights = v

    def read_csr(self, g, orientation=0):
        """(indptr int64 [N + 1], indices int32 [E], weights float32 [E] or None) of graph `g` as the device holds it (gm_store_read_csr): orientation 0 = by
        destination (the in-edge CSR, entries = sources), 1 = by source (entries = destinations)."""
        g, _ = self._pairs_of(g, [], 'read_csr')
        ptr = np.empty(self.n_nodes[g] + 1, np.int64)
        idx = np.empty(self.n_edges[g], np.int32)
        w = np.empty(self.n_edges[g], np.float32) if self.weighted else None
        _lib.check(_lib.lib().gm_store_read_csr(self.handle, g, int(orientation), _lib.ptr(ptr), _lib.ptr(idx), _lib.ptr(w)), 'gm_store_read_csr')
        return ptr, idx, w

    def _read_back(self):
        got = [self.read_csr(g) for g in range(self.n_graphs)]
        self._host_csr = [(p, i) for p, i, _ in got]
        self._host_weights = [w for _, _, w in got] if self.weighted else None

    def dims(self, g):
        """(nodes, stored edges, symmetric flag) of graph `g` as the library holds them (gm_store_dims); the flag is the store's, GM_EXTRACT_NO_SYM included."""
        n, e, sym = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _lib.check(_lib.lib().gm_store_dims(self.handle, int(g), C.byref(n), C.byref(e), C.byref(sym)), 'gm_store_dims')
        return n.value, e.value, bool(sym.value)

    def symmetric(self):
        """True when every out-edge list equals the in-edge list element for element (undirected graphs stored in both directions with
        ascending rows): extraction then walks the adjacency lists once for both CSR orientations (csrc/extract.hip).  A weighted store must
        also carry the same weight in both lists slot for slot (w_uv == w_vu): the one walk copies the in-edge's weight to both."""
        for g, (ptr, ix) in enumerate(self.host_csr):
            n = len(ptr) - 1
            dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
            order = np.argsort(ix, kind='stable')                      # out-CSR: by source, destinations in in-CSR (= ascending destination) order
            if not (np.array_equal(np.bincount(ix, minlength=n), np.diff(ptr)) and np.array_equal(dst[order], ix.astype(np.int64))):
                return False
            if self.weighted and not np.array_equal(self.host_weights[g][order], self.host_weights[g]):
                return False
        return True

    def _nodes_of(self, g, nodes, what, shape=(-1,)):
        """(g, the node ids as an int64 array of `shape`) after the graph-range and node-range checks every link-prediction call starts with."""
        g = int(g)
        if not 0 <= g < self.n_graphs:
            raise ValueError('%s: graph %d of a store with %d graph(s)' % (what, g, self.n_graphs))
        a = np.asarray(nodes, np.int64).reshape(shape)
        if len(a) and (a.min() < 0 or a.max() >= self.n_nodes[g]):
            raise ValueError('%s: node id outside graph %d (%d nodes)' % (what, g, self.n_nodes[g]))
        return g, a

    def _pairs_of(self, g, pairs, what):
        return self._nodes_of(g, pairs, what, (-1, 2))

    def _pair_call(self, name, g, p, shape, dtype, *tail):
        """The export `name` over the [m, 2] pairs `p` of graph `g`: the pairs as int32 on the device, the result allocated there as `shape` of `dtype`, the
        call (store, graph, pairs, m, *tail, result, stream; skipped for m == 0), the result brought back as a numpy array."""
        import torch
        out = torch.empty(shape, dtype=dtype, device='cuda')
        if len(p):
            d_p = torch.from_numpy(np.ascontiguousarray(p, np.int32)).cuda()
            _lib.check(getattr(_lib.lib(), name)(self.handle, g, _lib.ptr(d_p), len(p), *tail, _lib.ptr(out), _lib.stream_ptr()), name)
        return out.cpu().numpy()

    def _source_call(self, name, g, a, dtype, *tail):
        """The export `name` over the m sources `a` of graph `g`: the sources as int32 on the device, the [m, N] result of `dtype` allocated there, the call
        (store, graph, sources, m, *tail, result, stream; skipped for m == 0), the result brought back as a numpy array."""
        import torch
        out = torch.empty((len(a), self.n_nodes[g]), dtype=dtype, device='cuda')
        if len(a):
            d_a = torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
            _lib.check(getattr(_lib.lib(), name)(self.handle, g, _lib.ptr(d_a), len(a), *tail, _lib.ptr(out), _lib.stream_ptr()), name)
        return out.cpu().numpy()

    @staticmethod
    def _k_of(k, what):
        k = int(k)
        if not 1 <= k <= 1024:
            raise ValueError('%s: k = %d; 1 .. 1024' % (what, k))
        return k

    def _topk_call(self, name, g, a, k, *tail):
        """The export `name` over the m nodes `a` of graph `g`: the call (store, graph, nodes, m, k, *tail, partners, scores, totals, stream; skipped for
        m == 0) -> (partners int64 [m, k], scores float32 [m, k], totals int64 [m])."""
        import torch
        m = len(a)
        part = torch.empty((m, k), dtype=torch.int32, device='cuda')
        sc = torch.empty((m, k), dtype=torch.float32, device='cuda')
        tot = torch.empty(m, dtype=torch.int32, device='cuda')
        if m:
            d_a = torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
            _lib.check(getattr(_lib.lib(), name)(self.handle, g, _lib.ptr(d_a), m, k, *tail, _lib.ptr(part), _lib.ptr(sc), _lib.ptr(tot), _lib.stream_ptr()), name)
        return part.cpu().numpy().astype(np.int64), sc.cpu().numpy(), tot.cpu().numpy().astype(np.int64)

    def negative_pairs(self, g, n, seed=222, mode='uniform', exclude=None):
        """`n` distinct node pairs (u < v) of graph `g` with no edge between them in either direction, drawn on the device: int64 [n, 2], in the order
        include/gmeta_hip.h defines (gm_store_negative_pairs: a function of the graph, seed, mode, exclusion list and n alone; tests/negative_ref.py
        restates it).  mode: 'uniform' (both endpoints uniform) or 'two_hop' (the second endpoint two out-steps from the first).  `exclude`: [m, 2]
        pairs in any orientation that must not come back (e.g. positives taken out of the graph for validation).  ValueError when the draw budget
        of 64 n + 4096 candidates holds fewer than n such pairs; the message names the count found."""
        import torch
        if mode not in _lib.NEG_MODES:
            raise ValueError("mode must be 'uniform' or 'two_hop', not %r" % (mode,))
        n = int(n)
        g, ex = self._pairs_of(g, [] if exclude is None else exclude, 'negative_pairs(exclude=)')
        keys = self.pair_keys(g, ex)
        d_keys = torch.from_numpy(keys).cuda() if len(keys) else None
        out = torch.empty((max(n, 1), 2), dtype=torch.int32, device='cuda')
        found = C.c_int64(0)
        _lib.check(_lib.lib().gm_store_negative_pairs(self.handle, g, n, int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.NEG_MODES[mode], _lib.ptr(d_keys), len(keys),
                                                      _lib.ptr(out), C.byref(found), _lib.stream_ptr()), 'gm_store_negative_pairs')
        if found.value < n:
            raise ValueError('negative_pairs: graph %d holds only %d distinct non-adjacent %s pair(s) within the draw budget of %d candidates; %d asked for'
                             % (g, found.value, mode, 64 * n + 4096, n))
        return out[:n].cpu().numpy().astype(np.int64)

    def pair_keys(self, g, pairs):
        """int64 [k]: the canonical keys min(a, b) * N + max(a, b) of the [m, 2] node `pairs` of graph `g`, sorted and unique -- the list format of
        negative_pairs' exclusions and of without_edges.  Pairs may come in any orientation and may repeat; a pair (a, a) names the self loops of a."""
        g, p = self._pairs_of(g, pairs, 'pair_keys')
        return np.unique(np.minimum(p[:, 0], p[:, 1]) * self.n_nodes[g] + np.maximum(p[:, 0], p[:, 1]))      # canonical, keyed, sorted, unique

    def without_edges(self, removed):
        """A new GraphStore with the same nodes and features and every edge except those between the node pairs in `removed`, derived on the device
        (gm_store_without_edges; the definition is in include/gmeta_hip.h, tests/holdout_ref.py restates it).  `removed`: {g: pairs [m, 2]} or a list with one entry
        per graph (None: nothing); pairs in any orientation, duplicates allowed.  Removal is per pair: both directions and every parallel copy go, pairs that
        name no edge are ignored, weights travel with their edges.  The result equals the store the constructor builds from the filtered edges, bit for bit,
        and is independent of this one (either may be closed first): evaluate link prediction on it so that no structural input sees a held-out link."""
        import torch
        if isinstance(removed, dict):
            bad = [g for g in removed if not (isinstance(g, (int, np.integer)) and 0 <= g < self.n_graphs)]
            if bad:
                raise ValueError('without_edges: graph %r of a store with %d graph(s)' % (bad[0], self.n_graphs))
            removed = [removed.get(g) for g in range(self.n_graphs)]
        elif len(removed) != self.n_graphs:
            raise ValueError('without_edges: %d entries for a store with %d graph(s)' % (len(removed), self.n_graphs))
        keys = [self.pair_keys(g, [] if r is None else r) for g, r in enumerate(removed)]
        off = np.zeros(self.n_graphs + 1, np.int64)
        off[1:] = np.cumsum([len(k) for k in keys])
        d_keys = torch.from_numpy(np.concatenate(keys)).cuda() if off[-1] else None
        h = C.c_void_p()
        _lib.check(_lib.lib().gm_store_without_edges(self.handle, _lib.ptr(d_keys), _lib.ptr(off), C.byref(h), _lib.stream_ptr()), 'gm_store_without_edges')
        new = object.__new__(GraphStore)
        new.handle = h
        new.n_graphs, new.feat_dim = self.n_graphs, self.feat_dim
        new.weighted = bool(_lib.lib().gm_store_weighted(h))
        d = [new.dims(g) for g in range(new.n_graphs)]
        new.n_nodes, new.n_edges = [n for n, _, _ in d], [e for _, e, _ in d]
        new._host_csr = new._host_weights = None      # read back at first access
        return new

    def split_edges(self, g, val=0.05, test=0.10, seed=222):
        """(val_pairs int64 [n_v, 2], test_pairs int64 [n_t, 2]): a deterministic random split of the links of graph `g` -- the distinct node pairs u < v joined by an
        edge in either direction, self loops aside -- decided per pair by a hash on the device (gm_store_split_edges; the definition is in include/gmeta_hip.h):
        a link is test with probability `test`, validation with probability `val`, else it stays.  Each array ascends by u * N + v.  A function of the graph,
        the seed and the fractions alone; without_edges({g: both}) takes the pairs out."""
        import torch
        from fractions import Fraction
        g, _ = self._pairs_of(g, [], 'split_edges')
        fv, ft = Fraction(val), Fraction(test)
        if not (0 <= fv <= 1 and 0 <= ft <= 1 and fv + ft <= 1):
            raise ValueError('split_edges: val = %r, test = %r; fractions in [0, 1] with val + test <= 1' % (val, test))
        t_test, t_val = int(ft * 2 ** 32), int((ft + fv) * 2 ** 32)      # floor(fraction * 2^32) in exact arithmetic: no float reaches the ABI
        cnt = (C.c_int64 * 3)()
        call = lambda pairs, cls, cap: _lib.check(_lib.lib().gm_store_split_edges(self.handle, g, int(seed) & 0xFFFFFFFFFFFFFFFF, t_test, t_val, _lib.ptr(pairs),      # noqa: E731
                                                                                   _lib.ptr(cls), cap, cnt, _lib.stream_ptr()), 'gm_store_split_edges')
        call(None, None, 0)
        n = int(cnt[1] + cnt[2])
        pairs = torch.empty((max(n, 1), 2), dtype=torch.int32, device='cuda')
        cls = torch.empty(max(n, 1), dtype=torch.uint8, device='cuda')
        call(pairs, cls, n)
        pairs, cls = pairs[:n].cpu().numpy().astype(np.int64), cls[:n].cpu().numpy()
        return pairs[cls == 1], pairs[cls == 2]

    def has_edges(self, g, pairs):
        """bool [m]: whether graph `g` holds an edge between the two nodes of each of the [m, 2] `pairs`, in either direction (gm_store_has_edges: the
        negative sampler's own adjacency test)."""
        import torch
        g, p = self._pairs_of(g, pairs, 'has_edges')
        return self._pair_call('gm_store_has_edges', g, p, len(p), torch.uint8).astype(bool)

    def pair_scores(self, g, pairs, mask_target=False):
        """float32 [m, 5]: the neighbourhood heuristics of the [m, 2] node `pairs` of graph `g`, columns gmeta_amd.PAIR_SCORES = (cn, jaccard, adamic_adar,
        resource_allocation, pref_attachment), computed on the device (gm_store_pair_scores; the definition is in include/gmeta_hip.h, tests/pair_score_ref.py
        restates it).  Neighbourhoods are distinct nodes joined by an edge in either direction, self loops and weights aside; a pair may come in any
        orientation.  mask_target=True scores an adjacent pair as if its own edge were absent (both degrees one less): pass it when the positive pairs are
        edges of the graph, as with Subgraphs(mask_target=True)."""
        import torch
        g, p = self._pairs_of(g, pairs, 'pair_scores')
        return self._pair_call('gm_store_pair_scores', g, p, (len(p), 5), torch.float32, _lib.PAIR_MASK_TARGET if mask_target else 0)

    def pair_walks(self, g, pairs, mask_target=False):
        """int64 [m, 3]: the numbers of walks of length 1, 2 and 3 between the two nodes of each of the [m, 2] `pairs` of graph `g` in the distinct-neighbour
        graph of pair_scores, computed on the device (gm_store_pair_walks; the definition is in include/gmeta_hip.h, tests/path_walk_ref.py restates it).
        Exact integers; a pair may come in any orientation.  mask_target=True counts the walks of an adjacent pair without its own edge.
        gmeta_amd.local_path_index / katz_index turn the rows into scores."""
        import torch
        g, p = self._pairs_of(g, pairs, 'pair_walks')
        return self._pair_call('gm_store_pair_walks', g, p, (len(p), 3), torch.int64, _lib.PAIR_MASK_TARGET if mask_target else 0)

    @staticmethod
    def _walk_of(alpha, iters, what):
        alpha, iters = float(alpha), int(iters)
        if not (np.isfinite(alpha) and 0.0 < float(np.float32(alpha)) < 1.0):
            raise ValueError('%s: alpha = %r; 0 < alpha < 1' % (what, alpha))
        if not 1 <= iters <= 255:
            raise ValueError('%s: iters = %d; 1 .. 255' % (what, iters))
        return alpha, iters

    def rooted_pagerank(self, g, sources, alpha=0.15, iters=20):
        """float32 [m, N]: row r is the rooted PageRank vector of sources[r] in graph `g` after `iters` steps of the walk that returns to its source with
        probability `alpha`, over the distinct-neighbour graph of pair_scores, computed on the device (gm_store_rooted_pagerank; the definition is in
        include/gmeta_hip.h, tests/pagerank_ref.py restates it).  A node without neighbours keeps its mass, so every row sums to 1 up to rounding.  Duplicate sources
        are allowed."""
        import torch
        alpha, iters = self._walk_of(alpha, iters, 'rooted_pagerank')
        g, a = self._nodes_of(g, sources, 'rooted_pagerank')
        return self._source_call('gm_store_rooted_pagerank', g, a, torch.float32, alpha, iters)

    def pair_pagerank(self, g, pairs, mask_target=False, alpha=0.15, iters=20):
        """float32 [m, 2]: for each of the [m, 2] node `pairs` of graph `g`, canonicalised to (u, v) = (min, max), the rooted PageRank of v seen from u and of
        u seen from v (rooted_pagerank's entries, bit for bit), computed on the device (gm_store_pair_pagerank).  mask_target=True walks an adjacent pair's
        two columns in the graph without the pair's own edge.  gmeta_amd.rooted_pagerank_index turns the rows into the score."""
        import torch
        alpha, iters = self._walk_of(alpha, iters, 'pair_pagerank')
        g, p = self._pairs_of(g, pairs, 'pair_pagerank')
        return self._pair_call('gm_store_pair_pagerank', g, p, (len(p), 2), torch.float32, _lib.PAIR_MASK_TARGET if mask_target else 0, alpha, iters)

    @staticmethod
    def _max_dist_of(max_dist, what):
        max_dist = int(max_dist)
        if not 1 <= max_dist <= 254:
            raise ValueError('%s: max_dist = %d; 1 .. 254' % (what, max_dist))
        return max_dist

    def node_distances(self, g, sources, max_dist=8):
        """uint8 [m, N]: row r holds the shortest-path distance (edges) from sources[r] to every node of graph `g` in the distinct-neighbour graph of
        pair_scores, searched on the device one bit per (node, source) (gm_store_node_distances; the definition is in include/gmeta_hip.h,
        tests/distance_ref.py restates it).  A node that no path of at most `max_dist` (1..254) edges reaches holds gmeta_amd.DIST_UNREACHED (255).  Duplicate
        sources are allowed."""
        import torch
        max_dist = self._max_dist_of(max_dist, 'node_distances')
        g, a = self._nodes_of(g, sources, 'node_distances')
        return self._source_call('gm_store_node_distances', g, a, torch.uint8, max_dist)

    def pair_distance(self, g, pairs, mask_target=False, max_dist=8):
        """uint8 [m]: the shortest-path distance between the two nodes of each of the [m, 2] `pairs` of graph `g` (node_distances' entries), searched on
        the device (gm_store_pair_distance); gmeta_amd.DIST_UNREACHED (255) beyond `max_dist` (1..254) edges.  mask_target=True measures an adjacent pair in
        the graph without its own edge: the length of the detour, 255 when the edge is a bridge (or the detour is longer than max_dist).
        gmeta_amd.graph_distance_index turns the bytes into the score."""
        import torch
        max_dist = self._max_dist_of(max_dist, 'pair_distance')
        g, p = self._pairs_of(g, pairs, 'pair_distance')
        return self._pair_call('gm_store_pair_distance', g, p, len(p), torch.uint8, _lib.PAIR_MASK_TARGET if mask_target else 0, max_dist)

    @staticmethod
    def _profile_dist_of(max_dist, what):
        max_dist = int(max_dist)
        if not 1 <= max_dist <= 7:
            raise ValueError('%s: max_dist = %d; 1 .. 7' % (what, max_dist))
        return max_dist

    def pair_distance_profile(self, g, pairs, mask_target=False, max_dist=3):
        """int32 [m, D + 2, D + 2], D = `max_dist` (1..7): for each of the [m, 2] node `pairs` of graph `g`, canonicalised to (u, v) = (min, max), entry [a][b]
        counts the nodes a hops from u and b hops from v (node_distances' distances); index D + 1 gathers everything farther and the unreached.  Counted on
        the device from the search's state, only the tables come back (gm_store_pair_distance_profile; the definition is in include/gmeta_hip.h,
        tests/distance_profile_ref.py restates it).  Both orientations of a pair give the same table; gmeta_amd.link_distance_profiles orients it by the
        pair's name.  mask_target=True searches an adjacent pair's two columns in the graph without its own edge."""
        import torch
        max_dist = self._profile_dist_of(max_dist, 'pair_distance_profile')
        g, p = self._pairs_of(g, pairs, 'pair_distance_profile')
        return self._pair_call('gm_store_pair_distance_profile', g, p, (len(p), max_dist + 2, max_dist + 2), torch.int32, _lib.PAIR_MASK_TARGET if mask_target else 0,
                               max_dist)

    def sketches(self, g, hops=2, p=8, k=128, seed=222):
        """gmeta_amd.NodeSketches of graph `g`: per node and level 0 .. `hops` (1..4) a HyperLogLog sketch of 2^`p` registers (p in 4..10) and a MinHash
        sketch of `k` words (a multiple of 32 in 32..512) of its ball, built once on the device (gm_store_sketch_build; the definition is in
        include/gmeta_hip.h, tests/sketch_ref.py restates it).  Its pair_counts + gmeta_amd.sketch_distance_profile estimate the table of
        pair_distance_profile for any pair without a search.  No mask_target: the sketches describe the whole graph; pair_distance_profile(mask_target=True)
        gives the exact, masked table of a shortlist."""
        from .sketches import NodeSketches
        return NodeSketches(self, g, hops, p, k, seed)

    def propagated_features(self, g, hops=2, self_loops=True):
        """gmeta_amd.PropagatedFeatures of graph `g`: the SIGN / BUDDY levels x_0 = X, x_{t+1} = A^ x_t for t < `hops` (1..8) of the store's feature table, A^ the
        GraphConv normalisation over the WHOLE graph's in-edge CSR (parallel edges, self loops, directions and weights kept) with one self loop in front of every
        row under `self_loops`, built once on the device (gm_store_propagate_build; the definition is in include/gmeta_hip.h, tests/hop_feature_ref.py restates
        it).  Its pair_features gives the x_t[u] * x_t[v] inputs of a BUDDY predictor; the structural counts come from sketches.  No mask_target: the levels
        describe the whole graph, as the sketches do."""
        from .propagate import PropagatedFeatures
        return PropagatedFeatures(self, g, hops, self_loops)

    def neighbour_degrees(self, g):
        """int32 [N]: the number of distinct neighbours (either direction, itself aside) of every node of graph `g` -- the degrees the pair scores use."""
        import torch
        g, _ = self._pairs_of(g, [], 'neighbour_degrees')
        out = torch.empty(self.n_nodes[g], dtype=torch.int32, device='cuda')
        _lib.check(_lib.lib().gm_store_neighbour_degrees(self.handle, g, _lib.ptr(out), _lib.stream_ptr()), 'gm_store_neighbour_degrees')
        return out.cpu().numpy()

    def link_candidates(self, g, nodes, k=10, score='adamic_adar'):
        """Candidate partners of the `nodes` of graph `g` for a link predictor: per node the nodes at distance exactly two (not adjacent, at least one shared
        neighbour; neighbourhoods as in pair_scores), ranked by the heuristic `score` (a name of gmeta_amd.PAIR_SCORES) descending, equal scores by ascending
        node id, the best `k` (1..1024) kept -- enumerated, scored and selected on the device (gm_store_pair_candidates; the definition is in
        include/gmeta_hip.h, tests/candidate_ref.py restates it).  -> (partners int64 [m, k], scores float32 [m, k], totals int64 [m]): row r holds the first
        min(k, totals[r]) partners of nodes[r] and their scores, -1 / 0.0 behind them; totals[r] is the size of the whole candidate set.  The scores are those
        pair_scores gives for the same pairs, bit for bit.  gmeta_amd.candidate_names turns the partners into the names Subgraphs.query_batch takes."""
        from .heuristics import PAIR_SCORES
        if score not in PAIR_SCORES:
            raise ValueError('link_candidates: score must be one of %s, not %r' % (', '.join(PAIR_SCORES), score))
        k = self._k_of(k, 'link_candidates')
        g, a = self._nodes_of(g, nodes, 'link_candidates')
        return self._topk_call('gm_store_pair_candidates', g, a, k, PAIR_SCORES.index(score))

    def pagerank_candidates(self, g, nodes, k=10, alpha=0.15, iters=20):
        """Candidate partners of the `nodes` of graph `g` by the global score: per node the non-adjacent nodes with positive rooted-PageRank mass seen from
        it (rooted_pagerank's row, bit for bit; the node itself and its neighbours aside), ranked descending, equal scores by ascending node id, the best `k`
        (1..1024) kept -- walked and selected on the device, so that only [m, k] comes back (gm_store_pagerank_candidates; the definition is in
        include/gmeta_hip.h, tests/pagerank_candidate_ref.py restates it).  Unlike link_candidates it reaches every node within `iters` steps.
        -> (partners int64 [m, k], scores float32 [m, k], totals int64 [m]), laid out as link_candidates lays them out: gmeta_amd.candidate_names takes the
        partners.  The score is one-directional; pair_pagerank rescores a shortlist symmetrically."""
        k = self._k_of(k, 'pagerank_candidates')
        alpha, iters = self._walk_of(alpha, iters, 'pagerank_candidates')
        g, a = self._nodes_of(g, nodes, 'pagerank_candidates')
        return self._topk_call('gm_store_pagerank_candidates', g, a, k, alpha, iters)

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().gm_store_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
