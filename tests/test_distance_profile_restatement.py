"""CPU (-m "not gpu"): the restatement of the joint hop-distance profile (tests/distance_profile_ref.py) against an independent brute force on boolean matrix
powers and against the identities the definition states, the host helpers that orient the tables and turn them into features, and the declarations, the knob
and the build list of the feature.  No compute call of the library: that needs a GPU (tests/test_hip_distance_profile.py)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import distance_profile_ref as ref
import distance_ref
import negative_ref
import pair_score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTS = (1, 3, 4, 7)


@functools.lru_cache(maxsize=None)
def _multigraph():
    """The multigraph, its dense symmetric S, every canonical pair (u <= v) and the searched columns shared by the restatement's calls."""
    N, src, dst = negative_ref.multigraph_case()
    nb = pair_score_ref.neighbourhoods(N, src, dst)
    S = np.zeros((N, N), bool)
    for v, row in enumerate(nb):
        S[v, list(row)] = True
    pairs = np.array([(u, v) for u in range(N) for v in range(u, N)], np.int64)
    return N, src, dst, nb, S, pairs, {}


def _levels(S, sources):
    """int64 [len(sources), N]: the distances from the sources in the graph of the boolean matrix S by matrix powers; 255 where no walk leads."""
    N = len(S)
    k = np.arange(len(sources))
    seen = np.zeros((N, len(sources)), bool)
    seen[sources, k] = True
    front, d = seen.copy(), np.full((N, len(sources)), 255, np.int64)
    d[sources, k] = 0
    for t in range(1, N):
        front = (S.astype(np.float32) @ front.astype(np.float32) > 0) & ~seen
        if not front.any():
            break
        seen |= front
        d[front] = t
    return d.T


def _brute(N, S, pairs, flags, max_dist):
    """The tables of the canonical pairs from one-hot level matrices: P[u, v, a, b] = sum_z [cap d_u[z] == a][cap d_v[z] == b]; a masked adjacent pair from the
    two searches in S without its edge."""
    side = max_dist + 2
    full = ref.cap(_levels(S, np.arange(N)), max_dist)
    hot = [(full == a).astype(np.float32) for a in range(side)]
    out = np.zeros((len(pairs), side, side), np.int32)
    for a in range(side):
        for b in range(side):
            out[:, a, b] = (hot[a] @ hot[b].T)[pairs[:, 0], pairs[:, 1]]
    if flags:
        for k, (u, v) in enumerate(pairs.tolist()):
            if u != v and S[u, v]:
                T = S.copy()
                T[u, v] = T[v, u] = False
                du, dv = ref.cap(_levels(T, np.array([u, v])), max_dist)
                out[k] = np.bincount(du * side + dv, minlength=side * side).reshape(side, side)
    return out


@pytest.mark.parametrize('max_dist', DISTS)
def test_against_matrix_powers_and_the_identities_on_the_multigraph(max_dist):
    N, src, dst, nb, S, pairs, cols = _multigraph()
    side = max_dist + 2
    cn = pair_score_ref.pair_scores(N, src, dst, pairs, 0, nb)[:, 0].astype(np.int64)
    off = pairs[:, 0] != pairs[:, 1]
    adj = S[pairs[:, 0], pairs[:, 1]]
    got = {}
    for flags in (0, 1):
        P = ref.profile(N, src, dst, pairs, flags, max_dist, nb, cols)
        assert P.dtype == np.int32 and P.shape == (len(pairs), side, side)
        assert np.array_equal(P, _brute(N, S, pairs, flags, max_dist)), flags
        assert (P.sum((1, 2)) == N).all()
        d = ref.cap(distance_ref.pair_distance(N, src, dst, pairs, flags, 254, nb), max_dist)
        one = np.zeros((len(pairs), side), np.int32)
        one[np.arange(len(pairs)), d] = 1
        assert np.array_equal(P[:, 0, :], one) and np.array_equal(P[:, :, 0], one)               # a single 1 in row 0 and in column 0, at the capped distance
        assert np.array_equal(P[off, 1, 1], cn[off])                                             # the pair's own edge never joins a common neighbour
        same = P[~off]
        assert (same[:, 0, 0] == 1).all() and (same == same * np.eye(side, dtype=np.int32)).all()      # u == v: diagonal
        for k in (0, 1, 299, 300, len(pairs) - 1, 4567):
            u, v = pairs[k].tolist()
            cut = bool(flags) and u != v and v in nb[u]
            du = ref.cap(distance_ref.column(N, nb, u, v if cut else -1, 254), max_dist)
            dv = ref.cap(distance_ref.column(N, nb, v, u if cut else -1, 254), max_dist)
            assert np.array_equal(P[k].sum(1), np.bincount(du, minlength=side)) and np.array_equal(P[k].sum(0), np.bincount(dv, minlength=side))
        got[flags] = P
    assert np.array_equal(got[1][~adj], got[0][~adj]) and int(adj.sum()) == 1306                  # a non-adjacent pair under the flag: the unflagged bits
    assert (got[1][adj][:, 0, 1] == 0).all() and (got[0][adj][:, 0, 1] == 1).all()
    # both orientations, duplicates and nodes outside the graph
    some = pairs[::501]
    back = ref.profile(N, src, dst, some[:, ::-1], 1, max_dist, nb, cols)
    assert np.array_equal(back, got[1][::501]) and np.array_equal(ref.oriented(back, some[:, ::-1]), got[1][::501].transpose(0, 2, 1))
    odd = ref.profile(N, src, dst, [(0, N), (-1, 5), (5, 5), (5, 5)], 0, max_dist, nb, cols)
    assert not odd[:2].any() and np.array_equal(odd[2], odd[3]) and odd[2].sum() == N


def test_the_wide_case_and_the_cap():
    N, src, dst = ref.wide_case()
    assert N == 64 * 70 + 17 and (N + 63) // 64 > 64
    deg = pair_score_ref.degrees(N, src, dst)
    assert 2.5 < deg.mean() < 3.5
    assert ref.cap([0, 3, 4, 254, 255], 3).tolist() == [0, 3, 4, 4, 4]
    P = ref.profile(N, src, dst, [(5, 9), (9, 5), (5, 5)], 1, 7)
    assert np.array_equal(P[0], P[1]) and (P.sum((1, 2)) == N).all() and P[2][0, 0] == 1
    with pytest.raises(AssertionError):
        ref.profile(N, src, dst, [(0, 1)], 0, 8)


def test_the_export_is_declared_bound_tunable_and_built():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = 'gm_store_pair_distance_profile'
    assert re.search(r'\bint32_t\s+%s\s*\(' % name, code) and hasattr(lib, name)
    assert len(_lib.PROTOTYPES[name][1]) == 8
    assert 'tests/distance_profile_ref.py' in txt and 'dist_plane_kib' in txt
    assert hasattr(gmeta_amd.GraphStore, 'pair_distance_profile')
    for helper in ('link_distance_profiles', 'distance_profile_features'):
        assert helper in gmeta_amd.__all__ and hasattr(gmeta_amd, helper)
    build = open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert build.count("'distance_profile.hip'") == 1 and build.index("'pair_distance.hip'") < build.index("'distance_profile.hip'") < build.index("'pair_walks.hip'")
    internal = open(os.path.join(ROOT, 'g-meta_amd', 'csrc', 'gm_internal.h')).read()
    assert 'gm_prof_transpose' in internal and 'gm_prof_count' in internal
    for v in (16, 1, 2 ** 20, 0):
        assert _lib.lib().gm_set_tuning(b'dist_plane_kib', v) == 0 and _lib.lib().gm_get_tuning(b'dist_plane_kib') == v == _lib.lib().gm_get_tuning(b'GM_DIST_PLANE_KIB')
    assert _lib.lib().gm_set_tuning(b'GM_DIST_PLANE_KIB', 40) == 0 and _lib.lib().gm_get_tuning(b'dist_plane_kib') == 40
    assert _lib.lib().gm_set_tuning(b'dist_plane_kib', 0) == 0 and _lib.lib().gm_get_tuning(b'GM_DIST_PLANE_KIB') == 0


def test_graphstore_method_refuses_bad_arguments_before_the_library():
    """No GPU and no store behind the object: the checks come first."""
    import gmeta_amd
    store = object.__new__(gmeta_amd.GraphStore)
    store.handle, store.n_graphs, store.n_nodes = None, 1, [10]
    for max_dist in (0, 8, -1):
        with pytest.raises(ValueError, match=r'max_dist = %d; 1 \.\. 7' % max_dist):
            store.pair_distance_profile(0, [[1, 2]], max_dist=max_dist)
    with pytest.raises(ValueError, match='graph 1'):
        store.pair_distance_profile(1, [[1, 2]])
    with pytest.raises(ValueError, match='outside'):
        store.pair_distance_profile(0, [[0, 10]])
    with pytest.raises(ValueError, match='outside'):
        store.pair_distance_profile(0, [[-1, 3]], mask_target=True)


class _HostStore:
    """GraphStore.pair_distance_profile on the restatement (host logic of link_distance_profiles; no GPU)."""

    def __init__(self, graphs):
        self.graphs, self.calls = graphs, []

    def pair_distance_profile(self, g, pairs, mask_target=False, max_dist=3):
        self.calls.append((g, len(pairs), mask_target, max_dist))
        N, src, dst = self.graphs[g]
        return ref.profile(N, src, dst, pairs, 1 if mask_target else 0, max_dist)


def test_link_distance_profiles_calls_each_graph_once_keeps_the_order_and_orients():
    import gmeta_amd
    rng = np.random.default_rng(3)
    graphs = [(30, rng.integers(0, 30, 40), rng.integers(0, 30, 40)), (20, rng.integers(0, 20, 25), rng.integers(0, 20, 25))]
    names, want = [], []
    for k in range(70):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, graphs[g][0], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b))
        want.append(ref.oriented(ref.profile(*graphs[g], [(a, b)], 1, 2), [(a, b)])[0])
    want = np.asarray(want, np.int32)
    flipped = np.array([int(nm.split('_')[1]) > int(nm.split('_')[2]) for nm in names])
    assert flipped.any() and (~flipped).any() and any(not np.array_equal(w, w.T) for w in want[flipped])
    store = _HostStore(graphs)
    got = gmeta_amd.link_distance_profiles(store, names, mask_target=True, max_dist=2)
    assert got.dtype == np.int32 and got.shape == (70, 4, 4) and np.array_equal(got, want)
    assert sorted(c[0] for c in store.calls) == [0, 1] and all(c[2:] == (True, 2) for c in store.calls) and sum(c[1] for c in store.calls) == 70
    for k, nm in enumerate(names):                                             # row k reads: a hops from i, b hops from j
        g, i, j = (int(x) for x in nm.split('_'))
        assert got[k][0].sum() == 1 and got[k][:, 0].sum() == 1 and got[k].sum() == graphs[g][0]
    store.calls.clear()
    plain = gmeta_amd.link_distance_profiles(store, names)
    assert plain.shape == (70, 5, 5) and all(c[2:] == (False, 3) for c in store.calls)
    assert gmeta_amd.link_distance_profiles(store, [], max_dist=1).shape == (0, 3, 3)
    with pytest.raises(ValueError, match='g_i_j'):
        gmeta_amd.link_distance_profiles(store, ['0_1'])


def test_distance_profile_features_against_hand_values():
    import gmeta_amd
    P = np.array([[[1, 0, 2], [0, 3, 0], [4, 0, 10]]], np.int32)
    sym = gmeta_amd.distance_profile_features(P)
    assert sym.dtype == np.float64 and sym.shape == (1, 9)
    assert np.allclose(sym[0], np.log([3, 1, 7, 1, 7, 1, 7, 1, 21]), rtol=0, atol=1e-12)
    raw = gmeta_amd.distance_profile_features(P, symmetric=False)
    assert np.allclose(raw[0], np.log([2, 1, 3, 1, 4, 1, 5, 1, 11]), rtol=0, atol=1e-12)
    assert np.array_equal(gmeta_amd.distance_profile_features(P.transpose(0, 2, 1)), sym)        # symmetric: the orientation drops out
    assert gmeta_amd.distance_profile_features(np.zeros((0, 5, 5), np.int32)).shape == (0, 25)
    with pytest.raises(ValueError, match='shape'):
        gmeta_amd.distance_profile_features(np.zeros((2, 3, 4), np.int32))
