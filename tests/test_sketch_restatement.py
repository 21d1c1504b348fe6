"""CPU (-m "not gpu"): the restatement of the node sketches (tests/sketch_ref.py) by the definition against the recurrence, the exact identities the definition
states, the accuracy of the host estimators on the restatement (the device equals it bit for bit, so the accuracy carries over), and the declarations, knobs,
build list and host-side checks of the feature.  No compute call of the library: that needs a GPU (tests/test_hip_sketches.py).

The accuracy bounds are the estimators' theoretical deviations (sketch_ref.ball_bound / intersection_bound), five of them, not measurements."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import distance_profile_ref
import distance_ref
import negative_ref
import pair_score_ref
import sketch_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 222


@functools.lru_cache(maxsize=None)
def _graph(which):
    N, src, dst = {'multigraph': negative_ref.multigraph_case, 'chain': lambda: distance_ref.chain_case()[:3], 'wide': distance_profile_ref.wide_case,
                   'random': lambda: ref.random_case()[:3]}[which]()
    return N, src, dst, pair_score_ref.neighbourhoods(N, src, dst)


# ---------------------------------------------------------------------------------------------------- 1. the definition against the recurrence
@pytest.mark.parametrize('which,H,p,K', [('multigraph', 2, 8, 128), ('multigraph', 3, 10, 512), ('chain', 2, 8, 128), ('chain', 1, 4, 32), ('chain', 4, 6, 96),
                                         ('wide', 2, 8, 128)])
def test_definition_equals_recurrence_bit_for_bit(which, H, p, K):
    N, src, dst, nb = _graph(which)
    Rd, Md = ref.by_definition(N, nb, H, p, K, SEED)
    Rr, Mr = ref.by_recurrence(N, nb, H, p, K, SEED)
    assert Rd.shape == (H + 1, N, 1 << p) and Rd.dtype == np.uint8 and Md.shape == (H + 1, N, K) and Md.dtype == np.uint32
    assert np.array_equal(Rd, Rr) and np.array_equal(Md, Mr)
    assert ((Rd[0] != 0).sum(1) == 1).all() and Rd.max() <= 33 - p                                  # level 0: one register; rho <= 33 - p
    for k in (0, K - 1):                                                                           # mh_k is a bijection: distinct nodes, distinct values
        assert len(np.unique(Md[0][:, k])) == N
    R2, M2 = ref.level0(N, p, K, SEED + 1)
    assert not np.array_equal(M2, Md[0]) and not np.array_equal(R2, Rd[0])                          # the seed matters
    R3, M3 = ref.level0(N, p, K, SEED, g=1)
    assert not np.array_equal(M3, Md[0]) and not np.array_equal(R3, Rd[0])                          # ... and the graph index


def test_hashes_against_hand_values():
    s_h, s_m = ref.salts(SEED, 0)
    assert (s_h, s_m) == (int(ref.orc.sample_salt(SEED, 0, 0x534B4831, 0)), int(ref.orc.sample_salt(SEED, 0, 0x534B4D31, 0))) and s_h != s_m
    for p in (4, 8, 10):
        j, rho = ref.hll_insert(np.arange(5000), s_h, p)
        h = [int(ref.orc.lowbias32(np.uint32(z ^ s_h))) for z in range(5000)]
        for z in (0, 1, 77, 4999):
            w = (h[z] << p) & 0xFFFFFFFF
            assert j[z] == h[z] >> (32 - p) and rho[z] == (33 - p if w == 0 else 33 - w.bit_length())
        assert j.min() >= 0 and j.max() < (1 << p) and rho.min() >= 1 and rho.max() <= 33 - p
    m = ref.minhash(np.array([3, 9]), s_m, 32)
    q = int(ref.orc.lowbias32(np.uint32(9 ^ s_m)))
    assert m.dtype == np.uint32 and int(m[1, 5]) == int(ref.orc.lowbias32(np.uint32((q + 6 * 0x9E3779B9) & 0xFFFFFFFF)))


# ---------------------------------------------------------------------------------------------------- 2. the exact identities
@pytest.mark.parametrize('which,H,p,K', [('multigraph', 2, 6, 64), ('chain', 3, 8, 128)])
def test_exact_identities_of_the_pair_counts(which, H, p, K):
    N, src, dst, nb = _graph(which)
    R, M = ref.by_recurrence(N, nb, H, p, K, SEED)
    nodes = np.arange(N) if which == 'multigraph' else np.concatenate([np.arange(0, 12), np.arange(95, 106), np.arange(258, 264), np.arange(286, 292), np.arange(325, 331)])
    dist = ref.ball_distances(N, nb, nodes, H)
    rng = np.random.default_rng(1)
    idx = np.concatenate([np.stack([np.arange(len(nodes))] * 2, 1), rng.integers(0, len(nodes), (400, 2))])      # u == v, then random pairs
    pairs = nodes[idx]
    counts, balls = ref.pair_counts(R, M, pairs)
    flipped = ref.pair_counts(R, M, pairs[:, ::-1])
    assert np.array_equal(counts, flipped[0]) and np.array_equal(balls, flipped[1])                 # both orientations: the same bits
    assert (counts[..., 2] < 2 ** 43).all() and (counts[..., 2] > 0).all()
    every, every_balls = ref.pair_counts_all(R, M)                                                 # the all-pairs form the GPU tests use: the same numbers
    assert every.shape == (N, N, H + 1, H + 1, 3) and np.array_equal(every[pairs[:, 0], pairs[:, 1]], counts)
    assert np.array_equal(every_balls[pairs.min(1)], balls[:, 0]) and np.array_equal(every_balls[pairs.max(1)], balls[:, 1])
    assert (np.diff(counts[..., 1:], axis=1) <= 0).all() and (np.diff(counts[..., 1:], axis=2) <= 0).all()      # zeros, zsum do not increase in a or b
    seen = {'equal': 0, 'disjoint': 0, 'inside': 0}
    for i, (iu, iv) in enumerate(idx.tolist()):
        if pairs[i, 0] > pairs[i, 1]:
            iu, iv = iv, iu                                                                        # canonical: u = min
        for a in range(H + 1):
            for b in range(H + 1):
                Bu, Bv = dist[iu] <= a, dist[iv] <= b
                if np.array_equal(Bu, Bv):
                    assert counts[i, a, b, 0] == K
                    seen['equal'] += 1
                if not (Bu & Bv).any():
                    assert counts[i, a, b, 0] == 0
                    seen['disjoint'] += 1
                if not (Bu & ~Bv).any():                                                           # B_a(u) inside B_b(v): the union is v's ball
                    assert tuple(counts[i, a, b, 1:]) == tuple(balls[i, 1, b])
                    seen['inside'] += 1
                if not (Bv & ~Bu).any():
                    assert tuple(counts[i, a, b, 1:]) == tuple(balls[i, 0, a])
    assert min(seen.values()) > 50, seen
    lone = N - 1                                                                                   # an isolated node: its ball is itself at every level
    assert not nb[lone]
    c, _ = ref.pair_counts(R, M, [(lone, lone)])
    assert (c[0, :, :, 0] == K).all() and (c[0, :, :, 1] == (1 << p) - 1).all()
    c, b = ref.pair_counts(R, M, [(0, N), (-1, 3)])
    assert not c.any() and not b.any()                                                             # a node outside the graph


# ---------------------------------------------------------------------------------------------------- 3. the estimators on the restatement
@functools.lru_cache(maxsize=None)
def _accuracy(H, p, K):
    """-> (counts, balls of the restatement, exact I, U [n, H + 1, H + 1], exact ball sizes su, sv [n, H + 1], N, pairs canonical)"""
    N, src, dst, pairs = ref.random_case()
    nb = _graph('random')[3]
    R, M = ref.by_recurrence(N, nb, H, p, K, SEED)
    counts, balls = ref.pair_counts(R, M, pairs)
    pc = np.stack([pairs.min(1), pairs.max(1)], 1)
    nodes, inv = np.unique(pc, return_inverse=True)
    inv = inv.reshape(-1, 2)
    dist = ref.ball_distances(N, nb, nodes, H)
    ex = [ref.exact_cumulative(dist[iu], dist[iv], H) for iu, iv in inv.tolist()]
    return counts, balls, np.stack([e[0] for e in ex]), np.stack([e[1] for e in ex]), np.stack([e[2] for e in ex]), np.stack([e[3] for e in ex]), N, pc


@pytest.mark.parametrize('H,p,K', [(2, 8, 128), (3, 8, 128)])
def test_estimators_stay_within_their_theoretical_deviation(H, p, K):
    import gmeta_amd
    counts, balls, I, U, su, sv, N, pc = _accuracy(H, p, K)
    assert len(pc) == 300 and pair_score_ref.degrees(*ref.random_case()[:3]).mean() > 5.5
    size = gmeta_amd.hll_cardinality(balls[..., 0], balls[..., 1], p)
    exact = np.stack([su, sv], 1)
    ratio_b = np.abs(size - exact) / ref.ball_bound(exact, p)
    est = gmeta_amd.sketch_intersections(counts, p, K)
    ratio_i = np.abs(est - I) / ref.intersection_bound(I, U, p, K)
    print('worst |err| / bound at (H, p, K) = (%d, %d, %d): balls %.3f, intersections %.3f' % (H, p, K, ratio_b.max(), ratio_i.max()))
    assert (ratio_b <= 1.0).all() and (ratio_i <= 1.0).all()
    P = gmeta_amd.sketch_distance_profile(counts, balls, N, p, K)
    assert P.shape == (len(pc), H + 2, H + 2) and P.dtype == np.float64
    assert np.allclose(P.sum((1, 2)), N, rtol=1e-9, atol=0)


def _exact_as_counts(I, su, sv):
    """The exact cumulative counts in the slots the estimators read (test-local: with _exact_estimators the functions see no sketch at all)."""
    counts = np.zeros(I.shape + (3,), np.int64)
    counts[..., 0] = I
    balls = np.zeros((len(I), 2, I.shape[1], 2), np.int64)
    balls[:, 0, :, 0], balls[:, 1, :, 0] = su, sv
    return counts, balls


def test_profile_from_exact_cumulative_counts_is_the_exact_profile(monkeypatch):
    import gmeta_amd
    from gmeta_amd import heuristics
    H = 3
    _, _, I, U, su, sv, N, pc = _accuracy(H, 8, 128)
    monkeypatch.setattr(heuristics, 'sketch_intersections', lambda counts, p, k: np.asarray(counts)[..., 0].astype(np.float64))
    monkeypatch.setattr(heuristics, 'hll_cardinality', lambda zeros, zsum, p: np.asarray(zeros).astype(np.float64))
    counts, balls = _exact_as_counts(I, su, sv)
    got = heuristics.sketch_distance_profile(counts, balls, N, 8, 128)
    want = distance_profile_ref.profile(N, *ref.random_case()[1:3], pc, 0, H, _graph('random')[3])
    assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))
    assert np.array_equal(ref.cumulate(want)[0], I) and np.array_equal(ref.cumulate(want)[1], su) and np.array_equal(ref.cumulate(want)[2], sv)
    assert gmeta_amd.sketch_distance_profile is heuristics.sketch_distance_profile


def test_hll_cardinality_against_hand_values():
    import gmeta_amd
    m = 256.0
    alpha = 0.7213 / (1 + 1.079 / m)
    # every register 0: zsum = m 2^32, E = alpha m <= 2.5 m and zeros = m: m ln(1) = 0
    assert gmeta_amd.hll_cardinality(256, 256 << 32, 8) == 0.0
    # one register of rho 1: linear count m ln(m / (m - 1))
    assert np.isclose(gmeta_amd.hll_cardinality(255, (255 << 32) + (1 << 31), 8), m * np.log(m / 255), rtol=1e-15)
    # no zero register: the raw estimate even when small; a large sum: the raw estimate
    assert np.isclose(gmeta_amd.hll_cardinality(0, 256 << 31, 8), alpha * m * m / 128.0, rtol=1e-15)
    assert np.isclose(gmeta_amd.hll_cardinality(3, 256 << 22, 8), alpha * m * m / 0.25, rtol=1e-15)
    for p, a in ((4, 0.673), (5, 0.697), (6, 0.709)):
        mm = float(1 << p)
        assert np.isclose(gmeta_amd.hll_cardinality(0, int(mm) << 20, p), a * mm * mm / (mm / 4096.0), rtol=1e-15)
    out = gmeta_amd.hll_cardinality(np.array([[0, 256], [0, 0]]), np.array([[0, 256 << 32], [256 << 31, 0]]), 8)
    assert out.shape == (2, 2) and out.dtype == np.float64 and out[0, 0] == 0 and out[1, 1] == 0      # an all-zero record
    with pytest.raises(ValueError, match='p = 3'):
        gmeta_amd.hll_cardinality(1, 1, 3)


class _HostSketches:
    """NodeSketches.pair_counts on the restatement (host logic of link_sketch_profiles; no GPU)."""

    def __init__(self, N, src, dst, g, H=2, p=6, k=64):
        self.n_nodes, self.hops, self.p, self.k, self.calls = N, H, p, k, []
        self.R, self.M = ref.by_recurrence(N, pair_score_ref.neighbourhoods(N, src, dst), H, p, k, SEED, g)

    def pair_counts(self, pairs):
        self.calls.append(len(pairs))
        return ref.pair_counts(self.R, self.M, pairs)


def test_link_sketch_profiles_orients_by_name_and_features_have_the_exact_shape():
    import gmeta_amd
    rng = np.random.default_rng(3)
    graphs = [(30, rng.integers(0, 30, 40), rng.integers(0, 30, 40)), (20, rng.integers(0, 20, 25), rng.integers(0, 20, 25))]
    sk = {g: _HostSketches(*graphs[g], g) for g in (0, 1)}
    names, want = [], []
    for _ in range(60):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, graphs[g][0], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b))
        c, bl = ref.pair_counts(sk[g].R, sk[g].M, [(a, b)])
        t = gmeta_amd.sketch_distance_profile(c, bl, graphs[g][0], 6, 64)[0]
        want.append(t.T if a > b else t)
    got = gmeta_amd.link_sketch_profiles(sk, names)
    assert got.shape == (60, 4, 4) and got.dtype == np.float64 and np.array_equal(got, np.asarray(want))
    flipped = np.array([int(nm.split('_')[1]) > int(nm.split('_')[2]) for nm in names])
    assert flipped.any() and (~flipped).any() and any(not np.array_equal(w, w.T) for w in got[flipped])
    assert [len(s.calls) for s in sk.values()] == [1, 1] and sum(s.calls[0] for s in sk.values()) == 60
    assert np.array_equal(gmeta_amd.link_sketch_profiles([sk[0], sk[1]], names), got)              # a sequence indexed by graph
    assert gmeta_amd.link_sketch_profiles(sk, []).shape == (0, 2, 2)
    with pytest.raises(ValueError, match='g_i_j'):
        gmeta_amd.link_sketch_profiles(sk, ['0_1'])
    sk[1].hops = 3
    with pytest.raises(ValueError, match='different hops'):
        gmeta_amd.link_sketch_profiles(sk, names)
    # the features: the shape and the symmetry of distance_profile_features; negative estimates are clipped
    exact = distance_profile_ref.oriented(distance_profile_ref.profile(*graphs[0], [(3, 7)], 0, 2), [(3, 7)])
    f_exact = gmeta_amd.distance_profile_features(exact)
    f = gmeta_amd.sketch_profile_features(got)
    assert f.shape == (60, 16) and f.dtype == np.float64 and f.shape[1:] == f_exact.shape[1:] and (f >= 0).all()
    assert np.array_equal(gmeta_amd.sketch_profile_features(got.transpose(0, 2, 1)), f)
    assert np.array_equal(gmeta_amd.sketch_profile_features(exact.astype(np.float64)), f_exact)      # on exact tables: the exact features
    T = np.array([[[1.0, -0.5], [2.5, 10.0]]])
    assert np.allclose(gmeta_amd.sketch_profile_features(T, symmetric=False)[0], np.log1p([1.0, 0.0, 2.5, 10.0]), rtol=0, atol=1e-15)
    assert np.allclose(gmeta_amd.sketch_profile_features(T)[0], np.log1p([2.0, 2.0, 2.0, 20.0]), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='shape'):
        gmeta_amd.sketch_profile_features(np.zeros((2, 3, 4)))


# ---------------------------------------------------------------------------------------------------- 4. declarations and plumbing
def test_the_exports_are_declared_bound_tunable_and_built():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r'typedef\s+struct\s+gm_sketch\s+gm_sketch_t\s*;', code)
    for name, n_args in (('gm_store_sketch_build', 8), ('gm_sketch_dims', 6), ('gm_sketch_registers', 7), ('gm_sketch_pair_counts', 6), ('gm_sketch_destroy', 1)):
        assert re.search(r'\b(int32_t|void)\s+%s\s*\(' % name, code) and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    assert 'tests/sketch_ref.py' in txt and 'sketch_chunk' in txt and 'sketch_mib' in txt and 'GM_PAIR_MASK_TARGET' in txt and 'bijection' in txt
    assert hasattr(gmeta_amd.GraphStore, 'sketches')
    for name in ('NodeSketches', 'hll_cardinality', 'sketch_intersections', 'sketch_distance_profile', 'link_sketch_profiles', 'sketch_profile_features'):
        assert name in gmeta_amd.__all__ and hasattr(gmeta_amd, name)
    build = open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert build.count("'node_sketches.hip'") == 1
    assert build.index("'pair_distance.hip'") < build.index("'distance_profile.hip'") < build.index("'node_sketches.hip'") < build.index("'pair_walks.hip'")
    assert [ln for ln in build.splitlines() if "'node_sketches.hip'" in ln][0].startswith("SOURCES += ['node_sketches.hip']")      # a line of its own
    for knob, env in ((b'sketch_chunk', b'GM_SKETCH_CHUNK'), (b'sketch_mib', b'GM_SKETCH_MIB')):
        for v in (7, 1, 2 ** 20, -3, 0):
            assert _lib.lib().gm_set_tuning(knob, v) == 0 and _lib.lib().gm_get_tuning(knob) == v == _lib.lib().gm_get_tuning(env)
        assert _lib.lib().gm_set_tuning(env, 40) == 0 and _lib.lib().gm_get_tuning(knob) == 40
        assert _lib.lib().gm_set_tuning(knob, 0) == 0 and _lib.lib().gm_get_tuning(env) == 0


def test_host_side_checks_come_before_the_library():
    """No GPU and no store behind the object: the checks come first."""
    import gmeta_amd
    store = object.__new__(gmeta_amd.GraphStore)
    store.handle, store.n_graphs, store.n_nodes = None, 1, [10]
    for kw, msg in (({'hops': 0}, r'hops = 0; 1 \.\. 4'), ({'hops': 5}, 'hops = 5'), ({'p': 3}, r'p = 3; 4 \.\. 10'), ({'p': 11}, 'p = 11'), ({'k': 0}, 'k = 0'),
                    ({'k': 48}, 'k = 48; a multiple of 32'), ({'k': 544}, 'k = 544')):
        with pytest.raises(ValueError, match=msg):
            store.sketches(0, **kw)
    with pytest.raises(ValueError, match='graph 1'):
        store.sketches(1)
    sk = object.__new__(gmeta_amd.NodeSketches)
    sk.handle, sk.n_nodes, sk.hops, sk.p, sk.k = 1, 10, 2, 8, 128
    with pytest.raises(ValueError, match='outside'):
        sk.pair_counts([[0, 10]])
    with pytest.raises(ValueError, match='outside'):
        sk.registers([-1], 0)
    for level in (-1, 3):
        with pytest.raises(ValueError, match='level = %d' % level):
            sk.registers([1], level)
    sk.handle = None
    with pytest.raises(ValueError, match='closed'):
        sk.pair_counts([[0, 1]])


def test_sketch_kernels_do_not_spill():
    """The new translation unit with -Rpass-analysis=kernel-resource-usage: ScratchSize == 0 for every kernel, as test_cabi_and_host.py asks of gemm.hip and
    agg.hip."""
    csrc = os.path.join(ROOT, 'g-meta_amd', 'csrc')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-c', os.path.join(csrc, 'node_sketches.hip'), '-o', os.devnull,
                        '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen, bad = None, set(), []
    for line in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', line)
        if m and name:
            seen.add(name)
            if int(m.group(1)) > 0:
                bad.append((name, int(m.group(1))))
    for kernel in ('k_sketch_init', 'k_sketch_level', 'k_sketch_parts', 'k_sketch_hubs', 'k_sketch_read', 'k_sketch_pairsILi2', 'k_sketch_pairsILi3', 'k_sketch_pairsILi4',
                   'k_sketch_pairsILi5'):
        assert any(kernel in n for n in seen), kernel
    assert not bad, 'kernels spilling to scratch: %s' % bad
