"""CPU (-m "not gpu"): the per-pair, loop-written float64 restatement of gm_sketch_pair_features (tests/sketch_feature_ref.py; the definition is in
include/gmeta_hip.h) against the vectorised host chain of gmeta_amd.heuristics, on the integers of the sketch restatement (sketch_ref.pair_counts) of the fixed
random graph; the declaration, export and binding of the call; and the driver's flag.  The two chains share no code; before the log they differ only in the
order of sums of at most 36 terms."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import pair_score_ref
import sketch_feature_ref as fref
import sketch_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 222
P, K = 8, 128


@functools.lru_cache(maxsize=None)
def _case(H):
    """-> N, the 300 pairs of sketch_ref.random_case in both orientations (600 rows), counts, balls of the restatement"""
    N, src, dst, pairs = ref.random_case()
    R, M = ref.by_recurrence(N, pair_score_ref.neighbourhoods(N, src, dst), H, P, K, SEED)
    both = np.concatenate([pairs, pairs[:, ::-1]])
    counts, balls = ref.pair_counts(R, M, both)
    for w in (both, counts, balls):
        w.setflags(write=False)
    return N, both, counts, balls


def _largest_card(counts, balls, p):
    import gmeta_amd
    n = len(counts)
    return np.maximum(gmeta_amd.hll_cardinality(counts[..., 1], counts[..., 2], p).reshape(n, -1).max(1),
                      gmeta_amd.hll_cardinality(balls[..., 0], balls[..., 1], p).reshape(n, -1).max(1))


@pytest.mark.parametrize('symmetric', [True, False])
@pytest.mark.parametrize('H', [1, 2, 3, 4])
def test_restatement_equals_the_vectorised_host_chain(H, symmetric):
    import gmeta_amd
    N, both, counts, balls = _case(H)
    got, M, met = fref.features(counts, balls, both, N, P, K, symmetric)
    tables = gmeta_amd.sketch_distance_profile(counts, balls, N, P, K)
    swap = both[:, 0] > both[:, 1]
    assert swap.sum() >= 250 and (~swap).sum() >= 250
    oriented = tables.copy()
    oriented[swap] = oriented[swap].transpose(0, 2, 1)                          # the transposition rule of link_sketch_profiles
    want = gmeta_amd.sketch_profile_features(oriented, symmetric=symmetric)
    big = np.maximum(_largest_card(counts, balls, P), float(N))
    assert np.array_equal(M, big)
    assert got.shape == want.shape == (len(both), (H + 2) ** 2) and got.dtype == np.float64
    err = np.abs(got - want)
    tol = 1e-12 * np.abs(want) + 1e-12 * big[:, None]
    print('H %d symmetric %d: worst |restatement - host chain| / tolerance %.3g; branches %s' % (H, symmetric, (err / tol).max(), sorted(met)))
    assert (err <= tol).all()
    # both orientations: bit-equal when symmetric, exact transposes of each other otherwise
    n = len(both) // 2
    W = H + 2
    if symmetric:
        assert np.array_equal(got[:n], got[n:])
    else:
        assert np.array_equal(got[:n].reshape(n, W, W), got[n:].reshape(n, W, W).transpose(0, 2, 1))
        assert any(not np.array_equal(t, t.T) for t in got[:n].reshape(n, W, W))
    # the unclipped tables themselves, and that every table sums to N
    mine = fref.tables(counts, balls, N, P, K)
    assert (np.abs(mine - tables) <= 1e-12 * big[:, None, None]).all() and np.allclose(mine.sum((1, 2)), N, rtol=1e-9, atol=0)
    assert fref.branch_margin(counts, balls, P) >= fref.BRANCH_MARGIN
    # the batched form the GPU tests use is the same chain: equal up to the last place of numpy's log against math's (2^-48 M leaves room for 36 of them)
    many, M2, P2, met2 = fref.features_many(counts, balls, both, N, P, K, symmetric)
    assert (np.abs(P2 - mine) <= 2.0 ** -48 * M[:, None, None]).all() and np.allclose(M2, M, rtol=1e-15, atol=0)
    assert {b for b in ('zero', 'linear', 'raw') if met2[b]} == met
    assert (np.abs(many - got) <= 1e-15 * np.abs(got) + 2.0 ** -48 * M[:, None]).all()


def test_card_branches_zero_integers_and_hand_values():
    import gmeta_amd
    for p in range(4, 11):
        m = 1 << p
        assert fref.alpha_of(p) == {16: 0.673, 32: 0.697, 64: 0.709}.get(m, 0.7213 / (1.0 + 1.079 / m))
        zeros = np.array([0, 0, 1, m // 2, m - 1, 3, 0], np.int64)
        zsum = np.array([0, m << 20, (m - 1) << 31, m << 31, ((m - 1) << 32) + (1 << 31), m << 2, m << 31], np.int64)
        want = gmeta_amd.hll_cardinality(zeros, zsum, p)
        got = [fref.card(z, s, p) for z, s in zip(zeros.tolist(), zsum.tolist())]
        assert np.allclose([g[0] for g in got], want, rtol=1e-15, atol=0), p
        assert [g[1] for g in got] == ['zero', 'raw', 'linear', 'linear', 'linear', 'raw', 'raw'], (p, got)
    # all-zero integers (a node outside the graph): an empty table with everything in the corner
    L = 3
    f, M, met = fref.features(np.zeros((2, L, L, 3), np.int64), np.zeros((2, 2, L, 2), np.int64), [[5, 99], [99, 5]], 50, 8, 128, symmetric=False)
    want = np.zeros((L + 1) ** 2)
    want[-1] = np.log1p(50.0)
    assert np.array_equal(f[0], want) and np.array_equal(f[1], want) and met == {'zero'} and (M == 50.0).all()
    f, _, _ = fref.features(np.zeros((1, L, L, 3), np.int64), np.zeros((1, 2, L, 2), np.int64), [[5, 99]], 50, 8, 128, symmetric=True)
    assert f[0, -1] == np.log1p(100.0) and not f[0, :-1].any()
    # the bar
    ok, worst = fref.within_bar(np.array([[1.0 + 2.0 ** -24]]), np.array([[1.0]]), [0.0])
    assert ok and worst == 0.5
    assert not fref.within_bar(np.array([[1.0 + 2.0 ** -22]]), np.array([[1.0]]), [0.0])[0]
    assert fref.within_bar(np.array([[0.0]]), np.array([[2.0 ** -40 * 1000.0]]), [1000.0])[0]


def test_the_export_is_declared_bound_and_reaches_python():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r'\bint32_t\s+gm_sketch_pair_features\s*\(\s*const\s+gm_sketch_t\s*\*\s*sk\s*,\s*const\s+int32_t\s*\*\s*d_pairs\s*,\s*int64_t\s+n\s*,\s*int32_t\s+symmetric\s*,'
                     r'\s*float\s*\*\s*d_out\s*,\s*int64_t\s+ld\s*,\s*void\s*\*\s*stream\s*\)\s*;', code)
    assert hasattr(lib, 'gm_sketch_pair_features') and len(_lib.PROTOTYPES['gm_sketch_pair_features'][1]) == 7
    assert hasattr(_lib.lib(), 'gm_sketch_pair_features')
    assert 'tests/sketch_feature_ref.py' in txt and 'log1p' in txt
    assert 'link_sketch_features' in gmeta_amd.__all__ and callable(gmeta_amd.link_sketch_features)
    assert callable(gmeta_amd.NodeSketches.pair_features) and isinstance(gmeta_amd.NodeSketches.n_columns, property)
    import inspect
    for name in ('scores', 'step', 'fit', 'link_scores', 'auc'):
        assert inspect.signature(getattr(gmeta_amd.PairPredictor, name)).parameters['sketches'].default is None
    # the host-side checks come before the library: no GPU and no sketch behind the object
    sk = object.__new__(gmeta_amd.NodeSketches)
    sk.handle, sk.n_nodes, sk.hops, sk.p, sk.k = 1, 10, 3, 8, 128
    assert sk.n_columns == 25
    with pytest.raises(ValueError, match='outside'):
        sk.pair_features([[0, 10]])
    sk.handle = None
    with pytest.raises(ValueError, match='closed'):
        sk.pair_features([[0, 1]])


def test_train_flag_chooses_where_the_columns_are_formed():
    import train as drv
    base = ['--data_dir', 'x', '--task_setup', 'Shared', '--link_pred_mode', 'True']
    assert drv.parse(base).buddy_columns == 'host' and drv.parse(base + ['--buddy', '3']).buddy_columns == 'host'
    assert drv.parse(base + ['--buddy', '3', '--buddy_columns', 'device']).buddy_columns == 'device'
    assert drv.parse(base + ['--buddy_columns', 'host']).buddy_columns == 'host'
    with pytest.raises(SystemExit, match='--buddy_columns device'):
        drv.parse(base + ['--buddy_columns', 'device'])                             # nothing to form columns for
    with pytest.raises(SystemExit):
        drv.parse(base + ['--buddy', '3', '--buddy_columns', 'gpu'])
