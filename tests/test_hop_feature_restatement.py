"""CPU (-m "not gpu"): the restatement of the hop-propagated node features (tests/hop_feature_ref.py) against a dense float64 matrix power, its derived
tolerance against plain fp32 evaluations in three row orders, and the declarations, knobs, build list and host-side checks of the feature.  No compute call of
the library: that needs a GPU (tests/test_hip_hop_features.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hop_feature_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- 1. the restatement against a dense matrix power
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('self_loops', [0, 1])
def test_restatement_equals_a_dense_matrix_power(weighted, self_loops):
    N, src, dst, w = ref.small_case()
    ptr, idx, wt = ref.csr(N, src, dst, w if weighted else None)
    indeg, outdeg = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
    assert indeg[8] == outdeg[8] == 0 and indeg[7] == 0 and outdeg[7] > 0 and (src == dst).sum() == 3 and len(set(zip(src.tolist(), dst.tolist()))) < len(src)
    X = ref.features(N, 6, 1)
    A = ref.dense_operator(ptr, idx, wt, self_loops)
    got = ref.levels(ptr, idx, wt, X, 4, self_loops)
    assert got.shape == (5, N, 6) and got.dtype == np.float64 and np.array_equal(got[0], X.astype(np.float64))
    want = X.astype(np.float64)
    for t in range(1, 5):
        want = A @ want
        assert np.allclose(got[t], want, rtol=1e-13, atol=1e-15), t
    # the isolated node: zeros without the self loop, its own row with it (d = 1, norm = 1)
    assert (not got[1:, 8].any()) if not self_loops else np.array_equal(got[3, 8], got[0, 8])
    if not self_loops:
        assert not got[1:, 7].any()                                            # out-edges only: an empty row gives zeros
    # row 1 by hand: three parallel edges from 0 and one from 3
    ws = (wt if weighted else np.ones(len(idx)))[ptr[1]:ptr[2]].astype(np.float64)
    us = idx[ptr[1]:ptr[2]]
    assert sorted(us.tolist()) == [0, 0, 0, 3]
    deg = lambda v: (wt if weighted else np.ones(len(idx)))[ptr[v]:ptr[v + 1]].astype(np.float64).sum() + self_loops      # noqa: E731
    nm = lambda v: 1.0 / np.sqrt(deg(v) if deg(v) > 0 else 1.0)      # noqa: E731
    hand = sum(wk * nm(u) * X[u].astype(np.float64) for wk, u in zip(ws, us)) + (nm(1) * X[1].astype(np.float64) if self_loops else 0.0)
    assert np.allclose(got[1, 1], nm(1) * hand, rtol=1e-13, atol=0)


@pytest.mark.parametrize('self_loops', [0, 1])
def test_integer_weights_equal_repeated_edges(self_loops):
    N, src, dst, w = ref.small_case()
    rep = w.astype(np.int64)
    assert rep.max() == 3 and (rep == w).all()
    X = ref.features(N, 4, 2)
    a = ref.levels(*ref.csr(N, src, dst, w), X, 3, self_loops)
    b = ref.levels(*ref.csr(N, np.repeat(src, rep), np.repeat(dst, rep)), X, 3, self_loops)
    assert np.allclose(a, b, rtol=1e-13, atol=1e-15) and a[3].any()


def test_extended_rows_keep_the_stored_order_with_the_self_loop_in_front():
    N, src, dst, w = ref.small_case()
    ptr, idx, wt = ref.csr(N, src, dst, w)
    _, row, col, c = ref.entries(ptr, idx, wt, 1)
    assert len(row) == len(idx) + N and (np.diff(row) >= 0).all()
    for v in range(N):
        e = np.nonzero(row == v)[0]
        assert col[e[0]] == v and c[e[0]] == 1.0 and np.array_equal(col[e[1:]], idx[ptr[v]:ptr[v + 1]]) and np.array_equal(c[e[1:]], wt[ptr[v]:ptr[v + 1]])
    _, row0, col0, c0 = ref.entries(ptr, idx, None, 0)
    assert np.array_equal(col0, idx) and (c0 == 1.0).all() and np.array_equal(np.bincount(row0, minlength=N), np.diff(ptr))


# ---------------------------------------------------------------------------------------------------- 2. the derived tolerance covers fp32 in any row order
@pytest.mark.parametrize('which', ['small', 'hub'])
def test_bound_covers_plain_fp32_in_forward_reversed_and_shuffled_order(which):
    N, src, dst, w = ref.small_case() if which == 'small' else ref.hub_case()
    hops, F = (8, 5) if which == 'small' else (3, 3)
    X = ref.features(N, F, 3)
    worst = 0.0
    for weighted in (False, True):
        for self_loops in (0, 1):
            g = ref.csr(N, src, dst, w if weighted else None)
            want, E = ref.levels(*g, X, hops, self_loops), ref.bound(*g, X, hops, self_loops)
            assert not E[0].any() and (E[1:][np.abs(want[1:]) > 0] > 0).all()
            for order in ('forward', 'reversed', 'shuffled'):
                got = ref.levels_fp32(*g, X, hops, self_loops, order)
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= E).all(), (weighted, self_loops, order)
                worst = max(worst, float((err[1:] / np.maximum(E[1:], 1e-300)).max()))
    print('worst fp32 error / bound: %.3f' % worst)
    assert 0 < worst < 1
    rel = ref.bound(*ref.csr(N, src, dst, w), X, hops, 1)[hops] / np.maximum(np.abs(ref.levels(*ref.csr(N, src, dst, w), X, hops, 1)[hops]), 1e-30)
    assert np.median(rel) < 1e-3                                               # the tolerance is tight enough to catch a wrong coefficient


def test_pair_features_are_one_fp32_operation_and_symmetric():
    a, b = ref.features(50, 7, 4), ref.features(50, 7, 5)
    for op in ref.OPS:
        ab, ba = ref.pair_features(a, b, op), ref.pair_features(b, a, op)
        assert ab.dtype == np.float32 and np.array_equal(ab.view(np.uint32), ba.view(np.uint32))
    assert np.array_equal(ref.pair_features(a, b, 'hadamard'), a * b) and np.array_equal(ref.pair_features(a, a, 'abs_diff'), np.zeros_like(a))


# ---------------------------------------------------------------------------------------------------- 3. declarations and plumbing
def test_the_exports_are_declared_bound_tunable_and_built():
    import gmeta_amd
    from gmeta_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gmeta_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r'typedef\s+struct\s+gm_prop\s+gm_prop_t\s*;', code)
    for name, n_args in (('gm_store_propagate_build', 6), ('gm_prop_dims', 6), ('gm_prop_rows', 6), ('gm_prop_pair_features', 6), ('gm_prop_destroy', 1)):
        assert re.search(r'\b(int32_t|void)\s+%s\s*\(' % name, code) and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    for macro, value in (('GM_PROP_SELF_LOOPS', 1), ('GM_PROP_HADAMARD', 0), ('GM_PROP_ABS_DIFF', 1)):
        assert re.search(r'#define\s+%s\s+%d\b' % (macro, value), code), macro
    assert (_lib.PROP_SELF_LOOPS, _lib.PROP_OPS) == (1, {'hadamard': 0, 'abs_diff': 1})
    assert 'tests/hop_feature_ref.py' in txt and 'prop_chunk' in txt and 'prop_mib' in txt
    assert hasattr(gmeta_amd.GraphStore, 'propagated_features')
    for name in ('PropagatedFeatures', 'link_propagated_features'):
        assert name in gmeta_amd.__all__ and hasattr(gmeta_amd, name)
    build = open(os.path.join(ROOT, 'g-meta_amd', 'build.py')).read()
    assert build.count("'propagate.hip'") == 1
    assert build.index("'node_sketches.hip'") < build.index("'propagate.hip'") < build.index("'pair_walks.hip'")
    assert [ln for ln in build.splitlines() if "'propagate.hip'" in ln][0].startswith("SOURCES += ['propagate.hip']")      # a line of its own
    for knob, env in ((b'prop_chunk', b'GM_PROP_CHUNK'), (b'prop_mib', b'GM_PROP_MIB')):
        for v in (7, 1, 2 ** 30, -3, 0):
            assert _lib.lib().gm_set_tuning(knob, v) == 0 and _lib.lib().gm_get_tuning(knob) == v == _lib.lib().gm_get_tuning(env)
        assert _lib.lib().gm_set_tuning(env, 40) == 0 and _lib.lib().gm_get_tuning(knob) == 40
        assert _lib.lib().gm_set_tuning(knob, 0) == 0 and _lib.lib().gm_get_tuning(env) == 0


class _HostProps:
    """PropagatedFeatures.pair_features on the restatement (host logic of link_propagated_features; no GPU)."""

    def __init__(self, N, src, dst, F, hops=2, seed=0):
        self.n_nodes, self.hops, self.feat_dim, self.calls = N, hops, F, []
        self.x = ref.levels(*ref.csr(N, src, dst), ref.features(N, F, seed), hops, 1).astype(np.float32)

    def pair_features(self, pairs, op='hadamard', as_torch=False):
        p = np.asarray(pairs).reshape(-1, 2)
        self.calls.append(len(p))
        return ref.pair_features(self.x[:, p[:, 0]], self.x[:, p[:, 1]], op).transpose(1, 0, 2)


def test_link_propagated_features_one_call_per_graph_in_name_order():
    import gmeta_amd
    rng = np.random.default_rng(3)
    graphs = [(30, rng.integers(0, 30, 40), rng.integers(0, 30, 40)), (20, rng.integers(0, 20, 25), rng.integers(0, 20, 25))]
    pr = {g: _HostProps(*graphs[g], 5, seed=g) for g in (0, 1)}
    names, want = [], {op: [] for op in ref.OPS}
    for _ in range(60):
        g = int(rng.integers(0, 2))
        a, b = rng.integers(0, graphs[g][0], 2).tolist()
        names.append('%d_%d_%d' % (g, a, b))
        for op in ref.OPS:
            want[op].append(ref.pair_features(pr[g].x[:, a], pr[g].x[:, b], op))
    for op in ref.OPS:
        got = gmeta_amd.link_propagated_features(pr, names, op=op)
        assert got.shape == (60, 3, 5) and got.dtype == np.float32 and np.array_equal(got, np.asarray(want[op]))
    assert [len(p.calls) for p in pr.values()] == [2, 2] and sum(p.calls[0] for p in pr.values()) == 60
    assert np.array_equal(gmeta_amd.link_propagated_features([pr[0], pr[1]], names), np.asarray(want['hadamard']))      # a sequence indexed by graph
    assert gmeta_amd.link_propagated_features(pr, []).shape == (0, 1, 0)
    with pytest.raises(ValueError, match='g_i_j'):
        gmeta_amd.link_propagated_features(pr, ['0_1'])
    with pytest.raises(ValueError, match="op = 'sum'"):
        gmeta_amd.link_propagated_features(pr, names, op='sum')
    pr[1].hops = 3
    with pytest.raises(ValueError, match='different hops'):
        gmeta_amd.link_propagated_features(pr, names)
    pr[1].hops, pr[1].feat_dim = 2, 6
    with pytest.raises(ValueError, match='different feat_dim'):
        gmeta_amd.link_propagated_features(pr, names)


def test_host_side_checks_come_before_the_library():
    """No GPU and no store behind the object: the checks come first."""
    import gmeta_amd
    store = object.__new__(gmeta_amd.GraphStore)
    store.handle, store.n_graphs, store.n_nodes = None, 1, [10]
    for hops, msg in ((0, r'hops = 0; 1 \.\. 8'), (9, r'hops = 9; 1 \.\. 8'), (-1, 'hops = -1')):
        with pytest.raises(ValueError, match=msg):
            store.propagated_features(0, hops=hops)
    for g in (1, -1):
        with pytest.raises(ValueError, match='graph %d' % g):
            store.propagated_features(g)
    pf = object.__new__(gmeta_amd.PropagatedFeatures)
    pf.handle, pf.n_nodes, pf.hops, pf.feat_dim, pf.self_loops = 1, 10, 2, 4, True
    with pytest.raises(ValueError, match='outside'):
        pf.pair_features([[0, 10]])
    with pytest.raises(ValueError, match='outside'):
        pf.rows([-1], 0)
    for level in (-1, 3):
        with pytest.raises(ValueError, match='level = %d' % level):
            pf.rows([1], level)
    with pytest.raises(ValueError, match="op = 'max'"):
        pf.pair_features([[0, 1]], op='max')
    pf.handle = None
    with pytest.raises(ValueError, match='closed'):
        pf.pair_features([[0, 1]])
    with pytest.raises(ValueError, match='closed'):
        pf.rows([0], 0)
    pf.close()                                                                 # closed twice: nothing to do


def test_propagate_kernels_do_not_spill():
    """The new translation unit with -Rpass-analysis=kernel-resource-usage: ScratchSize == 0 for every kernel, as test_cabi_and_host.py asks of gemm.hip and
    agg.hip."""
    csrc = os.path.join(ROOT, 'g-meta_amd', 'csrc')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-c', os.path.join(csrc, 'propagate.hip'), '-o', os.devnull,
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
    for kernel in ('k_prop_norm', 'k_prop_norm_parts', 'k_prop_norm_hubs', 'k_prop_coef', 'k_prop_levelILi1', 'k_prop_levelILi2', 'k_prop_levelILi4', 'k_prop_partsILi1',
                   'k_prop_partsILi2', 'k_prop_partsILi4', 'k_prop_hubsILi1', 'k_prop_hubsILi2', 'k_prop_hubsILi4', 'k_prop_rowsILi1', 'k_prop_rowsILi4', 'k_prop_pairsILi1',
                   'k_prop_pairsILi4'):
        assert any(kernel in n for n in seen), kernel
    assert not bad, 'kernels spilling to scratch: %s' % bad
