"""CPU: the oracle's step functions with a dtype (oracle/gmeta_oracle.py) are what tests/test_hip_step_numerics.py takes them for.

  * float32 is the default and is the oracle bit for bit; the per-task parts it reports add up to what it returns.
  * float64: the two parts of the meta-gradient equal central finite differences of the first-order objective
    L(theta) = L_q(theta + d_K ; protos(theta + d_{K-1})) with the d's frozen from the unperturbed run -- g_q against the quotient in the first
    argument, g_p against the quotient in the second -- on a node case and a link case, biases moved off the relu kink.
  * the yardstick figures: per golden case and tensor, the distance of the fp32 oracle and of the reference's own golden gradient to fp64, in u = 2^-24
    of the tensor's largest entry, next to what atol = 1e-4 allows.  Printed, so that they live in the test's output (-s shows them).
  * the scored query rows of the golden cases are decided (tests/step_bar.py) but for the near-ties counted in UNDECIDED, a property of the fixtures: accuracies
    on decided rows are compared exactly, here against the reference's own."""
import numpy as np
import pytest

import gmeta_oracle as orc
import step_bar as sb
from golden_util import CASES, NAN_CASES, Fixture

f32, f64 = np.float32, np.float64
FINITE = [c for c in CASES if c not in NAN_CASES]
_REF = {}
UNDECIDED = sb.GOLDEN_UNDECIDED      # the fixtures' near-ties, listed there


def _ref(case):
    if case not in _REF:
        fx = Fixture(case)
        _REF[case] = (fx, sb.golden_reference(fx, sequential=True))
    return _REF[case]


def _step_args(fx):
    spt, qry = sb.golden_batches(fx)
    return (fx.graphs(), fx.feats, spt, qry, fx.z['y_spt'], fx.z['y_qry'], fx.vars0, fx.config, fx.args['k_spt'], fx.args['update_lr'], fx.args['meta_lr'], fx.K)


@pytest.mark.parametrize('case', CASES)
def test_float32_is_the_oracle_bit_for_bit(case):
    """dtype=float32 given explicitly, with the per-task detail collected, returns what the plain call returns; the mean over the tasks of g_q + g_p is the
    gradient; the last entry of 'fw' is K updates away from theta."""
    fx = Fixture(case)
    a = _step_args(fx)
    det = []
    with np.errstate(all='ignore'):
        plain = orc.meta_step(*a, adam_state={})
        given = orc.meta_step(*a, adam_state={}, dtype=f32, detail=det)
    for x, y in zip([plain[0], plain[3]] + plain[1] + plain[2], [given[0], given[3]] + given[1] + given[2]):
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
    assert len(det) == fx.T and all(len(d['fw']) == fx.K + 1 and len(d['protos']) == fx.K and len(d['scored']) == fx.K + 1 for d in det)
    if case in NAN_CASES:
        return
    for i, g in enumerate(plain[1]):
        s = np.zeros_like(g)
        for d in det:
            s = s + (d['g_q'][i] + d['g_p'][i])
        assert np.array_equal((s / f32(fx.T)).astype(f32), g)
    assert all(d['fw'][0][i].dtype == f32 for d in det for i in range(len(fx.vars0)))


def test_float64_runs_on_the_widened_fp32_inputs():
    """The learning rate is float(np.float32(update_lr)) in both precisions, the fast weights start at the fp32 theta widened, and everything returned is float64."""
    fx, ref = _ref('g2_shared')
    d = ref['det64'][0]
    lr = float(f32(fx.args['update_lr']))
    assert lr != fx.args['update_lr']
    for i, v in enumerate(fx.vars0):
        assert d['fw'][0][i].dtype == f64 and np.array_equal(d['fw'][0][i], v.astype(f64))
        assert d['fw'][fx.K][i].dtype == f64 and d['g_q'][i].dtype == f64 and d['g_p'][i].dtype == f64
    # fw_1 = theta - lr * g_0 with that lr: recover g_0 from the two and compare the bias update of the head (g_0 there is a plain column sum)
    spt, _ = sb.golden_batches(fx)
    logit_s, cs = orc.classifier_forward(spt[0], spt[0].features(fx.feats), d['fw'][0], fx.config, f64)
    _, _, _, dls = orc.proto_loss_spt(logit_s, fx.z['y_spt'][0], fx.args['k_spt'], dtype=f64)
    g0 = orc.classifier_backward(spt[0], d['fw'][0], fx.config, cs, dls, f64)
    for i in range(len(fx.vars0)):
        assert np.array_equal(d['fw'][1][i], d['fw'][0][i] - lr * g0[i])


def test_reduceat_aggregate_equals_the_edge_loop():
    """The float64 aggregate (np.add.reduceat over the non-empty rows) on a CSR with empty rows at the start, in the middle and at the end, parallel edges
    and a self-loop, against the edge loop; and its transpose."""
    indptr = np.array([0, 0, 3, 3, 3, 5, 6, 6], np.int64)
    indices = np.array([1, 1, 6, 0, 4, 5], np.int64)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((7, 3))
    want = np.zeros_like(x)
    for v in range(7):
        for e in range(indptr[v], indptr[v + 1]):
            want[v] += x[indices[e]]
    assert np.array_equal(orc.agg(indptr, indices, x, f64), want)
    np.testing.assert_allclose(orc.agg(indptr, indices, x.astype(f32)), want, rtol=0, atol=1e-6)      # (the float32 path, for the same CSR)
    b = sb.RefBatch(indptr, indices, np.ones(7, f32), np.zeros((1, 1)), np.zeros((7, 1)))
    want_t = np.zeros_like(x)
    for v in range(7):
        for e in range(indptr[v], indptr[v + 1]):
            want_t[indices[e]] += x[v]
    np.testing.assert_allclose(orc.agg_t(b, x, f64), want_t, rtol=0, atol=1e-15)
    empty = orc.agg(np.zeros(4, np.int64), np.zeros(0, np.int64), x[:3], f64)
    assert empty.shape == (3, 3) and not empty.any()


def _off_the_kink(theta, rng):
    return [t if t.ndim > 1 else (rng.uniform(0.15, 0.4, size=t.shape) * rng.choice([-1.0, 1.0], size=t.shape)).astype(f32) for t in theta]


@pytest.mark.parametrize('case', ['g2_shared', 'g3_linkpred'])
def test_float64_gradient_parts_against_finite_differences(case):
    """Central differences with eps = 1e-6 in fp64, as tests/test_head_ref.py takes them: the rounding error of a quotient is 2^-53 |L| / eps ~ 1e-10 |L|
    and the truncation error eps^2 |L'''| / 6 ~ 1e-12, so rtol 1e-6 with atol 1e-8 holds every entry that is not itself noise."""
    fx = Fixture(case)
    rng = np.random.default_rng(5)
    theta = _off_the_kink(fx.vars0, rng)
    spt, qry = sb.golden_batches(fx)
    K, k_spt, cfg = fx.K, fx.args['k_spt'], fx.config
    eps = 1e-6
    checked = 0
    for t in range(fx.T):
        xs, xq, ys, yq = spt[t].features(fx.feats), qry[t].features(fx.feats), fx.z['y_spt'][t], fx.z['y_qry'][t]
        det = {}
        lq, _, mg = orc.task_inner_loop(spt[t], qry[t], xs, xq, ys, yq, theta, cfg, k_spt, fx.args['update_lr'], K, True, dtype=f64, detail=det)
        th = [v.astype(f64) for v in theta]
        dK = [a - b for a, b in zip(det['fw'][K], th)]
        dK1 = [a - b for a, b in zip(det['fw'][K - 1], th)]

        def objective(th_q, th_p):
            ls, _ = orc.classifier_forward(spt[t], xs, [a + b for a, b in zip(th_p, dK1)], cfg, f64)
            _, _, protos, _ = orc.proto_loss_spt(ls, ys, k_spt, need_grad=False, dtype=f64)
            z, _ = orc.classifier_forward(qry[t], xq, [a + b for a, b in zip(th_q, dK)], cfg, f64)
            return float(orc.proto_loss_qry(z, yq, protos, dtype=f64)[0])

        assert objective(th, th) == float(lq[K])
        for i, v in enumerate(th):
            flat = rng.choice(v.size, size=min(12, v.size), replace=False)
            for f in flat:
                idx = tuple(int(a) for a in np.unravel_index(f, v.shape))
                for part, name in ((0, 'g_q'), (1, 'g_p')):
                    up = [a.copy() for a in th]; dn = [a.copy() for a in th]
                    up[i][idx] += eps; dn[i][idx] -= eps
                    fd = ((objective(up, th) - objective(dn, th)) if part == 0 else (objective(th, up) - objective(th, dn))) / (2 * eps)
                    np.testing.assert_allclose(det[name][i][idx], fd, rtol=1e-6, atol=1e-8, err_msg='%s task %d tensor %d %s' % (name, t, i, idx))
                    checked += 1
        for i in range(len(th)):
            assert np.array_equal(mg[i], det['g_q'][i] + det['g_p'][i])
        assert max(np.abs(g).max() for g in det['g_p'][:-1]) > 1e-6 and max(np.abs(g).max() for g in det['g_q'][:-1]) > 1e-6
    assert checked > 100


def test_yardstick_figures_of_the_golden_cases():
    """Per case and tensor: max|g32 - g64| / max|g64| in u for the fp32 oracle and the reference's golden gradient, and what atol = 1e-4 allows; the query
    losses the same way; 'sequential' is the fp32 oracle with its products as fmaf chains (orc.sequential_products).  The head bias (last tensor, mathematically zero) is measured against u/2 * sum|dlogits| instead (tests/step_bar.py)."""
    print()
    print('%-16s %-10s %12s %12s %14s %14s' % ('case', 'tensor', 'oracle32 [u]', 'golden [u]', 'sequential [u]', 'atol 1e-4 [u]'))
    for case in FINITE:
        fx, ref = _ref(case)
        n = len(fx.vars0)
        for i in range(n):
            R, others, floor = ref['q']['grad/%d' % i]
            _, scale = sb.yardstick(R, others, floor)
            unit = sb.U * scale
            errs = [float(np.abs(np.asarray(o, f64) - R).max()) / unit for o in others]
            assert np.isfinite(errs).all() and len(errs) == 3      # the fp32 oracle, the reference's golden gradient, the oracle with fmaf-chain products
            print('%-16s %-10s %12.2f %12.2f %14.2f %14.0f' % (case, 'grad/%d' % i + ('*' if i == n - 1 else ''), errs[0], errs[1], errs[2], 1e-4 / unit))
        R, others, _ = ref['q']['losses_q']
        unit = sb.U * float(np.abs(R).max())
        print('%-16s %-10s %12.2f %12s %14.2f %14.0f' % (case, 'losses_q', float(np.abs(others[0] - R).max()) / unit, '-', float(np.abs(others[1] - R).max()) / unit,
                                                         1e-4 / unit))
        gold = float(np.abs(fx.z['loss_q'].mean(0) - R).max()) / unit
        assert gold < 1e-4 / unit


@pytest.mark.parametrize('case', FINITE)
def test_scored_rows_of_the_golden_cases_are_decided(case):
    """Zero undecided rows but for the pinned near-ties of the fixtures; on the decided rows the fp64 accuracies are the reference's own."""
    fx, ref = _ref(case)
    rows = fx.z['qry_seeds'].shape[1]
    assert ref['rows_total'] == fx.T * (fx.K + 1) * rows
    assert ref['undecided_total'] == UNDECIDED.get(case, 0)
    for k in range(fx.K + 1):
        ok, und = sum(per_k[k][0] for per_k in ref['accs']), sum(per_k[k][1] for per_k in ref['accs'])
        sb.check_counts((ok, und, fx.T * rows), float(fx.z['accs'][k]), (case, k))
