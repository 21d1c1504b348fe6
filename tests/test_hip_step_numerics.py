"""GPU (-m gpu): the whole meta-step -- gm_meta_step, gm_meta_adapt, gm_proto_predict -- against the oracle's statement of the same step in fp64, per tensor, at
every class of schedule whose sums run in an order of their own.

What is compared (tests/step_bar.py): the meta-gradient that reaches Adam (p.grad after Meta.forward, the mean over the tasks) per parameter tensor;
losses_q[0..K]; the per-task accuracies [T, K+1] of the step's output block; per task and tensor the fast weights fw_K and the prototypes of step K-1 from
Meta.adapt with K = update_step; the query logits and predictions of predict(..., logits=True).

THE BAR is a yardstick, never the kernel: for a tensor X with fp64 reference R and err(A) = max|A - R|, Y = max(err(oracle at float32), u/2 max|R|), u = 2^-24
-- on the golden fixtures also err(the reference's own golden gradient) -- and the device passes when err(device) <= 4 Y.  4 is the project's factor for nonlinear
quantities (test_hip_head_numerics.py, test_hip_ragged.py) and is above the 2.5x by which the two fp32 implementations differ from each other
(tests/test_step_ref.py prints those figures).  The split-bf16 GEMM gets no allowance of its own (test_hip_gemm_numerics.py holds it to the fp32 kernels'
accuracy).  On ONE path, golden g7_wide_h2 (FMAF_CHAIN_CASES), which k_gemm_nn and k_wgrad serve (asserted), the fp32 oracle with its matrix products accumulated
term by term as an fmaf chain -- those kernels' arithmetic (csrc/gemm.hip), bounded per kernel by test_hip_gemm_numerics.py / test_hip_gemm_epilogue.py /
test_hip_wgrad_numerics.py -- is one more fp32 implementation in Y (orc.sequential_products); every other path has numpy's order alone.  A bias gradient's scale is
never below what it sums (tests/step_bar.py).  g1_sampled_h2 is the ill-conditioned fixture of DESIGN.md section 3: a relu' there hangs on rounding noise, the fp32
implementations themselves miss fp64 by ~4 % of grad/3, and its lines measure nothing.
The head bias's gradient is mathematically zero and is compared absolutely, with the floor u/2 sum|dlogits| of the fp64 reference (its fast weight likewise,
tests/step_bar.py).  losses_q is held as a vector by the same rule.  Every line -- error in u, yardstick in u, ratio -- is printed, and written to the file GMETA_STEP_FP64_OUT names
(profiles/step_fp64.txt is such a run).

DECIDED ROWS.  Accuracies and predictions must equal the fp64 reference's exactly on decided rows: a scored row is decided when the fp64 gap between its two best
log-probabilities exceeds 2^-10 max_c dist(q, c) -- a condition on the inputs, not a tolerance -- and 4u max_c|logp_c|, the spacing of the fp32 log-probabilities
whose argmax everybody takes (tests/step_bar.py).  Undecided rows are left out on both sides; they are at most 1 row in 50 of a synthetic world (asserted), and
the pinned near-ties of the golden fixtures (tests/test_step_ref.py).

INPUTS.  The reference reads what the kernels read: the batch's CSR, centre rows, norms and gathered feature rows from the device batch (extraction is held bit-exact
by test_hip_parity.py / test_hip_fuzz.py), theta widened, update_lr as float(np.float32(update_lr)).  In the synthetic worlds the biases are moved off the relu
kink as test_hip_fuzz.py does: with zero biases a centre without in-edges sits on the kink and fp noise in a mathematically zero bias gradient decides relu' in the
next inner step -- then fp32 and fp64 differ by a whole unit's gradient and no bar means anything.

SCHEDULE CLASSES, one representative each (variants that other tests prove bitwise equal to one of these are not repeated):
  golden x {(hoist_z1, sparse_bwd, cone)}   tiny batches on the generic kernels; the five schedules of test_hip_parity.py: the hoist reassociates layer 1, the
                                            row-sparse backward and the cone schedule sum over other row sets in another order
  golden, first task alone (T = 1)          the per-task gradient: a cross-task mix-up cannot cancel in the mean
  undirected / directed, default knobs      split-bf16 GEMMs and weight gradients, fused aggregate + GEMM, restricted plans (GM_DEAD_ROWS 4, GM_FUSE_DIFF 2)
  GM_FUSE_DIFF 0 / 1 / 2                    the differentiated passes unfused / fused: test_hip_pass_plan.py compares nothing across these values
  GM_AGG_STREAM 0 / 1 (MIN_ROWS 0)          window kernel everywhere / the LDS-DMA stream kernel on the full launches: another order inside a row sum
  serialize = 1                             one queue: the same kernels, held here because the two-stream schedule is what the last rewrites touched
  GM_DEAD_ROWS 0                            every row formed and stored (levels 1-4 are bitwise its equal, test_hip_pass_plan.py): the unrestricted launches
  GM_GEMM_MODE f32                          the exact-fp32 MFMA kernels at full size (the one other knob that changes how a stored sum is
                                            formed; GM_HEAD_THREADS / GM_HEAD_STAGE keep one association -- test_hip_head_numerics.py holds every such launch
                                            bitwise equal to the default's; every other knob of section 9 and of the table in section 4.3 -- GM_CENTRE_STORE,
                                            GM_DEAD_TILES, GM_AGG_OBS_LIST, GM_AGG_MID_LIST / _WIN, GM_FUSE_AGG, GM_QUERY_STREAMS -- is documented and tested bitwise)
  undirected, T = 1                         the first task alone on the forced split kernels
  three layers / multiply-first layer       [128, 256, 256, 256] and [128, 256, 128] on the undirected world
  link prediction                           two centres per subgraph (the world of test_hip_dead_rows_diff.py)
Three-piece kernels only: the opt-in two-piece fp16 path has its own bound machinery.

WHAT THE SEQUENTIAL ORDER IS FOR.  With numpy's blocked products alone in the yardstick, g7_wide_h2 (hidden 128, K = 3) exceeded the bar: task 0's prototypes of step
K-1 at 9.6 u against 1.1 u.  Measured on the device: the forward pass alone is at 4.2 u (an fp64 forward at the device's own fast weights), the rest is inherited through
the inner steps; with the split-bf16 GEMM forced onto the same case the chain ends at 4.2 u; the head kernel's launch shape changes nothing.  So the figure follows
k_gemm_nn, whose products are fmaf chains over K -- an order the per-kernel tests already bound -- and the oracle run with that chain (orc.sequential_products) itself
ends at 5.4 u on the same inputs, its bias fast weights at 7.5 / 11.6 u next to the device's 8.5 / 9.5 u."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import step_bar as sb
from golden_util import CASES, NAN_CASES, Fixture
from test_hip_dead_rows_diff import link_world      # noqa: F401  (a module fixture: the link-prediction world)
from test_hip_dead_rows_fwd import _meta, _need_split, _world, tuning

pytestmark = pytest.mark.gpu
FINITE = [c for c in CASES if c not in NAN_CASES]
SCHEDULES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)]
# The one path whose yardstick takes the fmaf-chain order of k_gemm_nn / k_wgrad (orc.sequential_products) beside numpy's: with numpy's order alone its task 0's
# prototypes of step K-1 stood at 9.59 u against 1.10 u (ratio 8.7), and the figure follows k_gemm_nn (module docstring).  Per-kernel bars of that order:
# test_hip_gemm_numerics.py / test_hip_gemm_epilogue.py / test_hip_wgrad_numerics.py, (C_DET + LAMBDA sqrt(K)) u sum|products| and K 2^-24.
FMAF_CHAIN_CASES = ('g7_wide_h2',)
_GOLDEN = {}


HEADER = """# The whole meta-step against fp64 (tests/test_hip_step_numerics.py): per launch path and tensor, the device's error and the fp32 yardstick in
# u = 2^-24 of the tensor's scale (its largest entry; for a bias gradient never less than what it sums), and their ratio.  The bar is 4.
# Optional summation order: the lines 'golden g7_wide_h2 ...' (all five schedules and T=1) carry in their yardstick the fp32 oracle with its products as fmaf
# chains over K, the arithmetic of k_gemm_nn / k_wgrad, which serve that case -- with numpy's blocked order alone its prototypes of step K-1 stood at 9.6 u
# against 1.1 u.  Every other line has numpy's order alone (and, on the goldens, the reference's own gradient).
# Ill-conditioned, not a measure of anything: g1_sampled_h2 grad/3 (and what it feeds).  Its layer-2 bias gradient is zero in exact arithmetic and the sign of
# its rounding noise decides a relu' in the next inner step (DESIGN.md section 3), so the fp32 implementations themselves miss fp64 by ~4 % of the tensor there.
# g8_wide_scales (feature scales 2^-20 .. 2^4) has yardsticks of 40 - 180 u.
"""


def _finish(rep):
    out = os.environ.get('GMETA_STEP_FP64_OUT')
    if out:
        new = not os.path.exists(out) or os.path.getsize(out) == 0
        with open(out, 'a') as f:
            f.write((HEADER if new else '') + rep.text() + '\n')
    rep.assert_ok()


# ---------------------------------------------------------------------------------------------------------------- 1. golden fixtures
def _golden(case, one_task=False):
    """The fixture's device batches (the reference's node lists replayed) and its fp64 reference on them, built once."""
    key = (case, one_task)
    if key not in _GOLDEN:
        import gmeta_amd
        import hip_util
        fx = Fixture(case)
        store = hip_util.make_store(fx)
        if one_task:
            mk = lambda tag: gmeta_amd.SubgraphBatch.from_nodes(store, fx.z[tag + '_seeds'][0], [0, fx.z[tag + '_seeds'].shape[1]],      # noqa: E731
                                                                fx.replay_lists(tag, 0), fx.link)
            S, Q = mk('spt'), mk('qry')
            ys, yq = [fx.z['y_spt'][0]], [fx.z['y_qry'][0]]
            ref = sb.reference(sb.device_sets(S, fx.feats), sb.device_sets(Q, fx.feats), ys, yq, fx.vars0, fx.config, fx.args['k_spt'], fx.args['update_lr'], fx.K,
                               sequential=case in FMAF_CHAIN_CASES)
        else:
            S, Q = hip_util.fixture_batches(fx, store, True)
            ys, yq = list(fx.z['y_spt']), list(fx.z['y_qry'])
            ref = sb.golden_reference(fx, sb.device_sets(S, fx.feats), sb.device_sets(Q, fx.feats), sequential=case in FMAF_CHAIN_CASES)
            # the fixtures' near-ties, on the device's batches too (g8_wide_scales: whether fp32 log-probabilities tie hangs on the last bit of the norms,
            # which the device and the oracle round differently: there a cap at half the rows instead of the CPU test's count)
            if case == 'g8_wide_scales':
                assert ref['undecided_total'] <= ref['rows_total'] // 2, ref['undecided_total']
            else:
                assert ref['undecided_total'] == sb.GOLDEN_UNDECIDED.get(case, 0), ref['undecided_total']
        tt = lambda ys_: [torch.from_numpy(y.astype(np.int64)) for y in ys_]      # noqa: E731
        _GOLDEN[key] = dict(fx=fx, store=store, S=S, Q=Q, ref=ref, batch=(S.views(), tt(ys), Q.views(), tt(yq)))
    return _GOLDEN[key]


def _golden_run(g, hoist, sparse, cone):
    import hip_util
    fx = g['fx']
    m = hip_util.fixture_meta(fx)
    m.hoist_z1, m.sparse_bwd, m.cone = hoist, sparse, cone
    dev = sb.run_device(m, g['batch'], fx.K, fx.feats)
    n = dev['launches']
    assert n[4] == 0 and n[5] == 0 and n[6] == 0 and n[7] == 0 and n[1] > 0, n      # the exact-fp32 kernels (k_gemm_nn; k_wgrad) served every launch, the split kernels none
    return dev


@pytest.mark.parametrize('case', FINITE)
@pytest.mark.parametrize('hoist,sparse,cone', SCHEDULES)
def test_golden_step_at_every_flagged_schedule(case, hoist, sparse, cone):
    g = _golden(case)
    dev = _golden_run(g, hoist, sparse, cone)
    rep = sb.Report()
    sb.hold_all(rep, 'golden %s h%d s%d c%d' % (case, hoist, sparse, cone), g['ref'], g['fx'].vars0, dev)
    _finish(rep)


@pytest.mark.parametrize('case', ['g1_h3', 'g3_linkpred', 'g7_wide_h2'])
def test_golden_first_task_alone(case):
    g = _golden(case, one_task=True)
    rep = sb.Report()
    for hoist, sparse, cone in ((0, 0, 0), (0, 0, 1)):
        dev = _golden_run(g, hoist, sparse, cone)
        sb.hold_all(rep, 'golden %s T=1 h%d s%d c%d' % (case, hoist, sparse, cone), g['ref'], g['fx'].vars0, dev)
    _finish(rep)


# ---------------------------------------------------------------------------------------------------------------- 2. - 4. the synthetic worlds
@pytest.fixture(scope='module')
def undirected():
    return _world(True)


@pytest.fixture(scope='module')
def directed():
    return _world(False)


@pytest.fixture(params=['undirected', 'directed'])
def world(request):
    return request.getfixturevalue(request.param)


def _theta(w, config):
    """The model _meta builds (same seed every time) with every bias moved off the relu kink; host arrays in Classifier.vars order."""
    m = _meta(w, config)
    rng = np.random.default_rng(7)
    out = []
    for p in m.net.parameters():
        t = p.detach().cpu().numpy().copy()
        if t.ndim == 1:
            t = (rng.uniform(0.15, 0.4, size=t.shape) * rng.choice([-1.0, 1.0], size=t.shape)).astype(np.float32)
        out.append(t)
    return out


def _labels(ys):
    return [np.asarray(y).reshape(-1) for y in ys]


def _reference(w, name, config, batch_key='batch'):
    """The fp64 reference (and fp32 yardstick) of a world's step for one model, computed once and left unchanged."""
    refs = w.setdefault('step_refs', {})
    key = (name, batch_key)
    if key not in refs:
        b = w[batch_key]
        S, Q = b[0][0].view_of, b[2][0].view_of
        theta = _theta(w, config)
        a = w['args']
        ref = sb.reference(sb.device_sets(S), sb.device_sets(Q), _labels(b[1]), _labels(b[3]), theta, config or _default_config(w), a.k_spt, a.update_lr, a.update_step)
        assert ref['undecided_total'] <= sb.MAX_UNDECIDED * ref['rows_total'], (ref['undecided_total'], ref['rows_total'])
        refs[key] = (theta, ref)
    return refs[key]


def _default_config(w):
    from gmeta_amd import synth
    cfg = w['cfg']
    return w.get('config') or synth.make_config(cfg['F0'], cfg['hidden'], cfg['h'], cfg['n_way'])


def _world_run(w, theta, config, batch_key='batch', gemm_mode=None, knobs=None, **attrs):
    from gmeta_amd import _lib
    lib = _lib.lib()
    prev = lib.gm_get_gemm_mode()
    with tuning(**dict(w['force'], **(knobs or {}))):
        if gemm_mode is not None:
            lib.gm_set_gemm_mode(gemm_mode)
        try:
            m = _meta(w, config, **attrs)
            with torch.no_grad():
                for p, v in zip(m.net.parameters(), theta):
                    p.copy_(torch.from_numpy(v))
            return sb.run_device(m, w[batch_key], w['args'].update_step)
        finally:
            lib.gm_set_gemm_mode(prev)


def _stream_segments(w):
    """stream row segments over both batches and orientations (gm_dense_agg_info: 0 until a batch's first stream-eligible launch built its tables)"""
    from gmeta_amd import _lib
    n = 0
    for B in (w['S'], w['Q']):
        for tr in (0, 1):
            info = (C.c_int64 * 16)()
            _lib.check(_lib.lib().gm_dense_agg_info(B.handle, tr, info), 'gm_dense_agg_info')
            n += int(info[9])
    return n


PATHS = {
    'default': dict(),
    'fuse_diff0': dict(knobs=dict(GM_FUSE_DIFF=0)),
    'fuse_diff1': dict(knobs=dict(GM_FUSE_DIFF=1)),
    'fuse_diff2': dict(knobs=dict(GM_FUSE_DIFF=2)),
    'agg_stream0': dict(knobs=dict(GM_AGG_STREAM=0, GM_AGG_STREAM_MIN_ROWS=0)),
    'agg_stream1': dict(knobs=dict(GM_AGG_STREAM=1, GM_AGG_STREAM_MIN_ROWS=0)),
    'serialize': dict(serialize=1),
    'dead_rows0': dict(knobs=dict(GM_DEAD_ROWS=0)),
    'gemm_f32': dict(gemm_mode=0),
}


def _fresh_stream_world(w, name):
    """A batch decides whether it gets stream tables at its first stream-eligible launch (gm_agg_stream_args), with the GM_AGG_STREAM_MIN_ROWS in force
    then -- so the stream path needs batches whose first launch happens under MIN_ROWS = 0: the same world built again (same seeds: the same batches, checked)."""
    w2 = _world(name == 'undirected')
    for k in ('S', 'Q'):
        assert np.array_equal(w2[k].parent(), w[k].parent()) and np.array_equal(w2[k].csr()[1], w[k].csr()[1])
    return w2


@pytest.mark.parametrize('path', list(PATHS))
def test_world_step_at_every_launch_path(world, path, request):
    _need_split(world, world['S'], world['Q'])
    name = request.node.callspec.params['world']
    theta, ref = _reference(world, 'default', None)
    run_on = world
    if path == 'agg_stream1':
        for B in (world['S'], world['Q']):
            assert 0 < B.edges <= 8 * B.rows, (B.edges, B.rows)       # stream-eligible (gm_stream_batch_ok): a world that is not does not cover this class
        with tuning(GM_AGG_STREAM=1, GM_AGG_STREAM_MIN_ROWS=0):
            run_on = _fresh_stream_world(world, name)
    if 'acct_default' not in world:
        d0 = _world_run(world, theta, None)
        world['acct_default'] = (d0['launches'][0], d0['work'][0])
    dev = _world_run(run_on, theta, None, **PATHS[path])
    n = dev['launches']
    assert n[6] == 0 and n[7] == 0                                    # never the two-piece kernels
    if path == 'gemm_f32':
        assert n[4] == 0 and n[5] == 0 and n[1] > 0 and n[2] > 0      # the exact-fp32 MFMA kernels took every launch
    else:
        assert n[4] > 0 and n[5] > 0, n                               # the split-bf16 GEMMs and weight gradients really ran
    assert n[0] > 0
    # what the knob did to the aggregate launches (category 0: count, algorithmic bytes) against the default run of the same world
    acct, acct0 = (n[0], dev['work'][0]), world['acct_default']
    if path == 'fuse_diff0':
        assert acct != acct0 and acct[1] > acct0[1], (acct, acct0)   # the differentiated passes write and re-read Z: full aggregate launches, more bytes
    elif path == 'dead_rows0':
        assert acct[1] > acct0[1], (acct, acct0)                      # every row formed and stored
    elif path == 'agg_stream1':
        # the support batch has stream tables, so under GM_FUSE_DIFF=2 its differentiated passes leave the fused path for FULL aggregate launches -- the
        # launches gm_stream_ok hands to k_agg_stream (the step reports no kernel ids; tests/test_hip_agg_numerics.py asserts them per launch)
        assert _stream_segments(run_on) > 0
        assert acct != acct0 and acct[1] > acct0[1], (acct, acct0)
    elif path in ('default', 'fuse_diff1', 'fuse_diff2', 'agg_stream0'):
        # on these worlds (no stream tables: fewer rows than GM_AGG_STREAM_MIN_ROWS) GM_FUSE_DIFF 1 and 2 plan the same launches, 2 is the default, and
        # GM_AGG_STREAM=0 takes away a kernel nobody had: the same launches as the default run, held here so that a change of that is seen
        assert acct == acct0, (acct, acct0)
    # serialize: the same kernels on one queue; gemm_f32: the GEMM categories above.  The accounting has no field for the queue.
    rep = sb.Report()
    sb.hold_all(rep, '%s %s' % (name, path), ref, theta, dev)
    _finish(rep)


def test_world_first_task_alone(undirected):
    """T = 1 on the forced split kernels: the per-task gradient, where no other task's share can cancel a mix-up."""
    w = undirected
    theta, ref = _reference(w, 'default', None, 'one')
    dev = _world_run(w, theta, None, 'one', knobs=dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0))
    assert ref['T'] == 1 and dev['launches'][4] > 0 and dev['launches'][5] > 0
    rep = sb.Report()
    sb.hold_all(rep, 'undirected T=1', ref, theta, dev)
    _finish(rep)


@pytest.mark.parametrize('dims', [[128, 256, 256, 256], [128, 256, 128]])
def test_model_variants(undirected, dims):
    """Three GraphConv layers, and a multiply-first last layer (in > out), at default knobs."""
    w = undirected
    _need_split(w, w['S'], w['Q'])
    assert dims[0] == w['cfg']['F0']
    config = [('GraphConv', [dims[l], dims[l + 1]]) for l in range(len(dims) - 1)] + [('Linear', [dims[-1], w['cfg']['n_way']])]
    name = 'x'.join(str(d) for d in dims)
    theta, ref = _reference(w, name, config)
    dev = _world_run(w, theta, config)
    assert dev['launches'][4] > 0 and dev['launches'][5] > 0
    rep = sb.Report()
    sb.hold_all(rep, 'undirected %s' % name, ref, theta, dev)
    _finish(rep)


def test_link_prediction(link_world):      # noqa: F811
    w = link_world
    assert w['S'].centres == 2 and w['Q'].centres == 2
    theta, ref = _reference(w, 'default', w['config'])
    dev = _world_run(w, theta, w['config'])
    assert dev['launches'][4] > 0 and dev['launches'][5] > 0
    rep = sb.Report()
    sb.hold_all(rep, 'link default', ref, theta, dev)
    _finish(rep)
