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
The flagged schedules at world size (section 5 of this file; multi-tile, multi-chunk launches).  Each path first shows from the launch accounting, against the
dense run of the same model and batch, that the flag's own chain ran -- sparse_bwd_ok and make_ctx fall back to the dense schedule without a word -- and which
kernel families served it (categories of gm_profile_read: 1 / 2 exact-fp32 GEMM / weight gradient, 4 / 5 split-bf16 GEMM / weight gradient).  The counts of one
step and the byte ratios below are a RECORD of the run behind profiles/step_fp64.txt, printed again by every run (_hold_flagged) and not asserted: what is asserted
is the inequality or the family named beside them, and a scheduling change may move the figures without failing anything:
  undirected / directed, hoist_z1           Z_1 of a batch from one full aggregate launch, layer 1 on the ungathered split GEMM: 11 aggregate launches for the
                                            default's 14; split GEMMs (14) and split weight gradients (8)
  ... hoist_z1, GM_AGG_STREAM 1 (MIN_ROWS 0) the same on batches with stream tables: the hoisted Z_1 from k_agg_stream (stream segments asserted)
  ... sparse_bwd                            gcn_backward_sparse behind PASS_PLAIN forwards: k_expand_edges, sparse_wgrad with a_row on k_wgrad (8), the transB GEMM
                                            over the centre tiles on the exact-fp32 kernel (4), split GEMMs forward (10); 10 aggregate launches, the weight
                                            gradients' accounted bytes about 1/34 (undirected) and 1/9 (directed) of the default's
  ... cone, cone + hoist_z1                 cone_forward / cone_backward on the level tables of cone.hip (gm_batch_cone_dims ok = 1 on both batches, asserted before
                                            the run): every GEMM exact-fp32 (14, none split), aggregate bytes priced on level rows; weight gradients on k_wgrad
                                            (undirected, 8) or the split kernel (directed, whose fixture forces it, and undirected with
                                            GM_WGRAD_SPLIT_MIN_CHUNKS = 0: 8); with the hoist 11 aggregate launches for cone's 14
  undirected, T = 1, cone                   a level's set_off / set_chunk_off with nothing to cancel a per-set mix-up
  three layers / multiply-first, cone       four levels (23 GEMMs, 12 weight gradients); [128, 256, 128]: k_colsum_rows, the source-level GEMM and the aggregate
                                            behind it.  sparse_bwd = 1 on these two models falls back to the dense backward: pinned bitwise (results and launch
                                            accounting) to the default run, not a class
  link prediction, sparse_bwd / cone / cone + hoist_z1   two centres per subgraph, ok = 1 on both batches; under cone both weight-gradient families (4 + 4)
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
from test_hip_dead_rows_fwd import _bits, _meta, _need_split, _world, tuning

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
# Flagged schedules on the worlds ('... hoist_z1', '... sparse_bwd', '... cone', '... cone+hoist_z1', 'link ...'): against the reference of the dense paths (the
# oracle has no schedule); each of these runs showed from its launch accounting that the flag's own chain ran.  Under cone every GEMM is on the exact-fp32 kernels.
# 'directed agg_stream1' and 'directed hoist_z1 agg_stream1' equal 'directed default' and 'directed hoist_z1' digit for digit: those batches have stream tables, but
# no row sum of theirs comes out in another association -- only the undirected blocks measure the stream kernel's order.
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


def _default_dev(w, theta, config=None, name='default', batch_key='batch'):
    """The dense schedule's run of one model on one batch of a world at default knobs, made once and kept: what a flagged run's launch accounting is compared
    with, and what a flag that must fall back to the dense schedule has to reproduce bit for bit.  `name` names `config` (callers pass the pair _variant
    returns, or the world's own model as 'default').  The kept result is shared between tests and is read only: nobody writes into its arrays or dicts."""
    devs = w.setdefault('dev_default', {})
    key = (name, batch_key)
    if key not in devs:
        devs[key] = _world_run(w, theta, config, batch_key)
        if key == ('default', 'batch'):
            w['acct_default'] = (devs[key]['launches'][0], devs[key]['work'][0])
    return devs[key]


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
    _default_dev(world, theta)
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


VARIANTS = [[128, 256, 256, 256], [128, 256, 128]]


def _variant(w, dims):
    assert dims[0] == w['cfg']['F0']
    config = [('GraphConv', [dims[l], dims[l + 1]]) for l in range(len(dims) - 1)] + [('Linear', [dims[-1], w['cfg']['n_way']])]
    return 'x'.join(str(d) for d in dims), config


@pytest.mark.parametrize('dims', VARIANTS)
def test_model_variants(undirected, dims):
    """Three GraphConv layers, and a multiply-first last layer (in > out), at default knobs."""
    w = undirected
    _need_split(w, w['S'], w['Q'])
    name, config = _variant(w, dims)
    theta, ref = _reference(w, name, config)
    dev = _default_dev(w, theta, config, name)
    assert dev['launches'][4] > 0 and dev['launches'][5] > 0
    rep = sb.Report()
    sb.hold_all(rep, 'undirected %s' % name, ref, theta, dev)
    _finish(rep)


def test_link_prediction(link_world):      # noqa: F811
    w = link_world
    assert w['S'].centres == 2 and w['Q'].centres == 2
    theta, ref = _reference(w, 'default', w['config'])
    dev = _default_dev(w, theta, w['config'])
    assert dev['launches'][4] > 0 and dev['launches'][5] > 0
    rep = sb.Report()
    sb.hold_all(rep, 'link default', ref, theta, dev)
    _finish(rep)


# ---------------------------------------------------------------------------------------------------------------- 5. the flagged schedules at world size
# hoist_z1, sparse_bwd and cone run host chains and kernels of their own (cone_forward / cone_backward, gcn_backward_sparse, the hoisted full aggregate launch), and
# each of them can fall back to the dense schedule without a word: sparse_bwd_ok refuses three layers and a multiply-first layer, make_ctx drops cone when
# gm_batch_cone reports ok = 0, and the step drops it for both batches when either dropped it.  So no path below passes on numbers alone: each first shows from
# the launch accounting (launches / algorithmic bytes per category, against the dense run of the same model, batch and knobs' defaults) that the flag changed what ran.
FLAGGED = {
    'hoist_z1': dict(hoist_z1=1),
    'sparse_bwd': dict(sparse_bwd=1),
    'cone': dict(cone=1),
    'cone_hoist_z1': dict(cone=1, hoist_z1=1),
}
WGRAD_BYTES = 14      # launch-accounting category (test_hip_dead_rows_diff.py): the A and G rows of every weight-gradient launch


def _n_gcn(w, config):
    return sum(1 for kind, _ in (config or _default_config(w)) if kind == 'GraphConv')


def _assert_cone_tables(w, config, batch_key):
    """gm_batch_cone's verdict on both batches, before the run: with ok = 0 on either (a self pair among the centres) the step runs the dense schedule."""
    from gmeta_amd import _lib
    lib = _lib.lib()
    L = _n_gcn(w, config)
    b = w[batch_key]
    for B in (b[0][0].view_of, b[2][0].view_of):
        _lib.check(lib.gm_batch_prepare_cone(B.handle, L, None), 'prepare_cone')
        ok = C.c_int32(); nrows = (C.c_int64 * (L + 1))(); nedges = (C.c_int64 * (L + 1))()
        _lib.check(lib.gm_batch_cone_dims(B.handle, L, C.byref(ok), nrows, nedges), 'cone_dims')
        assert ok.value == 1, 'no cone tables on this batch: cone = 1 would run the dense schedule'
        assert nrows[L] == B.subs * B.centres and 0 < nrows[0] <= B.rows, (list(nrows), B.rows)


def _flag_dev(w, theta, config, name, batch_key, flag):
    """A flagged run at default knobs, kept (cone + hoist_z1 is compared with cone alone); read only, like _default_dev's."""
    devs = w.setdefault('dev_flagged', {})
    key = (name, batch_key, flag)
    if key not in devs:
        devs[key] = _world_run(w, theta, config, batch_key, **FLAGGED[flag])
    return devs[key]


def _hold_flagged(w, label, flag, theta, ref, config=None, name='default', batch_key='batch', knobs=None, run_on=None, dense=None):
    """One flagged schedule of one model on one batch: the launch accounting shows that the flag's own chain ran, then every tensor is held to the bar.
    dense: the run without the flag that the accounting is compared with, where that is not the default-knob run (a run under the same `knobs`)."""
    on = run_on or w
    cone = 'cone' in FLAGGED[flag]
    if cone:
        _assert_cone_tables(on, config, batch_key)
    dev0 = dense or _default_dev(w, theta, config, name, batch_key)
    dev = _world_run(on, theta, config, batch_key, knobs=knobs, **FLAGGED[flag]) if (knobs or run_on) else _flag_dev(w, theta, config, name, batch_key, flag)
    n, wk, n0, wk0 = dev['launches'], dev['work'], dev0['launches'], dev0['work']
    print('%s: launches %s bytes(0) %d bytes(14) %d; dense: launches %s bytes(0) %d bytes(14) %d' % (label, n, wk[0], wk[WGRAD_BYTES], n0, wk0[0], wk0[WGRAD_BYTES]))
    assert n[6] == 0 and n[7] == 0                                                # never the two-piece kernels
    assert n[0] > 0 and n[2] + n[5] > 0
    if cone:
        assert 0 < wk[0] < wk0[0], (wk[0], wk0[0])                                # priced on level rows (cone_agg_bytes)
        assert n[4] == 0 and n[1] > 0, n                                          # no split weights under cone: every GEMM on the exact-fp32 kernels
    if flag == 'cone_hoist_z1':
        alone = _flag_dev(w, theta, config, name, batch_key, 'cone')['launches']
        assert n[0] < alone[0], (n[0], alone[0])                                  # Z_1 of a batch formed once, not once per pass
    if flag == 'sparse_bwd':
        assert 0 < wk[WGRAD_BYTES] < wk0[WGRAD_BYTES], (wk[WGRAD_BYTES], wk0[WGRAD_BYTES])      # the weight gradients read the centre level and the centre-in-edge level alone
        assert n[0] != n0[0] and wk[0] != wk0[0], (n[0], wk[0], n0[0], wk0[0])    # the differentiated passes planned PASS_PLAIN, no transposed aggregates behind them
    if flag == 'hoist_z1':
        assert n[0] < n0[0] and wk[0] != wk0[0], (n[0], wk[0], n0[0], wk0[0])     # fewer layer-1 aggregate launches
    rep = sb.Report()
    sb.hold_all(rep, label, ref, theta, dev)
    _finish(rep)
    return dev


@pytest.mark.parametrize('flag', list(FLAGGED))
def test_world_step_at_every_flagged_schedule(world, flag, request):
    """undirected / directed at default knobs under hoist_z1, sparse_bwd, cone and cone + hoist_z1, against the reference of the dense paths (the oracle has no
    schedule)."""
    _need_split(world, world['S'], world['Q'])
    name = request.node.callspec.params['world']
    theta, ref = _reference(world, 'default', None)
    _hold_flagged(world, '%s %s' % (name, flag.replace('cone_', 'cone+')), flag, theta, ref)


def test_world_cone_on_the_split_weight_gradient(undirected):
    """cone with GM_WGRAD_SPLIT_MIN_CHUNKS=0: the level chunk tables on the split-bf16 weight gradient (at default thresholds a cone level of the undirected world
    stays on k_wgrad; the directed world forces the knob already)."""
    w = undirected
    theta, ref = _reference(w, 'default', None)
    dev = _hold_flagged(w, 'undirected cone wgrad_split', 'cone', theta, ref, knobs=dict(GM_WGRAD_SPLIT_MIN_CHUNKS=0))
    assert dev['launches'][5] > 0, dev['launches']


def test_world_hoist_z1_with_the_stream_aggregate(world, request):
    """hoist_z1 on batches with stream tables: the one place where the hoisted Z_1, a full aggregate launch, comes from k_agg_stream (another association inside
    a hub row's sum than the window kernel's).  The accounting is compared with the dense run under the same stream knobs on the same batches, so that the
    difference is the flag's alone.  On the undirected world the numbers move with the stream kernel; on the directed world the block is digit for digit the
    'directed hoist_z1' block (as 'directed agg_stream1' is 'directed default'): its batches get stream tables (asserted) but no result moves by a digit,
    so the directed case shows that this chain runs and holds, and adds no other order of summation."""
    _need_split(world, world['S'], world['Q'])
    name = request.node.callspec.params['world']
    theta, ref = _reference(world, 'default', None)
    for B in (world['S'], world['Q']):
        assert 0 < B.edges <= 8 * B.rows, (B.edges, B.rows)       # stream-eligible (gm_stream_batch_ok)
    knobs = dict(GM_AGG_STREAM=1, GM_AGG_STREAM_MIN_ROWS=0)
    with tuning(**knobs):
        run_on = _fresh_stream_world(world, name)
    dense = _world_run(run_on, theta, None, knobs=knobs)
    _hold_flagged(world, '%s hoist_z1 agg_stream1' % name, 'hoist_z1', theta, ref, knobs=knobs, run_on=run_on, dense=dense)
    assert _stream_segments(run_on) > 0


def test_world_first_task_alone_under_cone(undirected):
    """T = 1 under cone: a per-set mix-up in a level's set_off / set_chunk_off cannot cancel in the task mean."""
    w = undirected
    theta, ref = _reference(w, 'default', None, 'one')
    assert ref['T'] == 1
    _hold_flagged(w, 'undirected T=1 cone', 'cone', theta, ref, batch_key='one')


@pytest.mark.parametrize('dims', VARIANTS)
def test_model_variants_under_cone(undirected, dims):
    """Three GraphConv layers (four cone levels) and the multiply-first last layer under cone.  [128, 256, 128] is the path of k_colsum_rows (the bias gradient
    of a multiply-first layer, summed over a set's centre rows), of the GEMM on the source level with the aggregate after it (cone_forward, fi > fo), and in the
    backward of the transposed aggregate of dQ, the weight gradient over the source level's chunk table and the transB + mask_h GEMM on it."""
    w = undirected
    name, config = _variant(w, dims)
    theta, ref = _reference(w, name, config)
    _hold_flagged(w, 'undirected %s cone' % name, 'cone', theta, ref, config, name)


@pytest.mark.parametrize('dims', VARIANTS)
def test_model_variants_pin_the_sparse_bwd_fallback(undirected, dims):
    """sparse_bwd_ok refuses more than two GCN layers and a multiply-first layer: sparse_bwd = 1 then runs the dense backward behind PASS_DIFF forwards.  Not a
    schedule class: everything is bitwise the default run's, and the launch accounting is the same."""
    w = undirected
    name, config = _variant(w, dims)
    theta, _ = _reference(w, name, config)
    dev0 = _default_dev(w, theta, config, name)
    dev = _world_run(w, theta, config, sparse_bwd=1)
    for k in ('grad', 'losses', 'fw', 'protos', 'accs_task'):
        assert dev[k].dtype == dev0[k].dtype and dev[k].shape == dev0[k].shape and np.array_equal(_bits(dev[k]), _bits(dev0[k])), k
    assert len(dev['logits']) == len(dev0['logits']) == len(w['batch'][0])
    for t, (a, b) in enumerate(zip(dev['logits'], dev0['logits'])):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), t
        assert np.array_equal(np.asarray(dev['pred'][t]), np.asarray(dev0['pred'][t])), t
    assert dev['launches'] == dev0['launches'] and dev['work'] == dev0['work'], (dev['launches'], dev0['launches'], dev['work'], dev0['work'])


@pytest.mark.parametrize('flag', ['sparse_bwd', 'cone', 'cone_hoist_z1'])
def test_link_prediction_at_flagged_schedules(link_world, flag):      # noqa: F811
    """Two centres per subgraph: the head with compact = 1 over pairs of centre rows, the centre level of twice the subgraphs."""
    w = link_world
    assert w['S'].centres == 2 and w['Q'].centres == 2
    theta, ref = _reference(w, 'default', w['config'])
    _hold_flagged(w, 'link %s' % flag.replace('cone_', 'cone+'), flag, theta, ref, w['config'])
