"""GPU (-m gpu): the row plan of the dense schedule at every crossing of its three knobs.

plan_pass (csrc/model.hip; the table in DESIGN.md section 4.3) decides per pass which rows each layer forms and stores and how dQ_L is left, from GM_DEAD_ROWS
(0..4), GM_CENTRE_STORE (0..2), GM_FUSE_DIFF (0..2) and the pass kind.  The other dead-row suites walk the levels at the default GM_CENTRE_STORE and visit
GM_CENTRE_STORE 0 / 1 at a level or two; this one runs one Meta.forward at each of the 15 (GM_DEAD_ROWS, GM_CENTRE_STORE) pairs per GM_FUSE_DIFF.  No
level drops or reorders a product or a sum that reaches a stored value, so every pair gives the results of (0, 0) BITWISE; what falls with the level is what
the launch accounting prices.  Nothing is compared across GM_FUSE_DIFF values: where the support chain keeps the stream aggregate its sums run in another order.

World and helpers: the `undirected` one of tests/test_hip_dead_rows_fwd.py (20,000-node preferential-attachment graph, F0 128, hidden 256, 8 tasks, K = 2)
and _step of tests/test_hip_dead_rows_diff.py, with the split kernels forced."""
import itertools

import numpy as np
import pytest
import torch

from test_hip_dead_rows_diff import _step
from test_hip_dead_rows_fwd import _assert_bitwise, _n_tiles, _world

pytestmark = pytest.mark.gpu

FORCE = dict(GM_GEMM_SPLIT_MIN_TILES=0, GM_WGRAD_SPLIT_MIN_CHUNKS=0)
LEVELS, STORES = (0, 1, 2, 3, 4), (0, 1, 2)


@pytest.fixture(scope='module')
def undirected():
    return _world(True)


@pytest.mark.parametrize('fuse_diff', [0, 1, 2])
def test_every_knob_crossing_is_bitwise_the_every_row_step(undirected, fuse_diff):
    w = undirected
    # what _need_split asks of the world (asserted, never skipped: the restricted plans engage on the split kernels only)
    need = torch.cuda.get_device_properties(0).multi_processor_count // 4
    assert min(_n_tiles(w['S']), _n_tiles(w['Q'])) >= need, (_n_tiles(w['S']), _n_tiles(w['Q']), need)
    res = {(lv, cs): _step(w, GM_DEAD_ROWS=lv, GM_CENTRE_STORE=cs, GM_FUSE_DIFF=fuse_diff, **FORCE) for lv, cs in itertools.product(LEVELS, STORES)}
    ref = res[0, 0]
    assert all(np.isfinite(ref[k]).all() for k in ('accs', 'losses', 'grad', 'theta')) and np.abs(ref['grad']).max() > 0
    for key, r in res.items():
        print('GM_FUSE_DIFF=%d GM_DEAD_ROWS=%d GM_CENTRE_STORE=%d: category 0 %d bytes, category 14 %d bytes' % ((fuse_diff,) + key + (r['agg_bytes'], r['wgrad_bytes'])))
        try:
            _assert_bitwise(r, ref)
        except AssertionError as e:
            raise AssertionError('(GM_DEAD_ROWS, GM_CENTRE_STORE) = %r differs from (0, 0) in %s' % (key, e))
    for cat in ('agg_bytes', 'wgrad_bytes'):
        assert ref[cat] > 0
        for cs in STORES:
            by = [res[lv, cs][cat] for lv in LEVELS]
            assert all(hi <= lo for lo, hi in zip(by, by[1:])), (cat, cs, by)      # never larger at a higher level
        assert len({res[lv, 0][cat] for lv in LEVELS}) == 1, (cat, [res[lv, 0][cat] for lv in LEVELS])      # GM_CENTRE_STORE=0 switches every level off
