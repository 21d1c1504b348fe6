"""GPU (-m gpu): bench.py's result line and --dump-outputs on the small syn0 configuration.  A plain run times --steps steps and
reports the headline only; two plain runs with the same arguments dump the same arrays; --full adds the secondary measurements
after the timed steps without changing what the timed steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('accs', 'losses_q', 'meta_grad', 'params')
SECONDARY = ('roofline', 'mfma', 'step_bound', 'two_queues', 'deferred_readback', 'box', 'extraction', 'end_to_end', 'extra', 'cpu_baseline')


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', 'syn0', '--steps', '3', '--warmup', '1',
           '--dump-outputs', str(out_dir)] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    lines = [l for l in out.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out[-3000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + '.npy')) for n in NAMES}


def test_plain_run_line_agrees_with_its_step_time_and_dumps_repeat(tmp_path):
    j1, d1 = _bench(tmp_path / 'a')
    j2, d2 = _bench(tmp_path / 'b')
    for j in (j1, j2):
        assert j['steps'] == 3 and j['warmup'] == 1 and j['ms_per_step'] > 0 and j['higher_is_better'] is True
        assert j['unit'] == 'meta-tasks/s' and j['dtype'] and j['metric'].startswith('meta-tasks/sec')
        # syn0: task_num 4.  `value` is 4 / the measured step time, `ms_per_step` that time rounded to 0.001 ms: they agree to that rounding
        assert abs(4e3 / j['value'] - j['ms_per_step']) <= 0.0005 + 1e-9
        assert not [k for k in SECONDARY if k in j], 'a plain run measures the headline only'
    for n in NAMES:
        assert d1[n].dtype in (np.float32, np.float64) and np.all(np.isfinite(d1[n])), n
        assert np.array_equal(d1[n], d2[n]), n
    assert d1['accs'].shape == d1['losses_q'].shape == (6,)                                   # syn0: update_step 5
    assert d1['meta_grad'].shape == d1['params'].shape and np.all((d1['accs'] >= 0) & (d1['accs'] <= 1))
    assert sum(os.path.getsize(tmp_path / 'a' / (n + '.npy')) for n in NAMES) < 64 << 20


def test_full_run_adds_measurements_after_the_same_steps(tmp_path):
    sizes = ('--no_cpu_baseline', '--extra_steps', '1', '--e2e_steps', '1', '--roofline_steps', '1')
    _, plain = _bench(tmp_path / 'plain', *sizes)
    j, full = _bench(tmp_path / 'full', '--full', *sizes)
    assert all(k in j for k in ('roofline', 'two_queues', 'extraction', 'end_to_end', 'extra')), sorted(j)
    for n in NAMES:
        assert np.array_equal(plain[n], full[n]), n
