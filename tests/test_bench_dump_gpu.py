"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step computed (losses, targets, a seeded sample of the enhanced
signals, the updated weights) as float32 .npy files, `--steps` sets the number of timed steps, and two runs with the same arguments
(seeded inputs, same initial weights) write the same arrays; a run without `--full` measures nothing beside the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L = 4, 24000


def _run(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--batch', str(B), '--length', str(L)] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def _bench(out_dir, steps):
    return _run(['--steps', str(steps), '--warmup', '1', '--companions', '0', '--cpu-utts', '0', '--no-isolated', '--dump-outputs', str(out_dir)])


def test_dump_outputs_of_the_last_timed_step_are_reproducible(tmp_path):
    a = _bench(tmp_path / 'a', 3)
    assert a['steps'] == 3 and a['ms_per_step'] > 0
    names = ('g_loss', 'd_loss', 'targets', 'enhanced_sample', 'g_weights', 'd_weights')
    assert sorted(a['dumped_outputs']['arrays']) == sorted(names)
    arr = {n: np.load(tmp_path / 'a' / (n + '.npy')) for n in names}
    assert sum(x.nbytes for x in arr.values()) <= 64 << 20
    for n, x in arr.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
    assert arr['targets'].shape == (B, 3)
    assert arr['enhanced_sample'].shape == (B, 256 * (L // 256))
    b = _bench(tmp_path / 'b', 3)
    assert b['dumped_outputs']['enhanced_rows'] == a['dumped_outputs']['enhanced_rows']
    for n in names:
        assert np.array_equal(np.load(tmp_path / 'b' / (n + '.npy')), arr[n]), n


def test_a_plain_run_measures_the_timed_steps_only():
    """Without --full nothing is measured after the timed steps: no CPU baseline, no companions, no isolated D.conv5 launches - the line
    holds the headline figure and what the library's event hook took inside the timed steps."""
    out = _run(['--steps', '2', '--warmup', '1'])
    assert out['steps'] == 2 and out['warmup'] == 1 and out['ms_per_step'] > 0 and out['value'] > 0
    assert out['unit'] == 'utterances/s' and out['higher_is_better'] is True and out['dtype'] == 'bf16'
    assert not {'cpu_baseline', 'configs1', 'nonperiodic', 'headline_f32', 'inference', 'epoch_equivalent', 'allreduce_ms_per_step'} & set(out)
    assert out['roofline_mfma']['isolated_launch_ms'] is None
