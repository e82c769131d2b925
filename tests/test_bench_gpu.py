"""bench.py on the GPU: a plain run times the headline alone (no side measurement on its line), `--steps` is the number of timed
steps, and `--dump-outputs` writes the last timed chunk, identical from run to run (seeded inputs and weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def _plain_run(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--dump-outputs', str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    a = _plain_run(tmp_path / 'a', 3)
    b = _plain_run(tmp_path / 'b', 4)
    for d, steps in ((a, 3), (b, 4)):
        assert d['metric'] == 'action_chunks_per_sec' and d['unit'] == 'action-chunks/s' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
        assert d['steps'] == steps and d['ms_per_step'] > 0 and abs(d['value'] - 1e3 / d['ms_per_step']) < 0.01 * d['value']
        for side in ('reference_signature', 'roofline', 'phases', 'cpu_baseline', 'sft', 'batched', 'two_in_flight', 'qa', 'qa_8b', 'vla_train'):
            assert side not in d, side
    assert sorted(os.listdir(tmp_path / 'a')) == ['actions.npy']
    x, y = np.load(tmp_path / 'a' / 'actions.npy'), np.load(tmp_path / 'b' / 'actions.npy')
    assert x.dtype == np.float32 and x.shape == (1, 4, 7) and np.isfinite(x).all()
    assert np.array_equal(x, y), 'two runs with the same inputs dumped different chunks'
