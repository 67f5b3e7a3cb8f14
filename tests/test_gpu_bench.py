"""-m gpu: bench.py on one GPU -- the plain run (contract fields only, --dump-outputs) and the --full run (the legs besides the
headline figure), at a small global batch so that each run takes seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _bench(cwd, *args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + list(args), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900, cwd=str(cwd))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_contract_and_dumps_the_last_step(tmp_path):
    """A plain run prints the contract fields and none of the --full legs; --dump-outputs writes the losses and every variable
    after the last timed step (float32, the large ones as a fixed sample, under 64 MB in all); the same arguments give the
    same inputs, so a second run writes the same arrays (to fp32 rounding: the filter gradients sum with atomics)."""
    dumps = [tmp_path / 'a', tmp_path / 'b']
    outs = [_bench(tmp_path, '--steps', '3', '--warmup', '1', '--global-batch', '16', '--dump-outputs', str(d)) for d in dumps]
    out = outs[0]
    for k in CONTRACT:
        assert k in out, k
    assert out['unit'] == 'images/sec' and out['higher_is_better'] is True and out['dtype'] == 'f32'
    assert out['steps'] == 3 and out['warmup'] == 1 and out['config']['global_batch'] == 16
    assert abs(out['value'] - 16 / (out['ms_per_step'] * 1e-3)) <= 0.01 * out['value']
    for k in ('roofline', 'conv_algo', 'cpu_baseline', 'parity', 'other_configs', 'allreduce'):
        assert k not in out, k
    files = sorted(os.listdir(dumps[0]))
    assert files == sorted(os.listdir(dumps[1])) and 'losses.npy' in files and len(files) > 40
    total = 0
    for f in files:
        a, b = np.load(dumps[0] / f), np.load(dumps[1] / f)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), f
        assert a.size <= 1 << 20, f
        total += a.nbytes
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6 * max(1e-30, float(np.abs(a).max())), err_msg=f)
    assert total <= 64 << 20
    losses = np.load(dumps[0] / 'losses.npy')
    np.testing.assert_allclose(losses, list(out['losses'].values()), rtol=1e-5, atol=1e-6)
    assert np.load(dumps[0] / 'classifier.fc_classifier.weights.npy').shape == (1 << 20,)
    assert np.load(dumps[0] / 'SphereNet.conv1.Conv.weights.npy').shape == (3, 3, 3, 64)


def test_full_run_keeps_the_launch_records(tmp_path):
    """--full: the timed steps take the launch records again and the line carries the roofline, the per-shape table and the
    conv algorithm's launch counts (the CPU baseline and other_configs are switched off here: they take a minute)."""
    out = _bench(tmp_path, '--full', '--steps', '4', '--warmup', '1', '--global-batch', '64', '--no-cpu-baseline', '--no-other-configs')
    for k in CONTRACT:
        assert k in out, k
    assert out['roofline']['frac'] > 0 and {'fwd', 'dgrad', 'wgrad'} <= set(e['op'] for e in out['roofline']['per_shape'])
    assert out['conv_algo']['winograd_launches_per_step'] + out['conv_algo']['direct_mfma_launches_per_step'] > 0
    assert out['cpu_baseline'] is None and 'other_configs' not in out
