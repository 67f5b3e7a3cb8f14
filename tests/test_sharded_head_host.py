"""CPU: the host side of the sharded margin head -- the shard ranges, the --shard_classes flag and its refusals,
the float64 restatement's own consistency (the shards merge to the dense head), and _HostComm.reduce_scatter_sum over gloo."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import margin_ref as mr
import sharded_head_ref as shr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import train                                   # noqa: E402
from tf_face_toolbox_amd import heads          # noqa: E402


def test_shard_ranges_tile_the_classes_in_order():
    for C in list(range(1, 40)) + [127, 128, 129, 1000, 1001, 85742]:
        for R in range(1, 10):
            cs = -(-C // R)
            if (R - 1) * cs >= C:                              # a rank would be left without a class
                for r in range(R):
                    with pytest.raises(ValueError, match='without a class'):
                        heads.shard_range(C, R, r)
                continue
            ranges = [heads.shard_range(C, R, r) for r in range(R)]
            assert ranges == shr.shard_ranges(C, R)
            assert ranges[0][0] == 0 and ranges[-1][1] == C
            assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            assert all(hi - lo == cs for lo, hi in ranges[:-1]) and 1 <= ranges[-1][1] - ranges[-1][0] <= cs
            ld = heads.shard_ld(C, R)
            assert ld % 128 == 0 and cs <= ld < cs + 128
    assert heads.shard_range(9, 5, 4) == (8, 9)
    with pytest.raises(ValueError, match='leaves rank 5 without a class'):
        heads.shard_range(9, 8, 0)
    for bad in ((0, 1, 0), (10, 0, 0), (10, 2, 2), (10, 2, -1)):
        with pytest.raises(ValueError):
            heads.shard_range(*bad)


BASE = ['--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--batch_size', '8', '--max_epoches', '1', '--synthetic', '1',
        '--synthetic_classes', '1000']


def _flags(*more):
    return train.build_parser().parse_args(BASE + list(more))


def test_flag_default_and_parsing():
    assert _flags().shard_classes == 0
    assert _flags('--shard_classes', '1', '--num_gpus', '2').shard_classes == 1
    train.shard_flags_check(_flags('--num_gpus', '1'))                         # off: nothing to refuse
    train.shard_flags_check(_flags('--shard_classes', '1', '--num_gpus', '2'))
    train.shard_flags_check(_flags('--shard_classes', '1', '--num_gpus', '4', '--net_name', 'SphereNet-CosFace'))
    text = ' '.join(train.build_parser().format_help().split())               # (argparse wraps the lines)
    assert '--shard_classes' in text and 'split by class over the ranks' in text


@pytest.mark.parametrize('more,reason', [
    (['--num_gpus', '1'], 'needs --num_gpus > 1'),
    (['--num_gpus', '2', '--sample_rate', '0.1'], 'does not compose with the class sampler'),
    (['--num_gpus', '2', '--sample_rate', '0.1', '--sync_sample', '1'], 'does not compose with the class sampler'),
    (['--num_gpus', '2', '--sync_sample', '1'], 'does not compose with sync_sample'),
    (['--num_gpus', '2', '--sub_centers', '2'], 'does not compose with sub_centers = 2'),
    (['--num_gpus', '2', '--net_name', 'SphereNet-ASoftmax'], 'only SphereNet-ArcFace / SphereNet-CosFace have a sharded classifier'),
    (['--num_gpus', '2', '--net_name', 'SphereNet-AdaFace'], 'only SphereNet-ArcFace / SphereNet-CosFace have a sharded classifier'),
    (['--num_gpus', '2', '--net_name', 'ResNet-50-arcface'], 'only SphereNet-ArcFace / SphereNet-CosFace have a sharded classifier'),
    (['--num_gpus', '8', '--synthetic_classes', '9'], 'leaves rank 5 without a class'),
])
def test_refusals_come_from_the_flags(more, reason, tmp_path):
    with pytest.raises(SystemExit) as e:
        train.shard_flags_check(_flags('--shard_classes', '1', *more))
    assert reason in str(e.value.code), e.value.code
    # ... and main() raises it before anything is built (no GPU here: going any further would fail differently)
    with pytest.raises(SystemExit) as e:
        train.main(BASE + ['--shard_classes', '1', '--train_dir', str(tmp_path / 't'), '--model_dir', str(tmp_path / 'm')] + more)
    assert reason in str(e.value.code), e.value.code
    assert not (tmp_path / 'm').exists()


def test_check_sharding_names_the_reason():
    heads.check_sharding('arcface')
    heads.check_sharding('cosface', None, False, 1)
    heads.check_sharding('arcface', 1.0)
    for args, reason in ((('asoftmax',), 'needs an ArcFace / CosFace head'), (('adaface',), 'needs an ArcFace / CosFace head'),
                         (('arcface', 0.5), 'class sampler'), (('arcface', None, True), 'sync_sample'), (('arcface', None, False, 4), 'sub_centers = 4')):
        with pytest.raises(ValueError, match=reason):
            heads.check_sharding(*args)


@pytest.mark.parametrize('N,C,R', [(7, 10, 3), (8, 1001, 4), (5, 513, 2), (4, 9, 5)])
@pytest.mark.parametrize('preset', [(64.0, 0.5, 0.0), (64.0, 0.0, 0.35)])
def test_the_restatement_of_the_shards_is_the_dense_restatement(N, C, R, preset):
    """float64 against float64: statistics per shard, merged in rank order, give the dense head's loss, G and rowcoef to rounding"""
    rng = np.random.default_rng(N + C + R)
    d = 16
    x, W = rng.standard_normal((N, d)), rng.standard_normal((d, C))
    y = rng.integers(0, C, N)
    y[0], y[-1] = 0, C - 1
    s, xn, wn = x @ W, np.sqrt((x * x).sum(1)), np.sqrt((W * W).sum(0))
    fd, ld_, Gd, rcd = mr.kernel_ref(s, xn, wn, y, *preset, 1.0 / N)
    ranges = shr.shard_ranges(C, R)
    stats = np.stack([shr.stats_ref(s[:, lo:hi], xn, wn[lo:hi], y, lo, C, *preset, hi - lo) for lo, hi in ranges])
    rc = np.zeros(N)
    for lo, hi in ranges:
        f, rows, G, part = shr.fwd_bwd_ref(s[:, lo:hi], xn, wn[lo:hi], y, lo, C, *preset, stats, 1.0 / N, hi - lo)
        np.testing.assert_allclose(rows, ld_, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(G, Gd[:, lo:hi], rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(f, fd[:, lo:hi], rtol=1e-12)
        rc += part
    np.testing.assert_allclose(rc, rcd, rtol=1e-9, atol=1e-14)
    bad = y.copy()
    bad[1] = C
    stats = np.stack([shr.stats_ref(s[:, lo:hi], xn, wn[lo:hi], bad, lo, C, *preset, hi - lo) for lo, hi in ranges])
    assert np.isnan(stats[:, :, 1]).all() and np.isfinite(np.delete(stats, 1, axis=2)).all()


def test_reduce_scatter_sum_over_gloo(tmp_path):
    """2 ranks as child processes on CPU tensors: gloo has no reduce-scatter, the all-reduce + copy must give the rank's rows of the sum"""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / 'rs')
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS='2')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(port), os.path.join(ROOT, 'tests', 'shard_dp_worker.py'), 'rs', '-', out, '-', '0'],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    res = [np.load(out + '.rank%d.npz' % k) for k in range(2)]
    total = res[0]['inp'] + res[1]['inp']
    assert not np.array_equal(res[0]['inp'], res[1]['inp'])
    for k, rk in enumerate(res):
        assert str(rk['backend']) == 'gloo'
        np.testing.assert_array_equal(rk['got'], total[3 * k:3 * k + 3])
