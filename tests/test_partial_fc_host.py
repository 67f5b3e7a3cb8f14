"""CPU: the sampled-class (Partial FC) head's restatement (tests/partial_fc_ref.py) -- the sampler's properties, its head against the
dense restatement and against finite differences -- and the host surface: train.py's flags, fte.h and the ctypes table."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import margin_ref as mr
import partial_fc_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARC, COS = (64.0, 0.5, 0.0), (64.0, 0.0, 0.35)
NEW_SYMBOLS = ('fte_pfc_sample_ws_bytes', 'fte_pfc_sample', 'fte_pfc_gather_cols', 'fte_pfc_scatter_cols')


def test_fmix32_known_values():
    """murmur3's finaliser: fmix32(0) = 0 and the published avalanche of 1"""
    assert int(pr.fmix32(0)) == 0
    assert int(pr.fmix32(1)) == 0x514e28b7
    h = pr.fmix32(np.arange(1 << 16))
    assert len(np.unique(h)) == 1 << 16                       # a bijection: no two classes share a hash


def test_sampler_properties():
    C, S, n = 20000, 2000, 512
    rng = np.random.default_rng(0)
    freq = np.zeros(C)
    steps = 200
    never_positive = np.ones(C, bool)
    prev = None
    for t in range(steps):
        y = rng.integers(0, C, n)
        index, inverse, ys = pr.sample(y, C, S, seed=7, step=t)
        assert len(index) == S and (np.diff(index) > 0).all() and index[0] >= 0 and index[-1] < C
        assert np.isin(y, index).all()                        # every class of the batch is in
        assert (index[ys] == y).all()
        assert (inverse[index] == np.arange(S)).all() and (inverse >= 0).sum() == S
        again = pr.sample(y, C, S, seed=7, step=t)
        assert all((a == b).all() for a, b in zip((index, inverse, ys), again))
        other = pr.sample(y, C, S, seed=7, step=t + 1)[0]
        assert not np.array_equal(index, other)
        assert prev is None or not np.array_equal(index, prev)
        prev = index
        never_positive[y] = False
        freq[index] += 1
    # classes that never were in a batch are chosen by the hash alone: each step takes S - P of the C - P others, P <= n, so the
    # selection probability lies in [(S - n) / C, S / C]; within 4 binomial sigmas of that band, and the mean inside it
    f = freq[never_positive] / steps
    assert never_positive.sum() > 100
    lo, hi = (S - n) / C, S / C
    sigma = np.sqrt(hi * (1 - hi) / steps)
    assert lo - 4 * sigma <= f.min() and f.max() <= hi + 4 * sigma, (f.min(), f.max(), lo, hi, sigma)
    assert lo <= f.mean() <= hi, (f.mean(), lo, hi)
    # and over all classes the spread is the binomial one (plus the positives' small excess)
    assert abs((freq / steps).std() - np.sqrt(0.1 * 0.9 / steps)) < 0.2 * np.sqrt(0.1 * 0.9 / steps)


def test_sampler_edge_cases():
    C = 1000
    index, inverse, ys = pr.sample(np.full(64, 17), C, 64, 3, 0)                # one class in the whole batch
    assert 17 in index and len(index) == 64 and (ys == inverse[17]).all()
    y = np.random.default_rng(1).permutation(C)[:64]
    index, inverse, ys = pr.sample(y, C, 64, 3, 0)                               # n distinct classes and S = n: the batch alone
    assert np.array_equal(index, np.sort(y))
    index, inverse, ys = pr.sample(np.array([5, -1, C, 7]), C, 10, 3, 0)         # labels outside [0, C) take no part
    assert list(ys[[1, 2]]) == [-1, -1] and ys[0] >= 0 and ys[3] >= 0 and len(index) == 10
    index, _, _ = pr.sample(y, C, C, 3, 0)                                       # S = C: every class
    assert np.array_equal(index, np.arange(C))
    assert pr.sample_size(85742, 0.1) == 8575 and pr.sample_size(1000, 1.0) == 1000 and pr.sample_size(10575, 0.05) == 529


def _case(seed, n=6, d=16, c=40):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)), rng.standard_normal((d, c)), rng.integers(0, c, n)


@pytest.mark.parametrize('preset', [ARC, COS])
def test_all_classes_sampled_equals_the_dense_restatement(preset):
    x, W, y = _case(2)
    loss, f, dx, dW, index = pr.head_fwd_bwd(x, W, y, W.shape[1], 5, 9, *preset)
    lr, fr, dxr, dWr = mr.head_fwd_bwd(x, W, y, *preset)
    assert np.array_equal(index, np.arange(W.shape[1]))
    assert abs(loss - lr) <= 1e-12 * max(1, abs(lr))
    for a, b in ((f, fr), (dx, dxr), (dW, dWr)):
        assert np.abs(a - b).max() <= 1e-12 * max(1, np.abs(b).max())


@pytest.mark.parametrize('preset', [(8.0, 0.3, 0.0), (8.0, 0.0, 0.35)])
def test_reference_gradient_against_finite_differences(preset):
    x, W, y = _case(3)
    S, seed, step = 12, 11, 4
    loss, _, dx, dW, index = pr.head_fwd_bwd(x, W, y, S, seed, step, *preset)
    assert abs(loss - pr.loss_only(x, W, y, S, seed, step, *preset)) <= 1e-12 * max(1, abs(loss))
    unsampled = np.setdiff1d(np.arange(W.shape[1]), index)
    assert len(unsampled) == W.shape[1] - S and (dW[:, unsampled] == 0).all()
    eps = 1e-6
    rng = np.random.default_rng(4)
    for _ in range(12):
        i, k = rng.integers(0, x.shape[0]), rng.integers(0, x.shape[1])
        xp, xm = x.copy(), x.copy()
        xp[i, k] += eps; xm[i, k] -= eps
        fd = (pr.loss_only(xp, W, y, S, seed, step, *preset) - pr.loss_only(xm, W, y, S, seed, step, *preset)) / (2 * eps)
        assert abs(fd - dx[i, k]) <= 1e-6 * max(1, abs(fd)), (i, k, fd, dx[i, k])
    for col in list(index[:6]) + list(unsampled[:3]):
        k = rng.integers(0, W.shape[0])
        Wp, Wm = W.copy(), W.copy()
        Wp[k, col] += eps; Wm[k, col] -= eps
        fd = (pr.loss_only(x, Wp, y, S, seed, step, *preset) - pr.loss_only(x, Wm, y, S, seed, step, *preset)) / (2 * eps)
        assert abs(fd - dW[k, col]) <= 1e-6 * max(1, abs(fd)), (k, col, fd, dW[k, col])


# ------------------------------------------------------------------------------------------------ host surface
def _train(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')] + args, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300)


def test_train_help_lists_the_flags():
    r = _train(['--help'])
    assert r.returncode == 0 and '--sample_rate' in r.stdout and '--sample_seed' in r.stdout


@pytest.mark.parametrize('net', ['SphereNet', 'SphereNet-ASoftmax', 'ResNet-50-arcface'])
def test_sample_rate_is_refused_for_other_nets(net, tmp_path):
    r = _train(['--net_name', net, '--model_name', 'm', '--synthetic', '1', '--batch_size', '8', '--num_gpus', '1', '--max_epoches', '1',
                '--lr_decay_epoch', '2', '--sample_rate', '0.1', '--train_dir', str(tmp_path / 't'), '--model_dir', str(tmp_path / 'm')])
    assert r.returncode != 0
    assert '--sample_rate 0.1: only SphereNet-ArcFace / SphereNet-CosFace have a sampled-class head' in r.stdout, r.stdout[-2000:]
    assert not (tmp_path / 'm').exists()                      # refused before anything is created


def test_sample_rate_range_and_rank_checks():
    import train as cli
    ok = ['--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--batch_size', '8', '--max_epoches', '1', '--num_gpus', '1']
    F = cli.build_parser().parse_args(ok)
    assert F.sample_rate == 1.0 and F.sample_seed == 0
    cli.sample_flags_check(F)
    cli.sample_flags_check(cli.build_parser().parse_args(ok + ['--sample_rate', '0.1', '--sample_seed', '5']))
    cli.sample_flags_check(cli.build_parser().parse_args(['--net_name', 'ResNet-50', '--model_name', 'm', '--sample_rate', '1']))
    for bad in ('0', '-0.5', '1.5'):
        with pytest.raises(SystemExit, match='must lie in'):
            cli.sample_flags_check(cli.build_parser().parse_args(ok + ['--sample_rate', bad]))
    with pytest.raises(SystemExit, match='one GPU only'):
        cli.sample_flags_check(cli.build_parser().parse_args(ok[:-1] + ['2', '--sample_rate', '0.1']))


def test_symbols_are_declared_and_bound():
    from tf_face_toolbox_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fte.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in doc, name


def test_nets_without_a_sampled_head_refuse():
    from tf_face_toolbox_amd import net_select
    from tf_face_toolbox_amd.loss import sample_size
    for name in ('SphereNet', 'SphereNet-ASoftmax', 'ResNet-50-arcface', 'ResNet-50'):
        with pytest.raises(ValueError, match='sampled-class head'):
            net_select(name).set_sample_rate(0.1, 0)
    net = net_select('SphereNet-ArcFace')
    assert net.sample_rate is None
    net.set_sample_rate(0.25, 3)
    assert net.sample_rate == 0.25 and net.sample_seed == 3
    net.set_sample_rate(1.0)
    assert net.sample_rate is None
    for bad in (0.0, -1.0, 1.5):
        with pytest.raises(ValueError):
            net.set_sample_rate(bad)
    assert sample_size(85742, 0.1) == pr.sample_size(85742, 0.1) == 8575 and sample_size(1000, None) == 1000
