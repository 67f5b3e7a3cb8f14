"""CPU: the sub-center ArcFace head's float64 restatement (tests/subcenter_ref.py) against the one-centre restatement and finite
differences, the lowest-k tie rule, what the host refuses, the checkpoint layout, and the cleaning decision on a hand-built case."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import margin_ref as mr
import subcenter_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESETS = [(64.0, 0.5, 0.0), (64.0, 0.0, 0.35), (30.0, 0.3, 0.2)]


def _case(seed, n, d, c, K, ld):
    rng = np.random.default_rng(seed)
    W = np.zeros((d, K, ld))
    W[:, :, :c] = rng.standard_normal((d, K, c))
    W = W.reshape(d, K * ld)
    x = rng.standard_normal((n, d)) * rng.uniform(0.5, 5.0, (n, 1))
    y = rng.integers(0, c, n)
    return x, W, y


@pytest.mark.parametrize('preset', PRESETS)
def test_one_centre_is_the_existing_restatement(preset):
    x, W, y = _case(1, 9, 16, 13, 1, 16)
    s, xn, wn = x @ W, np.sqrt((x * x).sum(1)), np.sqrt((W * W).sum(0))
    y[2] = 13                                                   # a NaN row
    got = sr.kernel_ref(s, xn, wn, y, 1, *preset, 1.0 / 9, 13, 16)
    want = mr.kernel_ref(s, xn, wn, y, *preset, 1.0 / 9, c=13)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_, equal_nan=True)
    ok = np.isfinite(want[1])
    assert np.array_equal(sr.colcoef_ref(got[2][ok], s[ok], wn, 1, 13, 16), mr.colcoef_ref(want[2][ok], s[ok], wn, 13))


@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('preset', PRESETS)
def test_gradient_against_finite_differences(K, preset):
    """dx and dW through both normalisations against central differences of the restatement's own loss; every top-two gap >= 1e-3, so no
    difference step (1e-6) moves a winner"""
    n, d, c = 5, 12, 7
    x, W, y = _case(10 * K + int(preset[0]), n, d, c, K, c)
    cos, _ = sr.plane_cos(x @ W, np.sqrt((x * x).sum(1)), np.sqrt((W * W).sum(0)), K, c, c)
    assert sr.gaps(cos).min() >= 1e-3
    loss, _, dx, dW = sr.head_fwd_bwd(x, W, y, K, *preset)
    assert abs(loss - sr.loss_only(x, W, y, K, *preset)) <= 1e-12 * max(1, abs(loss))
    h = 1e-6
    fd_x, fd_w = np.zeros_like(x), np.zeros_like(W)
    for idx in np.ndindex(*x.shape):
        a, b = x.copy(), x.copy()
        a[idx] += h
        b[idx] -= h
        fd_x[idx] = (sr.loss_only(a, W, y, K, *preset) - sr.loss_only(b, W, y, K, *preset)) / (2 * h)
    for idx in np.ndindex(*W.shape):
        a, b = W.copy(), W.copy()
        a[idx] += h
        b[idx] -= h
        fd_w[idx] = (sr.loss_only(x, a, y, K, *preset) - sr.loss_only(x, b, y, K, *preset)) / (2 * h)
    assert np.abs(dx - fd_x).max() <= 1e-6 * max(1.0, np.abs(fd_x).max()), np.abs(dx - fd_x).max()
    assert np.abs(dW - fd_w).max() <= 1e-6 * max(1.0, np.abs(fd_w).max()), np.abs(dW - fd_w).max()


def test_lowest_k_wins_exact_ties():
    n, c, K, ld = 3, 4, 3, 4
    rng = np.random.default_rng(3)
    s = rng.standard_normal((n, K, ld))
    wn = np.ones((K, ld))
    s[:, 2, 1] = s[:, 0, 1] = 5.0                               # class 1: centres 0 and 2 tie above centre 1
    s[:, 1, 1] = 1.0
    s[:, 1, 2] = s[:, 2, 2] = 4.0                               # class 2: centres 1 and 2 tie above centre 0
    s[:, 0, 2] = -1.0
    xn = np.full(n, 10.0)
    y = np.array([1, 2, 0])
    _, _, G, _ = sr.kernel_ref(s.reshape(n, -1), xn, wn.reshape(-1), y, K, 64.0, 0.5, 0.0, 1.0, c, ld)
    G = G.reshape(n, K, ld)
    assert (G[:, 0, 1] != 0).all() and (G[:, 1, 1] == 0).all() and (G[:, 2, 1] == 0).all()
    assert (G[:, 1, 2] != 0).all() and (G[:, 0, 2] == 0).all() and (G[:, 2, 2] == 0).all()
    assert ((G != 0).sum(1) == 1).all()                         # one centre per (row, class) pair


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_net_select_refuses_what_is_not_built():
    from tf_face_toolbox_amd import net_select
    for name in ('SphereNet-ArcFace', 'SphereNet-CosFace', 'ResNet-50-arcface', 'ResNet-50-cosface'):
        assert net_select(name, sub_centers=3).sub_centers == 3
        assert net_select(name).sub_centers == 1
    for name in ('SphereNet-ASoftmax', 'SphereNet-AdaFace', 'ResNet-50-adaface', 'SphereNet', 'ResNet-50', 'ShuffleNet-v2-small'):
        with pytest.raises(ValueError, match='sub_centers = 2'):
            net_select(name, sub_centers=2)
        net_select(name, sub_centers=1)
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match='1..8'):
            net_select('SphereNet-ArcFace', sub_centers=bad)
    net = net_select('SphereNet-ArcFace', sub_centers=2)
    with pytest.raises(ValueError, match='class sampler'):
        net.set_sample_rate(0.1, 0)
    net.set_sample_rate(1.0)
    from tf_face_toolbox_amd.nets.sphere import SphereNetAdditiveMargin
    with pytest.raises(ValueError, match='class sampler'):
        SphereNetAdditiveMargin(sample_rate=0.5, sub_centers=2)


def test_describe_keeps_the_one_centre_tuple():
    from tf_face_toolbox_amd import heads, net_select
    assert heads.describe(net_select('SphereNet-ArcFace')) == ('arcface', 64.0, 0.5, 0.0)
    assert heads.describe(net_select('SphereNet-CosFace', sub_centers=4)) == ('cosface', 64.0, 0.0, 0.35, 4)


def test_train_flag_messages(tmp_path):
    import train as cli
    ok = ['--net_name', 'SphereNet-ArcFace', '--model_name', 'm', '--batch_size', '8', '--num_gpus', '1']
    assert cli.build_parser().parse_args(ok).sub_centers == 1
    cli.sub_centers_flags_check(cli.build_parser().parse_args(ok + ['--sub_centers', '3']))
    cli.sub_centers_flags_check(cli.build_parser().parse_args(['--net_name', 'ResNet-50', '--model_name', 'm']))
    with pytest.raises(SystemExit, match='--sub_centers 3: .*class sampler'):
        cli.sub_centers_flags_check(cli.build_parser().parse_args(ok + ['--sub_centers', '3', '--sample_rate', '0.1']))
    with pytest.raises(SystemExit, match='--sub_centers 9: .*1..8'):
        cli.sub_centers_flags_check(cli.build_parser().parse_args(ok + ['--sub_centers', '9']))
    with pytest.raises(SystemExit, match='--sub_centers 2: .*not SphereNet-AdaFace'):
        cli.sub_centers_flags_check(cli.build_parser().parse_args(['--net_name', 'SphereNet-AdaFace', '--model_name', 'm', '--sub_centers', '2']))
    # the whole command leaves before anything is built
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')] + ok + ['--max_epoches', '1', '--lr_decay_epoch', '2', '--sub_centers', '3',
                       '--sample_rate', '0.1', '--train_dir', str(tmp_path / 't'), '--model_dir', str(tmp_path / 'm')],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode != 0 and '--sub_centers 3' in r.stdout and 'class sampler' in r.stdout, r.stdout[-2000:]
    assert not (tmp_path / 't').exists()


# ---- checkpoint ----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_width_mismatch(tmp_path):
    from tf_face_toolbox_amd import net_select, saver
    name = 'classifier/fc_classifier/weights'
    C = 10
    net = net_select('SphereNet-ArcFace', sub_centers=3).build(32, 32, 3, C, 'cpu')
    assert net.variables[name].size == 512 * 3 * net.cpad and net.variables[name].ref_shape == (512, 3 * C)
    W = net.get_variable(name)
    planes = net.view(name).reshape(512, 3, net.cpad)
    assert W.shape == (512, 3 * C) and torch.equal(W.reshape(512, 3, C), planes[:, :, :C]) and (planes[:, :, C:] == 0).all()
    assert not torch.equal(W[:, :C], W[:, C:2 * C]) and not torch.equal(W[:, C:2 * C], W[:, 2 * C:])      # planes drawn independently
    path = saver.save(net, [], 7, str(tmp_path / 'k3' / 'k3.ckpt'))
    assert torch.load(path)['variables'][name].shape == (512, 3 * C)
    other = net_select('SphereNet-ArcFace', sub_centers=3).build(32, 32, 3, C, 'cpu')
    other.params.zero_()
    assert saver.restore(other, path) == 7 and torch.equal(other.params, net.params)
    with pytest.raises(ValueError, match=r'30 columns.*1 \* 10 = 10'):
        saver.restore(net_select('SphereNet-ArcFace').build(32, 32, 3, C, 'cpu'), path)
    with pytest.raises(ValueError, match=r'30 columns.*2 \* 10 = 20'):
        saver.restore(net_select('SphereNet-ArcFace', sub_centers=2).build(32, 32, 3, C, 'cpu'), path)
    # one centre: the variable, its initial values and its file are what they were without the argument
    a, b = net_select('SphereNet-ArcFace').build(32, 32, 3, C, 'cpu'), net_select('SphereNet-ArcFace', sub_centers=1).build(32, 32, 3, C, 'cpu')
    assert torch.equal(a.params, b.params) and a.get_variable(name).shape == (512, C)


# ---- cleaning ----------------------------------------------------------------------------------------------------------------------------
def cleaning_case(d=128, C=5, K=3):
    """Mutually orthogonal unit centres e_(k * C + j); a feature `on centre k at angle a` is cos a * w_k + sin a * u with u a unit vector
    orthogonal to every centre: its cosines are cos a to w_k and exactly 0 to the other two.  -> (x [n, d] fp32, Wt [K * C, d], labels,
    lines, expected keep at --angle 50, expected dominant)."""
    Wt = np.zeros((K * C, d), np.float32)
    for r in range(K * C):
        Wt[r, r] = 1.0 + 0.25 * r                                # norms differ: the cosine, not the dot product, decides
    spec = [  # (class, centre, angle in degrees)
        (0, 0, 10), (0, 0, 45), (0, 0, 60), (0, 2, 10),         # class 0: dominant 0; 60 deg dropped; the sample on centre 2 is 90 deg away
        (1, 0, 10), (1, 0, 49), (1, 0, 51),                     # class 1: one degree either side of the threshold
        (2, 2, 10), (2, 0, 45), (2, 0, 10), (2, 0, 60),         # class 2: dominant 0 (3 of 4)
        (3, 1, 10), (3, 1, 45), (3, 0, 10), (3, 1, 60),         # class 3: its majority on centre 1: the sample on centre 0 goes
        (0, 0, 10),
    ]
    x = np.zeros((len(spec), d), np.float32)
    for i, (j, k, a) in enumerate(spec):
        r = k * C + j
        x[i, r] = np.cos(np.deg2rad(a)) * (1.0 + 0.1 * i)
        x[i, K * C + i] = np.sin(np.deg2rad(a)) * (1.0 + 0.1 * i)
    labels = np.array([j for j, _, _ in spec])
    keep = np.array([1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 1], bool)
    return x, Wt, labels, ['img_%02d.png %d\n' % (i, j) for i, j in enumerate(labels)], keep, np.array([0, 0, 0, 1, 0])


def test_cleaning_decision_on_the_hand_built_case():
    x, Wt, labels, _, keep, dominant = cleaning_case()
    sel, cosv, gap = sr.assign_ref(x, Wt, labels, 3, 5)
    assert gap.min() > 0.4
    dom, kp, kept, dropped, off = sr.clean_ref(sel, cosv, labels, 3, 5, 50.0)
    assert np.array_equal(dom, dominant) and np.array_equal(kp, keep)
    assert kept.tolist() == [3, 2, 2, 2, 0] and dropped.tolist() == [2, 1, 2, 2, 0] and off == 3
    # bad labels select nothing and are dropped
    sel, cosv, _ = sr.assign_ref(x[:2], Wt, np.array([5, -1]), 3, 5)
    assert sel.tolist() == [-1, -1] and np.isnan(cosv).all()


def test_reduce_checkpoint_zeroes_the_classifier_slots():
    from tf_face_toolbox_amd import subcenter
    name = subcenter.CLASSIFIER
    W = torch.arange(4 * 6, dtype=torch.float32).reshape(4, 6)
    state = {'global_step': 3, 'variables': {name: W, 'b': torch.ones(2)}, 'slots': [{name: torch.ones(4, 6), 'b': torch.full((2,), 2.0)}]}
    planes = subcenter.packed_planes(W, 3)
    w1 = planes[:, torch.tensor([2, 0]), torch.arange(2)]
    out = subcenter.reduce_checkpoint(state, w1)
    assert torch.equal(out['variables'][name], torch.stack([W[:, 4], W[:, 1]], 1)) and out['global_step'] == 3
    assert torch.equal(out['slots'][0][name], torch.zeros(4, 2)) and torch.equal(out['slots'][0]['b'], torch.full((2,), 2.0))
    assert state['variables'][name] is W and state['slots'][0][name].shape == (4, 6)
    with pytest.raises(ValueError, match='6 columns'):
        subcenter.packed_planes(W, 4)
    assert subcenter.threshold(75.0) == float(np.float32(np.cos(np.deg2rad(75.0))))
