"""CPU: the float64 restatement of the additive-margin head (tests/margin_ref.py) against central finite differences of the loss
as defined, the factory names of the margin nets, and the new entry point's declaration and binding."""
import os
import re

import numpy as np
import pytest

import margin_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fd_check(x, W, y, S, m, m3, rows=None, h=1e-6, rtol=1e-6):
    loss, f, dx, dW = mr.head_fwd_bwd(x, W, y, S, m, m3)
    assert np.isclose(loss, mr.loss_only(x, W, y, S, m, m3), rtol=1e-12, atol=0)
    for i in (range(x.shape[0]) if rows is None else rows):
        for k in range(x.shape[1]):
            hh = h * max(np.abs(x[i]).max(), 1e-300)
            xp, xm = x.copy(), x.copy()
            xp[i, k] += hh
            xm[i, k] -= hh
            fd = (mr.loss_only(xp, W, y, S, m, m3) - mr.loss_only(xm, W, y, S, m, m3)) / (2 * hh)
            assert abs(fd - dx[i, k]) <= rtol * max(1.0, np.abs(dx).max()), ('dx', i, k, fd, dx[i, k])
    for k in range(W.shape[0]):
        for j in range(W.shape[1]):
            Wp, Wm = W.copy(), W.copy()
            Wp[k, j] += h
            Wm[k, j] -= h
            fd = (mr.loss_only(x, Wp, y, S, m, m3) - mr.loss_only(x, Wm, y, S, m, m3)) / (2 * h)
            assert abs(fd - dW[k, j]) <= rtol * max(1.0, np.abs(dW).max()), ('dW', k, j, fd, dW[k, j])
    return dx, dW


PRESETS = {'arcface': (64.0, 0.5, 0.0), 'cosface': (64.0, 0.0, 0.35), 'combined': (30.0, 0.3, 0.2)}


@pytest.mark.parametrize('which', sorted(PRESETS))
def test_gradient_matches_finite_differences(which):
    S, m, m3 = PRESETS[which]
    rng = np.random.default_rng(3)
    x = rng.normal(size=(5, 6))
    W = rng.normal(size=(6, 7))
    y = rng.integers(0, 7, 5)
    _fd_check(x, W, y, S / 8, m, m3)          # S / 8: the softmax away from saturation, every term of the gradient is exercised
    _fd_check(x, W, y, S, m, m3)


def test_fallback_branch_and_target_near_one():
    """Row 0's target sits at theta + m > pi (the easy_margin = False fallback t = c - m sin m); row 1's target at c = 0.999."""
    S, m, m3 = 16.0, 0.5, 0.0
    rng = np.random.default_rng(4)
    W = rng.normal(size=(4, 5))
    x = rng.normal(size=(3, 4))
    y = np.array([2, 3, 0])
    w2 = W[:, 2] / np.linalg.norm(W[:, 2])
    x[0] = -w2 * 1.7 + 0.05 * rng.normal(size=4)
    c0 = x[0] @ W[:, 2] / np.linalg.norm(x[0]) / np.linalg.norm(W[:, 2])
    assert c0 < np.cos(np.pi - m)
    w3 = W[:, 3] / np.linalg.norm(W[:, 3])
    perp = rng.normal(size=4)
    perp -= (perp @ w3) * w3
    perp /= np.linalg.norm(perp)
    x[1] = 2.0 * (0.999 * w3 + np.sqrt(1 - 0.999 ** 2) * perp)
    c1 = x[1] @ W[:, 3] / np.linalg.norm(x[1]) / np.linalg.norm(W[:, 3])
    assert abs(c1 - 0.999) < 1e-12
    t, tp = mr.target(np.array([c0, c1]), m, m3)
    assert np.isclose(t[0], c0 - m * np.sin(m)) and tp[0] == 1.0
    assert np.isclose(t[1], np.cos(np.arccos(c1) + m))
    _fd_check(x, W, y, S, m, m3, h=1e-7)


def test_zero_feature_row():
    """A zero row: its norm is clamped to eps (c = 0 on every column), rowcoef is 0, and the gradient is the exact one of
    c = x.w / (eps |w|) -- checked with steps far below eps."""
    S, m, m3 = 8.0, 0.5, 0.0
    rng = np.random.default_rng(5)
    x = rng.normal(size=(3, 4))
    x[1] = 0.0
    W = rng.normal(size=(4, 5))
    y = np.array([0, 1, 4])
    s = x @ W
    xn, wn = np.sqrt((x * x).sum(1)), np.sqrt((W * W).sum(0))
    f, rows, G, rc = mr.kernel_ref(s, xn, wn, y, S, m, m3, 1.0 / 3)
    assert rc[1] == 0.0 and np.isfinite(G).all() and np.isfinite(rows).all()
    assert np.allclose(f[1], [S * mr.target(0.0, m, m3)[0] if j == 1 else 0.0 for j in range(5)])
    loss, _, dx, dW = mr.head_fwd_bwd(x, W, y, S, m, m3)
    for k in range(4):
        h = 1e-17
        xp, xm = x.copy(), x.copy()
        xp[1, k], xm[1, k] = h, -h
        fd = (mr.loss_only(xp, W, y, S, m, m3) - mr.loss_only(xm, W, y, S, m, m3)) / (2 * h)
        assert abs(fd - dx[1, k]) <= 1e-6 * np.abs(dx[1]).max(), (k, fd, dx[1, k])
    _fd_check(x, W, y, S, m, m3, rows=[0, 2])


def test_out_of_range_label_gives_a_nan_row():
    s = np.ones((2, 8))
    f, rows, G, rc = mr.kernel_ref(s, np.ones(2), np.ones(6), [1, 6], 64.0, 0.5, 0.0, 0.5, c=6)
    assert np.isfinite(rows[0]) and np.isnan(rows[1]) and np.isnan(G[1, :6]).all() and (G[:, 6:] == 0).all()


@pytest.mark.parametrize('name,cls,head,preset,labels_in_forward', [
    ('SphereNet-ArcFace', 'SphereNetAdditiveMargin', 'arcface', (64.0, 0.5, 0.0), True),
    ('SphereNet-CosFace', 'SphereNetAdditiveMargin', 'cosface', (64.0, 0.0, 0.35), True),
    ('ResNet-50-arcface', 'ResNet', 'arcface', (64.0, 0.5, 0.0), False),
    ('ResNet-50-cosface', 'ResNet', 'cosface', (64.0, 0.0, 0.35), False),
])
def test_factory_names_and_presets(name, cls, head, preset, labels_in_forward):
    from tf_face_toolbox_amd import net_select
    net = net_select(name, 'NCHW', 5e-4)
    assert type(net).__name__ == cls and net.head == head
    assert (net.margin_scale, net.margin, net.margin_cos) == preset
    assert net.needs_labels == labels_in_forward
    net.set_margin(margin=0.25)
    assert (net.margin_scale, net.margin, net.margin_cos) == (preset[0], 0.25, preset[2])
    with pytest.raises(ValueError):
        net.set_margin(scale=0.0)


def test_margin_kwargs_belong_to_margin_heads():
    from tf_face_toolbox_amd import net_select
    from tf_face_toolbox_amd.nets.resnet import SENet, ResNeXt
    assert SENet(50, head='cosface', margin_cos=0.4).margin_cos == 0.4
    assert ResNeXt(26, head='arcface', scale=32.0).margin_scale == 32.0
    with pytest.raises(ValueError):
        SENet(50, head='softmax', margin=0.5)
    with pytest.raises(ValueError):
        net_select('SphereNet-ASoftmax').set_margin(margin=0.5)


def test_train_flags_default_to_the_preset():
    import train
    f = train.build_parser().parse_args(['--net_name', 'SphereNet-ArcFace'])
    assert (f.margin_scale, f.margin, f.margin_cos) == (None, None, None)
    f = train.build_parser().parse_args(['--margin_scale', '32', '--margin', '0.3', '--margin_cos', '0.1'])
    assert (f.margin_scale, f.margin, f.margin_cos) == (32.0, 0.3, 0.1)


def test_header_declares_and_binding_covers_the_margin_entry():
    from tf_face_toolbox_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'fte.h')).read(), flags=re.S)
    decl = re.search(r'int\s+fte_margin_softmax_fwd_bwd\s*\(([^)]*)\)\s*;', src)
    assert decl, 'fte.h does not declare fte_margin_softmax_fwd_bwd'
    assert len(decl.group(1).split(',')) == 16
    assert 'fte_margin_softmax_fwd_bwd' in _lib.exported_names()
    restype, argtypes = _lib._SIGS['fte_margin_softmax_fwd_bwd']
    assert len(argtypes) == 16
