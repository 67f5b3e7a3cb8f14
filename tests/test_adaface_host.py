"""CPU: the float64 restatement of the AdaFace head (tests/adaface_ref.py) against torch autograd of the formula written
straightforwardly, its reductions to the ArcFace / CosFace restatement (tests/margin_ref.py), the algebra of the running
statistics, and the host surface: symbols, factory names, command line, the state through saver.py and the construction-pass
switch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import adaface_ref as ar
import margin_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('fte_margin_softmax_rows_fwd_bwd', 'fte_adaface_margins')
STATE = ('classifier/adaface/batch_mean', 'classifier/adaface/batch_std')
D = 512


# ------------------------------------------------------------------------------------------------ autograd
def _autograd(x, W, y, S, a=None, b=None, stats=None, m=None, h=None, t_alpha=None):
    """mean loss, dx, dW by torch autograd in float64: normalise, acos, clip, cos, cross-entropy; the margins either given or from
    the detached norms and `stats`"""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.long)
    xn = xt.norm(dim=1)
    if a is None:
        q = xn.detach().clamp(1e-3, 100.0)
        mu = t_alpha * q.mean() + (1 - t_alpha) * stats[0]
        sd = t_alpha * q.std() + (1 - t_alpha) * stats[1]          # torch.std: unbiased, n - 1
        k = ((q - mu) / (sd + 1e-3) * h).clamp(-1, 1)
        at, bt = -m * k, m + m * k
    else:
        at, bt = torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)
    cos = (xt @ Wt) / xn[:, None] / Wt.norm(dim=0)[None, :]
    idx = torch.arange(xt.shape[0])
    theta = torch.acos(cos[idx, yt])
    t = torch.cos(torch.clamp(theta + at, ar.CLIP, np.pi - ar.CLIP)) - bt
    z = S * cos
    z = z.index_put((idx, yt), S * t)
    loss = torch.nn.functional.cross_entropy(z, yt)
    loss.backward()
    return float(loss.detach()), xt.grad.numpy(), Wt.grad.numpy(), (theta + at).detach().numpy()


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


def test_restatement_equals_autograd_inside_the_clip():
    """random x, W at D = 512: theta near pi/2, |a| <= m, far from both clip boundaries (asserted, nothing excluded); the statistics
    are preset near the batch's own so that k spans both of its clip ends"""
    rng = np.random.default_rng(0)
    n, c = 48, 37
    W = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    x = rng.standard_normal((n, D)) * rng.uniform(0.2, 3.0, (n, 1))
    xn = np.sqrt((x * x).sum(1))
    stats = (xn.mean() * 1.02, xn.std(ddof=1) * 0.97)
    for S, m, h, ta in ((64.0, 0.4, 0.333, 0.01), (30.0, 0.5, 2.0, 0.3)):
        a, _, _ = ar.margins(xn, stats, m, h, ta)
        if h > 1:
            assert a.min() == -m and a.max() == m                  # k reaches -1 and 1
        lr, _, dxr, dWr, _ = ar.head_fwd_bwd(x, W, y, stats, S, m, h, ta)
        la, dxa, dWa, thp = _autograd(x, W, y, S, stats=stats, m=m, h=h, t_alpha=ta)
        assert (thp > ar.CLIP + 1e-3).all() and (thp < np.pi - ar.CLIP - 1e-3).all()
        assert abs(lr - la) <= 1e-9 * abs(la)
        assert _rel(dxr, dxa) <= 1e-9 and _rel(dWr, dWa) <= 1e-9, (_rel(dxr, dxa), _rel(dWr, dWa))


def _features(rng, W, y, cosines):
    """rows with the given target cosines (plus an orthogonal remainder), norms in [0.5, 20]"""
    n = len(cosines)
    wy = W[:, y] / np.linalg.norm(W[:, y], axis=0)
    e = rng.standard_normal((W.shape[0], n))
    e -= (e * wy).sum(0) * wy
    e /= np.linalg.norm(e, axis=0)
    return ((cosines * wy + np.sqrt(1 - cosines ** 2) * e) * rng.uniform(0.5, 20.0, n)).T


def clipped_case(rng=None):
    """(x, W, y, a, b): rows 0..3 at least 1e-2 rad below E (theta = 0.05, a <= -0.1), rows 4..7 at least 1e-2 rad above pi - E
    (theta = pi - 0.05, a >= 0.1), rows 8.. inside; the GPU kernel test reuses it"""
    rng = np.random.default_rng(3) if rng is None else rng
    n, c = 16, 24
    W = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    theta = np.concatenate([np.full(4, 0.05), np.full(4, np.pi - 0.05), rng.uniform(0.6, 2.4, n - 8)])
    a = np.concatenate([-rng.uniform(0.1, 0.4, 4), rng.uniform(0.1, 0.4, 4), rng.uniform(-0.4, 0.4, n - 8)])
    b = 0.4 - a
    return _features(rng, W, y, np.cos(theta)), W, y, a, b


def test_restatement_equals_autograd_in_the_clipped_regions():
    x, W, y, a, b = clipped_case()
    S = 64.0
    la, dxa, dWa, thp = _autograd(x, W, y, S, a=a, b=b)
    assert (thp[:4] < ar.CLIP - 1e-2).all() and (thp[4:8] > np.pi - ar.CLIP + 1e-2).all()
    assert (thp[8:] > ar.CLIP + 1e-2).all() and (thp[8:] < np.pi - ar.CLIP - 1e-2).all()
    lr, f, dxr, dWr = ar.rows_head_fwd_bwd(x, W, y, a, b, S)
    assert abs(lr - la) <= 1e-9 * abs(la)
    assert _rel(dxr, dxa) <= 1e-9 and _rel(dWr, dWa) <= 1e-9, (_rel(dxr, dxa), _rel(dWr, dWa))
    # t' = 0 and the constant logit where the clip binds
    cos = np.clip((x @ W) / np.linalg.norm(x, axis=1)[:, None] / np.linalg.norm(W, axis=0)[None, :], -1, 1)
    t, tp = ar.target(cos[np.arange(len(y)), y], a, b)
    assert (tp[:8] == 0).all() and (tp[8:] > 0).all()
    np.testing.assert_allclose(t[:4], np.cos(ar.CLIP) - b[:4], rtol=0, atol=1e-15)
    np.testing.assert_allclose(t[4:8], -np.cos(ar.CLIP) - b[4:8], rtol=0, atol=1e-15)
    np.testing.assert_allclose(f[np.arange(8), y[:8]], S * t[:8], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ reductions
def _spread(seed, n=40, c=50):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    cosines = rng.uniform(-0.97, 0.97, n)
    cosines[:2] = [-0.95, 0.9]
    return _features(rng, W, y, cosines), W, y, cosines


def test_constant_rows_reduce_to_cosface():
    x, W, y, _ = _spread(5)
    n = len(y)
    S, m3 = 64.0, 0.35
    got = ar.rows_head_fwd_bwd(x, W, y, np.zeros(n), np.full(n, m3), S)
    ref = mr.head_fwd_bwd(x, W, y, S, 0.0, m3)
    assert abs(got[0] - ref[0]) <= 1e-12 * abs(ref[0])
    for g, r in zip(got[1:], ref[1:]):
        assert _rel(g, r) <= 1e-11


def test_constant_rows_reduce_to_arcface_where_the_clip_does_not_bind():
    x, W, y, cosines = _spread(6)
    n = len(y)
    S, m = 64.0, 0.5
    s = x @ W
    xn, wn = np.linalg.norm(x, axis=1), np.linalg.norm(W, axis=0)
    fa, la, Ga, ra = ar.kernel_ref(s, xn, wn, y, S, np.full(n, m), np.zeros(n), 1.0 / n)
    fm, lm, Gm, rm = mr.kernel_ref(s, xn, wn, y, S, m, 0.0, 1.0 / n)
    rows = (cosines > -np.cos(m)) & (np.arccos(cosines) + m < np.pi - ar.CLIP)
    assert 0 < rows.sum() < n                                     # both kinds of row are present
    for g, r in ((fa, fm), (Ga, Gm), (la, lm), (ra, rm)):
        assert _rel(g[rows], r[rows]) <= 1e-11
    assert _rel(fa[~rows], fm[~rows]) > 1e-6                      # the fallback branch is ArcFace's alone


# ------------------------------------------------------------------------------------------------ running statistics
def test_ema_algebra_and_margin_identities():
    rng = np.random.default_rng(7)
    xn = rng.uniform(5.0, 40.0, 64)
    xn[:3] = [1e-5, 250.0, 100.0]                                  # clamped to [1e-3, 100]
    q = np.clip(xn, 1e-3, 100.0)
    stats = np.array([20.0, 100.0])
    m, h = 0.4, 0.333
    a, b, (mu, sd) = ar.margins(xn, stats, m, h, 0.01)
    assert (stats == [20.0, 100.0]).all()                          # the restatement never writes into its argument
    assert abs(mu - (0.01 * q.mean() + 0.99 * 20.0)) <= 1e-13 and abs(sd - (0.01 * q.std(ddof=1) + 0.99 * 100.0)) <= 1e-13
    np.testing.assert_allclose(a + b, m, rtol=0, atol=1e-15)       # a_i + b_i = m for every row
    assert (np.abs(a) <= m).all() and (b >= 0).all() and (b <= 2 * m).all()
    assert np.abs(a[3:]).max() < 0.03                              # from (20, 100) the k of every norm in [5, 40] is near 0
    _, _, keep = ar.margins(xn, stats, m, h, 0.0)                  # t_alpha = 0: the statistics stay
    assert keep == (20.0, 100.0)
    _, _, batch = ar.margins(xn, stats, m, h, 1.0)                 # t_alpha = 1: the batch's own
    assert abs(batch[0] - q.mean()) <= 1e-13 and abs(batch[1] - q.std(ddof=1)) <= 1e-13
    a1, b1, _ = ar.margins(xn, batch, m, 5.0, 1.0)                 # large h: k saturates at both ends
    assert a1.min() == -m and a1.max() == m and b1.min() == 0.0 and b1.max() == 2 * m
    # two steps compose: the second step's mean is t (mean_2) + (1 - t) (t mean_1 + (1 - t) mean_0)
    xn2 = rng.uniform(5.0, 40.0, 64)
    _, _, s1 = ar.margins(xn, stats, m, h, 0.25)
    _, _, s2 = ar.margins(xn2, s1, m, h, 0.25)
    assert abs(s2[0] - (0.25 * xn2.mean() + 0.75 * (0.25 * q.mean() + 0.75 * 20.0))) <= 1e-12
    # high norm -> k > 0 -> negative angular margin a, larger additive margin b (the paper's sign convention)
    a2, b2, _ = ar.margins(np.array([10.0, 30.0]), (20.0, 10.0), m, 1.0, 0.0)
    assert a2[0] > 0 > a2[1] and b2[0] < m < b2[1]


def test_construction_pass_switches_the_statistics_off():
    """Singular / DataParallel run their construction-time forward inside _Construction: the nets' update_moving_stats switch is off
    there and back on afterwards; the head passes it to fte_adaface_margins as `update`"""
    from tf_face_toolbox_amd import net_select, Singular
    for name in ('SphereNet-AdaFace', 'ResNet-50-adaface'):
        net = net_select(name)
        assert net.update_moving_stats is True
        with Singular._Construction(net):
            assert net.update_moving_stats is False
        assert net.update_moving_stats is True


# ------------------------------------------------------------------------------------------------ host surface
def test_symbols_are_declared_and_bound():
    from tf_face_toolbox_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fte.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in doc, name


def test_factory_builds_the_new_names():
    from tf_face_toolbox_amd import net_select
    for name in ('SphereNet-AdaFace', 'ResNet-50-adaface'):
        net = net_select(name, 'NCHW', 5e-4)
        assert net.head == 'adaface'
        assert (net.margin_scale, net.margin, net.adaface_h, net.adaface_t_alpha) == (64.0, 0.4, 0.333, 0.01)
        with pytest.raises(ValueError, match='sampled-class head'):
            net.set_sample_rate(0.1, 0)
        net.set_margin(margin=0.3)                                 # train.py --margin sets m
        assert (net.margin_scale, net.margin) == (64.0, 0.3)
        net.set_margin(scale=32.0)
        assert (net.margin_scale, net.margin) == (32.0, 0.3)
        with pytest.raises(ValueError):
            net.set_margin(margin_cos=0.2)
        with pytest.raises(ValueError):
            net.set_margin(margin=-0.1)
    assert net_select('SphereNet-AdaFace').needs_labels is True


def test_train_help_still_runs_and_names_the_head():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--help'], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and '--margin' in r.stdout and 'AdaFace' in r.stdout
    import train as cli
    F = cli.build_parser().parse_args(['--net_name', 'SphereNet-AdaFace', '--model_name', 'm', '--sample_rate', '0.1'])
    with pytest.raises(SystemExit, match='only SphereNet-ArcFace / SphereNet-CosFace have a sampled-class head'):
        cli.sample_flags_check(F)


@pytest.mark.parametrize('name,size,ncls', [('SphereNet-AdaFace', 16, 7), ('ResNet-50-adaface', 32, 11)])
def test_state_travels_through_saver(tmp_path, name, size, ncls):
    from tf_face_toolbox_amd import net_select, saver
    net = net_select(name, 'NCHW'); net.seed = 3
    net.build(size, size, 3, ncls, 'cpu')
    assert [k for k in net.state if k.startswith('classifier/adaface/')] == list(STATE)
    assert not any(k in net.variables for k in STATE)              # not in the arena
    assert float(net.get_variable(STATE[0])) == 20.0 and float(net.get_variable(STATE[1])) == 100.0
    net.adaface_stats.copy_(torch.tensor([23.5, 4.25]))            # the pair the kernel updates is what the names show
    assert float(net.get_variable(STATE[0])) == 23.5 and float(net.get_variable(STATE[1])) == 4.25
    path = saver.save(net, None, 5, str(tmp_path / 'a' / 'a.ckpt'))
    saved = torch.load(path, map_location='cpu')['variables']
    assert all(k in saved for k in STATE) and tuple(saved[STATE[0]].shape) == (1,)
    other = net_select(name, 'NHWC'); other.seed = 4
    other.build(size, size, 3, ncls, 'cpu')
    assert saver.restore(other, path) == 5
    assert other.adaface_stats.tolist() == [23.5, 4.25]
    for k in list(net.variables) + list(net.state):
        assert torch.equal(other.get_variable(k), net.get_variable(k)), k
    # fine-tuning restores the backbone only: the head's statistics stay at their initial values
    ft = net_select(name, 'NCHW'); ft.seed = 5
    ft.build(size, size, 3, ncls, 'cpu')
    assert not any(v.name in STATE for v in ft.pretrained_param())
    saver.restore(ft, path, only=ft.pretrained_param())
    assert ft.adaface_stats.tolist() == [20.0, 100.0]
