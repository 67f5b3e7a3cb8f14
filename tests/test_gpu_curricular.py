"""-m gpu: the CurricularFace head (include/fte.h fte_curricular_t, fte_curricular_softmax_fwd_bwd) -- both kernels against the
float64 restatement (tests/curricular_ref.py) at the shapes their code branches on, the public loss function,
SphereNet-CurricularFace against the oracle backbone composed with the restatement (gradients, training steps, t after each), the
graph nets' head, determinism, the construction pass, checkpoints, the command line and two data-parallel ranks.  Tolerances are
tests/test_gpu_adaface.py's for the same quantities.

THE MASK BOUNDARY.  The logit jumps by S c (t + c - 1) where c_ij crosses u_i, and the device decides the side with an fp32
compare.  The kernel tests form c and u in float64 from the DEVICE's s / xn / wn; the fp32 evaluation differs from that by the
roundings of s (ix rcp(wn)) (at most 3, about 2e-7 |c|) and of u (two products, one sqrt, cosf / sinf: below 5e-7).  BAND = 1e-6:
outside it the device's side of every pair must equal the float64 side, no exceptions; inside it the restatement is given the
device's side (read from f); the pairs inside may number at most 1e-5 of n c -- a condition on the test's inputs, asserted per
case: the seeds below are ones for which it holds.  The whole-net tests run on inputs whose float64 gap exceeds 1e-4 (asserted)
and exclude nothing."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import curricular_ref as cr
from oracle import spherenet as osn
from test_curricular_host import STATE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from util_gpu import dev, host, check_maxabs, check_rell2, kink_of, ws, call, stream
    from tf_face_toolbox_amd import net_select, Singular, _lib, saver
    from tf_face_toolbox_amd.loss import curricularface_loss

D = 512
NAME = 'SphereNet-CurricularFace'
BAND = 1e-6
CAP = 1e-5


def _close(got, ref):
    """t: 1e-5 relative, or 1e-6 absolute near 0"""
    return abs(got - ref) <= max(1e-5 * abs(ref), 1e-6)


# ------------------------------------------------------------------------------------------------ inputs
def _features(rng, W, y, n, a=None):
    """rows whose target cosine spreads over [-0.97, 0.97] plus noise (tests/test_gpu_adaface.py): u_i = cos(theta_y + m) runs from
    below every negative cosine (all of them hard; the rows below -cos m take the easy-margin fallback) to above all of them (none).
    `a`: the target cosines, given"""
    wy = W[:, y] / np.linalg.norm(W[:, y], axis=0)
    if a is None:
        a = rng.uniform(-0.97, 0.97, n)
        a[:min(n, 2)] = [-0.95, 0.9][:min(n, 2)]
    e = rng.standard_normal((D, n))
    e -= (e * wy).sum(0) * wy
    e /= np.linalg.norm(e, axis=0)
    x = (a * wy + np.sqrt(1 - a * a) * e) * rng.uniform(0.5, 20.0, n)
    return x.T.astype(np.float32)


def _products(x, W, c):
    """(s [n, ldp], xn [n], wn [ldp]) on the GPU: s = x @ W by the library's product, the norms by its kernels"""
    n, ldp = x.shape[0], W.shape[1]
    xd, Wd = dev(x), dev(W)
    s = torch.empty(n, ldp, dtype=torch.float32, device='cuda')
    xn = torch.empty(n, dtype=torch.float32, device='cuda')
    wn = torch.empty(ldp, dtype=torch.float32, device='cuda')
    w_, wb = ws(_lib.query('fte_gemm_ws_bytes', n, ldp, D))
    call('fte_gemm_nn', xd, Wd, None, s, n, ldp, D, w_, wb, stream())
    call('fte_row_norms', xd, xn, n, D, D, stream())
    call('fte_col_norms', Wd, wn, D, c, ldp, stream())
    return s, xn, wn


_RAW = {}


def _raw(n, c, seed):
    """made once per (n, c, seed) and shared: the tests only read it"""
    key = (n, c, seed)
    if key not in _RAW:
        rng = np.random.default_rng(seed)
        ldp = (c + 127) // 128 * 128
        W = np.zeros((D, ldp), np.float32)
        W[:, :c] = rng.standard_normal((D, c), dtype=np.float32)
        y = rng.integers(0, c, n)
        y[0] = 0
        y[-1] = c - 1
        s, xn, wn = _products(_features(rng, W, y, n), W, c)
        _RAW.clear()                                                # one case at a time stays on the device
        _RAW[key] = (s, xn, wn, dev(y, torch.int32))
    return _RAW[key]


# ------------------------------------------------------------------------------------------------ fte_curricular_t
def _t(s, xn, wn, labels, alpha, update, t0, c):
    n, ld = s.shape
    state, used = dev(np.array([t0], np.float32)), torch.full((1,), 7.0, device='cuda')
    call('fte_curricular_t', s, xn, wn, labels, alpha, update, state, used, n, c, ld, stream())
    torch.cuda.synchronize()
    return state, used


def _cy(s, xn, wn, labels, c):
    y = host(labels).astype(int)
    return cr.cosines(host(s), host(xn), host(wn), c)[np.arange(len(y)), np.clip(y, 0, c - 1)], (y >= 0) & (y < c)


@pytest.mark.parametrize('n', [1, 7, 257, 512])
def test_t_against_the_restatement(n):
    c = 1000
    s, xn, wn, labels = _raw(n, c, seed=100 + n)
    cy, valid = _cy(s, xn, wn, labels, c)
    for t0, alpha in ((0.0, 0.01), (0.35, 0.01), (0.35, 1.0), (-0.2, 0.3), (0.35, 0.0)):
        want = cr.t_update(np.float32(t0), cy, alpha)
        state, used = _t(s, xn, wn, labels, alpha, 1, t0, c)
        what = 'n=%d t0=%g alpha=%g' % (n, t0, alpha)
        print(what, 'got', float(state), 'want', want)
        assert _close(float(state), want), (what, float(state), want)
        assert torch.equal(state, used), what                       # the logits are made with the value that is stored
        # update = 0: the stored t is used as it stands and not written
        state0, used0 = _t(s, xn, wn, labels, alpha, 0, t0, c)
        assert float(state0) == float(np.float32(t0)) and torch.equal(state0, used0), what


def test_t_leaves_out_bad_labels_and_keeps_the_state_when_none_is_valid():
    n, c = 257, 1000
    s, xn, wn, labels = _raw(n, c, seed=100 + n)
    bad = labels.clone()
    bad[5] = c
    cy, valid = _cy(s, xn, wn, bad, c)
    assert valid.sum() == n - 1
    state, used = _t(s, xn, wn, bad, 0.5, 1, 0.35, c)
    want = cr.t_update(np.float32(0.35), cy, 0.5, valid)
    assert _close(float(state), want) and torch.equal(state, used)
    bad[6] = -1
    cy, valid = _cy(s, xn, wn, bad, c)
    state, _ = _t(s, xn, wn, bad, 0.5, 1, 0.35, c)
    assert _close(float(state), cr.t_update(np.float32(0.35), cy, 0.5, valid))
    none = torch.full_like(labels, c + 3)
    none[::2] = -7
    state, used = _t(s, xn, wn, none, 0.5, 1, 0.35, c)
    assert float(state) == float(np.float32(0.35)) and float(used) == float(np.float32(0.35))


def test_t_repeats_bit_for_bit():
    s, xn, wn, labels = _raw(512, 1000, seed=612)
    runs = [_t(s, xn, wn, labels, 0.01, 1, 0.35, 1000) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])


def test_t_sees_the_bits_of_the_main_kernel():
    """alpha = 1 on one row: t is that row's c_iy as the main kernel forms it; with m = 0 the main kernel's target logit is S c_iy"""
    s, xn, wn, labels = _raw(7, 1000, seed=107)
    for i in range(7):
        state, _ = _t(s[i:i + 1], xn[i:i + 1], wn, labels[i:i + 1], 1.0, 1, 0.0, 1000)
        f, _, _, _ = _kernel(s[i:i + 1].contiguous(), xn[i:i + 1], wn, labels[i:i + 1], 1000, 1.0, 0.0, 0.0, 1.0)
        assert float(f[0, int(labels[i])]) == float(state), i


def test_t_invalid_arguments_write_nothing():
    s, xn, wn, labels = _raw(7, 1000, seed=107)
    ld = s.shape[1]
    state, used = dev(np.array([0.35], np.float32)), torch.full((1,), 7.0, device='cuda')
    ok = dict(s=s, xn=xn, wn=wn, labels=labels, alpha=0.01, state=state, used=used, n=7, c=1000, ld=ld)
    for bad in (dict(s=None), dict(xn=None), dict(wn=None), dict(labels=None), dict(state=None), dict(used=None), dict(n=0), dict(n=-1),
                dict(c=0), dict(ld=999), dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=float('nan'))):
        k = dict(ok, **bad)
        with pytest.raises(_lib.FteError):
            call('fte_curricular_t', k['s'], k['xn'], k['wn'], k['labels'], k['alpha'], 1, k['state'], k['used'], k['n'], k['c'], k['ld'],
                 stream())
    torch.cuda.synchronize()
    assert float(state) == float(np.float32(0.35)) and float(used) == 7.0


# ------------------------------------------------------------------------------------------------ fte_curricular_softmax_fwd_bwd
def _kernel(s, xn, wn, labels, c, S, m, t, gs, with_f=True):
    n, ld = s.shape
    f = torch.full((n, ld), 7.0, device='cuda') if with_f else None
    G = torch.full((n, ld), 7.0, device='cuda')
    rows = torch.empty(n, device='cuda')
    rc = torch.empty(n, device='cuda')
    call('fte_curricular_softmax_fwd_bwd', s, xn, wn, labels, S, m, dev(np.array([t], np.float32)), f, rows, G, rc, n, c, ld, gs, stream())
    torch.cuda.synchronize()
    return f, rows, G, rc


def _sides(f, sh, xnh, wnh, y, c, S, m, t, what):
    """The mask the restatement is to use: the float64 side outside BAND -- where the device's side, read from f, must agree -- and
    the device's side inside it.  Asserts the cap on the pairs inside."""
    t = float(np.float32(t))
    n = sh.shape[0]
    cos = cr.cosines(sh, xnh, wnh, c)
    gap = cr.boundary_gap(sh, xnh, wnh, y, m, c)                    # inf on target columns and bad rows
    live = np.isfinite(gap)
    yc = np.clip(y, 0, c - 1)
    hard64 = live & (cos > cr.threshold(cos[np.arange(n), yc], m)[:, None])
    zs, zh = S * cos, S * cos * (t + cos)
    readable = live & (np.abs(zs - zh) > 1e-3)                      # where f tells the two logits apart
    hard_dev = np.abs(f[:, :c] - zh) < np.abs(f[:, :c] - zs)
    band = live & (gap <= BAND)
    print(what, 'pairs inside the band: %d of %d (cap %g), nearest %.2e, hard %d' % (band.sum(), n * c, CAP * n * c, gap.min(), hard64.sum()))
    assert band.sum() <= CAP * n * c, what
    wrong = readable & ~band & (hard_dev != hard64)
    assert not wrong.any(), (what, 'the device took the other side outside the band', np.argwhere(wrong)[:5], gap[wrong][:5])
    assert not (band & ~readable).any(), what                       # (a pair inside the band at c = 0 or t + c = 1: none here)
    return np.where(band, hard_dev, hard64), cos


def _check_head(got, s, xn, wn, labels, c, S, m, t, gs, what):
    """the kernel's (f, loss_rows, G, rowcoef) against the restatement on the same s / xn / wn / t"""
    f, rows, G, rc = got
    sh, xnh, wnh = host(s), host(xn), host(wn)
    y = host(labels).astype(int)
    n, ld = sh.shape
    hard, cos = _sides(host(f), sh, xnh, wnh, y, c, S, m, t, what)
    t32 = float(np.float32(t))
    fr, lr, Gr, rcr = cr.kernel_ref(sh, xnh, wnh, y, S, m, t32, gs, c=c, hard=hard)
    ok = np.isfinite(lr)
    print(what, 'f err', np.abs(host(f)[ok] - fr[ok]).max(), 'of', np.abs(fr[ok]).max())
    check_maxabs(host(f)[ok], fr[ok], what=what + ' f')
    assert (host(f)[:, c:] == 0).all(), what
    print(what, 'G err', np.abs(host(G)[ok] - Gr[ok]).max(), 'of', np.abs(Gr[ok]).max(), 'loss err', np.abs(host(rows)[ok] - lr[ok]).max())
    check_maxabs(host(G)[ok], Gr[ok], what=what + ' G')
    check_rell2(host(G)[ok], Gr[ok], what=what + ' G')
    assert (host(G)[:, c:ld] == 0).all(), what + ': padding columns'
    lg = host(rows)[ok]
    assert np.all(np.abs(lg - lr[ok]) <= 2e-5 * np.maximum(1.0, np.abs(lr[ok]))), (what, np.abs(lg - lr[ok]).max())
    # rowcoef is a sum of terms of both signs: judge its error against the sum of their magnitudes (tests/test_gpu_margin.py)
    idx, yc = np.arange(n), np.clip(y, 0, c - 1)
    xv = np.maximum(xnh, 1e-12)
    z = np.where(np.isfinite(fr[:, :c]), fr[:, :c], 0)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    _, tp = cr.target(cos[idx, yc], m, 0.0)
    wgt = p * np.where(hard, np.abs(t32 + 2 * cos), 1.0)
    wgt[idx, yc] = (p[idx, yc] + 1) * tp
    mag = abs(gs) * S * (wgt * np.abs(cos)).sum(1) / xv ** 2
    assert np.all(np.abs(host(rc)[ok] - rcr[ok]) <= 2e-5 * mag[ok]), (what, 'rowcoef', np.abs(host(rc)[ok] - rcr[ok]) / mag[ok])
    return hard


@pytest.mark.parametrize('n,c', [(1, 10), (7, 1000), (64, 1001), (64, 4100), (512, 10575), (64, 85742)])
def test_kernel_against_the_restatement(n, c):
    """ld % 4 == 0 throughout (the vector path); c = 1001 / 10575 / 85742 not a multiple of 4 under an aligned ld; c < 1024 one trip
    of the unrolled loop, c > 4096 several; n = 1 and n = 512.  The seeds are ones for which the pairs inside the band stay under
    the cap (the float64 restatement alone counts 0 .. 1e-6 of n c on them)."""
    s, xn, wn, labels = _raw(n, c, seed=n * 7 + c)
    assert s.shape[1] % 4 == 0
    for S in (64.0, 30.0):
        for t in (0.0, 0.35):
            hard = _check_head(_kernel(s, xn, wn, labels, c, S, 0.5, t, 1.0 / n), s, xn, wn, labels, c, S, 0.5, t, 1.0 / n,
                               'n=%d c=%d S=%g t=%g' % (n, c, S, t))
    if n >= 64:
        per_row = hard.sum(1)
        assert (per_row == 0).any() and (per_row >= c - 2).any() and ((per_row > 0) & (per_row < c - 2)).any()      # all three kinds of row


@pytest.mark.parametrize('n', [1, 7])
def test_unaligned_ld_takes_the_scalar_path(n):
    c = 1000
    s, xn, wn, labels = _raw(n, c, seed=100 + n)
    ld = c + 3
    su = torch.zeros(n, ld, device='cuda')
    su[:, :c] = s[:, :c]
    for t in (0.0, 0.35):
        _check_head(_kernel(su, xn, wn, labels, c, 64.0, 0.5, t, 1.0 / n), su, xn, wn, labels, c, 64.0, 0.5, t, 1.0 / n,
                    'ld=%d n=%d t=%g' % (ld, n, t))


def test_bad_labels_give_nan_rows_and_leave_their_neighbours_alone():
    n, c = 7, 1000
    s, xn, wn, labels = _raw(n, c, seed=100 + n)
    want = _kernel(s, xn, wn, labels, c, 64.0, 0.5, 0.35, 1.0 / n)
    bad = labels.clone()
    bad[3] = c
    bad[5] = -1
    f, rows, G, rc = _kernel(s, xn, wn, bad, c, 64.0, 0.5, 0.35, 1.0 / n)
    for i in (3, 5):
        assert np.isnan(float(rows[i])) and np.isnan(float(rc[i])), i
        assert torch.isnan(G[i, :c]).all() and torch.isnan(f[i, :c]).all(), i
    assert (G[:, c:] == 0).all() and (f[:, c:] == 0).all()                  # padding: 0, on the NaN rows too
    good = [0, 1, 2, 4, 6]
    for u, v in zip((f, rows, G, rc), want):
        assert torch.equal(u[good], v[good])                                # bit for bit


def test_f_null_gives_the_same_G_and_repeats_bit_for_bit():
    n, c = 64, 4100
    s, xn, wn, labels = _raw(n, c, seed=n * 7 + c)
    r1 = _kernel(s, xn, wn, labels, c, 64.0, 0.5, 0.35, 1.0 / n, with_f=True)
    r2 = _kernel(s, xn, wn, labels, c, 64.0, 0.5, 0.35, 1.0 / n, with_f=False)
    r3 = _kernel(s, xn, wn, labels, c, 64.0, 0.5, 0.35, 1.0 / n, with_f=False)
    for i in (1, 2, 3):
        assert torch.equal(r1[i], r2[i]) and torch.equal(r2[i], r3[i])


def test_rows_without_a_hard_column_reproduce_the_arcface_kernel():
    n, c = 64, 4100
    s, xn, wn, labels = _raw(n, c, seed=n * 7 + c)
    ld = s.shape[1]
    y = host(labels).astype(int)
    cos = cr.cosines(host(s), host(xn), host(wn), c)
    u = cr.threshold(cos[np.arange(n), y], 0.5)
    neg = cos.copy()
    neg[np.arange(n), y] = -np.inf
    sel = neg.max(1) < u - BAND                                     # no hard column, and none within the band of becoming one
    assert 4 <= sel.sum() < n
    got = _kernel(s, xn, wn, labels, c, 64.0, 0.5, 0.35, 1.0 / n)
    f, G = torch.empty_like(s), torch.empty_like(s)
    rows, rc = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
    call('fte_margin_softmax_fwd_bwd', s, xn, wn, labels, 64.0, 0.5, 0.0, f, rows, G, rc, n, c, ld, 1.0 / n, stream())
    torch.cuda.synchronize()
    ref = (f, rows, G, rc)
    check_maxabs(host(got[0])[sel], host(ref[0])[sel], what='f')
    check_maxabs(host(got[2])[sel], host(ref[2])[sel], what='G')
    lg, lr = host(got[1])[sel], host(ref[1])[sel]
    assert np.all(np.abs(lg - lr) <= 2e-5 * np.maximum(1.0, np.abs(lr)))
    mag = (np.abs(host(ref[2]) * host(s)).sum(1) / host(xn) ** 2)[sel]      # rowcoef: against the sum of its terms' magnitudes
    assert np.all(np.abs(host(got[3])[sel] - host(ref[3])[sel]) <= 2e-5 * mag)
    # the target column is ArcFace's on EVERY row, at the same tolerance (two kernels: the compiler is free to contract
    # c cos m - sin_t sin m differently in each, so the last bit may differ)
    idx = np.arange(n)
    check_maxabs(host(got[0])[idx, y], host(ref[0])[idx, y], what='target column')


def test_kernel_invalid_arguments():
    s, xn, wn, labels = _raw(7, 1000, seed=107)
    n, c, ld = 7, 1000, s.shape[1]
    G, rows, rc, t = torch.full_like(s, 7.0), torch.full((n,), 7.0, device='cuda'), torch.full((n,), 7.0, device='cuda'), dev(np.zeros(1, np.float32))
    for S, m, c_, ld_, n_ in ((0.0, 0.5, c, ld, n), (-1.0, 0.5, c, ld, n), (float('nan'), 0.5, c, ld, n), (64.0, -0.1, c, ld, n),
                              (64.0, 1.5708, c, ld, n), (64.0, float('nan'), c, ld, n), (64.0, 0.5, 0, ld, n), (64.0, 0.5, c, 999, n),
                              (64.0, 0.5, c, ld, 0)):
        with pytest.raises(_lib.FteError):
            call('fte_curricular_softmax_fwd_bwd', s, xn, wn, labels, S, m, t, None, rows, G, rc, n_, c_, ld_, 0.25, stream())
    for miss in range(8):
        ptrs = [s, xn, wn, labels, t, rows, G, rc]
        ptrs[miss] = None
        with pytest.raises(_lib.FteError):
            call('fte_curricular_softmax_fwd_bwd', ptrs[0], ptrs[1], ptrs[2], ptrs[3], 64.0, 0.5, ptrs[4], None, ptrs[5], ptrs[6], ptrs[7],
                 n, c, ld, 0.25, stream())
    torch.cuda.synchronize()
    assert (G == 7.0).all() and (rows == 7.0).all() and (rc == 7.0).all()   # nothing written
    call('fte_curricular_softmax_fwd_bwd', s, xn, wn, labels, 64.0, 0.0, t, None, rows, G, rc, n, c, ld, 0.25, stream())      # m = 0 is valid
    torch.cuda.synchronize()
    assert torch.isfinite(rows).all()


# ------------------------------------------------------------------------------------------------ loss.curricularface_loss
@pytest.mark.parametrize('update', [True, False])
def test_public_loss_function(update):
    rng = np.random.default_rng(17)
    n, c, ld = 64, 1000, 1024
    W = np.zeros((D, ld), np.float32)
    W[:, :c] = rng.standard_normal((D, c))
    y = rng.integers(0, c, n)
    # This function returns no logits to read the device's side of the mask from, so its inputs keep u_i = cos(theta_y + 0.5) clear of
    # the negatives' cosines (|c_ij| < 0.25 at D = 512): target cosines in [0.8, 0.97] (u > 0.39: no hard column) and in
    # [-0.97, 0.15] (u < -0.35: every negative hard, the fallback rows among them).  The kernel tests cover the mixed rows.
    a = np.where(np.arange(n) % 2 == 0, rng.uniform(0.8, 0.97, n), rng.uniform(-0.97, 0.15, n))
    a[1] = -0.95
    x = _features(rng, W, y, n, a)
    x64, W64 = x.astype(np.float64), W[:, :c].astype(np.float64)
    assert cr.head_gap(x64, W64, y, 0.5) > 1e-4                     # nothing near the jump: nothing excluded
    t = dev(np.array([0.35], np.float32))
    loss, dx, dW = curricularface_loss(dev(x), dev(W), dev(y, torch.int32), t, 64.0, 0.5, 0.05, update=update, num_classes=c)
    torch.cuda.synchronize()
    lr, _, dxr, dWr, new = cr.head_fwd_bwd(x64, W64, y, np.float32(0.35), 64.0, 0.5, 0.05, update)
    assert abs(float(loss) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(loss), lr)
    check_rell2(host(dx), dxr, what='dfeatures')
    check_rell2(host(dW)[:, :c], dWr, what='dweights')
    assert (host(dW)[:, c:] == 0).all()
    if update:                                                      # moved in place
        assert _close(float(t), new) and float(t) != float(np.float32(0.35)), (float(t), new)
    else:
        assert float(t) == float(np.float32(0.35)) and new == float(np.float32(0.35))
    with pytest.raises(TypeError):
        curricularface_loss(dev(x), dev(W), dev(y, torch.int32), torch.zeros(2, device='cuda'))


# ------------------------------------------------------------------------------------------------ SphereNet-CurricularFace
def _setup(n, h, w, ch, ncls, seed=21, name=NAME):
    p = osn.perturb_params(osn.init_params(seed, ch, ncls, h, w), seed + 1)
    rng = np.random.default_rng(seed + 2)
    x = rng.uniform(-1, 1, (n, h, w, ch)); y = rng.integers(0, ncls, n)
    net = net_select(name, 'NCHW', 5e-4)
    net.build(h, w, ch, ncls, 'cuda')
    net.load_params(p)
    return net, p, x, y


def _hyper(net):
    return net.margin_scale, net.margin, net.curricular_alpha


def _tof(net):
    return float(net.get_variable(STATE[0]))


@pytest.mark.parametrize('n,h,w,ch,ncls,t0,m', [(4, 32, 32, 3, 10, 0.0, None), (4, 32, 32, 3, 10, 0.35, 0.05), (2, 112, 112, 1, 10575, 0.35, None)])
def test_spherenet_forward_loss_and_every_gradient(n, h, w, ch, ncls, t0, m):
    """m = None: the preset 0.5 -- on a fresh net every target cosine is near 0, u near cos(pi/2 + 0.5), and EVERY negative is hard;
    m = 0.05 puts u just below the target cosine, among the negatives: rows with both kinds of column"""
    net, p, x, y = _setup(n, h, w, ch, ncls)
    if m is not None:
        net.set_margin(margin=m)
    net.curricular_alpha = 0.2                                      # t moves visibly in one step
    net.set_variable(STATE[0], [t0])
    xd, yd = dev(x), dev(y, torch.int32)
    net.tower_scale = 1.0
    logits = net.forward(xd, yd, num_classes=ncls, is_training=True)
    losses, names, others = net.loss_function('TOWER', yd, **logits)
    net.backward()
    torch.cuda.synchronize()
    losses_ref, g_ref, ex = cr.loss_and_grads(p, x, y, np.float32(t0), *_hyper(net), 5e-4, 'NCHW', kink=kink_of(net))
    print('boundary gap %.3e, t %g -> %g' % (ex['gap'], t0, ex['t']))
    assert ex['gap'] > 1e-4                                         # nothing near the jump: nothing excluded
    wc = p['classifier/fc_classifier/weights']
    cos = cr.cosines(ex['embedding'] @ wc, np.linalg.norm(ex['embedding'], axis=1), np.linalg.norm(wc, axis=0))
    hard = cos > cr.threshold(cos[np.arange(n), y], net.margin)[:, None]
    hard[np.arange(n), y] = False
    assert hard.any()
    if m is not None:
        assert not hard.all(1).any() and (~hard).sum() > n          # easy negatives too
    assert names == ['cross_entropy', 'reg_loss'] and not others
    check_maxabs(host(net.emb), ex['embedding'], what='embedding')
    check_maxabs(host(logits['logits']), ex['logits'], what='logits')
    assert abs(float(losses[0]) - losses_ref[0]) <= 1e-5 * max(1, abs(losses_ref[0])), (float(losses[0]), losses_ref[0])
    assert abs(float(losses[1]) - losses_ref[1]) <= 1e-5 * max(1, abs(losses_ref[1]))
    for k in p:
        data_grad = g_ref[k] - (5e-4 * p[k] if k.endswith('/weights') else 0)
        check_rell2(host(net.get_variable(k, net.grads)), data_grad, what='grad ' + k)
    assert _close(_tof(net), ex['t']) and _tof(net) != float(np.float32(t0)), (_tof(net), ex['t'])


def test_three_training_steps_match_oracle():
    n, h, w, ch, ncls = 4, 32, 32, 3, 10
    net, p, x, y = _setup(n, h, w, ch, ncls, seed=31)
    net.curricular_alpha = 0.2
    inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': ncls, 'num_examples': n}
    step, losses, names, others = Singular(net, 0.05, 'Momentum')(inputs)
    torch.cuda.synchronize()
    assert _tof(net) == 0.0                                         # the construction pass moved nothing
    slots = osn.zero_slots(p)
    t = 0.0
    for i in range(3):
        step()
        p, slots, t, l_ref, gap = cr.train_step(p, slots, t, x, y, 0.05, *_hyper(net), kink=kink_of(net))
        assert gap > 1e-4, (i, gap)
        assert abs(float(losses[0]) - l_ref[0]) <= 1e-5 * max(1, abs(l_ref[0])), (i, float(losses[0]), l_ref)
        assert _close(_tof(net), t), (i, _tof(net), t)
    assert abs(t) > 1e-3
    for k in p:
        check_maxabs(host(net.get_variable(k)), p[k], 2e-5, what='weights after 3 steps ' + k)


def test_construction_pass_leaves_t_at_zero():
    net, p, x, y = _setup(4, 32, 32, 3, 10, seed=33)
    inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': 10, 'num_examples': 4}
    step, losses, _, _ = Singular(net, 0.05, 'Momentum')(inputs)
    torch.cuda.synchronize()
    assert _tof(net) == 0.0 and np.isfinite(float(losses[0]))
    assert net.update_moving_stats is True
    step()
    torch.cuda.synchronize()
    assert _tof(net) != 0.0


def test_two_identical_runs_are_bit_identical():
    outs = []
    for _ in range(2):
        net, p, x, y = _setup(16, 112, 112, 3, 1000, seed=41)
        inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': 1000, 'num_examples': 16}
        step, losses, _, _ = Singular(net, 0.05, 'Momentum')(inputs)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        outs.append((net.params.clone(), net.grads.clone(), net.cf_state.clone()))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    assert float(outs[0][1].abs().max()) > 0 and float(outs[0][2]) != 0.0


# ------------------------------------------------------------------------------------------------ graph nets
def test_graph_net_head_parity():
    """the CurricularFace head of the BN nets on the classifier's own input (the dropped-out pooled features) and weights: loss, the
    classifier-weight gradient, the gradient into the features and t (tests/test_gpu_adaface.py)"""
    from tf_face_toolbox_amd.nets.resnet import ResNet
    n, h, w, ncls = 8, 64, 64, 10
    net = ResNet(num_layers=26, data_format='NCHW', weight_decay=5e-4, head='curricularface')
    assert net.head == 'curricularface' and _hyper(net) == (64.0, 0.5, 0.01)
    rng = np.random.default_rng(51)
    xd, yd = dev(rng.uniform(-1, 1, (n, h, w, 3))), dev(rng.integers(0, ncls, n), torch.int32)
    net.build(h, w, 3, ncls, 'cuda')
    wname = 'classifier/fc_classifier/weights'
    inp = net.plan[-1].inp                                          # the classifier's input
    fdim = net.shapes[inp][0]
    net.set_variable(wname, torch.tensor(rng.standard_normal((fdim, ncls)) * 0.05, dtype=torch.float32))
    net.tower_scale = 1.0
    net.curricular_alpha = 0.2
    # a construction-style pass first (update_moving_stats off): it must move nothing
    net.update_moving_stats = False
    logits = net.forward(xd, num_classes=ncls, is_training=True)
    net.loss_function('TOWER', yd, **logits)
    torch.cuda.synchronize()
    assert _tof(net) == 0.0
    net.update_moving_stats = True
    net.set_variable(STATE[0], [0.35])
    logits = net.forward(xd, num_classes=ncls, is_training=True)
    losses, names, _ = net.loss_function('TOWER', yd, **logits)
    stages = net.backward_stages()
    stages[0]()                                               # the classifier bucket
    torch.cuda.synchronize()
    feat = host(net.t[inp])
    gin = host(net._grad[inp])
    gw = host(net.get_variable(wname, net.grads))
    W = host(net.get_variable(wname))
    y = host(yd).astype(int)
    gap = cr.head_gap(feat, W, y, net.margin)
    print('boundary gap %.3e' % gap)
    assert gap > 1e-4
    lr, fr, dxr, dWr, new = cr.head_fwd_bwd(feat, W, y, np.float32(0.35), *_hyper(net))
    assert names[0] == 'cross_entropy' and abs(float(losses[0]) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(losses[0]), lr)
    check_rell2(gw, dWr, what='classifier weight gradient')
    check_rell2(gin, dxr, what='gradient into the features')
    assert _close(_tof(net), new) and _tof(net) != float(np.float32(0.35)), (_tof(net), new)
    for st in stages[1:]:
        st()
    torch.cuda.synchronize()
    assert torch.isfinite(net.grads).all()


# ------------------------------------------------------------------------------------------------ checkpoints, CLI, two ranks
def test_checkpoint_round_trip_resumes_bit_for_bit(tmp_path):
    n, h, w, ch, ncls = 4, 32, 32, 3, 10

    def start():
        net, p, x, y = _setup(n, h, w, ch, ncls, seed=61)
        net.curricular_alpha = 0.2                                  # t moves visibly in two steps
        inputs = {'images': dev(x), 'labels': dev(y, torch.int32), 'num_classes': ncls, 'num_examples': n}
        model = Singular(net, 0.05, 'Momentum')
        step, losses, _, _ = model(inputs)
        return net, model, step, losses
    net, model, step, losses = start()
    step(); step()
    torch.cuda.synchronize()
    path = saver.save(net, model._opt.slots, model.global_step, str(tmp_path / 'c' / 'c.ckpt'))
    saved_t = _tof(net)
    assert saved_t != 0.0
    step()
    torch.cuda.synchronize()
    want = (net.params.clone(), net.cf_state.clone(), float(losses[0]))
    net2, model2, step2, losses2 = start()
    assert _tof(net2) == 0.0
    model2.global_step = saver.restore(net2, path, optimizer=model2._opt)
    assert model2.global_step == 2 and _tof(net2) == saved_t
    step2()
    torch.cuda.synchronize()
    assert torch.equal(net2.params, want[0]) and torch.equal(net2.cf_state, want[1]) and float(losses2[0]) == want[2]


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def test_train_synthetic_save_evaluate(tmp_path):
    from PIL import Image
    from scipy.io import loadmat
    rng = np.random.default_rng(0)
    lines = []
    for i in range(6):
        path = str(tmp_path / ('im%d.png' % i))
        Image.fromarray(rng.integers(0, 255, (32, 32, 3), dtype=np.uint8)).save(path)
        lines.append('%s %d' % (path, i % 3))
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    out = _run([os.path.join(ROOT, 'train.py'), '--net_name', NAME, '--model_name', 'm', '--synthetic', '1',
                '--synthetic_classes', '10', '--input_height', '32', '--input_width', '32', '--batch_size', '8', '--num_gpus', '1',
                '--init_lr', '0.01', '--lr_decay_epoch', '2', '--max_epoches', '50', '--display_interval', '1',
                '--save_interval', '1000', '--max_steps', '3', '--margin', '0.3', '--margin_scale', '32'], str(tmp_path))
    assert 'Loss #0: cross_entropy' in out and 'Model has been saved in Iteration 2' in out
    ckpt = str(tmp_path / 'models' / (NAME + '_m') / (NAME + '_m.ckpt-3'))
    saved = torch.load(ckpt, map_location='cpu')['variables']
    assert STATE[0] in saved and tuple(saved[STATE[0]].shape) == (1,) and float(saved[STATE[0]]) != 0.0
    # the extractor neither touches nor needs t: it also runs on a checkpoint that lacks it
    state = torch.load(ckpt, map_location='cpu')
    del state['variables'][STATE[0]]
    torch.save(state, ckpt)
    out = _run([os.path.join(ROOT, 'evaluate.py'), '--net_name', NAME, '--model_name', 'm', '--fea_name', 'f',
                '--data_list_path', str(tmp_path / 'list.txt'), '--input_height', '32', '--input_width', '32', '--batch_size', '4'],
               str(tmp_path))
    assert 'Totally extracted 6 features.' in out
    m = loadmat(str(tmp_path / 'features' / (NAME + '_m') / 'f_3.mat'))
    assert m['wfea'].shape == (6, 512) and np.isfinite(m['wfea']).all() and np.abs(m['wfea']).max() > 0


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_keep_the_trainable_variables_identical(tmp_path):
    """two DataParallel_margin ranks (tests/dp_worker.py; one GPU: both on it over gloo): the all-reduced gradients keep every
    trainable variable bit-identical across the ranks, the losses are finite, and each rank's t follows its own shard (per-tower
    state, never all-reduced)"""
    n, h, w, ch, ncls, steps = 8, 32, 32, 3, 20, 2
    p = osn.perturb_params(osn.init_params(71, ch, ncls, h, w), 72)
    rng = np.random.default_rng(73)
    x = rng.uniform(-1, 1, (n, h, w, ch)); y = rng.integers(0, ncls, n)
    fix = str(tmp_path / 'fix.npz')
    np.savez(fix, x=x, y=y, ncls=ncls, **{'p:' + k: v for k, v in p.items()})
    out = str(tmp_path / 'out')
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                        '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
                        os.path.join(ROOT, 'tests', 'dp_worker.py'), fix, out, NAME, str(steps)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:]
    r0, r1 = np.load(out + '.rank0.npz'), np.load(out + '.rank1.npz')
    for k in r0.files:
        if k.startswith('w:'):
            np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)
    assert np.isfinite(r0['losses']).all() and np.isfinite(r1['losses']).all() and r0['losses'].shape == (steps, 2)
    ts = [float(r_['s:' + STATE[0]][0]) for r_ in (r0, r1)]
    assert all(np.isfinite(t) and t != 0.0 for t in ts) and ts[0] != ts[1]      # moved, and per tower
