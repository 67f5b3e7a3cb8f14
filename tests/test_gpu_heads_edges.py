"""-m gpu: the loss heads of csrc/kernels.hip (softmax-CE, focal, A-softmax and its norm / coefficient kernels, center loss,
batch-hard triplet) through the C ABI at the shapes their code branches on, against the float64 oracle evaluated on the
float32-rounded inputs.  Tolerances are the project's stated ones (util_gpu.TOL_MAXABS / TOL_RELL2, 1e-5 on a mean loss);
where a bound is this file's own, the reasoning stands next to it.

Which kernel a case reaches is decided in the host launchers by a threshold on one argument (k_softmax_ce: ld <= 2048 ->
softmax_ce_reg_kernel<8>, ld <= 12288 -> <48>, above -> softmax_ce_kernel; k_center_loss: n <= 8192 -> labels staged in LDS,
above -> read from global memory).  The launch profiler (fte_prof_enable) records the MFMA families only, not these launches, so
the cases below sit on both sides of each threshold and rely on it."""
import numpy as np
import pytest
import torch

from oracle import ops

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, dev, host, stream, ws, check_maxabs, check_rell2, TOL_MAXABS, TOL_RELL2

EINVAL, EWORKSPACE = -1, -2
INT_MAX = 2 ** 31 - 1
R2 = np.sqrt(0.5)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _i32(y):
    return torch.tensor(np.asarray(y, np.int64).astype(np.int32), dtype=torch.int32, device='cuda')


def _mean_close(got_rows, ref_mean, what=''):
    got = host(got_rows).mean()
    assert abs(got - ref_mean) <= 1e-5 * max(1.0, abs(ref_mean)), '%s: mean loss %.9g vs %.9g' % (what, got, ref_mean)


# ------------------------------------------------------------------------------------------------------------------------
# softmax cross-entropy
# ------------------------------------------------------------------------------------------------------------------------
def _padded(z, ld, fill=77.0):
    n, c = z.shape
    zp = np.full((n, ld), fill, np.float32)
    zp[:, :c] = z
    return zp


def _sce(zp, y, c, gs):
    n, ld = zp.shape
    rows = torch.full((n,), 5.0, device='cuda')
    d = torch.full((n, ld), 5.0, device='cuda')
    call('fte_softmax_ce_fwd_bwd', dev(zp), _i32(y), rows, d, n, c, ld, gs, stream())
    torch.cuda.synchronize()
    return rows, d


def _sce_check(z, y, ld, gs, what):
    n, c = z.shape
    ref_loss, ref_d = ops.softmax_ce(z.astype(np.float64), y, gs)
    rows, d = _sce(_padded(z, ld), y, c, gs)
    _mean_close(rows, ref_loss, what)
    check_maxabs(host(d)[:, :c], ref_d, TOL_MAXABS, what + ' dlogits')
    check_rell2(host(d)[:, :c], ref_d, TOL_RELL2, what + ' dlogits')
    assert float(d[:, c:].abs().max()) == 0.0 if ld > c else True, what + ': pad columns'
    return rows, d


@pytest.mark.parametrize('full', [True, False])
@pytest.mark.parametrize('ld', [128, 2048, 2176, 12288, 12416])
def test_softmax_ce_on_both_sides_of_each_dispatch_boundary(ld, full):
    c = ld if full else ld - 127
    n = 6
    r = np.random.default_rng(ld + full)
    z = _f32(r.standard_normal((n, c)) * 4)
    y = r.integers(0, c, n); y[0] = 0; y[-1] = c - 1
    _sce_check(z, y, ld, 0.37 / n, 'ld %d c %d' % (ld, c))


def test_softmax_ce_generic_kernel_on_a_large_identity_list():
    n, c, ld = 8, 85742, 85760
    r = np.random.default_rng(85742)
    z = _f32(r.standard_normal((n, c)) * 4)
    y = r.integers(0, c, n); y[0] = 0; y[-1] = c - 1
    _sce_check(z, y, ld, 1.0 / n, 'c 85742')


def test_softmax_ce_three_kernels_are_bit_identical():
    """fte.h: the kernel is chosen by ld alone and the three give bit-identical results for the same [n, c] logits."""
    n, c = 5, 2000
    r = np.random.default_rng(2000)
    z = _f32(r.standard_normal((n, c)) * 4)
    y = r.integers(0, c, n); y[0] = 0; y[-1] = c - 1
    out = [_sce(_padded(z, ld), y, c, 0.37 / n) for ld in (2048, 2176, 12416)]      # <8>, <48>, generic
    for rows, d in out[1:]:
        assert torch.equal(rows, out[0][0])
        assert torch.equal(d[:, :c], out[0][1][:, :c])


@pytest.mark.parametrize('ld', [1024, 2176, 12416])
def test_softmax_ce_logit_ranges(ld):
    n, c = 6, 1000
    r = np.random.default_rng(ld)
    z = r.standard_normal((n, c))
    z[0] = 3.25                                   # equal logits: loss log(c), gradient 1/c - onehot
    z[1] = r.uniform(-80, 80, c)                  # spread +-80
    z[2] = r.uniform(-80, 80, c); z[2, 7] = 80.0; z[2, 8] = -80.0
    z[3, 11] += 1e4; z[4, 11] += 1e4; z[5, 999] += 1e4        # one logit 1e4 above the rest
    y = np.array([5, 0, 8, 11, 12, 0])            # rows 4, 5: the label is one of the others, loss ~1e4
    z = _f32(z)
    rows, d = _sce_check(z, y, ld, 1.0 / n, 'ranges ld %d' % ld)
    got = host(rows)
    assert np.isfinite(got).all()
    m = z.astype(np.float64)
    ref_rows = np.array([-(m[i, y[i]] - m[i].max() - np.log(np.exp(m[i] - m[i].max()).sum())) for i in range(n)])
    check_maxabs(got, ref_rows, TOL_MAXABS, 'loss rows')
    assert abs(got[0] - np.log(c)) <= 1e-5 * np.log(c) and got[4] > 9.9e3 and got[5] > 9.9e3


def _bad_label_layout(n, c, ld):
    y = np.arange(n) * 7 % c
    y[1] = 0; y[2] = c - 1
    bad = {0: -1, 3: c, 5: INT_MAX, n - 1: -7}
    if ld > c + 1:
        bad[6] = c + (ld - c) // 2                # a pad column
    for i, v in bad.items():
        y[i] = v
    return y, np.array(sorted(bad)), np.array([i for i in range(n) if i not in bad])


@pytest.mark.parametrize('c,ld', [(300, 384), (2100, 2176), (12300, 12416), (128, 128)])
def test_softmax_ce_bad_labels_give_nan_rows_and_leave_the_others_alone(c, ld):
    n = 10
    r = np.random.default_rng(c)
    z = _f32(r.standard_normal((n, c)) * 4)
    y, bad, good = _bad_label_layout(n, c, ld)
    rows, d = _sce(_padded(z, ld), y, c, 0.5)
    rows_g, d_g = _sce(_padded(z[good], ld), y[good], c, 0.5)
    assert torch.isnan(rows[bad]).all() and torch.isnan(d[bad][:, :c]).all()
    assert float(d[:, c:].abs().max()) == 0.0 if ld > c else True          # pads of NaN rows too (fte.h)
    assert torch.equal(rows[good], rows_g) and torch.equal(d[good], d_g)
    assert torch.isfinite(rows_g).all()


# ------------------------------------------------------------------------------------------------------------------------
# focal loss, direct
# ------------------------------------------------------------------------------------------------------------------------
def _focal(zp, y, c, gamma, alpha, gs):
    n, ld = zp.shape
    rows = torch.full((n,), 5.0, device='cuda')
    d = torch.full((n, ld), 5.0, device='cuda')
    call('fte_focal_loss_fwd_bwd', dev(zp), _i32(y), rows, d, n, c, ld, gamma, alpha, gs, stream())
    torch.cuda.synchronize()
    return rows, d


def _focal_check(z, y, ld, gamma, alpha, gs, what):
    n, c = z.shape
    ref_loss, ref_d = ops.focal_loss(z.astype(np.float64), y, gamma, alpha, gs)
    assert np.isfinite(ref_d).all() and np.isfinite(ref_loss)
    rows, d = _focal(_padded(z, ld), y, c, gamma, alpha, gs)
    assert torch.isfinite(rows).all() and torch.isfinite(d).all(), what
    _mean_close(rows, ref_loss, what)
    check_maxabs(host(d)[:, :c], ref_d, TOL_MAXABS, what + ' dlogits')
    check_rell2(host(d)[:, :c], ref_d, TOL_RELL2, what + ' dlogits')
    assert float(d[:, c:].abs().max()) == 0.0, what + ': pad columns'


@pytest.mark.parametrize('n,c,ld', [(16, 10, 128), (7, 1000, 1152)])
@pytest.mark.parametrize('gamma', [0.5, 1.0, 2.0])
@pytest.mark.parametrize('alpha', [1.0, 1.5, 2.0, 3.5])
def test_focal_direct(alpha, gamma, n, c, ld):
    r = np.random.default_rng(int(alpha * 10 + gamma * 100) + c)
    z = _f32(r.standard_normal((n, c)) * 3)
    y = r.integers(0, c, n); y[0] = 0; y[-1] = c - 1
    _focal_check(z, y, ld, gamma, alpha, 0.37 / n, 'focal alpha %g gamma %g c %d' % (alpha, gamma, c))


def saturated_focal_batch():
    """c = 10: six ordinary rows, then target logits 20 and 40 above the rest (1 - q below fp32 epsilon) and 20 below (q ~ 0)"""
    r = np.random.default_rng(77)
    n, c = 12, 10
    z = r.standard_normal((n, c)) * 3
    y = r.integers(0, c, n)
    for i, gap in zip(range(6, 12), (20, 20, 40, 40, -20, -20)):
        z[i] = r.standard_normal(c) * 0.5
        rest = np.delete(z[i], y[i])
        z[i, y[i]] = rest.max() + gap if gap > 0 else rest.min() + gap
    return _f32(z), y


@pytest.mark.parametrize('alpha', [1.0, 1.5, 2.0, 3.5])
def test_focal_saturated_rows_are_finite_and_right(alpha):
    """where 1 - q rounds to 0 in fp32, powf(0, alpha - 1) * log q decides between 0 and NaN; the batch-wide bound (TOL_MAXABS of
    the batch's largest gradient entry, which check_maxabs applies) is met by the float64 reference on its own: its saturated rows
    hold entries <= 2e-16"""
    z, y = saturated_focal_batch()
    _focal_check(z, y, 128, 1.0, alpha, 1.0 / 12, 'saturated alpha %g' % alpha)
    rows, d = _focal(_padded(z, 128), y, 10, 1.0, alpha, 1.0 / 12)
    assert float(d[6:10].abs().max()) <= 1e-6 and float(rows[6:10].abs().max()) <= 1e-6


def test_focal_rejects_alpha_below_one_and_marks_bad_labels():
    n, c, ld = 10, 300, 384
    r = np.random.default_rng(5)
    z = _f32(r.standard_normal((n, c)) * 3)
    y = r.integers(0, c, n)
    zd, yd = dev(_padded(z, ld)), _i32(y)
    for alpha in (0.5, 0.999):
        rows = torch.full((n,), 5.0, device='cuda'); d = torch.full((n, ld), 5.0, device='cuda')
        assert query('fte_focal_loss_fwd_bwd', zd.data_ptr(), yd.data_ptr(), rows.data_ptr(), d.data_ptr(), n, c, ld, 1.0, alpha, 1.0, stream()) == EINVAL
        torch.cuda.synchronize()
        assert float((rows - 5.0).abs().max()) == 0.0 and float((d - 5.0).abs().max()) == 0.0       # nothing written
    y, bad, good = _bad_label_layout(n, c, ld)
    rows, d = _focal(_padded(z, ld), y, c, 1.0, 2.0, 0.5)
    rows_g, d_g = _focal(_padded(z[good], ld), y[good], c, 1.0, 2.0, 0.5)
    assert torch.isnan(rows[bad]).all() and torch.isnan(d[bad][:, :c]).all()
    assert float(d[:, c:].abs().max()) == 0.0
    assert torch.equal(rows[good], rows_g) and torch.equal(d[good], d_g)


# ------------------------------------------------------------------------------------------------------------------------
# A-softmax and the norm / coefficient kernels
# ------------------------------------------------------------------------------------------------------------------------
THRESHOLDS = (0.0, R2, -R2)
FORCED = [1.0, -1.0, 0.0, R2, -R2] + [t + e for t in THRESHOLDS for e in (1e-3, -1e-3)]      # 3 of the 11 lie ON a threshold


def asoftmax_inputs(n, d, c, seed):
    """x [n, d], w [d, c] (float32 values), labels, and how many rows were placed on a k threshold.  Row i < 11 (rotated by n so
    that the small batches take different entries) has its target cosine forced to FORCED[.] as a float64 value before rounding."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((n, d)); w = r.standard_normal((d, c)) * 0.05
    y = r.integers(0, c, n); y[0] = 0; y[-1] = c - 1
    on_threshold = 0
    for i in range(min(n, len(FORCED))):
        t = FORCED[(i + 3 * n) % len(FORCED)]
        on_threshold += t in THRESHOLDS
        v = w[:, y[i]] / np.linalg.norm(w[:, y[i]])
        o = r.standard_normal(d); o -= o.dot(v) * v; o /= np.linalg.norm(o)
        x[i] = 3.0 * (t * v + np.sqrt(max(1 - t * t, 0.0)) * o)
    return _f32(x), _f32(w), y, on_threshold


def _asoftmax(sd, xn, wn, y, lam, c, gs, with_f=True):
    n, ld = sd.shape
    f = torch.full((n, ld), 5.0, device='cuda') if with_f else None
    G = torch.full((n, ld), 5.0, device='cuda')
    rows = torch.full((n,), 5.0, device='cuda'); rcf = torch.full((n,), 5.0, device='cuda')
    call('fte_asoftmax_fwd_bwd', sd, xn, wn, _i32(y), lam, f, rows, G, rcf, n, c, ld, gs, stream())
    torch.cuda.synchronize()
    return f, rows, G, rcf


@pytest.mark.parametrize('lam', [1000.0, 5.0, 0.5])
@pytest.mark.parametrize('n,d,c,ld', [(1, 512, 300, 384), (3, 512, 65, 128), (17, 512, 300, 300), (29, 128, 1000, 1024),
                                      (512, 512, 10575, 10624)])
def test_asoftmax_shapes_thresholds_and_optional_f(n, d, c, ld, lam):
    x32, w32, y, on_thr = asoftmax_inputs(n, d, c, n + c)
    x, w = x32.astype(np.float64), w32.astype(np.float64)
    gs = 1.0 / n
    loss_ref, f_ref, dx_ref, _ = ops.asoftmax_fwd_bwd(x, w, y, lam, gs)
    wp = np.zeros((d, ld)); wp[:, :c] = w
    sd = dev(x @ wp)
    xn = torch.empty(n, device='cuda'); wn = torch.full((ld,), 5.0, device='cuda')
    call('fte_row_norms', dev(x), xn, n, d, d, stream())
    call('fte_col_norms', dev(wp), wn, d, c, ld, stream())
    f, rows, G, rcf = _asoftmax(sd, xn, wn, y, lam, c, gs)
    f0, rows0, G0, rcf0 = _asoftmax(sd, xn, wn, y, lam, c, gs, with_f=False)
    assert f0 is None and torch.equal(G, G0) and torch.equal(rows, rows0) and torch.equal(rcf, rcf0)
    # psi is continuous at the thresholds: logits and loss agree whichever k each precision picked
    check_maxabs(host(f)[:, :c], f_ref, TOL_MAXABS, 'margin logits')
    _mean_close(rows, loss_ref, 'asoftmax')
    if ld > c:
        assert float(f[:, c:].abs().max()) == 0.0 and float(G[:, c:].abs().max()) == 0.0
    # the gradient is not: rows within 1e-5 of a threshold are left out, and those are at most the rows put there by construction
    cy = (x * w[:, y].T).sum(1) / (np.linalg.norm(x, axis=1) * np.linalg.norm(w[:, y], axis=0))
    keep = np.min(np.abs(cy[:, None] - np.array(THRESHOLDS)[None, :]), axis=1) > 1e-5
    assert (~keep).sum() <= on_thr, (cy[~keep], on_thr)
    if not keep.any():
        return
    Gh, rch = host(G), host(rcf)
    dx = Gh @ wp.T + rch[:, None] * x
    check_rell2(dx[keep], dx_ref[keep], TOL_RELL2, 'dx')
    # dw of the kept rows alone: oracle on that sub-batch, kernel's colcoef over the same rows of its G
    k = np.nonzero(keep)[0]
    _, _, _, dw_ref = ops.asoftmax_fwd_bwd(x[k], w, y[k], lam, gs)
    Gk = G[torch.tensor(k, device='cuda')].contiguous(); sk = sd[torch.tensor(k, device='cuda')].contiguous()
    ccf = torch.full((ld,), 5.0, device='cuda')
    call('fte_asoftmax_colcoef', Gk, sk, wn, ccf, len(k), c, ld, stream())
    dw = (x[k].T @ Gh[k] + host(ccf)[None, :] * wp)[:, :c]
    check_rell2(dw, dw_ref, TOL_RELL2, 'dw')


def test_asoftmax_bad_labels():
    n, d, c, ld = 10, 128, 300, 384
    x32, w32, y, _ = asoftmax_inputs(n, d, c, 9)
    yb, bad, good = _bad_label_layout(n, c, ld)
    y = np.where(np.isin(np.arange(n), bad), yb, y)
    x, w = x32.astype(np.float64), w32.astype(np.float64)
    wp = np.zeros((d, ld)); wp[:, :c] = w
    sd = dev(x @ wp)
    xn = torch.empty(n, device='cuda'); wn = torch.full((ld,), 5.0, device='cuda')
    call('fte_row_norms', dev(x), xn, n, d, d, stream())
    call('fte_col_norms', dev(wp), wn, d, c, ld, stream())
    f, rows, G, rcf = _asoftmax(sd, xn, wn, y, 5.0, c, 0.5)
    gi = torch.tensor(good, device='cuda')
    fg, rowsg, Gg, rcfg = _asoftmax(sd[gi].contiguous(), xn[gi].contiguous(), wn, y[good], 5.0, c, 0.5)
    assert torch.isnan(rows[bad]).all() and torch.isnan(rcf[bad]).all()
    assert torch.isnan(G[bad][:, :c]).all() and torch.isnan(f[bad][:, :c]).all()
    assert float(G[:, c:].abs().max()) == 0.0 and float(f[:, c:].abs().max()) == 0.0
    assert torch.equal(rows[gi], rowsg) and torch.equal(rcf[gi], rcfg) and torch.equal(G[gi], Gg) and torch.equal(f[gi], fg)
    assert torch.isfinite(rowsg).all() and torch.isfinite(Gg).all()


@pytest.mark.parametrize('cols', [1, 63, 64, 65, 300])
def test_row_col_norms_and_colcoef_tails(cols):
    """rows 1 .. 512 walk the 16-row trips and the 4-row tail of the column kernels with every remainder; ld > cols puts garbage
    beside the last column block.  Bounds: a sum of m squares in any order is within (m + 1) * 2^-24 of itself (no cancellation) and
    the square root halves that: m <= 300 per row-kernel thread chain, 36 adds per column lane at 512 rows -> 2e-6 covers both.
    colcoef sums signed products: at most 32 sequential adds per lane plus 5 combining ones, a product and a division by wn^2:
    (37 + 3) * 2^-24 = 2.4e-6 of sum_i |G s| / wn^2, held at 4e-6."""
    r = np.random.default_rng(cols)
    ld = cols + 7
    for rows in (1, 3, 4, 13, 16, 17, 29, 512):
        a = _f32(r.standard_normal((rows, ld))); a[:, cols:] = 77.0
        a64 = a.astype(np.float64)
        rn = torch.full((rows + 8,), 5.0, device='cuda'); cn = torch.full((ld + 8,), 5.0, device='cuda')
        ad = dev(a)
        call('fte_row_norms', ad, rn, rows, cols, ld, stream())
        call('fte_col_norms', ad, cn, rows, cols, ld, stream())
        what = '%d x %d' % (rows, cols)
        ref_r, ref_c = np.sqrt((a64[:, :cols] ** 2).sum(1)), np.sqrt((a64[:, :cols] ** 2).sum(0))
        assert (np.abs(host(rn)[:rows] - ref_r) <= 2e-6 * ref_r).all(), 'row norms ' + what
        assert (np.abs(host(cn)[:cols] - ref_c) <= 2e-6 * ref_c).all(), 'col norms ' + what
        assert float((rn[rows:] - 5.0).abs().max()) == 0.0 and float((cn[cols:] - 5.0).abs().max()) == 0.0      # nothing past the end
        G = _f32(r.standard_normal((rows, ld))); s = _f32(r.standard_normal((rows, ld)))
        wn = _f32(r.uniform(0.5, 2.0, ld)); wn[cols:] = 0.0
        Gd, sd_, wnd = dev(G), dev(s), dev(wn)
        cc = torch.full((ld + 8,), 5.0, device='cuda'); cc2 = torch.full((ld + 8,), 6.0, device='cuda')
        call('fte_asoftmax_colcoef', Gd, sd_, wnd, cc, rows, cols, ld, stream())
        call('fte_asoftmax_colcoef', Gd, sd_, wnd, cc2, rows, cols, ld, stream())
        prod = G.astype(np.float64)[:, :cols] * s.astype(np.float64)[:, :cols]
        w2 = wn.astype(np.float64)[:cols] ** 2
        got = host(cc)
        assert (np.abs(got[:cols] + prod.sum(0) / w2) <= 4e-6 * np.abs(prod).sum(0) / w2).all(), 'colcoef ' + what
        assert (got[cols:ld] == 0).all() and (got[ld:] == 5.0).all(), 'colcoef pads ' + what
        assert torch.equal(cc[:ld], cc2[:ld])


# ------------------------------------------------------------------------------------------------------------------------
# center loss
# ------------------------------------------------------------------------------------------------------------------------
def _center(f, y, cen, alpha, ncls):
    n, d = f.shape
    cd = dev(cen); rows = torch.full((n,), 5.0, device='cuda'); df = torch.full((n, d), 5.0, device='cuda')
    wsb, nb = ws(n * d * 4)
    call('fte_center_loss_fwd_bwd_update', dev(f), _i32(y), cd, rows, df, n, d, ncls, alpha, 1.0 / (n * d), wsb, nb, stream())
    torch.cuda.synchronize()
    return cd, rows, df, wsb


def center_labels(n, ncls, kind, seed):
    r = np.random.default_rng(seed)
    if kind == 'distinct':
        return r.permutation(ncls)[:n]
    return r.integers(0, ncls, n)


@pytest.mark.parametrize('n,d,ncls,kind', [(1, 512, 3, 'random'), (32, 100, 11, 'random'), (32, 1030, 11, 'random'),
                                           (128, 2048, 10575, 'random'), (37, 256, 1, 'random'), (37, 256, 1000, 'distinct'),
                                           (8200, 64, 50, 'random')])
def test_center_loss_shapes_and_both_label_paths(n, d, ncls, kind):
    """n = 8200 > 8192 is the global-memory label path of center_update_kernel; d = 100 / 1030 leave the j0 + u*256 < d guards
    partly open; one class / all distinct labels are the two ends of the ownership scan"""
    r = np.random.default_rng(n + d)
    f = _f32(r.standard_normal((n, d))); cen = _f32(r.standard_normal((ncls, d)) * 0.1)
    y = center_labels(n, ncls, kind, n)
    loss_ref, df_ref, c_ref = ops.center_loss(f.astype(np.float64), y, cen.astype(np.float64), 0.99)
    cd, rows, df, _ = _center(f, y, cen, 0.99, ncls)
    got = host(rows).sum() / (n * d)
    assert abs(got - loss_ref) <= 1e-5 * loss_ref
    check_maxabs(host(df), df_ref, 1e-5, 'dfeat'); check_maxabs(host(cd), c_ref, 1e-5, 'centers')
    unused = np.setdiff1d(np.arange(ncls), y)
    np.testing.assert_array_equal(cd.cpu().numpy()[unused], cen[unused])              # bitwise untouched
    used = np.unique(y)
    check_maxabs(host(cd)[used], c_ref[used], 1e-5, 'updated rows')
    assert (np.abs(host(cd)[used] - cen[used].astype(np.float64)).max(axis=1) > 0).all()         # every used row did move
    cd2, _, _, _ = _center(f, y, cen, 0.99, ncls)
    assert torch.equal(cd, cd2)
    # alpha == 1: no update, ws holds f - c_y; the separate scatter of that ws equals the fused call bit for bit
    cd1, rows1, df1, wsb = _center(f, y, cen, 1.0, ncls)
    np.testing.assert_array_equal(cd1.cpu().numpy(), cen)
    assert torch.equal(rows1, rows) and torch.equal(df1, df)
    np.testing.assert_array_equal(wsb[:n * d].cpu().numpy().reshape(n, d), f - cen[y])
    call('fte_center_scatter_update', wsb, _i32(y), cd1, n, d, ncls, 0.99, stream())
    torch.cuda.synchronize()
    assert torch.equal(cd1, cd)


@pytest.mark.parametrize('n,d,ncls', [(16, 100, 5), (8200, 64, 50)])
def test_center_loss_bad_labels(n, d, ncls):
    r = np.random.default_rng(n)
    f = _f32(r.standard_normal((n, d))); cen = _f32(r.standard_normal((ncls, d)) * 0.1)
    y = r.integers(0, ncls, n)
    y[0] = -1; y[n // 2] = ncls; y[n - 1] = INT_MAX
    y[1] = 3; y[2] = INT_MAX; y[3] = 3; y[4] = 4; y[5] = -5           # class 4's first good sample follows bad ones
    y[6:] = np.where(y[6:] == 4, 2, y[6:])
    bad = np.nonzero((y < 0) | (y >= ncls))[0]; good = np.setdiff1d(np.arange(n), bad)
    assert (y[:4] != 4).all() and y[4] == 4 and len(bad) >= 5
    cd, rows, df, wsb = _center(f, y, cen, 0.99, ncls)
    assert torch.isnan(rows[bad]).all() and torch.isnan(df[bad]).all()
    diff = wsb[:n * d].reshape(n, d)
    assert float(diff[bad].abs().max()) == 0.0
    _, _, c_ref = ops.center_loss(f[good].astype(np.float64), y[good], cen.astype(np.float64), 0.99)
    check_maxabs(host(cd), c_ref, 1e-5, 'centers of the good samples only')
    cdg, rowsg, dfg, _ = _center(f[good], y[good], cen, 0.99, ncls)
    gi = torch.tensor(good, device='cuda')
    assert torch.equal(cd, cdg) and torch.equal(rows[gi], rowsg)
    # dfeat carries grad_scale = 1 / (n d) of its own batch: compare the unscaled rows
    check_maxabs(host(df[gi]) * (n * d), host(dfg) * (len(good) * d), 1e-6, 'dfeat of the good rows')


def test_center_loss_workspace_and_arguments():
    n, d, ncls = 8, 64, 3
    t = torch.zeros(n * d + 64, device='cuda'); y = _i32(np.zeros(n))
    p = t.data_ptr()
    args = lambda nb, nn=n, dd=d, nc=ncls: (p, y.data_ptr(), p, p, p, nn, dd, nc, 0.99, 1.0, p, nb, stream())
    assert query('fte_center_loss_fwd_bwd_update', *args(n * d * 4 - 4)) == EWORKSPACE
    assert query('fte_center_loss_fwd_bwd_update', *args(n * d * 4, dd=0)) == EINVAL
    assert query('fte_center_loss_fwd_bwd_update', *args(n * d * 4, nc=0)) == EINVAL
    assert query('fte_center_scatter_update', p, y.data_ptr(), p, 0, d, ncls, 0.99, stream()) == EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# batch-hard triplet
# ------------------------------------------------------------------------------------------------------------------------
LW = 0.37
MARGINS = (None, 0.3, -1.0, 0.0)


def triplet_labels(n, layout):
    i = np.arange(n)
    if layout == 'pk':
        return i // 4
    if layout == 'one':
        return np.zeros(n, np.int64)
    if layout == 'distinct':
        return i * 3 + 1
    if layout == 'singleton':
        y = i // 4; y[n // 2] = 9999
        return y
    if layout == 'far':                          # members 64 (and 128) rows apart: one lane holds the whole group across its strides
        return i % 64
    raise ValueError(layout)


def triplet_inputs_are_decided(f, y, margin):
    """input sanity, float64 only: fp32 and float64 can only be asked to pick the same hardest positive / negative and the same
    side of the hinge when the runner-up is not within rounding of the winner.  Exact ties (equal rows) are decided by the index rule
    and allowed; a gap below 1e-5 relative that is not exactly zero is an input to re-seed, not a tolerance."""
    f = f.astype(np.float64); n = len(y)
    dist = np.sqrt(((f[:, None, :] - f[None, :, :]) ** 2).sum(-1) + 1e-12)
    same = y[:, None] == y[None, :]
    for i in range(n):
        pos = np.sort(dist[i][same[i] & (np.arange(n) != i)])[::-1]
        neg = np.sort(dist[i][~same[i]])
        for v in (pos, neg):
            if len(v) > 1 and v[0] != v[1] and abs(v[0] - v[1]) <= 1e-5 * max(v[0], v[1]):
                return False
        hp = pos[0] if len(pos) else 0.0; hn = neg[0] if len(neg) else 1e6
        if margin is not None and 0 < abs(hp - hn + margin) <= 1e-5 * max(hp, hn):
            return False
    return True


def _triplet(f, y, margin, lw=LW):
    n, d = f.shape
    rows = torch.full((n,), 5.0, device='cuda'); g = torch.full((n, d), 5.0, device='cuda')
    wsb, nb = ws(2 * n * n * 4)
    call('fte_batch_hard_triplet_fwd_bwd', dev(f), _i32(y), 0.0 if margin is None else margin, int(margin is None), lw,
         rows, g, n, d, wsb, 2 * n * n * 4, stream())                     # exactly the documented workspace size
    torch.cuda.synchronize()
    return rows, g


def _triplet_check(f, y, margin, what, by_row=False):
    assert triplet_inputs_are_decided(f, y, margin), what
    l_ref, g_ref = ops.batch_hard_triplet(f.astype(np.float64), y, margin)
    rows, g = _triplet(f, y, margin)
    what = '%s margin %s' % (what, margin)
    check_maxabs(host(rows), l_ref, TOL_MAXABS, what + ' loss')
    check_rell2(host(g), LW * g_ref, TOL_RELL2, what + ' grad')
    check_maxabs(host(g), LW * g_ref, TOL_MAXABS, what + ' grad')
    if by_row:
        gh = host(g); norms = np.sqrt((g_ref ** 2).sum(1)) * LW
        for i in range(len(y)):
            err = np.sqrt(((gh[i] - LW * g_ref[i]) ** 2).sum())
            assert err <= TOL_RELL2 * max(norms[i], 1e-3 * norms.max()), '%s row %d: %.3e vs |ref| %.3e' % (what, i, err, norms[i])
    return rows, g


TRIPLET_SHAPES = [(1, 100), (2, 1), (2, 100), (63, 100), (64, 1), (64, 2048), (65, 100), (65, 1), (130, 2048), (130, 100), (256, 100),
                  (256, 1)]


# (d = 2048: the float64 oracle holds an [n, n, d] difference tensor; two layouts and two margins there)
TRIPLET_CASES = [(n, d, layout) for n, d in TRIPLET_SHAPES for layout in (('pk', 'far') if d == 2048 else ('pk', 'one', 'distinct', 'singleton', 'far'))]


@pytest.mark.parametrize('n,d,layout', TRIPLET_CASES)
def test_triplet_shapes_layouts_margins(n, d, layout):
    r = np.random.default_rng(1000 * n + d)
    f = _f32(r.standard_normal((n, d)))
    y = triplet_labels(n, layout)
    for margin in (MARGINS if d < 2048 else (None, 0.3)):
        _triplet_check(f, y, margin, 'n %d d %d %s' % (n, d, layout))


def tied_triplet_batch():
    """n = 130, d = 100.  Anchor 0 (identity 500, with rows 5 and 69 = 5 + 64: one lane, two strides) has two equidistant hardest
    positives 5, 69 and two equidistant hardest negatives 7, 71; anchor 1 (identity 501, with rows 10 and 67) has its tied positives
    in different lanes with the lower index in the higher lane (10 in lane 10, 67 in lane 3), and tied negatives 12 (lane 12) and 66
    (lane 2).  The lower index must win every time."""
    r = np.random.default_rng(130)
    n, d = 130, 100
    f = r.standard_normal((n, d))
    y = 1000 + np.arange(n)
    y[[0, 5, 69]] = 500; y[[1, 10, 67]] = 501
    f[5] = f[0] + 3.0 * r.standard_normal(d); f[69] = f[5]
    f[7] = f[0] + 0.01 * r.standard_normal(d); f[71] = f[7]
    f[10] = f[1] + 3.0 * r.standard_normal(d); f[67] = f[10]
    f[12] = f[1] + 0.01 * r.standard_normal(d); f[66] = f[12]
    return _f32(f), y


@pytest.mark.parametrize('margin', MARGINS)
def test_triplet_exact_ties_go_to_the_lower_index(margin):
    f, y = tied_triplet_batch()
    f64 = f.astype(np.float64)
    dist = np.sqrt(((f64[:, None] - f64[None]) ** 2).sum(-1))
    assert dist[0, 5] == dist[0, 69] and dist[0, 7] == dist[0, 71] and dist[1, 10] == dist[1, 67] and dist[1, 12] == dist[1, 66]
    assert dist[0, 7] == np.delete(dist[0], 0).min() and dist[1, 12] == np.delete(dist[1], 1).min()
    rows, g = _triplet_check(f, y, margin, 'ties', by_row=True)
    # rows 5 / 69 and 10 / 67 are equal as anchors; they differ exactly by what anchors 0 and 1 sent to the winner alone
    gh = host(g)
    assert np.abs(gh[5] - gh[69]).max() > 1e-3 * np.abs(gh[5]).max() and np.abs(gh[10] - gh[67]).max() > 1e-3 * np.abs(gh[10]).max()


def test_triplet_duplicate_of_the_anchor_as_its_only_positive():
    r = np.random.default_rng(8)
    n, d = 8, 100
    f = _f32(r.standard_normal((n, d))); f[1] = f[0]
    y = np.array([0, 0, 1, 2, 3, 4, 5, 6])
    for margin in MARGINS:
        rows, g = _triplet_check(f, y, margin, 'duplicate anchor', by_row=True)
        assert torch.isfinite(g).all() and torch.isfinite(rows).all()


@pytest.mark.parametrize('scale', [100.0, 1e-3])
def test_triplet_softplus_branches_and_small_features(scale):
    r = np.random.default_rng(66)        # (65 puts two positives of one anchor 7e-6 apart: see triplet_inputs_are_decided)
    n, d = 65, 100
    f = _f32(r.standard_normal((n, d)) * scale)
    f[1:4] = f[0] + _f32(r.standard_normal((3, d)) * 0.01 * scale)       # a tight identity under 'pk': pos - neg far below -20 at scale 100
    for layout in ('pk', 'far', 'singleton'):
        y = triplet_labels(n, layout)
        for margin in MARGINS:
            _triplet_check(f, y, margin, 'scale %g %s' % (scale, layout))
        if scale == 100.0 and layout == 'pk':       # both softplus branches are in the batch: v > 20 and v < -20
            f64 = f.astype(np.float64)
            dist = np.sqrt(((f64[:, None] - f64[None]) ** 2).sum(-1) + 1e-12)
            same = y[:, None] == y[None, :]
            v = (dist * (same ^ np.eye(n, dtype=bool))).max(1) - np.where(same, 1e6, dist).min(1)
            assert v.max() > 20 and v.min() < -20, (v.min(), v.max())


def test_triplet_limits_and_workspace():
    t = torch.zeros(1024, device='cuda'); y = _i32(np.zeros(64))
    p, yp = t.data_ptr(), y.data_ptr()
    big = 2 * 8193 * 8193 * 4
    assert query('fte_batch_hard_triplet_fwd_bwd', p, yp, 0.3, 0, 1.0, p, p, 8193, 4, p, big, stream()) == EINVAL        # no launch
    assert query('fte_batch_hard_triplet_fwd_bwd', p, yp, 0.3, 0, 1.0, p, p, 4, 0, p, 4096, stream()) == EINVAL
    assert query('fte_batch_hard_triplet_fwd_bwd', p, yp, 0.3, 0, 1.0, p, p, 0, 4, p, 4096, stream()) == EINVAL
    assert query('fte_batch_hard_triplet_fwd_bwd', p, yp, 0.3, 0, 1.0, p, p, 8, 4, p, 2 * 8 * 8 * 4 - 4, stream()) == EWORKSPACE
    assert query('fte_batch_hard_triplet_fwd_bwd', p, yp, 0.3, 0, 1.0, p, p, 8, 4, 0, 1 << 20, stream()) == EWORKSPACE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
