"""-m gpu: the flat-arena kernels of csrc/kernels.hip (momentum, Adam, sums, row reductions, the small element-wise helpers,
the bf16 conversion) at the sizes their code branches on: scalar tails (n % 4 != 0), the grid-stride loop past the block cap,
every loop tail of the generic row reduction, the fall-back conditions of the slab reduction.  References are float64 numpy
(oracle.ops for the optimizers).  Every output buffer carries a canary of 8 floats that must come back bit for bit.

Which reduction kernel a case reaches is decided in k_reduce_rows2 (kernels.hip): the 16-byte slab kernels need no bias,
scale == 1, rows >= 2, cols >= 4096, cols % 4 == 0 and 16-byte aligned pointers; anything else through fte_reduce_rows is
reduce_rows_kernel in one launch.  The launch profiler does not record these kernels; the cases sit on both sides of each condition."""
import numpy as np
import pytest
import torch

from oracle import ops

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import call, query, dev, host, stream, ws, check_maxabs
    from tf_face_toolbox_amd._lib import FteError

EINVAL = -1
CANARY = np.array([3.0, -1.5, 2.0 ** -30, 1e30, -7.0, 11.0, 0.5, -2.0 ** 20], np.float32)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _guarded(a):
    """device copy of a flat float32 array followed by the canary"""
    return torch.tensor(np.concatenate([np.asarray(a, np.float32).ravel(), CANARY]), device='cuda')


def _intact(t, n):
    return np.array_equal(t[n:].cpu().numpy().view(np.uint32), CANARY.view(np.uint32))


TAIL_SIZES = [1, 2, 3, 5, 1023, 4 * 100003 + 1, 4 * 100003 + 2, 4 * 100003 + 3]


@pytest.mark.parametrize('n', TAIL_SIZES + [4096 * 1024 + 4099])
def test_momentum_scalar_tail_and_grid_stride(n):
    """momentum_kernel: f32x4 body, threads 0 .. (n & 3) - 1 of block 0 take the tail; at most 4096 blocks x 1024 elements per trip"""
    r = np.random.default_rng(n % 100000)
    w = _f32(r.standard_normal(n)); acc = _f32(r.standard_normal(n) * 0.1); g = _f32(r.standard_normal(n))
    w64, a64, g64 = w.astype(np.float64), acc.astype(np.float64), g.astype(np.float64)
    w_ref, acc_ref = ops.momentum_step(w64, a64, 0.5 * g64 + 5e-4 * w64, 0.1, 0.9)
    wd_, ad, gd = _guarded(w), _guarded(acc), _guarded(g)
    call('fte_momentum_update', wd_, ad, gd, n, 0.1, 0.9, 5e-4, 0.5, stream())
    torch.cuda.synchronize()
    check_maxabs(host(wd_)[:n], w_ref, 1e-6, 'momentum w'); check_maxabs(host(ad)[:n], acc_ref, 1e-6, 'momentum acc')
    t = max(n & 3, 1)                                             # the tail on its own: a batch-wide maximum cannot hide it
    wh, ah = host(wd_), host(ad)
    for k in range(n - t, n):
        assert abs(wh[k] - w_ref[k]) <= 1e-6 * max(abs(w_ref[k]), abs(w64[k])), ('w tail', k)
        assert abs(ah[k] - acc_ref[k]) <= 1e-6 * max(abs(acc_ref[k]), abs(a64[k]), abs(g64[k])), ('acc tail', k)
        assert ah[k] != a64[k]                                    # it was updated at all
    assert _intact(wd_, n) and _intact(ad, n) and _intact(gd, n)
    np.testing.assert_array_equal(gd[:n].cpu().numpy(), g)


@pytest.mark.parametrize('n', TAIL_SIZES + [1024 * 8192 + 8195])
def test_sum_and_sumsq_scalar_tail_and_grid_stride(n):
    """partial_sum_kernel: at most 1024 blocks x 8192 elements per trip, tail in block 0.  Bound: 1e-5 of sum |a_i| (of sum a_i^2),
    not of the sum, which can cancel."""
    r = np.random.default_rng(n % 100000 + 1)
    a = _f32(r.standard_normal(n)); a64 = a.astype(np.float64)
    out = torch.full((9,), 5.0, device='cuda'); out[1:] = torch.tensor(CANARY, device='cuda')
    wsb, nb = ws(4096)
    ad = _guarded(a)
    call('fte_sum', ad, n, 2.0, out, wsb, nb, stream())
    assert abs(float(out[0]) - 2.0 * a64.sum()) <= 1e-5 * 2.0 * np.abs(a64).sum()
    call('fte_sumsq', ad, n, 0.25, out, wsb, nb, stream())
    assert abs(float(out[0]) - 0.25 * (a64 * a64).sum()) <= 1e-5 * 0.25 * (a64 * a64).sum()
    assert _intact(out, 1) and _intact(ad, n)
    # the tail alone: zero body, so the result IS the tail's sum (at most three terms: two roundings, and the scale is a power of two)
    t = n & 3
    if t:
        b = np.zeros(n, np.float32); b[n - t:] = a[n - t:] + np.float32(3.0)
        b64 = b.astype(np.float64)
        bd = _guarded(b)
        call('fte_sum', bd, n, 2.0, out, wsb, nb, stream())
        assert abs(float(out[0]) - 2.0 * b64.sum()) <= 2.0 ** -22 * 2.0 * np.abs(b64).sum(), 'sum tail'
        call('fte_sumsq', bd, n, 0.25, out, wsb, nb, stream())
        assert abs(float(out[0]) - 0.25 * (b64 * b64).sum()) <= 2.0 ** -21 * 0.25 * (b64 * b64).sum(), 'sumsq tail'


def test_arena_kernels_reject_misaligned_and_empty_arguments():
    t = torch.zeros(64, device='cuda'); out = torch.zeros(1, device='cuda'); wsb, nb = ws(4096)
    with pytest.raises(FteError):
        call('fte_momentum_update', t[1:], t, t, 8, 0.1, 0.9, 0.0, 1.0, stream())
    with pytest.raises(FteError):
        call('fte_momentum_update', t, t[1:], t, 8, 0.1, 0.9, 0.0, 1.0, stream())
    with pytest.raises(FteError):
        call('fte_sum', t[1:], 8, 1.0, out, wsb, nb, stream())
    with pytest.raises(FteError):
        call('fte_sumsq', t[3:], 8, 1.0, out, wsb, nb, stream())
    p = t.data_ptr()
    for name in ('fte_sum', 'fte_sumsq'):
        assert query(name, p, 0, 1.0, out.data_ptr(), wsb.data_ptr(), nb, stream()) == EINVAL
        assert query(name, p, -3, 1.0, out.data_ptr(), wsb.data_ptr(), nb, stream()) == EINVAL
        assert query(name, p, 8, 1.0, out.data_ptr(), wsb.data_ptr(), 1023 * 4, stream()) == -2
    assert query('fte_momentum_update', p, p, p, 0, 0.1, 0.9, 0.0, 1.0, stream()) == EINVAL
    assert query('fte_adam_update', p, p, p, p, 8, 0.01, 0.5, 0.999, 1e-8, 0.0, 1.0, 0, stream()) == EINVAL          # t = 0
    assert query('fte_adam_update', p, p, p, p, 0, 0.01, 0.5, 0.999, 1e-8, 0.0, 1.0, 1, stream()) == EINVAL
    assert query('fte_to_bf16', p, p, 6, stream()) == EINVAL
    assert query('fte_bcast_add', p, p, 1, 2, 6, 1.0, stream()) == EINVAL                                           # c % 4
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and float(out[0]) == 0.0


@pytest.mark.parametrize('t', [1, 3, 100000])
@pytest.mark.parametrize('n', [1, 255, 257, 4096 * 256 + 3])
def test_adam_weight_decay_grad_scale_steps_and_grid_stride(n, t):
    """(1 - beta2) is formed in fp32 like TF's ApplyAdam does: 1 - 0.999f is off by 1.3e-5 relative, hence 2e-5 on w and v"""
    r = np.random.default_rng(n + t)
    w = _f32(r.standard_normal(n)); m = _f32(r.standard_normal(n) * 0.1); v = _f32(np.abs(r.standard_normal(n)) * 0.01)
    g = _f32(r.standard_normal(n))
    w64, g64 = w.astype(np.float64), g.astype(np.float64)
    w2, m2, v2 = ops.adam_step(w64, m.astype(np.float64), v.astype(np.float64), 0.5 * g64 + 5e-4 * w64, 0.01, t)
    wd_, md, vd, gd = _guarded(w), _guarded(m), _guarded(v), _guarded(g)
    call('fte_adam_update', wd_, md, vd, gd, n, 0.01, 0.5, 0.999, 1e-8, 5e-4, 0.5, t, stream())
    torch.cuda.synchronize()
    check_maxabs(host(wd_)[:n], w2, 2e-5, 'adam w'); check_maxabs(host(md)[:n], m2, 1e-6, 'adam m'); check_maxabs(host(vd)[:n], v2, 2e-5, 'adam v')
    k = n - 1                                                     # the last element (past the cap: reached only by the grid-stride loop)
    assert abs(host(md)[k] - m2[k]) <= 1e-6 * max(abs(m2[k]), abs(g64[k])) and abs(host(vd)[k] - v2[k]) <= 2e-5 * abs(v2[k])
    assert abs(host(wd_)[k] - w2[k]) <= 2e-5 * max(abs(w2[k]), abs(w2[k] - w64[k])) and host(wd_)[k] != w64[k]
    assert _intact(wd_, n) and _intact(md, n) and _intact(vd, n) and _intact(gd, n)


GENERIC_ROWS = [1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 36, 37, 61, 300]


@pytest.mark.parametrize('cols', [1, 24, 63, 64, 65, 96, 1000])
def test_reduce_rows_generic_loop_tails(cols):
    """reduce_rows_kernel: four row lanes, each with a 32-row trip (r + 28 < r1), an 8-row trip (r + 4 < r1) and a last row; 64
    columns per block.  Bound per column, valid for ANY summation order: a sum of m terms is within (m - 1) * 2^-24 * sum |terms|
    (first order), plus one rounding each for the scale and the bias: (m + 2) * 2^-24 * (|scale| sum |a| + |bias|).  A dropped or
    doubled row is an error of a whole term, 1 / m of that sum, orders of magnitude above it."""
    r = np.random.default_rng(cols)
    for rows in GENERIC_ROWS:
        a = _f32(r.standard_normal((rows, cols))); a64 = a.astype(np.float64)
        ad = dev(a)
        for fold in (1, 4):
            if cols % fold:
                continue
            oc = cols // fold
            m = rows * fold
            s = a64.reshape(m, oc).sum(0); sabs = np.abs(a64).reshape(m, oc).sum(0)
            for bmod in sorted({0, cols, oc, oc // 4 if oc % 4 == 0 else oc}):
                bias = _f32(r.standard_normal(bmod)) if bmod else None
                for scale in (1.0, 0.5):
                    o = _guarded(np.full(oc, 5.0))
                    call('fte_reduce_rows', ad, o, None if bias is None else dev(bias), bmod, rows, cols, fold, scale, stream())
                    bj = bias.astype(np.float64)[np.arange(oc) % bmod] if bmod else np.zeros(oc)
                    ref = scale * s + bj
                    bound = (m + 2) * 2.0 ** -24 * (scale * sabs + np.abs(bj)) * 1.01
                    err = np.abs(host(o)[:oc] - ref)
                    assert (err <= bound).all(), ('rows %d cols %d fold %d bmod %d scale %g' % (rows, cols, fold, bmod, scale), (err / np.maximum(bound, 1e-300)).max())
                    assert _intact(o, oc)


@pytest.mark.parametrize('rows,cols,offset', [(1, 4096, 0), (2, 4092, 0), (2, 4096, 0), (31, 4100, 0), (32, 4096, 0), (2, 4096, 1), (32, 4096, 1)])
def test_reduce_rows_slab_path_edges(rows, cols, offset):
    """(1, 4096): one row, (2, 4092): too narrow, out offset by one float: not 16-byte aligned -> generic kernel; (2, 4096) and
    (31, 4100): reduce_slabs_kernel<64> (rows < 32), (32, 4096): <16>.  The existing slab bound."""
    r = np.random.default_rng(rows * cols + offset)
    a = _f32(r.standard_normal((rows, cols)))
    buf = _guarded(np.full(cols + 4, 5.0))
    o = buf[offset:]
    call('fte_reduce_rows', dev(a), o, None, 1, rows, cols, 1, 1.0, stream())
    torch.cuda.synchronize()
    check_maxabs(host(o)[:cols], a.astype(np.float64).sum(0), 4e-6 * np.sqrt(rows) * 4, 'reduce_rows %dx%d +%d' % (rows, cols, offset))
    assert (buf[:offset].cpu().numpy() == 5.0).all() and (buf[offset + cols:cols + 4].cpu().numpy() == 5.0).all() and _intact(buf, cols + 4)


@pytest.mark.parametrize('use_rc,use_cc', [(True, False), (False, True), (False, False), (True, True)])
def test_add_scaled_rows_cols_optional_vectors_and_pitch(use_rc, use_cc):
    r = np.random.default_rng(2 * use_rc + use_cc)
    for rows, cols, ld in ((5, 37, 48), (1, 1, 3), (300, 65, 65), (17, 256, 300)):
        a = _f32(r.standard_normal((rows, ld))); b = _f32(r.standard_normal((rows, ld)))
        rc = _f32(r.standard_normal(rows)); cc = _f32(r.standard_normal(cols))
        at = _guarded(a); bt = _guarded(b)
        call('fte_add_scaled_rows_cols', at, bt, dev(rc) if use_rc else None, dev(cc) if use_cc else None, rows, cols, ld, stream())
        torch.cuda.synchronize()
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        ref = a64.copy()
        if use_rc:
            ref[:, :cols] += rc.astype(np.float64)[:, None] * b64[:, :cols]
        if use_cc:
            ref[:, :cols] += cc.astype(np.float64)[None, :] * b64[:, :cols]
        got = at[:rows * ld].cpu().numpy().reshape(rows, ld)
        check_maxabs(got[:, :cols], ref[:, :cols], 1e-6, 'add_scaled')
        np.testing.assert_array_equal(got[:, cols:], a[:, cols:])                  # pitch columns untouched, bit for bit
        if not use_rc and not use_cc:
            np.testing.assert_array_equal(got, a)
        np.testing.assert_array_equal(bt[:rows * ld].cpu().numpy().reshape(rows, ld), b)
        assert _intact(at, rows * ld)


@pytest.mark.parametrize('n', [1, 3, 1000003])
def test_axpby_sizes_and_aliasing(n):
    """a, b powers of two: both products are exact, so the result is the correctly rounded sum whether or not the compiler fuses them"""
    r = np.random.default_rng(n)
    x = _f32(r.standard_normal(n)); y = _f32(r.standard_normal(n))
    ref = np.float32(0.5) * x + np.float32(0.25) * y
    xd, yd, o = _guarded(x), _guarded(y), _guarded(np.full(n, 5.0))
    call('fte_axpby', 0.5, xd, 0.25, yd, o, n, stream())
    np.testing.assert_array_equal(o[:n].cpu().numpy(), ref)
    call('fte_axpby', 0.5, xd, 0.25, yd, xd, n, stream())                          # out aliases x
    np.testing.assert_array_equal(xd[:n].cpu().numpy(), ref)
    call('fte_axpby', 0.5, o, 0.25, yd, yd, n, stream())                           # out aliases y
    np.testing.assert_array_equal(yd[:n].cpu().numpy(), np.float32(0.5) * ref + np.float32(0.25) * y)
    assert _intact(xd, n) and _intact(yd, n) and _intact(o, n)


@pytest.mark.parametrize('hw', [49, 1])
@pytest.mark.parametrize('c', [4, 2048])
def test_bcast_add_direct(hw, c):
    n = 3
    r = np.random.default_rng(hw + c)
    dx = _f32(r.standard_normal((n, hw, c))); v = _f32(r.standard_normal((n, c)))
    dxd, vd = _guarded(dx), _guarded(v)
    call('fte_bcast_add', dxd, vd, n, hw, c, 1.0 / 49, stream())
    torch.cuda.synchronize()
    ref = dx.astype(np.float64) + v.astype(np.float64)[:, None, :] * float(np.float32(1.0 / 49))
    check_maxabs(host(dxd)[:n * hw * c].reshape(n, hw, c), ref, 1e-6, 'bcast_add')
    assert _intact(dxd, n * hw * c) and _intact(vd, n * c)


def _bits(u):
    return np.array(u, np.uint32).view(np.float32)


def test_to_bf16_bit_for_bit():
    """round to nearest even against torch's CPU conversion: ties in both directions, overflow to inf, infinities, zeros of both
    signs, denormals (kept, not flushed), NaN stays a NaN (any NaN)"""
    r = np.random.default_rng(16)
    hand = _bits([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,          # ties: down to even, up to even, and their negatives
                  0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001,          # one ulp beside a tie
                  0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,          # largest finite float -> inf; the tie below it -> inf; just below -> finite
                  0x7F800000, 0xFF800000, 0x00000000, 0x80000000,          # +-inf, +-0
                  0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x807FFFFF, 0x00010000, 0x80018000,      # denormals
                  0x00800000, 0x3F800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x7FFFFFFF, 0xFF800001])      # ..., NaNs
    rnd = np.concatenate([_f32(r.standard_normal(4096)), _f32(r.standard_normal(4096) * 1e30), _f32(r.standard_normal(4096) * 1e-30),
                          r.integers(0, 2 ** 32, 8192, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = np.concatenate([hand, rnd])
    assert len(x) % 4 == 0
    ref = torch.tensor(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    y = torch.zeros(len(x) + 8, dtype=torch.int16, device='cuda')
    call('fte_to_bf16', torch.tensor(x, device='cuda'), y, len(x), stream())
    got = y.cpu().numpy().view(np.uint16)
    assert (got[len(x):] == 0).all()
    got = got[:len(x)]
    nan = np.isnan(x)
    assert nan.sum() >= 6
    np.testing.assert_array_equal(got[~nan], ref[~nan])
    assert (((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x007F) != 0)).all()       # still a NaN
    assert ref[0] == 0x3F80 and ref[1] == 0x3F82 and ref[8] == 0x7F80 and ref[17] == 0x0000 and ref[18] == 0x0002      # the reference itself
