"""The fused BN + PReLU kernels against their ReLU siblings on the same buffers: fte_bn_prelu_apply vs fte_bn_apply(relu = 1) and
fte_bn_prelu_train_bwd vs fte_bn_train_bwd_zmask, at the four IResNet shapes of a B-image shard (default 128).  The new kernels move
the same bytes per element plus 4c of alpha read (and 4c of dalpha written), so parity within the sibling's own run-to-run spread is
the expectation.  Repeats are interleaved (sibling, new, sibling, new, ...): `rounds` windows of `reps` calls each, per window the mean
time per call from device events; reported: median and min..max over the windows.  Prints a markdown table.

  python scripts/bench_bn_prelu.py [B] [rounds] [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tf_face_toolbox_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 50
PEAK = 8000.0          # GB/s
f32 = dict(dtype=torch.float32, device='cuda')


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3          # us per call


def ab(fa, fb):
    """interleaved windows of two callables -> two sorted lists of us per call"""
    for f in (fa, fb):                                # warm-up: code objects, the workspace's first touch
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(window(fa))
        tb.append(window(fb))
    return sorted(ta), sorted(tb)


def main():
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    st = torch.cuda.current_stream().cuda_stream
    q = _lib.query
    print('| pass | shape | MB moved | sibling us (min..max) | BN + PReLU us (min..max) | ratio of medians | BN + PReLU GB/s | of 8 TB/s |')
    print('|---|---|---|---|---|---|---|---|')
    for h, c in [(56, 64), (28, 128), (14, 256), (7, 512)]:
        rows = B * h * h
        g = torch.Generator(device='cuda').manual_seed(c)
        z = torch.randn(rows, c, generator=g, **f32) * 2 + 1
        dy = torch.randn(rows, c, generator=g, **f32)
        y, dz = torch.empty_like(z), torch.empty_like(z)
        gamma = torch.rand(c, generator=g, **f32) + 0.5
        beta = torch.randn(c, generator=g, **f32) * 0.3
        alpha = torch.full((c,), 0.25, **f32)
        mean, rstd, scale, shift, dg, db, da = (torch.empty(c, **f32) for _ in range(7))
        ws = torch.empty(max(q('fte_bn_ws_bytes', c), q('fte_bn_prelu_ws_bytes', c)) // 4 + 1024, **f32)
        wsb = ws.numel() * 4
        _lib.call('fte_bn_train_stats', z, gamma, beta, mean, rstd, scale, shift, None, None, rows, c, 1e-5, 0.9, ws, wsb, st)
        tb = z.numel() * 4
        shape = '%dx%dx%dx%d' % (B, h, h, c)
        cases = [('apply', 2 * tb,
                  lambda: _lib.call('fte_bn_apply', z, scale, shift, None, y, rows, c, 1, 0, st),
                  lambda: _lib.call('fte_bn_prelu_apply', z, scale, shift, alpha, y, rows, c, st)),
                 ('backward', 5 * tb,          # (dy, z) twice, dz once
                  lambda: _lib.call('fte_bn_train_bwd_zmask', dy, z, gamma, mean, rstd, scale, shift, dz, dg, db, rows, c, ws, wsb, st),
                  lambda: _lib.call('fte_bn_prelu_train_bwd', dy, z, gamma, mean, rstd, scale, shift, alpha, dz, dg, db, da, rows, c, ws, wsb, st))]
        for what, nbytes, fa, fb in cases:
            ta, tn = ab(fa, fb)
            ma, mn = ta[len(ta) // 2], tn[len(tn) // 2]
            gbs = nbytes / mn / 1e3
            print('| %s | %s | %.1f | %.1f (%.1f..%.1f) | %.1f (%.1f..%.1f) | %.3f | %.0f | %.0f %% |' % (
                what, shape, nbytes / 1e6, ma, ta[0], ta[-1], mn, tn[0], tn[-1], mn / ma, gbs, 100 * gbs / PEAK))


if __name__ == '__main__':
    main()
