"""The two split reductions of the SE-IResNet block tail against their unsplit siblings on the same buffers: fte_se_lin_squeeze vs
fte_se_squeeze and fte_se_lin_bwd_sums vs fte_se_bwd_gate, at the four IResNet shapes of a B-image shard (default 128); and the apply
pass, fte_se_lin_apply_fwd vs fte_se_apply_fwd.  The squeeze reads z once; fte_se_lin_bwd_sums reads dy and z, fte_se_bwd_gate reads
dy, out and z and writes g -- the byte counts below are each entry point's own.  Repeats are interleaved (sibling, new, sibling, new,
...): `rounds` windows of `reps` calls each, per window the mean time per call from device events; reported: median and min..max over
the windows, and the split count S the launcher planned (FTE_SE_LIN_BLOCKS=0: never split; =2048: a target of 2048 blocks, which also
splits the 28 x 28 x 128 stage).  Prints a markdown table.

  [FTE_SE_LIN_BLOCKS=N] python scripts/bench_se_lin.py [B] [rounds] [reps]"""
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
    q, call = _lib.query, _lib.call
    print('FTE_SE_LIN_BLOCKS=%s, %d compute units' % (os.environ.get('FTE_SE_LIN_BLOCKS', '(default)'), torch.cuda.get_device_properties(0).multi_processor_count))
    print('| pass | shape | S | sibling MB, us (min..max) | new MB, us (min..max) | ratio of medians | faster outside the sibling\'s min..max | new GB/s | of 8 TB/s |')
    print('|---|---|---|---|---|---|---|---|---|')
    for h, c in [(56, 64), (28, 128), (14, 256), (7, 512)]:
        n, hw = B, h * h
        g = torch.Generator(device='cuda').manual_seed(c)
        z = torch.randn(n, hw, c, generator=g, **f32) * 2 + 1
        dy = torch.randn(n, hw, c, generator=g, **f32)
        sc = torch.randn(n, hw, c, generator=g, **f32)
        out, gbuf = torch.empty_like(z), torch.empty_like(z)
        gamma = torch.rand(c, generator=g, **f32) + 0.5
        beta = torch.randn(c, generator=g, **f32) * 0.3
        gate = torch.sigmoid(torch.randn(n, c, generator=g, **f32))
        mean, rstd, scale, shift = (torch.empty(c, **f32) for _ in range(4))
        sq, xm, s1, s2, dg = (torch.empty(n, c, **f32) for _ in range(5))
        need = q('fte_se_lin_ws_bytes', n, hw, c)
        S = need // (2 * n * c * 4)
        ws = torch.empty(max(q('fte_bn_ws_bytes', c), need) // 4 + 1024, **f32)
        wsb = ws.numel() * 4
        call('fte_bn_train_stats', z, gamma, beta, mean, rstd, scale, shift, None, None, n * hw, c, 1e-5, 0.9, ws, wsb, st)
        call('fte_se_apply_fwd', z, scale, shift, gate, sc, out, n, hw, c, 0, st)          # `out` of the ReLU block, for its backward
        tb = z.numel() * 4
        shape = '%dx%dx%dx%d' % (B, h, h, c)
        cases = [('squeeze', tb, tb,
                  lambda: call('fte_se_squeeze', z, scale, shift, mean, rstd, sq, xm, n, hw, c, 0, st),
                  lambda: call('fte_se_lin_squeeze', z, scale, shift, mean, rstd, sq, xm, n, hw, c, ws, wsb, st)),
                 ('backward sums', 4 * tb, 2 * tb,
                  lambda: call('fte_se_bwd_gate', dy, out, z, gamma, beta, mean, rstd, gate, gbuf, s1, s2, dg, n, hw, c, 0, st),
                  lambda: call('fte_se_lin_bwd_sums', dy, z, gamma, beta, mean, rstd, gate, s1, s2, dg, n, hw, c, ws, wsb, st)),
                 ('apply', 3 * tb, 3 * tb,
                  lambda: call('fte_se_apply_fwd', z, scale, shift, gate, sc, gbuf, n, hw, c, 0, st),
                  lambda: call('fte_se_lin_apply_fwd', z, scale, shift, gate, sc, gbuf, n, hw, c, st))]
        for what, ba, bn, fa, fb in cases:
            ta, tn = ab(fa, fb)
            ma, mn = ta[len(ta) // 2], tn[len(tn) // 2]
            gbs = bn / mn / 1e3
            print('| %s | %s | %s | %.1f, %.1f (%.1f..%.1f) | %.1f, %.1f (%.1f..%.1f) | %.3f | %s | %.0f | %.0f %% |' % (
                what, shape, S if what != 'apply' else '-', ba / 1e6, ma, ta[0], ta[-1], bn / 1e6, mn, tn[0], tn[-1], mn / ma,
                'yes' if tn[-1] < ta[0] else 'no', gbs, 100 * gbs / PEAK))


if __name__ == '__main__':
    main()
