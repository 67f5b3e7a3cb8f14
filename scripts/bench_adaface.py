"""The AdaFace head's two kernels next to the batch-margin kernel they replace, at n = 512, D = 512, fp32:
fte_adaface_margins + fte_margin_softmax_rows_fwd_bwd against fte_margin_softmax_fwd_bwd on the same s / xn / wn / labels, in one
process on one GPU, every buffer allocated once.

    python scripts/bench_adaface.py [--classes 10575,85742] [--steps 20] [--repeats 7]
    python scripts/bench_adaface.py --net 1 [--classes 10575]             # whole training step, SphereNet-AdaFace and -ArcFace
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/bench_adaface.py --classes 85742 --repeats 1

Per class count it prints each kernel (HIP events around --steps back-to-back launches after warm-up, the median and the spread of
--repeats such groups), the rate of the margin kernels on the bytes they have to move (s read twice, G written: 3 n ld 4 bytes),
and the verdict of the yardstick: the new pair may be slower than the existing kernel by that run's own min..max spread of the
existing kernel plus 3 % (one extra launch, event granularity).  Nothing is gated on a time."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import _lib  # noqa: E402

N, D = 512, 512
ARC = (64.0, 0.5, 0.0)
ADA = (0.4, 0.333, 0.01)      # m, h, t_alpha


def timed(fn, steps, repeats, warm=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return float(np.median(out)), float(min(out)), float(max(out))


def head(c, steps, repeats):
    call, q = _lib.call, _lib.query
    st = torch.cuda.current_stream().cuda_stream
    ld = (c + 127) // 128 * 128
    f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    W = torch.randn(D, ld, generator=g, **f32)
    W[:, c:] = 0
    x = torch.randn(N, D, generator=g, **f32) * (0.5 + torch.rand(N, 1, generator=g, **f32))
    y = torch.randint(0, c, (N,), generator=g, **i32)
    wsb = max(q('fte_gemm_ws_bytes', N, ld, D), 4096)
    ws = torch.empty(wsb // 4 + 1024, **f32)
    s, G = torch.empty(N, ld, **f32), torch.empty(N, ld, **f32)
    xn, wn = torch.empty(N, **f32), torch.empty(ld, **f32)
    rows, rowcoef, a_rows, b_rows = (torch.empty(N, **f32) for _ in range(4))
    call('fte_gemm_nn', x, W, None, s, N, ld, D, ws, ws.numel() * 4, st)
    call('fte_row_norms', x, xn, N, D, D, st)
    call('fte_col_norms', W, wn, D, c, ld, st)
    torch.cuda.synchronize()
    q_ = xn.clamp(1e-3, 100.0)
    stats = torch.stack([q_.mean(), q_.std()])          # near the batch's own: the margins span both clip ends

    def batch():
        call('fte_margin_softmax_fwd_bwd', s, xn, wn, y, *ARC, None, rows, G, rowcoef, N, c, ld, 1.0 / N, st)

    def margins():
        call('fte_adaface_margins', xn, N, *ADA, 0, stats, a_rows, b_rows, st)

    def per_row():
        call('fte_margin_softmax_rows_fwd_bwd', s, xn, wn, y, ARC[0], a_rows, b_rows, None, rows, G, rowcoef, N, c, ld, 1.0 / N, st)

    def pair():
        margins()
        per_row()
    res = {}
    for name, fn in (('batch', batch), ('pair', pair), ('per_row', per_row), ('margins', margins), ('batch_again', batch)):
        res[name] = timed(fn, steps, repeats)
    nbytes = 3.0 * N * ld * 4
    print('C=%d ld=%d (n=%d, D=%d, fp32; %d launches per group, median [min, max] of %d groups)' % (c, ld, N, D, steps, repeats))
    for name, label in (('batch', 'fte_margin_softmax_fwd_bwd'), ('batch_again', 'fte_margin_softmax_fwd_bwd (again)'),
                        ('per_row', 'fte_margin_softmax_rows_fwd_bwd'), ('margins', 'fte_adaface_margins'),
                        ('pair', 'margins + per-row kernel')):
        rate = '   %.2f TB/s' % (nbytes / res[name][0] / 1e6) if name != 'margins' else ''
        print('  %-36s %8.1f us [%.1f, %.1f]%s' % ((label,) + res[name] + (rate,)))
    base = res['batch']
    allowed = base[0] + (base[2] - base[1]) + 0.03 * base[0]
    print('  yardstick: existing %.1f us + its spread %.1f us + 3 %% = %.1f us; the new pair %.1f us: %s'
          % (base[0], base[2] - base[1], allowed, res['pair'][0], 'within' if res['pair'][0] <= allowed else 'SLOWER'))


def net_step(c, steps, repeats):
    from tf_face_toolbox_amd import net_select, Singular
    out = {}
    for name in ('SphereNet-ArcFace', 'SphereNet-AdaFace'):
        net = net_select(name, 'NCHW', 5e-4)
        g = torch.Generator(device='cuda').manual_seed(0)
        inputs = {'images': torch.rand(N, 112, 96, 3, generator=g, device='cuda') * 2 - 1,
                  'labels': torch.randint(0, c, (N,), generator=g, device='cuda', dtype=torch.int32), 'num_classes': c, 'num_examples': N}
        step, losses, names, others = Singular(net, 0.01, 'Momentum')(inputs)
        out[name] = timed(step, steps, repeats, warm=3)
        assert np.isfinite(float(losses[0]))
        del net, step, inputs
        torch.cuda.empty_cache()
    print('training step, %d images of 112x96x3, C=%d, fp32 (%d steps per group, median [min, max] of %d groups)' % (N, c, steps, repeats))
    for name in out:
        print('  %-18s %9.1f us [%.1f, %.1f]' % ((name,) + out[name]))
    print('  AdaFace / ArcFace: %.4f' % (out['SphereNet-AdaFace'][0] / out['SphereNet-ArcFace'][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=str, default='10575,85742')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--net', type=int, default=0)
    a = ap.parse_args()
    _lib.load()
    for c in [int(v) for v in a.classes.split(',')]:
        (net_step if a.net else head)(c, a.steps, a.repeats)


if __name__ == '__main__':
    main()
