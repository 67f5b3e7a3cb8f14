"""The MagFace head's kernel next to the ArcFace kernel and the AdaFace pair, at n = 512, D = 512, fp32:
fte_magface_softmax_fwd_bwd against fte_margin_softmax_fwd_bwd and fte_adaface_margins + fte_margin_softmax_rows_fwd_bwd on the same
s / xn / wn / labels / G, in one process on one GPU, every buffer allocated once.

    python scripts/bench_magface.py [--classes 10575,85742] [--steps 20] [--repeats 9]
    python scripts/bench_magface.py --net 1 [--classes 10575]          # whole training step, SphereNet-MagFace and -ArcFace

The sides ALTERNATE: each of the --repeats rounds times one group of --steps back-to-back launches of every variant in turn (HIP
events around the group, after a warm-up of all of them), so a drift of the machine falls on all.  Per class count it prints the
median [min, max] of each variant, the rate of the softmax kernels on the bytes they have to move (s read twice, G written:
3 n ld 4 bytes) against the HBM roof, the ratios to ArcFace round by round, and ArcFace's own spread.  Nothing is gated on a time."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import _lib  # noqa: E402

N, D = 512, 512
ARC = (64.0, 0.5, 0.0)
ADA = (0.4, 0.333, 0.01)                 # m, h, t_alpha
MAG = (64.0, 10.0, 110.0, 0.45, 0.8, 35.0)
HBM_SPEC, HBM_COPY = 8.0, 6.29      # TB/s: the part's specification, and what a float4 copy reaches on it


def group(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def alternate(fns, steps, repeats, warm=5):
    """name -> the per-launch microseconds of `repeats` groups, the variants taking turns within every round"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = dict((k, []) for k in fns)
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(group(fn, steps))
    return out


def mmm(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def head(c, steps, repeats):
    call, q = _lib.call, _lib.query
    st = torch.cuda.current_stream().cuda_stream
    ld = (c + 127) // 128 * 128
    f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    W = torch.randn(D, ld, generator=g, **f32)
    W[:, c:] = 0
    y = torch.randint(0, c, (N,), generator=g, **i32)
    # target cosines spread over [-0.9, 0.9]; norms over [2, 150]: rows below l_a, inside [l_a, u_a] and above u_a
    wy = W[:, y.long()] / W[:, y.long()].norm(dim=0)
    a = torch.rand(N, generator=g, **f32) * 1.8 - 0.9
    e = torch.randn(D, N, generator=g, **f32)
    e = e - (e * wy).sum(0) * wy
    x = ((a * wy + (1 - a * a).sqrt() * e / e.norm(dim=0)) * (2 + 148 * torch.rand(N, generator=g, **f32))).t().contiguous()
    wsb = max(q('fte_gemm_ws_bytes', N, ld, D), 4096)
    ws = torch.empty(wsb // 4 + 1024, **f32)
    s, G = torch.empty(N, ld, **f32), torch.empty(N, ld, **f32)
    xn, wn = torch.empty(N, **f32), torch.empty(ld, **f32)
    rows, reg, rowcoef = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, **f32)
    stats, a_rows, b_rows = torch.tensor([60.0, 40.0], **f32), torch.empty(N, **f32), torch.empty(N, **f32)
    call('fte_gemm_nn', x, W, None, s, N, ld, D, ws, ws.numel() * 4, st)
    call('fte_row_norms', x, xn, N, D, D, st)
    call('fte_col_norms', W, wn, D, c, ld, st)
    torch.cuda.synchronize()

    def arc():
        call('fte_margin_softmax_fwd_bwd', s, xn, wn, y, *ARC, None, rows, G, rowcoef, N, c, ld, 1.0 / N, st)

    def ada():
        call('fte_adaface_margins', xn, N, *ADA, 0, stats, a_rows, b_rows, st)              # update = 0: the same margins in every launch
        call('fte_margin_softmax_rows_fwd_bwd', s, xn, wn, y, 64.0, a_rows, b_rows, None, rows, G, rowcoef, N, c, ld, 1.0 / N, st)

    def mag():
        call('fte_magface_softmax_fwd_bwd', s, xn, wn, y, *MAG, None, rows, reg, G, rowcoef, N, c, ld, 1.0 / N, st)
    inside = float(((xn >= MAG[1]) & (xn <= MAG[2])).float().mean())
    res = alternate(dict(arc=arc, ada=ada, mag=mag), steps, repeats)
    nbytes = 3.0 * N * ld * 4
    print('C=%d ld=%d (n=%d, D=%d, fp32, %.0f %% of the rows inside [l_a, u_a]; %d launches per group, median [min, max] of %d alternating rounds)'
          % (c, ld, N, D, 100 * inside, steps, repeats))
    for name, label in (('arc', 'fte_margin_softmax_fwd_bwd'), ('ada', 'adaface_margins + rows kernel'), ('mag', 'fte_magface_softmax_fwd_bwd')):
        tb = nbytes / mmm(res[name])[0] / 1e6
        rate = '   %.2f TB/s = %.0f %% of %.1f (spec), %.0f %% of %.2f (copy)' % (tb, 100 * tb / HBM_SPEC, HBM_SPEC, 100 * tb / HBM_COPY, HBM_COPY)
        print('  %-32s %8.1f us [%.1f, %.1f]%s' % ((label,) + mmm(res[name]) + (rate,)))
    for name, label in (('mag', 'MagFace / ArcFace'), ('ada', 'AdaFace pair / ArcFace')):
        ratio = [p / b for p, b in zip(res[name], res['arc'])]
        print('  %-32s %.4f [%.4f, %.4f] round by round' % ((label,) + mmm(ratio)))
    b = mmm(res['arc'])
    print('  ArcFace spread (max - min) / median: %.4f' % ((b[2] - b[1]) / b[0]))


def net_step(c, steps, repeats):
    from tf_face_toolbox_amd import net_select, Singular
    fns, keep = {}, []
    for name in ('SphereNet-ArcFace', 'SphereNet-MagFace'):
        net = net_select(name, 'NCHW', 5e-4)
        g = torch.Generator(device='cuda').manual_seed(0)
        inputs = {'images': torch.rand(N, 112, 96, 3, generator=g, device='cuda') * 2 - 1,
                  'labels': torch.randint(0, c, (N,), generator=g, device='cuda', dtype=torch.int32), 'num_classes': c, 'num_examples': N}
        step, losses, names, others = Singular(net, 0.01, 'Momentum')(inputs)
        fns[name] = step
        keep.append((net, inputs, losses))
    res = alternate(fns, steps, repeats, warm=3)
    assert all(np.isfinite(float(k[2][0])) for k in keep)
    print('training step, %d images of 112x96x3, C=%d, fp32 (%d steps per group, median [min, max] of %d alternating rounds)' % (N, c, steps, repeats))
    for name in res:
        print('  %-26s %9.1f us [%.1f, %.1f]' % ((name,) + mmm(res[name])))
    ratio = [p / b for p, b in zip(res['SphereNet-MagFace'], res['SphereNet-ArcFace'])]
    print('  MagFace / ArcFace: %.4f [%.4f, %.4f] round by round' % mmm(ratio))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=str, default='10575,85742')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--net', type=int, default=0)
    a = ap.parse_args()
    _lib.load()
    for c in [int(v) for v in a.classes.split(',')]:
        (net_step if a.net else head)(c, a.steps, a.repeats)


if __name__ == '__main__':
    main()
