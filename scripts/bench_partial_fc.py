"""The sampled-class (Partial FC) margin head next to the dense one at n = 512, D = 512, fp32:
one head step = sample + gather + three classifier products + margin kernel + colcoef + scatter (sampled) against the calls of
loss.additive_margin_loss (dense), every buffer allocated once.

    python scripts/bench_partial_fc.py [--classes 85742,1000000] [--rate 0.1] [--steps 20] [--repeats 5]
    python scripts/bench_partial_fc.py --net 1 [--classes 1000000]        # whole SphereNet-ArcFace training step, rate 1 and --rate
    python scripts/bench_partial_fc.py --update 1 [--classes 85742,1000000]  # scatter + dense Momentum update against the fused update
    python scripts/bench_partial_fc.py --net 1 --compact 1 --classes 1000000  # the sampled step with and without compact_head_update
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/bench_partial_fc.py --classes 1000000 --repeats 1

Per class count it prints: the dense and the sampled head step (HIP events around --steps back-to-back steps after warm-up, the
median and the spread of --repeats such groups), their ratio, the share of gather + scatter in the sampled step, and each new
kernel on its own with its rate on the bytes it has to move: gather = the 128-byte lines of W that hold a sampled column (counted
from the index) + Ws written; scatter = dW written + dWs and the inverse map read; sampler = six passes over the class flags + the
inverse map and index written.

--update 1 times the classifier's share of the optimizer step on one set of buffers in one process: fte_pfc_scatter_cols into the dense
dW followed by fte_momentum_update over D * cpad (what the step runs without compact_head_update) against
fte_pfc_momentum_update_cols, the two alternating group by group (same events, same warm-up), the inverse map from a real
fte_pfc_sample.  Bytes the two have to move: pair = dW written and read + W and the slot read and written (6 x D x cpad x 4) + dWs
+ the inverse map; fused = W and the slot read and written (4 x D x cpad x 4) + dWs + the inverse map."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import _lib  # noqa: E402
from tf_face_toolbox_amd.loss import sample_size  # noqa: E402

N, D = 512, 512
PRESET = (64.0, 0.5, 0.0)


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


def head(c, rate, steps, repeats):
    call, q = _lib.call, _lib.query
    st = torch.cuda.current_stream().cuda_stream
    ld = (c + 127) // 128 * 128
    S = sample_size(c, rate)
    spad = (S + 63) // 64 * 64
    f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    W = torch.randn(D, ld, generator=g, **f32)
    W[:, c:] = 0
    x = torch.randn(N, D, generator=g, **f32) * 4
    y = torch.randint(0, c, (N,), generator=g, **i32)
    wsb = max(q('fte_gemm_ws_bytes', N, ld, D), q('fte_gemm_ws_bytes', N, spad, D), q('fte_pfc_sample_ws_bytes', c), 4096)
    ws = torch.empty(wsb // 4 + 1024, **f32)
    wsb = ws.numel() * 4
    xn, rowcoef, rows, dx = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, D, **f32)
    dW = torch.empty(D, ld, **f32)
    res = {}

    # ---- dense: the calls of loss.additive_margin_loss
    s, G = torch.empty(N, ld, **f32), torch.empty(N, ld, **f32)
    wn, colcoef = torch.empty(ld, **f32), torch.empty(ld, **f32)

    def dense():
        call('fte_gemm_nn', x, W, None, s, N, ld, D, ws, wsb, st)
        call('fte_row_norms', x, xn, N, D, D, st)
        call('fte_col_norms', W, wn, D, c, ld, st)
        call('fte_margin_softmax_fwd_bwd', s, xn, wn, y, *PRESET, None, rows, G, rowcoef, N, c, ld, 1.0 / N, st)
        call('fte_asoftmax_colcoef', G, s, wn, colcoef, N, c, ld, st)
        call('fte_gemm_tn', x, G, dW, N, ld, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dW, W, None, colcoef, D, ld, ld, st)
        call('fte_gemm_nt', G, W, None, None, 0, None, dx, None, N, ld, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dx, x, rowcoef, None, N, D, D, st)
    res['dense'] = timed(dense, steps, repeats)
    del s, G, wn, colcoef

    # ---- sampled
    index, inverse, ys = torch.empty(spad, **i32), torch.empty(c, **i32), torch.empty(N, **i32)
    Ws, dWs = torch.empty(D, spad, **f32), torch.empty(D, spad, **f32)
    s, G = torch.empty(N, spad, **f32), torch.empty(N, spad, **f32)
    wn, colcoef = torch.empty(spad, **f32), torch.empty(spad, **f32)
    t = [0]

    def sample():
        t[0] += 1
        call('fte_pfc_sample', y, N, c, S, 1, t[0], index, inverse, ys, ws, wsb, st)

    def gather():
        call('fte_pfc_gather_cols', W, index, Ws, D, c, ld, S, spad, st)

    def scatter():
        call('fte_pfc_scatter_cols', dWs, inverse, dW, D, c, ld, S, spad, st)

    def sampled():
        sample()
        gather()
        call('fte_gemm_nn', x, Ws, None, s, N, spad, D, ws, wsb, st)
        call('fte_row_norms', x, xn, N, D, D, st)
        call('fte_col_norms', Ws, wn, D, S, spad, st)
        call('fte_margin_softmax_fwd_bwd', s, xn, wn, ys, *PRESET, None, rows, G, rowcoef, N, S, spad, 1.0 / N, st)
        call('fte_asoftmax_colcoef', G, s, wn, colcoef, N, S, spad, st)
        call('fte_gemm_tn', x, G, dWs, N, spad, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dWs, Ws, None, colcoef, D, spad, spad, st)
        scatter()
        call('fte_gemm_nt', G, Ws, None, None, 0, None, dx, None, N, spad, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dx, x, rowcoef, None, N, D, D, st)
    res['sampled'] = timed(sampled, steps, repeats)
    for name, fn in (('sample', sample), ('gather', gather), ('scatter', scatter)):
        res[name] = timed(fn, steps, repeats)
    torch.cuda.synchronize()
    idx = index[:S].cpu().numpy()
    lines = len(np.unique(idx // 32))                          # 128-byte lines of one row of W that hold a sampled column
    nbytes = {'sample': 6.0 * c + 4.0 * c + 4.0 * S, 'gather': D * (lines * 128.0 + spad * 4.0),
              'scatter': D * (ld * 4.0 + spad * 4.0) + 4.0 * c}
    dm, sm = res['dense'][0], res['sampled'][0]
    print('C=%d ld=%d rate=%g S=%d Spad=%d (n=%d, D=%d, fp32; %d steps per group, median [min, max] of %d groups)'
          % (c, ld, rate, S, spad, N, D, steps, repeats))
    print('  dense head   %9.1f us [%.1f, %.1f]' % res['dense'])
    print('  sampled head %9.1f us [%.1f, %.1f]   ratio %.2fx' % (res['sampled'] + (dm / sm,)))
    print('  gather + scatter share of the sampled head: %.1f %%' % (100.0 * (res['gather'][0] + res['scatter'][0]) / sm))
    for name in ('sample', 'gather', 'scatter'):
        us = res[name][0]
        print('  %-8s %9.1f us [%.1f, %.1f]   %.3f GB -> %.2f TB/s' % ((name,) + res[name] + (nbytes[name] / 1e9, nbytes[name] / us / 1e6)))


def timed_ab(fa, fb, steps, repeats, warm=5):
    """timed() for two callables on the same buffers, their groups alternating: A B A B ..."""
    for _ in range(warm):
        fa()
        fb()
    out = ([], [])
    for _ in range(repeats):
        for k, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / steps)
    return tuple((float(np.median(o)), float(min(o)), float(max(o))) for o in out)


def update(c, rate, steps, repeats):
    call, q = _lib.call, _lib.query
    st = torch.cuda.current_stream().cuda_stream
    ld = (c + 127) // 128 * 128
    S = sample_size(c, rate)
    spad = (S + 63) // 64 * 64
    f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    W = torch.randn(D, ld, generator=g, **f32)
    acc = torch.zeros(D, ld, **f32)
    dW = torch.empty(D, ld, **f32)
    dWs = torch.randn(D, spad, generator=g, **f32) * 1e-3
    y = torch.randint(0, c, (N,), generator=g, **i32)
    index, inverse, ys = torch.empty(spad, **i32), torch.empty(c, **i32), torch.empty(N, **i32)
    ws = torch.empty(q('fte_pfc_sample_ws_bytes', c) // 4 + 1024, **f32)
    call('fte_pfc_sample', y, N, c, S, 1, 1, index, inverse, ys, ws, ws.numel() * 4, st)
    scal = (0.01, 0.9, 5e-4, 1.0)

    def pair():
        call('fte_pfc_scatter_cols', dWs, inverse, dW, D, c, ld, S, spad, st)
        call('fte_momentum_update', W, acc, dW, D * ld, *scal, st)

    def fused():
        call('fte_pfc_momentum_update_cols', W, acc, dWs, inverse, D, c, ld, S, spad, *scal, st)
    a, b = timed_ab(pair, fused, steps, repeats)
    assert bool(torch.isfinite(W).all())
    small = D * spad * 4.0 + 4.0 * c
    ba, bb = 6.0 * D * ld * 4 + small, 4.0 * D * ld * 4 + small
    print('C=%d ld=%d rate=%g S=%d Spad=%d (D=%d, fp32 Momentum; %d calls per group, groups alternating, median [min, max] of %d groups)'
          % (c, ld, rate, S, spad, D, steps, repeats))
    print('  scatter + dense update %9.1f us [%.1f, %.1f]   %.3f GB -> %.2f TB/s' % (a + (ba / 1e9, ba / a[0] / 1e6)))
    print('  fused update           %9.1f us [%.1f, %.1f]   %.3f GB -> %.2f TB/s' % (b + (bb / 1e9, bb / b[0] / 1e6)))
    print('  ratio %.2fx (by bytes at most %.2fx)' % (a[0] / b[0], ba / bb))


def net_step(c, rate, steps, repeats, compact=False):
    from tf_face_toolbox_amd import net_select, Singular
    out = {}
    for r in ((rate, 'compact') if compact else (1.0, rate)):
        net = net_select('SphereNet-ArcFace', 'NCHW', 5e-4)
        net.set_sample_rate(rate if r == 'compact' else r, 0)
        net.compact_head_update = r == 'compact'
        g = torch.Generator(device='cuda').manual_seed(0)
        inputs = {'images': torch.rand(N, 112, 96, 3, generator=g, device='cuda') * 2 - 1,
                  'labels': torch.randint(0, c, (N,), generator=g, device='cuda', dtype=torch.int32), 'num_classes': c, 'num_examples': N}
        step, losses, names, others = Singular(net, 0.01, 'Momentum')(inputs)
        out[r] = timed(step, steps, repeats, warm=3)
        assert np.isfinite(float(losses[0]))
        del net, step, inputs
        torch.cuda.empty_cache()
    print('SphereNet-ArcFace training step, %d images of 112x96x3, C=%d, fp32 (%d steps per group, median [min, max] of %d groups)'
          % (N, c, steps, repeats))
    if compact:
        print('  --sample_rate %-4g                        %9.1f us [%.1f, %.1f]' % ((rate,) + out[rate]))
        print('  --sample_rate %-4g --compact_head_update 1%9.1f us [%.1f, %.1f]   ratio %.2fx'
              % ((rate,) + out['compact'] + (out[rate][0] / out['compact'][0],)))
        return
    print('  --sample_rate 1   %9.1f us [%.1f, %.1f]' % out[1.0])
    print('  --sample_rate %-4g%9.1f us [%.1f, %.1f]   ratio %.2fx' % ((rate,) + out[rate] + (out[1.0][0] / out[rate][0],)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=str, default='85742,1000000')
    ap.add_argument('--rate', type=float, default=0.1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--net', type=int, default=0)
    ap.add_argument('--update', type=int, default=0)
    ap.add_argument('--compact', type=int, default=0)
    a = ap.parse_args()
    _lib.load()
    for c in [int(v) for v in a.classes.split(',')]:
        if a.net:
            net_step(c, a.rate, a.steps, a.repeats, bool(a.compact))
        else:
            (update if a.update else head)(c, a.rate, a.steps, a.repeats)


if __name__ == '__main__':
    main()
