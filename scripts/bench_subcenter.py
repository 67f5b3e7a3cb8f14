"""The sub-center ArcFace kernels at n = 512 (profiles/subcenter.md):

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/bench_subcenter.py --kernels 1 [--runs 5]
    python scripts/bench_subcenter.py --kernels 1        # the same launches under HIP events
    python scripts/bench_subcenter.py --net 1            # whole SphereNet-ArcFace training step at 512 images, K = 1 and K = --K
    python scripts/bench_subcenter.py --assign 1         # fte_subcenter_assign, samples/s at d = 512

--kernels: fte_subcenter_margin_softmax_fwd_bwd at c = --classes, K = --K against fte_margin_softmax_fwd_bwd at c = K * classes --
the same bytes of s and G -- the two alternating run by run; under rocprofv3 read the two kernels' rows of the kernel statistics."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import _lib  # noqa: E402

N, D = 512, 512
PRESET = (64.0, 0.5, 0.0)


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def kernels(c, K, runs):
    call = _lib.call
    st = torch.cuda.current_stream().cuda_stream
    ld = (c + 127) // 128 * 128
    wide = (K * c + 127) // 128 * 128
    f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    xn = torch.rand(N, generator=g, **f32) * 10 + 1
    y = torch.randint(0, c, (N,), generator=g, **i32)
    rows, rc = torch.empty(N, **f32), torch.empty(N, **f32)
    # planar K-centre operands, and the one-centre head over K * c classes: the same bytes of s and G
    sK = torch.randn(N, K * ld, generator=g, **f32) * 30
    wK = torch.rand(K * ld, generator=g, **f32) * 3 + 20
    GK = torch.empty(N, K * ld, **f32)
    s1 = torch.randn(N, wide, generator=g, **f32) * 30
    w1 = torch.rand(wide, generator=g, **f32) * 3 + 20
    G1 = torch.empty(N, wide, **f32)

    def pooled():
        call('fte_subcenter_margin_softmax_fwd_bwd', sK, xn, wK, y, K, *PRESET, None, rows, GK, rc, N, c, ld, 1.0 / N, st)

    def plain():
        call('fte_margin_softmax_fwd_bwd', s1, xn, w1, y, *PRESET, None, rows, G1, rc, N, K * c, wide, 1.0 / N, st)
    for _ in range(3):
        pooled()
        plain()
    torch.cuda.synchronize()
    tp, tq = [], []
    for _ in range(runs):
        tp.append(_events(pooled))
        tq.append(_events(plain))
    nbytes = 3.0 * N * K * ld * 4                                # s read twice, G written once
    for name, t in (('fte_subcenter_margin_softmax_fwd_bwd n=%d c=%d K=%d' % (N, c, K), tp), ('fte_margin_softmax_fwd_bwd n=%d c=%d' % (N, K * c), tq)):
        print('%-58s mean %8.1f us [%.1f, %.1f] over %d runs   %.2f TB/s' % (name, np.mean(t), min(t), max(t), runs, nbytes / np.mean(t) / 1e6))


def assign(K, n, runs):
    from tf_face_toolbox_amd import subcenter
    c = 85742
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(n, D, generator=g, device='cuda')
    Wt = torch.randn(K * c, D, generator=g, device='cuda')
    y = torch.randint(0, c, (n,), generator=g, device='cuda', dtype=torch.int32)
    for _ in range(2):
        subcenter.assign(x, Wt, y, K, c)
    t = [_events(lambda: subcenter.assign(x, Wt, y, K, c)) for _ in range(runs)]
    print('fte_subcenter_assign n=%d d=%d K=%d c=%d: mean %.1f us [%.1f, %.1f] over %d runs (output allocation included) -> %.1f M samples/s'
          % (n, D, K, c, np.mean(t), min(t), max(t), runs, n / np.mean(t)))


def net_step(c, K, steps, runs):
    from tf_face_toolbox_amd import net_select, Singular
    for k in (1, K):
        net = net_select('SphereNet-ArcFace', 'NCHW', 5e-4, sub_centers=k)
        g = torch.Generator(device='cuda').manual_seed(0)
        inputs = {'images': torch.rand(N, 112, 96, 3, generator=g, device='cuda') * 2 - 1,
                  'labels': torch.randint(0, c, (N,), generator=g, device='cuda', dtype=torch.int32), 'num_classes': c, 'num_examples': N}
        step, losses, names, others = Singular(net, 0.01, 'Momentum')(inputs)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t = [_events(lambda: [step() for _ in range(steps)]) / steps for _ in range(runs)]
        assert np.isfinite(float(losses[0]))
        print('SphereNet-ArcFace step, %d images of 112x96x3, C=%d, sub_centers=%d, fp32: mean %.1f us [%.1f, %.1f] over %d groups of %d steps'
              % (N, c, k, np.mean(t), min(t), max(t), runs, steps))
        del net, step, inputs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=int, default=85742)
    ap.add_argument('--K', type=int, default=3)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--kernels', type=int, default=0)
    ap.add_argument('--assign', type=int, default=0)
    ap.add_argument('--samples', type=int, default=1 << 18)
    ap.add_argument('--net', type=int, default=0)
    a = ap.parse_args()
    _lib.load()
    if a.kernels:
        kernels(a.classes, a.K, a.runs)
    if a.assign:
        assign(a.K, a.samples, a.runs)
    if a.net:
        net_step(a.classes, a.K, a.steps, a.runs)


if __name__ == '__main__':
    main()
