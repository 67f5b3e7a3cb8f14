"""The additive-margin head's kernel next to A-softmax's at the classifier shapes of the 512-image step:
n = 512, C = 10575 (ld 10624) and C = 85742 (ld 85760, MS1MV2), f = NULL for both.  Both read s and write G.

    python scripts/bench_margin.py [--iters 50]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/bench_margin.py

Prints one line per kernel and shape: mean time from HIP events and the rate on 2 * n * ld * 4 bytes (the s read and the G write;
the second pass over s is not counted)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import _lib  # noqa: E402

SHAPES = [(512, 10575, 10624), (512, 85742, 85760)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for n, c, ld in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(0)
        s = torch.randn(n, ld, device='cuda', generator=g) * 3.0
        s[:, c:] = 0
        xn = torch.rand(n, device='cuda', generator=g) * 10 + 5
        wn = torch.rand(ld, device='cuda', generator=g) * 2 + 22
        labels = torch.randint(0, c, (n,), device='cuda', dtype=torch.int32, generator=g)
        G = torch.empty(n, ld, device='cuda')
        rows, rc = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
        runs = {
            'margin_softmax_kernel': lambda: _lib.call('fte_margin_softmax_fwd_bwd', s, xn, wn, labels, 64.0, 0.5, 0.0, None, rows, G, rc,
                                                       n, c, ld, 1.0 / n, st),
            'asoftmax_kernel': lambda: _lib.call('fte_asoftmax_fwd_bwd', s, xn, wn, labels, 5.0, None, rows, G, rc, n, c, ld, 1.0 / n, st),
        }
        for name, fn in runs.items():
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.iters
            tbs = 2.0 * n * ld * 4 / (us * 1e-6) / 1e12
            print('%-22s n=%d C=%d ld=%d: %8.1f us  %.2f TB/s on 2*n*ld*4 bytes (%.0f %% of 6.3)' % (name, n, c, ld, us, tbs, tbs / 6.3 * 100))


if __name__ == '__main__':
    main()
