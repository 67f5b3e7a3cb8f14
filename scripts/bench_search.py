"""Evaluation kernels at the issue's shapes: fused similarity + top-k (fte_topk_search, via
verification.topk_search) and fused similarity + score histograms (verification.score_histograms), against torch.mm + torch.topk
and torch.mm + torch.histc at the same shapes (outside the product path, for comparison only).  Inputs come from a seed.
Prints one line per shape: ms, executed TFLOP/s (2 m n d; n (n - 1) d for the triangle) and the fraction of the 157.3 TF fp32
MFMA peak.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel times."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import verification as V  # noqa: E402

PEAK = 157.3e12


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def torch_topk(P, G, k, rows):
    best = None
    for g0 in range(0, G.shape[0], rows):
        s, i = torch.topk(torch.mm(P, G[g0:g0 + rows].t()), k, dim=1)
        i = i + g0
        if best is not None:
            s, j = torch.topk(torch.cat((best[0], s), 1), k, dim=1)
            i = torch.gather(torch.cat((best[1], i), 1), 1, j)
        best = (s, i)
    return best


def torch_hist(X, nbins, rows):
    n = X.shape[0]
    h = torch.zeros(nbins, device=X.device)
    for a0 in range(0, n, rows):
        for b0 in range(a0, n, rows):
            s = torch.mm(X[a0:a0 + rows], X[b0:b0 + rows].t())
            if a0 == b0:
                s = s[torch.triu(torch.ones_like(s, dtype=torch.bool), 1)]
            h += torch.histc(s, nbins, -1.0, 1.0)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch comparison')
    ap.add_argument('--scale', type=float, default=1.0, help='scale n (a quick run at a smaller size)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device='cuda').manual_seed(a.seed)
    out = []
    for m, n, d, k in ((3530, 1000000, 512, 10), (4096, 262144, 512, 64)):
        n = int(n * a.scale)
        P = V.normalize(torch.randn(m, d, device='cuda', generator=g))
        G = V.normalize(torch.randn(n, d, device='cuda', generator=g))
        fl = 2.0 * m * n * d
        ms = timed(lambda: V.topk_search(P, G, k), a.iters)
        r = {'op': 'topk', 'm': m, 'n': n, 'd': d, 'k': k, 'ms': round(ms, 3), 'tflops': round(fl / ms / 1e9, 2),
             'of_peak': round(fl / ms / 1e-3 / PEAK, 3)}
        if not a.no_torch:
            tms = timed(lambda: torch_topk(P, G, k, 131072), a.iters)
            r.update(torch_ms=round(tms, 3), speedup=round(tms / ms, 2))
        print(json.dumps(r), flush=True)
        out.append(r)
        del G
        torch.cuda.empty_cache()
    n, d = int(100000 * a.scale), 512
    X = V.normalize(torch.randn(n, d, device='cuda', generator=g))
    labels = (torch.arange(n) // 10).numpy()
    fl = float(n) * (n - 1) * d
    ms = timed(lambda: V.score_histograms(X, labels, 8192), a.iters)
    r = {'op': 'histograms', 'n': n, 'd': d, 'nbins': 8192, 'ms': round(ms, 3), 'tflops': round(fl / ms / 1e9, 2),
         'of_peak': round(fl / ms / 1e-3 / PEAK, 3)}
    if not a.no_torch:
        tms = timed(lambda: torch_hist(X, 8192, 16384), a.iters)
        r.update(torch_ms=round(tms, 3), speedup=round(tms / ms, 2))
    print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
