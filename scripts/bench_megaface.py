"""The MegaFace scan at challenge-1 shape: 3,530 probes in 80 identity clusters (genuine cosines about
0.4 - 0.8), 1,000,000 random distractors, d = 512, all six sizes 10 .. 10^6 in one pass (verification.megaface_scan, i.e.
fte_megaface_scan per size bucket), against a torch baseline of the same counts (chunked torch.mm, torch.searchsorted of every
score into the probe's thresholds, torch.histc; outside the product path, for comparison only).  Inputs come from a seed.
Prints one JSON line: ms per call (wall, with synchronise), executed TFLOP/s (2 m n d) and the fraction of the 157.3 TF fp32
MFMA peak.  Run it under `rocprofv3 --kernel-trace --stats` (on its own) for the kernel times."""
import argparse
import json
import os
import sys
import time

import numpy as np
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


def probes_in_clusters(m, ids, d, g):
    """unit rows around `ids` unit centres; per cluster a noise level s^2 in [0.3, 1.4], so same-cluster cosines are about
    1 / (1 + s^2): 0.4 .. 0.8"""
    labels = torch.arange(m) % ids
    c = torch.nn.functional.normalize(torch.randn(ids, d, device='cuda', generator=g), dim=1)
    s2 = 0.3 + 1.1 * torch.rand(ids, device='cuda', generator=g)
    x = c[labels.cuda()] + torch.sqrt(s2[labels.cuda()] / d)[:, None] * torch.randn(m, d, device='cuda', generator=g)
    return V.normalize(x), labels.numpy()


def torch_counts(P, D, sizes, off, thr, nbins, rows):
    """the same counts and histograms: thresholds padded per probe (ascending, +inf pads), searchsorted of every score, a
    per-probe bincount turned into suffix sums"""
    m = P.shape[0]
    per = np.diff(off)
    tm = int(per.max()) if len(per) else 1
    pad = np.full((m, tm), np.inf, np.float32)
    for p in range(m):
        pad[p, :per[p]] = thr[off[p]:off[p + 1]][::-1]
    tasc = torch.from_numpy(pad).cuda()
    base = (torch.arange(m, device='cuda') * (tm + 1))[:, None]
    cnt, hist = [], []
    lo = 0
    for hi in sizes:
        c = torch.zeros(m * (tm + 1), dtype=torch.int64, device='cuda')
        h = torch.zeros(nbins, dtype=torch.float64, device='cuda')     # fp32 sums would lose counts past 2^24
        for g0 in range(lo, hi, rows):
            S = torch.mm(P, D[g0:min(hi, g0 + rows)].t())
            idx = torch.searchsorted(tasc, S, right=True)          # thresholds <= s
            c += torch.bincount((idx + base).view(-1), minlength=m * (tm + 1))
            h += torch.histc(S, nbins, -1.0, 1.0).double()
        cnt.append(c.view(m, tm + 1))
        hist.append(h)
        lo = hi
    cnt = torch.cumsum(torch.stack(cnt), 0)
    # #{s >= thr_asc[k]} = #{idx > k}
    ge = torch.flip(torch.cumsum(torch.flip(cnt, [2]), 2), [2])[:, :, 1:]
    return ge, torch.cumsum(torch.stack(hist), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch comparison')
    ap.add_argument('--scale', type=float, default=1.0, help='scale the distractor count (a quick run at a smaller size)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device='cuda').manual_seed(a.seed)
    m, ids, d, nbins = 3530, 80, 512, 8192
    n = int(1000000 * a.scale)
    sizes = [N for N in (10, 100, 1000, 10000, 100000, 1000000) if N < n] + [n]
    P, labels = probes_in_clusters(m, ids, d, g)
    D = V.normalize(torch.randn(n, d, device='cuda', generator=g))
    ip, ig, off, _ = V.megaface_pairs(labels)
    t0 = time.perf_counter()
    sg = V.megaface_pair_scores(P, ip, ig).cpu().numpy()
    pair_ms = (time.perf_counter() - t0) * 1e3
    thr, perm = V.megaface_thresholds(sg, off)
    fl = 2.0 * m * n * d
    res = {}
    ms = timed(lambda: res.__setitem__('r', V.megaface_scan(P, D, sizes, off, thr, nbins)), a.iters)
    counts, hist = res['r']
    rank1 = float(np.mean(counts[-1] == 0))
    r = {'op': 'megaface_scan', 'm': m, 'n': n, 'd': d, 'sizes': sizes, 'genuine_pairs': len(ip),
         'genuine_min': round(float(sg.min()), 3), 'genuine_median': round(float(np.median(sg)), 3), 'rank1_at_max': round(rank1, 4),
         'ms': round(ms, 3), 'tflops': round(fl / ms / 1e9, 2), 'of_peak': round(fl / ms / 1e-3 / PEAK, 3),
         'pair_scores_ms_first_call': round(pair_ms, 3)}
    if not a.no_torch:
        tres = {}
        tms = timed(lambda: tres.__setitem__('r', torch_counts(P, D, sizes, off, thr, nbins, 32768)), a.iters)
        ge, th = tres['r']
        # the baseline's counts in CSR order (its own fp32 products: a few pairs may differ at a tie)
        per = np.diff(off)
        got = ge.cpu().numpy()
        tc = np.concatenate([got[:, p, :per[p]][:, ::-1] for p in range(m)], 1) if len(thr) else np.zeros((len(sizes), 0))
        r.update(torch_ms=round(tms, 3), speedup=round(tms / ms, 2), torch_counts_equal=round(float(np.mean(tc == counts)), 6),
                 torch_hist_total_equal=bool(int(th[-1].sum().item()) == int(hist[-1].sum())))
    print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
