"""Template kernels at IJB-C scale: media-aware pooling (fte_template_pool, via verification.template_pool) and
set-to-set softmax score fusion (fte_set_pair_scores, via verification.set_pair_scores) on a synthetic case of 469,375 images,
23,124 templates of skewed size (media of 1..30 frames) and 15.7M template pairs, d = 512, 21 betas.  Inputs come from a seed.
Compared with torch baselines of the same arithmetic (outside the product path, for comparison only): index_add pooling, and
gather + padded bmm + per-beta weights in size-bucketed batches (on --torch_pairs pairs, against the kernel on the same pairs).
Prints one JSON line per measurement: pooling GB/s against a device copy of x; fusion TFLOP/s on useful (sum 2 d |A| |B|) and
executed (16 x 16 tiles) FLOPs against the 157.3 TF fp32 MFMA peak.  Run it under `rocprofv3 --kernel-trace --stats` for the
kernel times."""
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


def synth(rng, n_images, n_templates, max_frames=30):
    """template sizes from a lognormal, scaled to n_images in all; each template's members split into media of 1..max_frames"""
    s = rng.lognormal(2.0, 1.1, n_templates)
    sizes = np.maximum(1, np.floor(s * n_images / s.sum())).astype(np.int64)
    extra = n_images - sizes.sum()
    idx = rng.choice(n_templates, abs(int(extra)), replace=True)
    np.add.at(sizes, idx, 1 if extra > 0 else 0)
    sizes[-1] += n_images - sizes.sum()
    members = rng.permutation(n_images).astype(np.int32)
    media_off, tmpl_off = [0], [0]
    pos = 0
    for sz in sizes.tolist():
        left = sz
        while left:
            f = min(left, int(rng.integers(1, max_frames + 1)) if rng.random() < 0.3 else 1)
            pos += f
            media_off.append(pos)
            left -= f
        tmpl_off.append(len(media_off) - 1)
    return members, np.asarray(media_off, np.int32), np.asarray(tmpl_off, np.int32), sizes


def torch_pool(X, members, media_off, tmpl_off, w):
    dev = X.device
    nm = len(media_off) - 1
    seg = torch.repeat_interleave(torch.arange(nm, device=dev), torch.diff(media_off.long()))
    tseg = torch.repeat_interleave(torch.arange(len(tmpl_off) - 1, device=dev), torch.diff(tmpl_off.long()))
    wm = w[members.long()]
    M = torch.zeros(nm, X.shape[1], device=dev).index_add_(0, seg, X[members.long()] * wm[:, None])
    ws = torch.zeros(nm, device=dev).index_add_(0, seg, wm)
    M = torch.where(ws[:, None] != 0, M / ws[:, None], torch.zeros_like(M))
    T = torch.zeros(len(tmpl_off) - 1, X.shape[1], device=dev).index_add_(0, tseg, M)
    return T / T.norm(dim=1, keepdim=True).clamp_min(1e-12)


def torch_set_scores(X, members, starts, sizes, ta, tb, betas, budget=1 << 28):
    """gather + padded bmm + per-beta weights, pairs bucketed by the powers of two above |A| and |B|"""
    dev = X.device
    out = torch.empty(len(ta), device=dev)
    pa = 1 << np.ceil(np.log2(sizes[ta])).astype(np.int64)
    pb = 1 << np.ceil(np.log2(sizes[tb])).astype(np.int64)
    mem = members.long()
    for key in sorted(set(zip(pa.tolist(), pb.tolist()))):
        sel = np.nonzero((pa == key[0]) & (pb == key[1]))[0]
        per = max(1, budget // (key[0] * key[1]))
        for c0 in range(0, len(sel), per):
            s = sel[c0:c0 + per]

            def gather(t, P):
                j = np.arange(P)[None, :]
                ok = j < sizes[t][:, None]
                idx = np.where(ok, starts[t][:, None] + np.minimum(j, sizes[t][:, None] - 1), 0)
                return X[mem[torch.as_tensor(idx, device=dev)]], torch.as_tensor(ok, device=dev)
            A, ma = gather(ta[s], key[0])
            B, mb = gather(tb[s], key[1])
            S = torch.bmm(A, B.transpose(1, 2))
            m = (ma[:, :, None] & mb[:, None, :]).float()
            acc = torch.zeros(len(s), device=dev)
            for b in betas:
                e = torch.exp(b * (S - 1.0)) * m
                acc += (S * e).sum((1, 2)) / e.sum((1, 2))
            out[torch.as_tensor(s, device=dev)] = acc / len(betas)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--images', type=int, default=469375)
    ap.add_argument('--templates', type=int, default=23124)
    ap.add_argument('--pairs', type=int, default=15658489)
    ap.add_argument('--torch_pairs', type=int, default=200000, help='pairs of the torch fusion comparison (0: skip)')
    ap.add_argument('--no-torch', action='store_true', help='skip the torch comparisons')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(a.seed)
    d = 512
    members, media_off, tmpl_off, sizes = synth(rng, a.images, a.templates)
    g = torch.Generator(device='cuda').manual_seed(a.seed)
    X = V.normalize(torch.randn(a.images, d, device='cuda', generator=g))
    w = torch.rand(a.images, device='cuda', generator=g) + 0.5
    nt = len(tmpl_off) - 1
    # ---- pooling
    bytes_ = (len(members) * d + nt * d) * 4.0
    dm, dmo, dto = (torch.as_tensor(v, device='cuda') for v in (members, media_off, tmpl_off))
    ms = timed(lambda: V.template_pool(X, dm, dmo, dto, w), a.iters)
    cms = timed(lambda: X.clone(), a.iters)
    copy_gbs = 2.0 * X.numel() * 4 / cms / 1e6
    r = {'op': 'template_pool', 'images': a.images, 'templates': nt, 'media': len(media_off) - 1, 'max_size': int(sizes.max()),
         'd': d, 'ms': round(ms, 3), 'gbs': round(bytes_ / ms / 1e6, 1), 'copy_gbs': round(copy_gbs, 1),
         'of_copy': round(bytes_ / ms / 1e6 / copy_gbs, 3)}
    if not a.no_torch:
        tms = timed(lambda: torch_pool(X, dm, dmo, dto, w), a.iters)
        r.update(torch_ms=round(tms, 3), speedup=round(tms / ms, 2))
        ref = torch_pool(X, dm, dmo, dto, w)
        r.update(max_abs_diff_vs_torch=float((ref - V.template_pool(X, dm, dmo, dto, w)).abs().max()))
    print(json.dumps(r), flush=True)
    # ---- set-to-set fusion
    betas = list(range(0, 21))
    ta = rng.integers(0, nt, a.pairs)
    tb = rng.integers(0, nt, a.pairs)
    starts = media_off[tmpl_off[:-1]].astype(np.int64)

    def flops(sel):
        A, B = sizes[ta[sel]].astype(np.float64), sizes[tb[sel]].astype(np.float64)
        ex = 16 * np.ceil(A / 16) * 16 * np.ceil(B / 16)
        return 2.0 * d * (A * B).sum(), 2.0 * d * ex.sum()
    useful, executed = flops(slice(None))
    dta, dtb = torch.as_tensor(ta, device='cuda'), torch.as_tensor(tb, device='cuda')
    ms = timed(lambda: V.set_pair_scores(X, dm, dmo, dto, dta, dtb, betas), max(1, a.iters - 2))
    r = {'op': 'set_pair_scores', 'pairs': a.pairs, 'betas': len(betas), 'd': d, 'ms': round(ms, 3),
         'useful_tflops': round(useful / ms / 1e9, 2), 'executed_tflops': round(executed / ms / 1e9, 2),
         'useful_of_peak': round(useful / ms / 1e-3 / PEAK, 3), 'executed_of_peak': round(executed / ms / 1e-3 / PEAK, 3)}
    print(json.dumps(r), flush=True)
    if not a.no_torch and a.torch_pairs:
        sel = np.arange(min(a.torch_pairs, a.pairs))
        u, e = flops(sel)
        sa, sb = dta[:len(sel)], dtb[:len(sel)]
        kms = timed(lambda: V.set_pair_scores(X, dm, dmo, dto, sa, sb, betas), a.iters)
        tms = timed(lambda: torch_set_scores(X, torch.as_tensor(members, device='cuda'), starts, sizes, ta[sel], tb[sel], betas), 1)
        ref = torch_set_scores(X, torch.as_tensor(members, device='cuda'), starts, sizes, ta[sel], tb[sel], betas)
        got = V.set_pair_scores(X, dm, dmo, dto, sa, sb, betas)
        r = {'op': 'set_pair_scores_vs_torch', 'pairs': len(sel), 'ms': round(kms, 3), 'useful_tflops': round(u / kms / 1e9, 2),
             'executed_tflops': round(e / kms / 1e9, 2), 'torch_ms': round(tms, 3), 'speedup': round(tms / kms, 2),
             'max_abs_diff_vs_torch': float((ref - got).abs().max())}
        print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
