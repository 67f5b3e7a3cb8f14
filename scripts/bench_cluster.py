"""The clustering stage at list scale: n = 1,000,000 rows, d = 512, k = 32, synthetic rows in identity clusters
with per-cluster noise (the generator of bench_megaface.py: same-cluster cosines about 0.4 .. 0.8).  Times, from in-stream events
around each stage on the current stream (one synchronise at the end of a stage's repeats): knn_graph (the leave-one-out fused
similarity + top-k, chunked over probes and gallery), each link kernel (threshold, mutual threshold, rank-order), fte_components.
Baseline of the components on the host: scipy.sparse.csgraph.connected_components over the same kept edges (wall, with the
copy of index / keep to the host reported apart).  theta and min_score here are picked for the generator, they are no
recommendation.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import clustering as C  # noqa: E402


def rows_in_clusters(n, ids, d, g, chunk=1 << 17):
    """unit-ish rows around `ids` unit centres; per cluster a noise level s^2 in [0.3, 1.4] (cosines about 1 / (1 + s^2))"""
    labels = torch.randint(0, ids, (n,), device='cuda', generator=g)
    c = torch.nn.functional.normalize(torch.randn(ids, d, device='cuda', generator=g), dim=1)
    s2 = 0.3 + 1.1 * torch.rand(ids, device='cuda', generator=g)
    x = torch.empty(n, d, dtype=torch.float32, device='cuda')
    for i in range(0, n, chunk):
        lab = labels[i:i + chunk]
        x[i:i + chunk] = c[lab] + torch.sqrt(s2[lab] / d)[:, None] * torch.randn(len(lab), d, device='cuda', generator=g)
    return x, labels.cpu().numpy()


def event_ms(fn, iters):
    """mean ms per call between two events recorded on the stream around `iters` calls, after one warm call"""
    out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=512)
    ap.add_argument('--k', type=int, default=32)
    ap.add_argument('--per', type=int, default=20, help='mean rows per identity')
    ap.add_argument('--theta', type=float, default=1.0)
    ap.add_argument('--min_score', type=float, default=0.45)
    ap.add_argument('--iters', type=int, default=5, help='repeats of the link and component stages (the search runs once)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-host', action='store_true', help='skip the scipy baseline')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device='cuda').manual_seed(a.seed)
    n, d, k = a.n, a.d, a.k
    x, planted = rows_in_clusters(n, max(1, n // a.per), d, g)
    torch.cuda.synchronize()
    knn_ms, (scores, index) = event_ms(lambda: C.knn_graph(x, k), 1)         # one warm call, one timed
    r = {'op': 'cluster', 'n': n, 'd': d, 'k': k, 'identities': max(1, n // a.per), 'theta': a.theta, 'min_score': a.min_score,
         'knn_graph_ms': round(knn_ms, 2), 'knn_tflops': round(2.0 * n * n * d / knn_ms / 1e9, 2)}
    keeps = {}
    for name, fn in (('links_threshold', lambda: C.knn_links(scores, index, 'threshold', min_score=a.min_score)),
                     ('links_mutual', lambda: C.knn_links(scores, index, 'threshold', min_score=a.min_score, mutual=True)),
                     ('links_rank_order', lambda: C.knn_links(scores, index, 'rank_order', theta=a.theta)),
                     ('links_rank_order_floor', lambda: C.knn_links(scores, index, 'rank_order', theta=a.theta, min_score=a.min_score))):
        ms, keeps[name] = event_ms(fn, a.iters)
        r[name + '_ms'] = round(ms, 3)
        r[name + '_kept'] = round(float(keeps[name].float().mean()), 4)
    for name in ('links_mutual', 'links_rank_order'):
        keep = keeps[name]
        ms, label = event_ms(lambda: C.components(index, keep), a.iters)
        tag = name.replace('links_', 'components_')
        r[tag + '_ms'] = round(ms, 3)
        ids = C.renumber(label.cpu().numpy())
        sc = C.clustering_scores(ids, planted)
        r[tag] = {'clusters': sc['clusters'], 'singletons': sc['singletons'], 'pairwise_f': round(sc['pairwise_f'], 4),
                  'bcubed_f': round(sc['bcubed_f'], 4), 'nmi': round(sc['nmi'], 4)}
        if not a.no_host:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
            t0 = time.perf_counter()
            hi, hk = index.cpu().numpy(), keep.cpu().numpy()
            t1 = time.perf_counter()
            ok = (hk != 0) & (hi >= 0) & (hi < n) & (hi != np.arange(n)[:, None])
            rows = np.repeat(np.arange(n), k)[ok.reshape(-1)]
            graph = coo_matrix((np.ones(len(rows), np.int8), (rows, hi[ok])), shape=(n, n)).tocsr()
            ncomp, hl = connected_components(graph, directed=False)
            t2 = time.perf_counter()
            r[tag + '_host_copy_ms'] = round((t1 - t0) * 1e3, 2)
            r[tag + '_host_scipy_ms'] = round((t2 - t1) * 1e3, 2)
            r[tag + '_host_equal'] = bool(ncomp == sc['clusters'] and (C.renumber(hl) == ids).all())
    r['links_plus_components_over_knn'] = round((r['links_rank_order_ms'] + r['components_rank_order_ms']) / knn_ms, 5)
    print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
