"""The fixed case of the sampled-class head's data-parallel tests (tests/test_gpu_partial_fc_dp.py, tests/test_partial_fc_dp_host.py):
parameters, images and labels of a global batch, and how far the ORACLE's target cosines lie from the ArcFace branch threshold."""
import numpy as np

from oracle import spherenet as osn

H, W, CH, NCLS, RATE, SAMPLE_SEED = 32, 32, 3, 1000, 0.1, 6
PRESETS = {'SphereNet-ArcFace': (64.0, 0.5, 0.0), 'SphereNet-CosFace': (64.0, 0.0, 0.35)}
# float32 evaluates a cosine of unit-norm 512-vectors to ~1e-6; a target cosine at least this far from cos(pi - m) takes the same
# branch of the ArcFace target in float32 and in float64
ARC_GAP = 1e-3


def labels_for(world, per_rank):
    """shards with different classes, class 120 in the first two of them, a duplicate inside shard 0 when it has room"""
    pool = [5, 730, 999, 42, 0, 311, 640, 87, 456, 901, 13, 577, 268, 834, 399, 702]
    y = []
    for r in range(world):
        shard = [pool[(r * per_rank + i) % len(pool)] for i in range(per_rank)]
        if r < 2:
            shard[-1] = 120
        if r == 0 and per_rank >= 4:
            shard[2] = shard[0]
        y += shard
    return np.array(y)


def case(world, per_rank, seed=91):
    n = world * per_rank
    p = osn.perturb_params(osn.init_params(seed, CH, NCLS, H, W), seed + 1)
    x = np.random.default_rng(seed + 2).uniform(-1, 1, (n, H, W, CH))
    return p, x, labels_for(world, per_rank)


def arc_gap(p, x, y, m):
    """min over the rows of |cos(theta_y) - cos(pi - m)| with the oracle's own embedding and classifier (m = 0: no threshold, inf)"""
    if m == 0:
        return np.inf
    emb, _ = osn.backbone_fwd(p, x, 'NCHW')
    wc = np.asarray(p['classifier/fc_classifier/weights'], np.float64)[:, y]
    cos = (emb * wc.T).sum(1) / np.sqrt((emb * emb).sum(1)) / np.sqrt((wc * wc).sum(0))
    return float(np.abs(cos - np.cos(np.pi - m)).min())
