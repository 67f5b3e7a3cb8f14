"""Float64 numpy restatement of the sharded margin head (include/fte.h fte_margin_shard_stats / fte_margin_shard_fwd_bwd): the
per-shard statistics, their merge in rank order and the per-shard gradient, built on tests/margin_ref.py's target term."""
import numpy as np

import margin_ref as mr

EPS = mr.EPS


def shard_ranges(C, R):
    """[(lo, hi)] of the R shards: Cs = ceil(C / R) classes each, the last one short (may come out empty: the host refuses those)"""
    cs = -(-C // R)
    return [(r * cs, min(C, (r + 1) * cs)) for r in range(R)]


def _logits(s, xn, wn, labels, lo, C, scale, m, m3, c):
    """z [n, c] of this shard with the margin on the target column where the shard owns it, t' [n], the local target column [n]
    (-1: another shard's), den [n, c]; rows with a label outside [0, C) are NaN"""
    s = np.asarray(s, np.float64)[:, :c]
    n = s.shape[0]
    xn, wn = np.asarray(xn, np.float64), np.asarray(wn, np.float64)[:c]
    den = np.maximum(xn, EPS)[:, None] * wn[None, :]
    cos = np.clip(s / den, -1, 1)
    z = scale * cos
    tp, yl = np.ones(n), np.full(n, -1)
    for i in range(n):
        y = int(labels[i])
        if not 0 <= y < C:
            z[i] = np.nan
            continue
        if lo <= y < lo + c:
            t, tpi = mr.target(cos[i, y - lo], m, m3)
            z[i, y - lo], tp[i], yl[i] = scale * t, tpi, y - lo
    return z, tp, yl, den


def stats_ref(s, xn, wn, labels, lo, C, scale, m, m3, c):
    """stats [3, n]: max, sum of exp against it, target logit (0 where another shard owns the label); NaN rows for a bad label"""
    z, _, yl, _ = _logits(s, xn, wn, labels, lo, C, scale, m, m3, c)
    mx = z.max(1)
    se = np.exp(z - mx[:, None]).sum(1)
    t = np.where(yl >= 0, z[np.arange(len(yl)), np.maximum(yl, 0)], 0.0)
    t = np.where(np.isnan(mx), np.nan, t)
    return np.stack([mx, se, t])


def merge_ref(all_stats):
    """(M, Z, T) per row from all_stats [R, 3, n]; a NaN anywhere in a row's statistics makes all three NaN"""
    a = np.asarray(all_stats, np.float64)
    bad = np.isnan(a).any((0, 1))
    a = np.where(bad[None, None, :], 0.0, a)
    M = a[:, 0].max(0)
    Z = (a[:, 1] * np.exp(a[:, 0] - M[None, :])).sum(0)
    T = a[:, 2].sum(0)
    nan = np.where(bad, np.nan, 0.0)
    return M + nan, Z + nan, T + nan


def fwd_bwd_ref(s, xn, wn, labels, lo, C, scale, m, m3, all_stats, grad_scale, c):
    """(f [n, ld], loss_rows [n], G [n, ld], rowcoef_part [n]) of one shard from the stacked statistics of all of them"""
    s = np.asarray(s, np.float64)
    n, ld = s.shape
    z, tp, yl, den = _logits(s, xn, wn, labels, lo, C, scale, m, m3, c)
    M, Z, T = merge_ref(all_stats)
    p = np.exp(z - M[:, None]) / Z[:, None]
    dc = p.copy()
    own = yl >= 0
    rows = np.arange(n)[own]
    dc[rows, yl[own]] = (p[rows, yl[own]] - 1) * tp[own]
    f, G = np.zeros((n, ld)), np.zeros((n, ld))
    G[:, :c] = grad_scale * scale * dc / den
    f[:, :c] = z
    bad = np.isnan(M)
    G[bad, :c] = f[bad, :c] = np.nan
    xn = np.asarray(xn, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        rc = np.where(xn > EPS, -(G[:, :c] * s[:, :c]).sum(1) / xn ** 2, 0.0)
    rc[bad] = np.nan
    return f, np.log(Z) + M - T, G, rc
