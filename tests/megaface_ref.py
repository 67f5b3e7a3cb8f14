"""float64 numpy restatement of the MegaFace protocol (include/fte.h "MegaFace", verification.py megaface_*): genuine pairs,
noise removal, sizes, ranks with ties against the genuine pair, CMC and the impostor histogram.  Written from the contract,
independently of the package code."""
import numpy as np

import verify_ref as vr


def pairs(labels):
    """every ordered (p, g), p != g, same label; probe-major, targets ascending"""
    labels = np.asarray(labels)
    out = [(p, g) for p in range(len(labels)) for g in range(len(labels)) if p != g and labels[p] == labels[g]]
    return np.asarray([a for a, _ in out], np.int64), np.asarray([b for _, b in out], np.int64)


def singletons(labels):
    _, c = np.unique(np.asarray(labels), return_counts=True)
    return int(np.sum(c == 1))


def excluded(paths, exclude):
    """keep mask: a path goes when it equals a listed path or ends with '/' + one"""
    return np.array([not any(p == e or p.endswith('/' + e) for e in exclude) for p in paths], bool)


def sizes(requested, kept):
    out = []
    for v in sorted(set(requested)):
        N = min(v, kept)
        if not out or out[-1][0] != N:
            out.append((N, v > kept))
    return out


def ranks(probes, distractors, ip, ig, Ns, gallery=None, eps=0.0):
    """rank [len(Ns), pairs] = 1 + #{d < N : s(p, d) >= s(p, g) - eps} from float64 scores (eps > 0: the loose count, eps < 0
    the strict one: s(p, d) > s(p, g) + |eps| ... see counts())"""
    gallery = probes if gallery is None else gallery
    P = np.asarray(probes, np.float64)
    D = np.asarray(distractors, np.float64)
    sg = (P[ip] * np.asarray(gallery, np.float64)[ig]).sum(1)
    S = P[ip] @ D.T                                          # [pairs, n]
    out = np.empty((len(Ns), len(ip)), np.int64)
    for b, N in enumerate(Ns):
        out[b] = 1 + np.sum(S[:, :N] >= (sg - eps)[:, None], 1)
    return out


def counts_bounds(probes, distractors, ip, ig, Ns, tol=1e-6):
    """(strict, loose) distractor counts: strict counts s_pd > s_pg + tol, loose s_pd >= s_pg - tol"""
    P = np.asarray(probes, np.float64)
    D = np.asarray(distractors, np.float64)
    sg = (P[ip] * P[ig]).sum(1)
    S = P[ip] @ D.T
    lo = np.empty((len(Ns), len(ip)), np.int64)
    hi = np.empty((len(Ns), len(ip)), np.int64)
    for b, N in enumerate(Ns):
        lo[b] = np.sum(S[:, :N] > (sg + tol)[:, None], 1)
        hi[b] = np.sum(S[:, :N] >= (sg - tol)[:, None], 1)
    return lo, hi


def impostor_hist(probes, distractors, N, nbins):
    """histogram of every (probe, distractor d < N) score, binned with fte.h's fp32 formula on the fp32-rounded score"""
    s = (np.asarray(probes, np.float64) @ np.asarray(distractors, np.float64)[:N].T).astype(np.float32)
    return np.bincount(vr.bins(s.ravel(), nbins), minlength=nbins).astype(np.uint64)


def cmc(rank, ks):
    rank = np.asarray(rank)
    return {k: float(np.mean(rank <= k)) for k in ks}
