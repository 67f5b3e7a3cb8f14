"""float64 numpy restatement of the evaluation path (include/fte.h "Evaluation: similarity search and score statistics",
tf_face_toolbox_amd/verification.py): normalisation, pair scores, top-k with its tie rule, the histogram bin formula, the
k-fold protocol, TAR@FAR and CMC.  Written from the contracts, independently of the package code."""
import numpy as np


def normalize(x):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(1)), 1e-12)[:, None]


def pair_scores(x, ia, ib):
    x = np.asarray(x, np.float64)
    return (x[np.asarray(ia)] * x[np.asarray(ib)]).sum(1)


def topk(probes, gallery, k, exclude_self=False):
    """(scores, index) [m, k]: score descending, equal scores by the smaller index; (-inf, -1) where fewer than k remain."""
    s = np.asarray(probes, np.float64) @ np.asarray(gallery, np.float64).T
    m, n = s.shape
    if exclude_self:
        s[np.arange(m), np.arange(m)] = -np.inf
    out_s = np.full((m, k), -np.inf)
    out_i = np.full((m, k), -1, np.int64)
    for i in range(m):
        order = np.lexsort((np.arange(n), -s[i]))
        if exclude_self:
            order = order[order != i]
        order = order[:k]
        out_s[i, :len(order)] = s[i, order]
        out_i[i, :len(order)] = order
    return out_s, out_i


def bins(scores32, nbins):
    """the fp32 bin formula of fte.h, evaluated in float32 on float32 scores"""
    s = np.asarray(scores32, np.float32)
    v = (s + np.float32(1.0)) * np.float32(0.5 * nbins)
    return np.clip(np.trunc(v).astype(np.int64), 0, nbins - 1)


def histograms(x, labels, nbins):
    """genuine / impostor counts of all pairs i < j, binned from the float64 score rounded to float32;
    also the float64 scores and bins, for the edge allowance"""
    x = np.asarray(x, np.float64)
    labels = np.asarray(labels)
    n = len(x)
    iu, ju = np.triu_indices(n, 1)
    s = (x @ x.T)[iu, ju]
    b = bins(s.astype(np.float32), nbins)
    g = labels[iu] == labels[ju]
    hg = np.bincount(b[g], minlength=nbins)
    hi = np.bincount(b[~g], minlength=nbins)
    return hg, hi, s, b, g


def edge_distance(s, nbins):
    """distance of each score to its nearest bin edge"""
    e = (np.asarray(s, np.float64) + 1.0) * 0.5 * nbins
    return np.abs(e - np.round(e)) * 2.0 / nbins


def kfold_accuracy(scores, same, folds=10):
    scores = np.asarray(scores, np.float64)
    same = np.asarray(same, bool)
    f = len(scores) // folds
    accs, thrs = [], []
    for i in range(folds):
        te = np.zeros(len(scores), bool)
        te[i * f:(i + 1) * f] = True
        best_t, best_acc = None, -1.0
        for t in sorted(set(scores[~te].tolist()) | {np.inf}):
            acc = np.mean((scores[~te] >= t) == same[~te])
            if acc > best_acc:
                best_t, best_acc = t, acc
        accs.append(np.mean((scores[te] >= best_t) == same[te]))
        thrs.append(best_t)
    return float(np.mean(accs)), float(np.std(accs)), thrs


def tar_at_far_sorted(genuine, impostor, nbins, fars):
    """TAR@FAR from raw scores: the threshold is the smallest bin lower edge t with #(impostor >= t) <= far * #impostor"""
    genuine = np.asarray(genuine, np.float64)
    impostor = np.asarray(impostor, np.float64)
    out = []
    for far in fars:
        if len(impostor) < round(1.0 / far) or len(genuine) == 0:
            out.append(None)
            continue
        res = (0.0, 0.0, 1.0)
        for b in range(nbins):
            t = -1.0 + 2.0 * b / nbins
            fa = np.sum(impostor >= t)
            if fa <= far * len(impostor):
                res = (np.sum(genuine >= t) / len(genuine), fa / len(impostor), t)
                break
        out.append(res)
    return out


def cmc(index, probe_labels, gallery_labels, ranks):
    index = np.asarray(index)
    out = {}
    for r in ranks:
        hits = 0
        for i in range(len(index)):
            row = [j for j in index[i, :r] if j >= 0]
            hits += any(gallery_labels[j] == probe_labels[i] for j in row)
        out[r] = hits / float(len(index))
    return out
