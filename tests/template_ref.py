"""float64 numpy restatement of the template path (include/fte.h "Templates", tf_face_toolbox_amd/verification.py): media-aware
pooling, set-to-set softmax score fusion, exact TAR@FAR from listed scores and open-set identification.  Written from the
contracts, independently of the package code."""
import numpy as np


def pool(x, members, media_off, tmpl_off, w=None):
    """[n_templates, d]: per template the sum over media of the weighted member mean, normalised; zero-weight media skipped"""
    x = np.asarray(x, np.float64)
    w = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    out = np.zeros((len(tmpl_off) - 1, x.shape[1]))
    for t in range(len(tmpl_off) - 1):
        v = np.zeros(x.shape[1])
        for m in range(tmpl_off[t], tmpl_off[t + 1]):
            rows = np.asarray(members[media_off[m]:media_off[m + 1]], np.int64)
            ws = w[rows].sum()
            if len(rows) and ws != 0:
                v += (w[rows, None] * x[rows]).sum(0) / ws
        out[t] = v / max(np.sqrt((v * v).sum()), 1e-12)
    return out


def template_rows(members, media_off, tmpl_off, t):
    return np.asarray(members[media_off[tmpl_off[t]]:media_off[tmpl_off[t + 1]]], np.int64)


def softmax_score(x, rows_a, rows_b, betas):
    """mean over beta of sum s exp(beta s) / sum exp(beta s) over all |A| |B| image scores"""
    x = np.asarray(x, np.float64)
    s = (x[rows_a] @ x[rows_b].T).ravel()
    vals = []
    for b in betas:
        e = np.exp(b * (s - s.max()))
        vals.append((s * e).sum() / e.sum())
    return float(np.mean(vals))


def tar_at_far(scores, genuine, fars):
    """None where fewer than round(1 / far) impostors; else (tar, achieved far, threshold), accept s > the k-th largest impostor"""
    scores = np.asarray(scores, np.float64)
    genuine = np.asarray(genuine, bool)
    g, imp = scores[genuine], scores[~genuine]
    out = []
    for far in fars:
        if len(imp) < round(1.0 / far) or not len(g):
            out.append(None)
            continue
        k = int(np.floor(far * len(imp)))
        thr = sorted(imp.tolist(), reverse=True)[min(k, len(imp) - 1)]
        out.append((sum(v > thr for v in g) / len(g), sum(v > thr for v in imp) / len(imp), thr))
    return out


def open_set(scores, probe_subjects, gallery_subjects, ranks, fpirs):
    """from the full probe x gallery score matrix: (cmc {r: rate over mated probes}, [tpir or None per fpir]); ties in the
    ranking go to the smaller gallery index"""
    scores = np.asarray(scores, np.float64)
    gs = np.asarray(gallery_subjects)
    mated = np.array([p in set(gs.tolist()) for p in probe_subjects])
    rank_of_mate, top1, top1_hit = [], [], []
    for i, p in enumerate(probe_subjects):
        order = np.lexsort((np.arange(len(gs)), -scores[i]))
        top1.append(scores[i, order[0]])
        top1_hit.append(gs[order[0]] == p)
        pos = [j for j, g in enumerate(order) if gs[g] == p]
        rank_of_mate.append(pos[0] if pos else len(gs))
    rank_of_mate, top1, top1_hit = np.asarray(rank_of_mate), np.asarray(top1), np.asarray(top1_hit)
    cmc = {r: float(np.mean(rank_of_mate[mated] < r)) for r in ranks}
    tp = []
    for f in fpirs:
        neg = top1[~mated]
        if len(neg) < round(1.0 / f):
            tp.append(None)
            continue
        thr = sorted(neg.tolist(), reverse=True)[min(int(np.floor(f * len(neg))), len(neg) - 1)]
        tp.append(float(np.mean(top1_hit[mated] & (top1[mated] > thr))))
    return cmc, tp
