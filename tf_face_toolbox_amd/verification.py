"""Face verification and 1:N identification scoring of extracted embeddings (verify.py).

Device side (torch CUDA tensors in): every product and reduction is a libfte.so call (include/fte.h, "Evaluation: similarity
search and score statistics"); there is no torch fallback for the arithmetic.  torch only allocates, pads and stacks.

Host side (numpy, importable without a GPU): the LFW pairs.txt parser and row mapping, the 10-fold accuracy protocol, TAR@FAR
from score histograms, and CMC from top-k indices."""
import os

import numpy as np

from . import _lib

MAX_K = 64
_TENSOR_LIMIT = (1 << 31) - 1          # every tensor handed to the library stays below 2 GiB (fte.h conventions)


# ------------------------------------------------------------------ device side
def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def normalize(x, return_norms=False):
    """Rows of x [n, d] (float32, CUDA) scaled to unit length: y = x / max(|x|, 1e-12).  d is zero-padded up to a multiple of 32
    (zero columns change no dot product), so the result feeds topk_search / score_histograms directly."""
    import torch
    if x.dim() != 2 or not x.is_cuda:
        raise ValueError('normalize: expected a 2-D CUDA tensor, got %s' % (tuple(x.shape),))
    n, d = x.shape
    dp = (d + 31) // 32 * 32
    y = torch.zeros(n, dp, dtype=torch.float32, device=x.device)
    y[:, :d] = x
    norms = torch.empty(n, dtype=torch.float32, device=x.device)
    _lib.call('fte_l2_normalize_rows', y, y, norms, n, dp, _stream())
    return (y, norms) if return_norms else y


def pair_scores(feats, ia, ib):
    """out[p] = dot(feats[ia[p]], feats[ib[p]]) for normalised rows (the LFW protocol's listed pairs)."""
    import torch
    dev = feats.device
    ia = torch.as_tensor(np.asarray(ia), dtype=torch.int32).to(dev).contiguous()
    ib = torch.as_tensor(np.asarray(ib), dtype=torch.int32).to(dev).contiguous()
    if ia.numel() != ib.numel() or ia.numel() < 1:
        raise ValueError('pair_scores: ia and ib must be equal, non-empty lists')
    out = torch.empty(ia.numel(), dtype=torch.float32, device=dev)
    feats = feats.contiguous()
    _lib.call('fte_pair_scores', feats, ia, ib, out, feats.shape[0], feats.shape[1], ia.numel(), _stream())
    return out


def _chunks(n, rows):
    """[start, stop) ranges of n rows, each of at least `rows` rows (the last one takes the remainder)"""
    c = max(1, n // rows)
    edges = [n * i // c for i in range(c + 1)]
    return list(zip(edges[:-1], edges[1:]))


def _default_rows(d, elem=4):
    return max(1, (_TENSOR_LIMIT // (d * elem)) // 2)      # a chunk may take up to twice this (see _chunks)


def topk_search(probes, gallery, k, exclude_self=False, chunk_rows=None):
    """The k best gallery rows of every probe row: (scores [m, k] float32, index [m, k] int32), sorted by score descending,
    equal scores by the smaller gallery index.  probes / gallery are normalised [*, d] with d % 32 == 0 (normalize() output).
    exclude_self drops (i, i) pairs: leave-one-out search when probes and gallery are the same set.  The gallery is passed to the
    library in chunks below 2 GiB (or of about `chunk_rows` rows) whose top-k lists are merged by fte_topk_merge."""
    import torch
    m, d = probes.shape
    n = gallery.shape[0]
    if gallery.shape[1] != d or d % 32:
        raise ValueError('topk_search: probes %s and gallery %s need the same d, a multiple of 32' % (tuple(probes.shape), tuple(gallery.shape)))
    if not 1 <= k <= min(MAX_K, n):
        raise ValueError('topk_search: k = %d outside 1..min(%d, n = %d)' % (k, MAX_K, n))
    rows = chunk_rows or _default_rows(d)
    rows = max(rows, k)
    if 2 * rows * d * 4 > _TENSOR_LIMIT:
        rows = _default_rows(d)
    dev = probes.device
    probes, gallery = probes.contiguous(), gallery.contiguous()
    st = _stream()
    best_s = best_i = None
    for g0, g1 in _chunks(n, rows):
        nc = g1 - g0
        cs = torch.empty(m, k, dtype=torch.float32, device=dev)
        ci = torch.empty(m, k, dtype=torch.int32, device=dev)
        wsb = _lib.query('fte_topk_search_ws_bytes', m, nc, d, k)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        _lib.call('fte_topk_search', probes, gallery[g0:g1], m, nc, d, k, g0, int(bool(exclude_self)), 0, cs, ci, ws, wsb, st)
        if best_s is None:
            best_s, best_i = cs, ci
            continue
        ins, ini = torch.stack((best_s, cs), 1).contiguous(), torch.stack((best_i, ci), 1).contiguous()
        best_s = torch.empty(m, k, dtype=torch.float32, device=dev)
        best_i = torch.empty(m, k, dtype=torch.int32, device=dev)
        _lib.call('fte_topk_merge', ins, ini, m, 2, k, best_s, best_i, st)
    return best_s, best_i


def score_histograms(feats, labels, nbins=8192, chunk_rows=None):
    """Genuine / impostor histograms (uint64 numpy [nbins] each) of the scores of all pairs i < j of normalised rows feats [n, d]
    (d % 32 == 0) with int labels.  Bin of a score s: clamp(int((s + 1) * nbins / 2), 0, nbins - 1) (fte.h states the exact fp32
    expression).  The set is walked in chunk pairs (I <= J) below 2 GiB each (or of about `chunk_rows` rows)."""
    import torch
    n, d = feats.shape
    if d % 32:
        raise ValueError('score_histograms: d = %d is not a multiple of 32 (use normalize())' % d)
    if nbins < 256 or nbins > 8192 or nbins & (nbins - 1):
        raise ValueError('score_histograms: nbins = %d is not a power of two in 256..8192' % nbins)
    dev = feats.device
    feats = feats.contiguous()
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.int32).to(dev).contiguous()
    if lab.numel() != n:
        raise ValueError('score_histograms: %d labels for %d rows' % (lab.numel(), n))
    hg = torch.zeros(nbins, dtype=torch.int64, device=dev)
    hi = torch.zeros(nbins, dtype=torch.int64, device=dev)
    st = _stream()
    ch = _chunks(n, chunk_rows or _default_rows(d))
    for I, (a0, a1) in enumerate(ch):
        for b0, b1 in ch[I:]:
            same = int(a0 == b0)
            _lib.call('fte_score_histograms', feats[a0:a1], lab[a0:a1], a1 - a0, feats[b0:b1], lab[b0:b1], b1 - b0, d, same, nbins,
                      hg, hi, st)
    return hg.cpu().numpy().astype(np.uint64), hi.cpu().numpy().astype(np.uint64)


# ------------------------------------------------------------------ host side: protocols
def read_lfw_pairs(path):
    """LFW pairs.txt: a header `folds pairs_per_class` (10 300), then per line `name i j` (same person) or `name1 i name2 j`
    (different people).  Returns (pairs [(name1, i1, name2, i2)], same [bool], folds)."""
    lines = [ln.split() for ln in open(os.path.expanduser(path)) if ln.strip()]
    if not lines:
        raise ValueError('%s is empty' % path)
    head = lines[0]
    folds = int(head[0]) if len(head) in (1, 2) else 10
    body = lines[1:] if len(head) in (1, 2) else lines
    pairs, same = [], []
    for t in body:
        if len(t) == 3:
            pairs.append((t[0], int(t[1]), t[0], int(t[2])))
            same.append(True)
        elif len(t) == 4:
            pairs.append((t[0], int(t[1]), t[2], int(t[3])))
            same.append(False)
        else:
            raise ValueError('%s: bad pairs line %r' % (path, ' '.join(t)))
    return pairs, np.asarray(same, bool), folds


def lfw_image_key(name, i):
    return '%s/%s_%04d' % (name, name, i)


def map_pairs_to_rows(pairs, image_paths):
    """Rows of the image list (the one evaluate.py was given) for each pair: `name/name_%04d` is matched against the path with
    its extension dropped, as a suffix at a path-component boundary.  Raises KeyError naming the first image not in the list."""
    index = {}
    for row, p in enumerate(image_paths):
        stem = os.path.splitext(p.replace('\\', '/'))[0]
        parts = stem.split('/')
        if len(parts) >= 2:
            index.setdefault('/'.join(parts[-2:]), row)
    ia, ib = [], []
    for n1, i1, n2, i2 in pairs:
        k1, k2 = lfw_image_key(n1, i1), lfw_image_key(n2, i2)
        for k in (k1, k2):
            if k not in index:
                raise KeyError('%s is not in the image list' % k)
        ia.append(index[k1])
        ib.append(index[k2])
    return np.asarray(ia, np.int64), np.asarray(ib, np.int64)


def _best_threshold(scores, same):
    """The candidate (training scores and +inf) with the best accuracy of `same <=> score >= t`; ties: the smallest threshold"""
    cand = np.unique(np.concatenate([scores, [np.inf]]))
    order = np.argsort(scores, kind='stable')
    s_sorted = scores[order]
    pos_sorted = same[order].astype(np.int64)
    # for threshold t: correct = #(same and s >= t) + #(not same and s < t)
    below = np.searchsorted(s_sorted, cand, side='left')          # rows with s < t
    cum_pos = np.concatenate([[0], np.cumsum(pos_sorted)])
    npos = cum_pos[-1]
    pos_below = cum_pos[below]
    neg_below = below - pos_below
    correct = (npos - pos_below) + neg_below
    best = np.argmax(correct)                                     # first maximum = smallest threshold (cand is ascending)
    return float(cand[best]), correct[best] / float(len(scores))


def kfold_accuracy(scores, same, folds=10):
    """The LFW protocol: `folds` consecutive equal blocks; for each test fold the threshold is chosen on the other folds.
    Returns (mean accuracy, std (ddof = 0), per-fold thresholds)."""
    scores = np.asarray(scores, np.float64)
    same = np.asarray(same, bool)
    n = len(scores)
    if n % folds or n == 0:
        raise ValueError('kfold_accuracy: %d pairs do not split into %d equal folds' % (n, folds))
    f = n // folds
    accs, thrs = [], []
    for i in range(folds):
        test = np.zeros(n, bool)
        test[i * f:(i + 1) * f] = True
        t, _ = _best_threshold(scores[~test], same[~test])
        accs.append(np.mean((scores[test] >= t) == same[test]))
        thrs.append(t)
    return float(np.mean(accs)), float(np.std(accs)), thrs


def tar_at_far(hist_genuine, hist_impostor, fars=(1e-6, 1e-5, 1e-4, 1e-3)):
    """TAR at each target FAR from score histograms over [-1, 1].  The threshold is the lower edge of the lowest bin whose tail
    (that bin and above) holds impostor fraction <= FAR; TAR is the genuine fraction in the same tail.  Returns one dict per
    target: far, tar, achieved_far, threshold -- or tar 'n/a' where fewer than 1 / FAR impostor pairs exist."""
    hg = np.asarray(hist_genuine, np.float64)
    hi = np.asarray(hist_impostor, np.float64)
    nb = len(hg)
    ng, ni = hg.sum(), hi.sum()
    tail_g = np.cumsum(hg[::-1])[::-1]
    tail_i = np.cumsum(hi[::-1])[::-1]
    out = []
    for far in fars:
        if ni < round(1.0 / far) or ng == 0:
            out.append({'far': far, 'tar': 'n/a', 'achieved_far': 'n/a', 'threshold': 'n/a'})
            continue
        ok = np.nonzero(tail_i <= far * ni)[0]
        if len(ok):
            b = int(ok[0])
            tar, afar, thr = tail_g[b] / ng, tail_i[b] / ni, -1.0 + 2.0 * b / nb
        else:                                       # even the top bin holds too many impostors: accept nothing
            tar, afar, thr = 0.0, 0.0, 1.0
        out.append({'far': far, 'tar': float(tar), 'achieved_far': float(afar), 'threshold': float(thr)})
    return out


def cmc(index, probe_labels, gallery_labels, ranks=(1, 5, 10)):
    """Closed-set identification: the fraction of probes whose label appears among their first r retrieved gallery rows, for
    each r in ranks (r beyond the list length counts the whole list).  index [m, k] (index < 0: an empty slot)."""
    index = np.asarray(index)
    pl = np.asarray(probe_labels)
    gl = np.asarray(gallery_labels)
    ok = index >= 0
    hit = np.zeros(index.shape, bool)
    hit[ok] = gl[index[ok]] == np.broadcast_to(pl[:, None], index.shape)[ok]
    first = np.where(hit.any(1), hit.argmax(1), index.shape[1])
    return {r: float(np.mean(first < r)) for r in ranks}
