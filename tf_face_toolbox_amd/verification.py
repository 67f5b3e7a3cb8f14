"""Face verification and 1:N identification scoring of extracted embeddings (verify.py).

Device side (torch CUDA tensors in): every product and reduction is a libfte.so call (include/fte.h, "Evaluation: similarity
search and score statistics"); there is no torch fallback for the arithmetic.  torch only allocates, pads and stacks.

Host side (numpy, importable without a GPU): the LFW pairs.txt parser and row mapping, the 10-fold accuracy protocol, TAR@FAR
from score histograms, and CMC from top-k indices; for templates (IJB-style sets of images grouped into media): the metadata and
template-pair parsers, the CSR grouping the kernels take, exact TAR@FAR from listed scores and open-set identification; for
MegaFace (FaceScrub probes against up to a million distractors): the genuine-pair CSR, noise removal, distractor sizes, ranks -> CMC
and the per-size TAR table."""
import csv
import ctypes
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


def feature_quality(feats):
    """The norm of every row of the raw features [n, d] (float32, CUDA; a numpy array is moved there) -> [n] on the device: the
    norms normalize(..., return_norms=True) returns.  For a MagFace model this is the quality score of the image."""
    import numpy as np
    import torch
    if not isinstance(feats, torch.Tensor):
        feats = torch.from_numpy(np.ascontiguousarray(np.asarray(feats, np.float32))).cuda()
    return normalize(feats, return_norms=True)[1]


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


def _check_x(x, what):
    import torch
    if x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError('%s: expected a 2-D float32 CUDA tensor, got %s' % (what, tuple(x.shape)))
    if x.numel() * 4 > _TENSOR_LIMIT:
        raise ValueError('%s: x is %d x %d = %.2f GiB; the library takes tensors below 2 GiB (pass fewer rows)'
                         % (what, x.shape[0], x.shape[1], x.numel() * 4 / 2.0 ** 30))


def _i32(a, dev):
    """an int32 device copy of a list / numpy array; a tensor already there is taken as it is"""
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.int32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.int64)).astype(np.int32)).to(dev)


def template_pool(x, members, media_off, tmpl_off, weights=None):
    """Media-aware template pooling (fte_template_pool): out [n_templates, d] float32, row t = normalize(sum over media of t of
    the weighted mean of the media's member rows of x).  members / media_off / tmpl_off: the CSR lists of build_templates();
    weights: optional per-row weights [n] (None: 1).  Lists, numpy arrays or tensors.  A template with no media gives a zero row, a bad member row a NaN row."""
    import torch
    _check_x(x, 'template_pool')
    n, d = x.shape
    dev = x.device
    nt = len(tmpl_off) - 1
    if len(members) < 1 or len(media_off) < 2 or nt < 1:
        raise ValueError('template_pool: empty members / media_off / tmpl_off')
    w = None
    if weights is not None:
        w = (weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights, np.float32)))
        w = w.to(device=dev, dtype=torch.float32).contiguous()
        if w.numel() != n:
            raise ValueError('template_pool: %d weights for %d rows' % (w.numel(), n))
    out = torch.empty(nt, d, dtype=torch.float32, device=dev)
    x = x.contiguous()
    _lib.call('fte_template_pool', x, w, n, d, _i32(members, dev), len(members), _i32(media_off, dev), len(media_off) - 1,
              _i32(tmpl_off, dev), nt, out, _stream())
    return out


def _host(a):
    import torch
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def template_sizes(media_off, tmpl_off):
    """members per template (media ignored), from the CSR lists"""
    media_off = np.asarray(media_off, np.int64)
    tmpl_off = np.asarray(tmpl_off, np.int64)
    return media_off[tmpl_off[1:]] - media_off[tmpl_off[:-1]]


def set_pair_scores(x, members, media_off, tmpl_off, ta, tb, betas=range(0, 21)):
    """Set-to-set softmax score fusion (fte_set_pair_scores) of the listed template pairs (ta[p], tb[p]) over normalised image
    rows x [n, d] (d % 32 == 0): the mean over betas of the exp(beta s)-weighted mean of the |A| |B| image scores.  The pairs are
    handed to the library largest first (by the power of two at or below their 16 x 16 tile count), and within one such class
    grouped by template so that consecutive waves reuse the same rows from cache; a pair's result does not depend on its
    position.  The output is returned in the listed order, float32 [npairs].  Lists, numpy arrays or tensors."""
    import torch
    _check_x(x, 'set_pair_scores')
    n, d = x.shape
    if d % 32:
        raise ValueError('set_pair_scores: d = %d is not a multiple of 32 (use normalize())' % d)
    betas = np.asarray(list(betas), np.float32)
    if not 1 <= len(betas) <= 32 or np.any(~(betas >= 0)) or np.any(betas > 40):
        raise ValueError('set_pair_scores: betas must be 1..32 values in [0, 40], got %s' % (betas.tolist(),))
    dev = x.device
    ta, tb = _i32(ta, dev).reshape(-1), _i32(tb, dev).reshape(-1)
    if ta.shape != tb.shape or ta.numel() < 1:
        raise ValueError('set_pair_scores: ta and tb must be equal, non-empty lists')
    nt = len(tmpl_off) - 1
    # the order handed to the library, computed on the device (a host sort of 15M pairs takes seconds): largest first by the
    # power of two at or below the pair's 16 x 16 tile count, and within one such class by template A, so that consecutive
    # waves reuse its rows from cache; an out-of-range id costs nothing (NaN)
    tiles16 = torch.as_tensor(np.concatenate([(template_sizes(_host(media_off), _host(tmpl_off)) + 15) // 16, [0]]), device=dev)
    ok = lambda t: torch.where((t >= 0) & (t < nt), t.long(), torch.full_like(t, nt, dtype=torch.int64))
    tiles = (tiles16[ok(ta)] * tiles16[ok(tb)]).clamp_min(1).double()
    cls = torch.floor(torch.log2(tiles)).long()                                 # 0 .. 62
    key = (63 - cls) * (nt + 1) + ok(ta)
    order = torch.sort(key, stable=True)[1]
    out = torch.empty(ta.numel(), dtype=torch.float32, device=dev)
    x = x.contiguous()
    _lib.call('fte_set_pair_scores', x, n, d, _i32(members, dev), len(members), _i32(media_off, dev), len(media_off) - 1,
              _i32(tmpl_off, dev), nt, ta[order].contiguous(), tb[order].contiguous(), ta.numel(),
              betas.ctypes.data_as(ctypes.c_void_p), len(betas), out, _stream())
    res = torch.empty_like(out)
    res[order] = out
    return res


def megaface_pair_scores(probes, ip, ig, rows=None):
    """s(probes[ip[j]], rows[ig[j]]) float32 [npairs] (fte_megaface_pair_scores), in fte_megaface_scan's arithmetic; rows=None:
    the probe set itself (the MegaFace genuine pairs).  probes / rows: normalised [*, d], d % 32 == 0."""
    import torch
    rows = probes if rows is None else rows
    _check_x(probes, 'megaface_pair_scores')
    _check_x(rows, 'megaface_pair_scores')
    m, d = probes.shape
    if rows.shape[1] != d or d % 32:
        raise ValueError('megaface_pair_scores: probes %s and rows %s need the same d, a multiple of 32' % (tuple(probes.shape), tuple(rows.shape)))
    dev = probes.device
    ip, ig = _i32(ip, dev).reshape(-1), _i32(ig, dev).reshape(-1)
    if ip.shape != ig.shape or ip.numel() < 1:
        raise ValueError('megaface_pair_scores: ip and ig must be equal, non-empty lists')
    out = torch.empty(ip.numel(), dtype=torch.float32, device=dev)
    probes, rows = probes.contiguous(), rows.contiguous()
    _lib.call('fte_megaface_pair_scores', probes, m, rows, rows.shape[0], d, ip, ig, ip.numel(), out, _stream())
    return out


def megaface_scan(probes, distractors, sizes, thr_off, thr, nbins=8192, chunk_rows=None):
    """Fused rank count + impostor histogram (fte_megaface_scan) of probes [m, d] against the first N rows of distractors for
    every N in `sizes` (ascending, each <= len(distractors)), in one pass: bucket [N_{b-1}, N_b) is scanned as its own range (in
    chunks below 2 GiB, or of about `chunk_rows` rows) and the buckets are summed on the host.  thr_off [m + 1] / thr [T]: each
    probe's genuine scores sorted descending (megaface_thresholds).  Returns (counts uint64 [len(sizes), T]: counts[b, j] =
    #{d < N_b : s(p, d) >= thr[j]}, hist uint64 [len(sizes), nbins]: the impostor histogram of probes x distractors[:N_b])."""
    import torch
    m, d = probes.shape
    n = distractors.shape[0]
    if distractors.shape[1] != d or d % 32:
        raise ValueError('megaface_scan: probes %s and distractors %s need the same d, a multiple of 32'
                         % (tuple(probes.shape), tuple(distractors.shape)))
    if nbins < 256 or nbins > 8192 or nbins & (nbins - 1):
        raise ValueError('megaface_scan: nbins = %d is not a power of two in 256..8192' % nbins)
    sizes = [int(v) for v in sizes]
    if not sizes or sizes[0] < 1 or sizes[-1] > n or any(b <= a for a, b in zip(sizes, sizes[1:])):
        raise ValueError('megaface_scan: sizes %s must ascend strictly within 1..%d' % (sizes, n))
    dev = probes.device
    off = _i32(thr_off, dev).reshape(-1)
    if off.numel() != m + 1:
        raise ValueError('megaface_scan: thr_off has %d entries for %d probes' % (off.numel(), m))
    T = len(thr)
    t = (thr if isinstance(thr, torch.Tensor) else torch.as_tensor(np.asarray(thr, np.float32))).to(device=dev, dtype=torch.float32)
    if T == 0:                                      # no genuine pair: one unused slot that no probe's list reaches
        t = torch.zeros(1, dtype=torch.float32, device=dev)
    t = t.contiguous()
    nt = t.numel()
    rows = chunk_rows or _default_rows(d)
    if 2 * rows * d * 4 > _TENSOR_LIMIT:
        rows = _default_rows(d)
    probes, distractors = probes.contiguous(), distractors.contiguous()
    wsb = _lib.query('fte_megaface_scan_ws_bytes', m, nt)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(len(sizes), nt, dtype=torch.int64, device=dev)
    hist = torch.zeros(len(sizes), nbins, dtype=torch.int64, device=dev)
    st = _stream()
    lo = 0
    for b, hi in enumerate(sizes):
        for g0, g1 in _chunks(hi - lo, rows):
            _lib.call('fte_megaface_scan', probes, m, distractors[lo + g0:lo + g1], g1 - g0, d, off, t, nt, nbins, cnt[b], hist[b],
                      ws, wsb, st)
        lo = hi
    cnt = np.cumsum(cnt.cpu().numpy().astype(np.uint64), 0, dtype=np.uint64)
    hist = np.cumsum(hist.cpu().numpy().astype(np.uint64), 0, dtype=np.uint64)
    return cnt[:, :T], hist


def megaface_evaluate(probes, labels, distractors, sizes, nbins=8192, chunk_rows=None):
    """The MegaFace protocol (fte.h "MegaFace") on normalised device rows: FaceScrub probes [m, d] with int labels against the
    first N kept distractor rows for each N of `sizes` (already capped, ascending: megaface_sizes).  Returns a dict: pairs,
    singletons, scores float32 [pairs] and rank int64 [len(sizes), pairs] in genuine-pair order (megaface_pairs), genuine_hist
    uint64 [nbins] (the unordered same-label pairs of the probe set) and impostor_hist uint64 [len(sizes), nbins]."""
    if len(labels) != probes.shape[0]:
        raise ValueError('megaface: %d labels for %d probe rows' % (len(labels), probes.shape[0]))
    ip, ig, off, singles = megaface_pairs(labels)
    if len(ip):
        scores = megaface_pair_scores(probes, ip, ig).cpu().numpy()
    else:
        scores = np.zeros(0, np.float32)
    thr, perm = megaface_thresholds(scores, off)
    counts, hist = megaface_scan(probes, distractors, sizes, off, thr, nbins, chunk_rows)
    rank = np.empty((len(sizes), len(ip)), np.int64)
    rank[:, perm] = counts.astype(np.int64) + 1
    hg, _ = score_histograms(probes, labels, nbins, chunk_rows)
    return {'pairs': len(ip), 'singletons': singles, 'scores': scores, 'rank': rank, 'genuine_hist': hg, 'impostor_hist': hist}


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


# ------------------------------------------------------------------ host side: templates (IJB-A / -B / -C style)
def read_template_metadata(path, weight_column=None):
    """IJB-A-style metadata CSV with a header row.  Columns are read by name (case and surrounding blanks ignored):
    TEMPLATE_ID, SUBJECT_ID, FILE, MEDIA_ID, and `weight_column` when given; every other column is ignored.  Returns a dict of
    per-row lists: template (int64), subject (int64), file (str), media (str) and weight (float32, or None).  Raises ValueError
    for a missing column or a template whose rows name two subjects."""
    with open(os.path.expanduser(path), newline='') as f:
        rows = [r for r in csv.reader(f) if r and any(c.strip() for c in r)]
    if not rows:
        raise ValueError('%s is empty' % path)
    head = [c.strip().upper() for c in rows[0]]
    want = ['TEMPLATE_ID', 'SUBJECT_ID', 'FILE', 'MEDIA_ID'] + ([weight_column.strip().upper()] if weight_column else [])
    col = {}
    for name in want:
        if name not in head:
            raise ValueError('%s: no column %s in the header %s' % (path, name, rows[0]))
        col[name] = head.index(name)
    tid, sid, files, media, weight = [], [], [], [], []
    for ln, r in enumerate(rows[1:], 2):
        try:
            tid.append(int(float(r[col['TEMPLATE_ID']])))
            sid.append(int(float(r[col['SUBJECT_ID']])))
            files.append(r[col['FILE']].strip())
            media.append(r[col['MEDIA_ID']].strip())
            if weight_column:
                weight.append(float(r[col[want[-1]]]))
        except (IndexError, ValueError):
            raise ValueError('%s:%d: bad metadata row %r' % (path, ln, ','.join(r)))
    tid = np.asarray(tid, np.int64)
    sid = np.asarray(sid, np.int64)
    subj = {}
    for t, s in zip(tid.tolist(), sid.tolist()):
        if subj.setdefault(t, s) != s:
            raise ValueError('%s: template %d names subjects %d and %d' % (path, t, subj[t], s))
    return {'template': tid, 'subject': sid, 'file': files, 'media': media,
            'weight': np.asarray(weight, np.float32) if weight_column else None}


def build_templates(meta):
    """The CSR grouping the template kernels take, from read_template_metadata() output (feature row i = metadata row i).
    Templates in ascending id, media of a template in order of first appearance, members of a media in metadata order.  Returns a
    dict: members int32 [rows], media_off int32 [n_media + 1], tmpl_off int32 [n_templates + 1], template_ids int64
    [n_templates], subjects int64 [n_templates]."""
    tid = np.asarray(meta['template'], np.int64)
    sid = np.asarray(meta['subject'], np.int64)
    media = meta['media']
    ids = np.unique(tid)
    members, media_off, tmpl_off, subjects = [], [0], [0], []
    rows_of = {}
    for i, t in enumerate(tid.tolist()):
        rows_of.setdefault(t, []).append(i)
    for t in ids.tolist():
        groups = {}
        for i in rows_of[t]:
            groups.setdefault(media[i], []).append(i)                  # dicts keep first-appearance order
        for g in groups.values():
            members.extend(g)
            media_off.append(len(members))
        tmpl_off.append(len(media_off) - 1)
        subjects.append(sid[rows_of[t][0]])
    return {'members': np.asarray(members, np.int32), 'media_off': np.asarray(media_off, np.int32),
            'tmpl_off': np.asarray(tmpl_off, np.int32), 'template_ids': ids, 'subjects': np.asarray(subjects, np.int64)}


def read_template_pairs(path, template_subjects=None):
    """Template pairs `t1 t2 [label]`, comma- or blank-separated, one per line (a non-numeric first line is taken as a header).
    Without a label a pair is genuine when both templates have the same subject in `template_subjects` ({template id: subject}).
    Returns (t1 int64, t2 int64, genuine bool)."""
    t1, t2, gen = [], [], []
    for ln, line in enumerate(open(os.path.expanduser(path)), 1):
        tok = line.replace(',', ' ').split()
        if not tok:
            continue
        try:
            a, b = int(float(tok[0])), int(float(tok[1]))
        except (IndexError, ValueError):
            if ln == 1 and not t1:
                continue
            raise ValueError('%s:%d: bad pairs line %r' % (path, ln, line.strip()))
        if len(tok) >= 3:
            g = bool(int(float(tok[2])))
        else:
            if template_subjects is None:
                raise ValueError('%s:%d: no label and no template subjects to derive it from' % (path, ln))
            for t in (a, b):
                if t not in template_subjects:
                    raise ValueError('%s:%d: template %d is not in the metadata' % (path, ln, t))
            g = template_subjects[a] == template_subjects[b]
        t1.append(a)
        t2.append(b)
        gen.append(g)
    if not t1:
        raise ValueError('%s lists no pairs' % path)
    return np.asarray(t1, np.int64), np.asarray(t2, np.int64), np.asarray(gen, bool)


def template_index(template_ids, ids, what='template'):
    """positions of `ids` in the ascending `template_ids` of build_templates(); KeyError naming the first unknown id"""
    template_ids = np.asarray(template_ids, np.int64)
    ids = np.asarray(ids, np.int64)
    pos = np.searchsorted(template_ids, ids)
    bad = (pos >= len(template_ids)) | (template_ids[np.minimum(pos, len(template_ids) - 1)] != ids)
    if bad.any():
        raise KeyError('%s %d is not in the metadata' % (what, ids[np.argmax(bad)]))
    return pos


def check_data_list(image_paths, meta, list_path='the data list'):
    """Row i of the feature file must be metadata row i: the list has the metadata's row count and path i ends with FILE i (at a
    path-component boundary).  Raises ValueError naming the first mismatch."""
    files = meta['file']
    if len(image_paths) != len(files):
        raise ValueError('%s lists %d images, the template metadata has %d rows' % (list_path, len(image_paths), len(files)))
    for i, (p, f) in enumerate(zip(image_paths, files)):
        p, f = p.replace('\\', '/'), f.replace('\\', '/').lstrip('/')
        if not (p == f or p.endswith('/' + f)):
            raise ValueError('%s row %d is %s, but metadata row %d names FILE %s' % (list_path, i, p, i, f))


def write_template_list(meta, image_root, out):
    """The image list evaluate.py reads, one `path subject` line per metadata row in metadata order (feature row i = metadata
    row i), with path = image_root/FILE."""
    with open(os.path.expanduser(out), 'w') as f:
        for name, s in zip(meta['file'], np.asarray(meta['subject']).tolist()):
            f.write('%s %d\n' % (os.path.join(image_root, name.replace('\\', '/').lstrip('/')), s))


def _kth_threshold(neg, rate):
    """the k-th largest (0-based) of the negative scores, k = floor(rate * n): accepting s > it admits at most k negatives"""
    neg = np.sort(np.asarray(neg, np.float64))[::-1]
    return neg[min(int(np.floor(rate * len(neg))), len(neg) - 1)]


def tar_at_far_scores(scores, genuine, fars=(1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)):
    """Exact TAR at each target FAR from listed pair scores: with i_k the k-th largest impostor score (0-based),
    k = floor(FAR * n_imp), the threshold accepts s > i_k.  Returns one dict per target: far, tar, achieved_far, threshold -- or
    'n/a' where fewer than round(1 / FAR) impostor pairs (or no genuine pair) exist, as tar_at_far."""
    scores = np.asarray(scores, np.float64)
    genuine = np.asarray(genuine, bool)
    if scores.shape != genuine.shape:
        raise ValueError('tar_at_far_scores: %d scores for %d labels' % (scores.size, genuine.size))
    if np.isnan(scores).any():
        raise ValueError('tar_at_far_scores: %d NaN scores (a bad or empty template)' % int(np.isnan(scores).sum()))
    g, imp = scores[genuine], scores[~genuine]
    out = []
    for far in fars:
        if len(imp) < round(1.0 / far) or len(g) == 0:
            out.append({'far': far, 'tar': 'n/a', 'achieved_far': 'n/a', 'threshold': 'n/a'})
            continue
        thr = _kth_threshold(imp, far)
        out.append({'far': far, 'tar': float(np.mean(g > thr)), 'achieved_far': float(np.mean(imp > thr)), 'threshold': float(thr)})
    return out


def open_set_identification(top_scores, top_index, probe_subjects, gallery_subjects, ranks=(1, 5, 10), fpirs=(0.01, 0.1)):
    """Open-set 1:N identification of probe templates against gallery templates from the search result (top_scores /
    top_index [m, k], best first; index < 0 an empty slot).  A probe is mated when its subject has a gallery template.
    cmc: over mated probes, the fraction whose mate is among the first r results.  TPIR@FPIR: the threshold is the k-th largest
    (0-based, k = floor(FPIR * n_nonmated)) of the non-mated probes' top-1 scores; TPIR is the fraction of mated probes whose
    rank-1 result is the mate and scores above it ('n/a' where fewer than round(1 / FPIR) non-mated probes exist)."""
    ts = np.asarray(top_scores, np.float64)
    ti = np.asarray(top_index, np.int64)
    ps = np.asarray(probe_subjects, np.int64)
    gs = np.asarray(gallery_subjects, np.int64)
    mated = np.isin(ps, gs)
    hit = np.zeros(ti.shape, bool)
    ok = ti >= 0
    hit[ok] = gs[ti[ok]] == np.broadcast_to(ps[:, None], ti.shape)[ok]
    first = np.where(hit.any(1), hit.argmax(1), ti.shape[1])
    nm = int(mated.sum())
    cmc_ = {r: (float(np.mean(first[mated] < r)) if nm else 'n/a') for r in ranks}
    top1 = ts[:, 0]
    tp = []
    for fpir in fpirs:
        neg = top1[~mated]
        if len(neg) < round(1.0 / fpir) or nm == 0:
            tp.append({'fpir': fpir, 'tpir': 'n/a', 'achieved_fpir': 'n/a', 'threshold': 'n/a'})
            continue
        thr = _kth_threshold(neg, fpir)
        tpir = float(np.mean((first[mated] == 0) & (top1[mated] > thr)))
        tp.append({'fpir': fpir, 'tpir': tpir, 'achieved_fpir': float(np.mean(neg > thr)), 'threshold': float(thr)})
    return {'mated': nm, 'non_mated': int((~mated).sum()), 'cmc': cmc_, 'tpir_at_fpir': tp}


# ------------------------------------------------------------------ host side: MegaFace (challenge 1 style)
MEGAFACE_SIZES = (10, 100, 1000, 10000, 100000, 1000000)
MEGAFACE_RANKS = (1, 5, 10, 100, 1000, 10000, 100000, 1000000)


def megaface_pairs(labels):
    """The genuine pairs: every ordered pair (p, g) of distinct rows with the same label, probe-major, targets ascending.
    Returns (ip int64, ig int64, off int64 [n + 1]: probe p's pairs are off[p] .. off[p + 1] - 1, singletons: the number of
    labels with a single row, which add no pair)."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    n = len(labels)
    _, inv, cnt = np.unique(labels, return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind='stable')                  # rows grouped by label, ascending within a label
    start = np.concatenate([[0], np.cumsum(cnt)])
    per = cnt[inv] - 1                                      # pairs of each probe
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    ip = np.repeat(np.arange(n, dtype=np.int64), per)
    ig = np.empty(off[-1], np.int64)
    for p in range(n):
        grp = order[start[inv[p]]:start[inv[p] + 1]]
        ig[off[p]:off[p + 1]] = grp[grp != p]
    return ip, ig, off, int(np.sum(cnt == 1))


def megaface_thresholds(scores, off):
    """The scan's CSR thresholds: each probe's genuine scores (pair order of megaface_pairs) sorted descending, ties in pair
    order.  Returns (thr float32 [T], perm int64 [T]): thr[j] = scores[perm[j]]; thr_off is `off`."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    off = np.asarray(off, np.int64)
    probe = np.repeat(np.arange(len(off) - 1), np.diff(off))
    perm = np.lexsort((np.arange(len(scores)), -scores.astype(np.float64), probe)).astype(np.int64)
    return scores[perm], perm


def _path_key(p):
    return p.replace('\\', '/').strip()


def megaface_exclude(paths, exclude):
    """Noise removal: a keep mask over the distractor list.  Row i goes when paths[i] equals a listed path or ends with '/' +
    a listed path."""
    ex = set(_path_key(e) for e in exclude if _path_key(e))
    keep = np.ones(len(paths), bool)
    for i, p in enumerate(paths):
        p = _path_key(p)
        if p in ex:
            keep[i] = False
            continue
        j = p.find('/')
        while j >= 0:
            if p[j + 1:] in ex:
                keep[i] = False
                break
            j = p.find('/', j + 1)
    return keep


def megaface_sizes(sizes, kept):
    """The distractor sizes to report: each requested size capped to the kept count, ascending, each once.  Returns
    [(N, capped)]; capped is True when N stands for a larger request."""
    req = sorted(set(int(v) for v in sizes))
    if not req or req[0] < 1:
        raise ValueError('megaface: distractor sizes must be positive, got %s' % (list(sizes),))
    if kept < 1:
        raise ValueError('megaface: no distractor row is left')
    out = []
    for v in req:
        N, capped = min(v, kept), v > kept
        if out and out[-1][0] == N:
            continue
        out.append((N, capped))
    return out


def megaface_cmc(rank, ranks):
    """CMC(k) = the fraction of genuine pairs with rank <= k, for each k of ranks: {k: fraction} ('n/a' with no pair)"""
    rank = np.asarray(rank, np.int64)
    return {int(k): (float(np.mean(rank <= k)) if rank.size else 'n/a') for k in ranks}


def megaface_report_ranks(N, extra=()):
    """The ranks reported at size N: MEGAFACE_RANKS (and `extra`) up to N + 1, the largest rank a pair can have"""
    return tuple(sorted(set(k for k in tuple(MEGAFACE_RANKS) + tuple(extra) if k <= N + 1)))


def megaface_tar_table(hist_genuine, impostor_hists, sizes, fars=(1e-6, 1e-5, 1e-4, 1e-3)):
    """Per size N: tar_at_far of the genuine histogram against that size's impostor histogram.  Returns [{'size': N, 'impostor':
    n_imp, 'tar_at_far': [...]}]."""
    out = []
    for N, hi in zip(sizes, impostor_hists):
        out.append({'size': int(N), 'impostor': int(np.asarray(hi, np.uint64).sum()), 'tar_at_far': tar_at_far(hist_genuine, hi, fars)})
    return out
