"""Face clustering of extracted embeddings (cluster.py): the stage between extraction and training that groups the
rows of an unlabelled or badly labelled list into identities.

Device side (torch CUDA tensors): the kNN graph is a leave-one-out fte_topk_search of the normalised set against itself, chunked
over probes and gallery; the link rules (cosine threshold on the (mutual) kNN graph, approximate rank-order of Otto, Wang and
Jain, TPAMI 2018) and the connected components are libfte.so calls (include/fte.h, "Clustering").  There is no torch fallback;
torch only allocates.

Host side (numpy, importable without a GPU): dense renumbering with a minimum cluster size, and the clustering scores against
known labels (pairwise and BCubed precision / recall / F, NMI) from the contingency table in integer arithmetic."""
import numpy as np

from . import _lib
from .verification import MAX_K, _TENSOR_LIMIT, _chunks, _default_rows, _stream

METHODS = ('rank_order', 'threshold')


# ------------------------------------------------------------------ device side
def knn_graph(feats, k, chunk_rows=None):
    """(scores [n, k] float32, index [n, k] int32) on the device: for every row of feats [n, d] (a CUDA tensor or a numpy array;
    normalised here, d zero-padded to a multiple of 32) its k best other rows by cosine, sorted by score descending, equal scores
    by the smaller row number (fte_topk_search with exclude_self).  Rows with fewer than k other rows end in (-inf, -1) slots.
    Both the probe side and the gallery side are passed in chunks below 2 GiB (or of about `chunk_rows` rows, at least k), with
    probe_base / gallery_base carrying the global row numbers; gallery chunks are merged by fte_topk_merge."""
    import torch
    if not isinstance(feats, torch.Tensor):
        feats = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).cuda()
    if feats.dim() != 2 or not feats.is_cuda or feats.dtype != torch.float32:
        raise ValueError('knn_graph: expected a 2-D float32 CUDA tensor or numpy array, got %s' % (tuple(feats.shape),))
    n, d = feats.shape
    if n < 1 or d < 1:
        raise ValueError('knn_graph: empty set %s' % (tuple(feats.shape),))
    if not 1 <= k <= MAX_K:
        raise ValueError('knn_graph: k = %d outside 1..%d' % (k, MAX_K))
    if n * k >= 1 << 29:
        raise ValueError('knn_graph: n * k = %d * %d reaches 2^29, the limit of the clustering entry points' % (n, k))
    dev = feats.device
    st = _stream()
    dp = (d + 31) // 32 * 32
    rows = max(chunk_rows or _default_rows(dp), 1)
    if 2 * rows * dp * 4 > _TENSOR_LIMIT:
        rows = _default_rows(dp)
    kk = min(k, n)                                  # the search needs k <= rows of a gallery chunk
    ch = _chunks(n, max(rows, kk))
    x = torch.zeros(n, dp, dtype=torch.float32, device=dev)
    x[:, :d] = feats
    for c0, c1 in ch:
        _lib.call('fte_l2_normalize_rows', x[c0:c1], x[c0:c1], None, c1 - c0, dp, st)
    scores = torch.full((n, k), float('-inf'), dtype=torch.float32, device=dev)
    index = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    for p0, p1 in ch:
        m = p1 - p0
        best_s = best_i = None
        for g0, g1 in ch:
            nc = g1 - g0
            cs = torch.empty(m, kk, dtype=torch.float32, device=dev)
            ci = torch.empty(m, kk, dtype=torch.int32, device=dev)
            wsb = _lib.query('fte_topk_search_ws_bytes', m, nc, dp, kk)
            ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            _lib.call('fte_topk_search', x[p0:p1], x[g0:g1], m, nc, dp, kk, g0, 1, p0, cs, ci, ws, wsb, st)
            if best_s is None:
                best_s, best_i = cs, ci
                continue
            ins, ini = torch.stack((best_s, cs), 1).contiguous(), torch.stack((best_i, ci), 1).contiguous()
            best_s = torch.empty(m, kk, dtype=torch.float32, device=dev)
            best_i = torch.empty(m, kk, dtype=torch.int32, device=dev)
            _lib.call('fte_topk_merge', ins, ini, m, 2, kk, best_s, best_i, st)
        scores[p0:p1, :kk] = best_s
        index[p0:p1, :kk] = best_i
    return scores, index


def _lists(scores, index, what):
    import torch
    if (scores.dim() != 2 or scores.shape != index.shape or not scores.is_cuda or not index.is_cuda or scores.dtype != torch.float32
            or index.dtype != torch.int32):
        raise ValueError('%s: expected scores float32 [n, k] and index int32 [n, k] on the device' % what)
    return scores.contiguous(), index.contiguous()


def knn_links(scores, index, method, theta=None, min_score=None, mutual=False):
    """The keep mask uint8 [n, k] over the slots of the kNN lists (fte.h "Clustering" states both rules).
    method 'rank_order': theta is required, min_score is an optional cosine floor; 'threshold': min_score is required, mutual
    additionally asks that the neighbour lists the row back at or above the floor."""
    import torch
    if method not in METHODS:
        raise ValueError('knn_links: method %r is not one of %s' % (method, METHODS))
    scores, index = _lists(scores, index, 'knn_links')
    n, k = scores.shape
    keep = torch.empty(n, k, dtype=torch.uint8, device=scores.device)
    if method == 'rank_order':
        if theta is None:
            raise ValueError('knn_links: rank_order needs theta')
        floor = float('-inf') if min_score is None else float(min_score)
        _lib.call('fte_knn_links_rank_order', scores, index, n, k, float(theta), floor, keep, _stream())
    else:
        if min_score is None:
            raise ValueError('knn_links: threshold needs min_score')
        if theta is not None:
            raise ValueError('knn_links: theta belongs to rank_order, not to threshold')
        _lib.call('fte_knn_links_threshold', scores, index, n, k, float(min_score), int(bool(mutual)), keep, _stream())
    return keep


def components(index, keep):
    """label int32 [n] on the device: the smallest row number of each row's connected component under the kept slots
    (fte_components)."""
    import torch
    if (index.dim() != 2 or keep.shape != index.shape or not index.is_cuda or not keep.is_cuda or index.dtype != torch.int32
            or keep.dtype != torch.uint8):
        raise ValueError('components: expected index int32 [n, k] and keep uint8 [n, k] on the device')
    index, keep = index.contiguous(), keep.contiguous()
    n, k = index.shape
    parent = torch.empty(n, dtype=torch.int32, device=index.device)
    label = torch.empty(n, dtype=torch.int32, device=index.device)
    _lib.call('fte_components', index, keep, n, k, parent, label, _stream())
    return label


def cluster(feats, k, method, theta=None, min_score=None, mutual=False, min_size=1, chunk_rows=None):
    """feats [n, d] -> cluster ids, an int32 numpy array [n]: dense, numbered by first appearance; the rows of clusters smaller
    than min_size get -1."""
    scores, index = knn_graph(feats, k, chunk_rows)
    keep = knn_links(scores, index, method, theta=theta, min_score=min_score, mutual=mutual)
    return renumber(components(index, keep).cpu().numpy(), min_size)


# ------------------------------------------------------------------ host side
def renumber(label, min_size=1):
    """Component labels (any ints) -> int32 ids 0, 1, ... in order of first appearance; rows of components with fewer than
    min_size rows get -1 and take no id."""
    label = np.asarray(label).reshape(-1)
    if min_size < 1:
        raise ValueError('renumber: min_size = %d < 1' % min_size)
    uniq, first, inv, cnt = np.unique(label, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    kept = cnt >= min_size
    order = np.argsort(first[kept], kind='stable')              # kept components by first appearance
    ids = np.full(len(uniq), -1, np.int64)
    ids[np.nonzero(kept)[0][order]] = np.arange(int(kept.sum()))
    return ids[inv].astype(np.int32)


def _pairs(c):
    c = c.astype(np.int64)
    return int(np.sum(c * (c - 1) // 2))


def _f(p, r):
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def clustering_scores(pred, truth):
    """Scores of predicted cluster ids against known labels, both int arrays [n]; rows with pred == -1 are singletons of their
    own.  From the contingency table n_ij (np.unique on combined keys), a_i its row sums (predicted cluster sizes), b_j its
    column sums (class sizes), all int64:
      pairwise  precision = sum C(n_ij, 2) / sum C(a_i, 2), recall = sum C(n_ij, 2) / sum C(b_j, 2)  (a ratio with no pair in
                its denominator is 1.0), F = their harmonic mean;
      BCubed    precision = (1 / n) sum n_ij^2 / a_i, recall = (1 / n) sum n_ij^2 / b_j, F = their harmonic mean;
      NMI       2 I(pred; truth) / (H(pred) + H(truth)), natural logarithms; 1.0 when both entropies are 0.
    Returns a dict with those seven values plus n, clusters and singletons (predicted clusters of one row)."""
    pred = np.asarray(pred, np.int64).reshape(-1).copy()
    truth = np.asarray(truth, np.int64).reshape(-1)
    n = len(pred)
    if n < 1 or len(truth) != n:
        raise ValueError('clustering_scores: %d predictions for %d labels' % (n, len(truth)))
    lone = pred < 0
    pred[lone] = (pred.max() if n else 0) + 1 + np.arange(int(lone.sum()))
    _, pi = np.unique(pred, return_inverse=True)
    _, ti = np.unique(truth, return_inverse=True)
    pi, ti = pi.reshape(-1).astype(np.int64), ti.reshape(-1).astype(np.int64)
    nt = int(ti.max()) + 1
    key, nij = np.unique(pi * nt + ti, return_counts=True)
    nij = nij.astype(np.int64)
    ci, cj = key // nt, key % nt
    a = np.bincount(pi).astype(np.int64)
    b = np.bincount(ti).astype(np.int64)
    tp, pp, tpairs = _pairs(nij), _pairs(a), _pairs(b)
    pw_p = tp / pp if pp else 1.0
    pw_r = tp / tpairs if tpairs else 1.0
    sq = nij * nij
    b3_p = float(np.sum(sq / a[ci])) / n
    b3_r = float(np.sum(sq / b[cj])) / n
    ha = -float(np.sum(a / n * np.log(a / n)))
    hb = -float(np.sum(b / n * np.log(b / n)))
    mi = float(np.sum(nij / n * (np.log(nij * float(n)) - np.log(a[ci] * b[cj].astype(np.float64)))))
    nmi = 1.0 if ha + hb <= 0 else min(1.0, max(0.0, 2.0 * mi / (ha + hb)))
    return {'n': n, 'clusters': int(len(a)), 'singletons': int(np.sum(a == 1)),
            'pairwise_precision': pw_p, 'pairwise_recall': pw_r, 'pairwise_f': _f(pw_p, pw_r),
            'bcubed_precision': b3_p, 'bcubed_recall': b3_r, 'bcubed_f': _f(b3_p, b3_r), 'nmi': nmi}
