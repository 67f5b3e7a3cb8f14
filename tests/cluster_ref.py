"""numpy restatement of the clustering stage (include/fte.h "Clustering", tf_face_toolbox_amd/clustering.py): test infrastructure
only.  Brute-force float64 top-k in the library's tie order, the two link rules as the header states them (loops over slots, sets
for the membership questions, the one fp32 product in np.float32), a union-find with min-index labels, a brute-force transitive
closure, and pair counting for the metrics."""
import numpy as np


def topk(x, k):
    """leave-one-out top-k of the rows of x (float64 products): scores float32 [n, k], index int32 [n, k]; score descending, then
    the smaller index; rows with fewer than k other rows end in (-inf, -1)"""
    x = np.asarray(x, np.float64)
    n = len(x)
    s = x @ x.T
    scores = np.full((n, k), -np.inf, np.float32)
    index = np.full((n, k), -1, np.int32)
    for a in range(n):
        cand = [j for j in range(n) if j != a]
        cand.sort(key=lambda j: (-s[a, j], j))
        cand = cand[:k]
        scores[a, :len(cand)] = s[a, cand]
        index[a, :len(cand)] = cand
    return scores, index


def valid(index, a, t):
    n = index.shape[0]
    b = int(index[a, t])
    return 0 <= b < n and b != a


def links_threshold(scores, index, min_score, mutual):
    n, k = index.shape
    keep = np.zeros((n, k), np.uint8)
    ms = np.float32(min_score)
    for a in range(n):
        for t in range(k):
            if not valid(index, a, t) or not scores[a, t] >= ms:
                continue
            b = int(index[a, t])
            if mutual and not any(int(index[b, u]) == a and scores[b, u] >= ms for u in range(k)):
                continue
            keep[a, t] = 1
    return keep


def _list(index, a):
    """L_a as (entries at positions 0..k, live flags, member set, first position of each member): a hole or a repeated entry is
    not live"""
    k = index.shape[1]
    entries, live, seen, pos = [a], [True], {a}, {a: 0}
    for t in range(k):
        e = int(index[a, t])
        ok = valid(index, a, t) and e not in seen
        entries.append(e)
        live.append(ok)
        if ok:
            seen.add(e)
            pos[e] = t + 1
    return entries, live, seen, pos


def _rank(index, a, b, lists):
    """r(a,b) for a valid b != a: 1 + the first slot of row a that holds b, k + 1 if none"""
    return lists[a][3].get(b, index.shape[1] + 1)


def _missing(index, a, b, lists):
    k = index.shape[1]
    ea, la = lists[a][0], lists[a][1]
    mb = lists[b][2]
    top = min(_rank(index, a, b, lists), k)
    return sum(1 for p in range(top + 1) if la[p] and ea[p] not in mb)


def rank_order_parts(index, a, b, lists=None):
    """(m(a,b) + m(b,a), min(r(a,b), r(b,a))) for rows a != b"""
    lists = lists or {a: _list(index, a), b: _list(index, b)}
    return _missing(index, a, b, lists) + _missing(index, b, a, lists), min(_rank(index, a, b, lists), _rank(index, b, a, lists))


def rank_order_table(index):
    """(valid [n, k] bool, num [n, k], den [n, k] int64): the two sides of the rank-order test for every valid slot; it does not
    depend on theta or the floor, so one table serves every case on the same lists"""
    n, k = index.shape
    ok = np.zeros((n, k), bool)
    num = np.zeros((n, k), np.int64)
    den = np.ones((n, k), np.int64)
    lists = [_list(index, a) for a in range(n)]
    for a in range(n):
        for t in range(k):
            if valid(index, a, t):
                ok[a, t] = True
                num[a, t], den[a, t] = rank_order_parts(index, a, int(index[a, t]), lists)
    return ok, num, den


def links_rank_order(scores, index, theta, min_score=-np.inf, table=None):
    ok, num, den = table or rank_order_table(index)
    with np.errstate(invalid='ignore'):
        floor = np.asarray(scores, np.float32) >= np.float32(min_score)
    near = num.astype(np.float32) < np.float32(theta) * den.astype(np.float32)        # one fp32 product, one compare
    return (ok & floor & near).astype(np.uint8)


def edges(index, keep):
    n, k = index.shape
    return [(a, int(index[a, t])) for a in range(n) for t in range(k) if keep[a, t] and valid(index, a, t)]


def components(index, keep):
    """label[i] = the smallest row of i's component (union-find, smaller root wins)"""
    n = index.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges(index, keep):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.asarray([find(i) for i in range(n)], np.int32)


def closure_labels(index, keep):
    """the same labels from a boolean transitive closure (n <= a few hundred)"""
    n = index.shape[0]
    reach = np.eye(n, dtype=bool)
    for a, b in edges(index, keep):
        reach[a, b] = reach[b, a] = True
    for m in range(n):                                    # Warshall
        reach |= np.outer(reach[:, m], reach[m, :])
    return np.asarray([int(np.nonzero(reach[i])[0][0]) for i in range(n)], np.int32)


def renumber(label, min_size=1):
    label = [int(v) for v in label]
    size = {}
    for v in label:
        size[v] = size.get(v, 0) + 1
    ids, out = {}, []
    for v in label:
        if size[v] < min_size:
            out.append(-1)
            continue
        if v not in ids:
            ids[v] = len(ids)
        out.append(ids[v])
    return np.asarray(out, np.int32)


def pair_counts(pred, truth):
    """(pairs together in both, pairs together in pred, pairs together in truth) by brute force; pred == -1 is alone"""
    n = len(pred)
    both = inp = intr = 0
    for i in range(n):
        for j in range(i + 1, n):
            p = pred[i] == pred[j] and pred[i] >= 0
            t = truth[i] == truth[j]
            both += p and t
            inp += p
            intr += t
    return int(both), int(inp), int(intr)


def bcubed(pred, truth):
    """(precision, recall) by the per-row definition"""
    n = len(pred)
    pr = rc = 0.0
    for i in range(n):
        same_p = [j for j in range(n) if j == i or (pred[i] >= 0 and pred[j] == pred[i])]
        same_t = [j for j in range(n) if truth[j] == truth[i]]
        inter = len(set(same_p) & set(same_t))
        pr += inter / len(same_p)
        rc += inter / len(same_t)
    return pr / n, rc / n
