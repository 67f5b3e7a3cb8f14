"""-m gpu: the clustering stage (include/fte.h "Clustering", tf_face_toolbox_amd/clustering.py, cluster.py) against the numpy
restatement (tests/cluster_ref.py).  Everything after the fp32 scores is integer logic, so every comparison is exact: keep masks
byte for byte, labels value for value.  The link kernels run on synthetic lists (holes, planted bad entries, scores equal to the
floor), the union-find on the graph shapes that give the deepest trees and the most contended roots, and the whole path end to
end on exactly representable rows (all chunkings) and on Gaussian rows."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import cluster_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 0.5                                     # scores are multiples of 1/16: some are exactly the floor


def _mods():
    from tf_face_toolbox_amd import _lib, clustering as C
    return _lib, C


# ------------------------------------------------------------------ links, direct, on synthetic lists
def _synthetic_lists(n, k, seed):
    """Per row a random permutation of the other rows, group-mates (groups of 3..12 consecutive rows) first so that lists of one
    group overlap, cut to k; k > n - 1 leaves (-inf, -1) tails.  Then planted bad entries n, -7 and the row itself, and (n >= 63)
    some rows that are all holes.  Scores: multiples of 1/16 in [0, 1]."""
    rng = np.random.default_rng(seed)
    group = np.zeros(n, np.int64)
    i = g = 0
    while i < n:
        s = int(rng.integers(3, 13))
        group[i:i + s] = g
        i, g = i + s, g + 1
    index = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), -np.inf, np.float32)
    for a in range(n):
        mates = rng.permutation([j for j in range(n) if j != a and group[j] == group[a]])
        rest = rng.permutation([j for j in range(n) if group[j] != group[a]])
        row = np.concatenate([mates, rest]).astype(np.int64)
        cut = int(rng.integers(0, len(mates) + 1))                   # some mates fall behind strangers
        row = np.concatenate([row[:cut], rng.permutation(row[cut:])])[:k] if rng.random() < 0.3 else row[:k]
        index[a, :len(row)] = row
        scores[a, :len(row)] = rng.integers(0, 17, len(row)) / 16.0
    if n > 1:
        bad = rng.random((n, k)) < 0.08
        index[bad] = rng.choice([n, -7], int(bad.sum()))
        for a in rng.choice(n, max(1, n // 10), replace=False):
            if n > 2 or k > 1:                                       # (n = 2, k = 1 would lose one of its two valid slots)
                index[a, rng.integers(0, k)] = a
    if n >= 63:
        for a in rng.choice(n, 3, replace=False):
            index[a] = rng.choice([n, -7, -1, a], k)
    return scores, index


def _one_answer(n, k, method, theta, floor, mutual):
    """why the valid slots of this case cannot hold both a 0 and a 1 (None: they can, and the case must show both)"""
    if n == 1:
        return 'n = 1: no valid slot'
    if n == 2 and method == 'threshold' and mutual:
        return 'n = 2, mutual: the two slots of the one pair get the same answer'
    if n == 2 and method == 'rank_order' and floor is None:
        return 'n = 2, no floor: the one pair has distance 0'
    if k == 1 and method == 'rank_order' and floor is None and theta == 2.5:
        return 'k = 1: m(a,b) + m(b,a) <= 2 < 2.5 * 1 for every valid slot'
    return None


@functools.lru_cache(maxsize=None)
def _lists_and_table(n, k, seed):
    scores, index = _synthetic_lists(n, k, seed)
    return scores, index, cr.rank_order_table(index)


def _link_case(n, k, method, theta, floor, mutual):
    """(scores, index, expected keep, all_zero): the first seed whose reference mask holds a 0 and a 1 among the valid slots"""
    why = _one_answer(n, k, method, theta, floor, mutual)
    for seed in range(16):
        scores, index, table = _lists_and_table(n, k, seed)
        if method == 'threshold':
            want = cr.links_threshold(scores, index, floor, mutual)
        else:
            want = cr.links_rank_order(scores, index, theta, -np.inf if floor is None else floor, table)
        got = set(want[table[0]].tolist())
        if why is not None or got == {0, 1}:
            break
    else:
        raise AssertionError('no seed gives a mask with both values for %s' % ((n, k, method, theta, floor, mutual),))
    assert want[~table[0]].sum() == 0
    if n == 1:
        assert table[0].sum() == 0 and want.sum() == 0              # marked: the expectation is all zeros
    return scores, index, want, why


VARIANTS = [('threshold', None, FLOOR, False), ('threshold', None, FLOOR, True)] + \
           [('rank_order', th, fl, False) for th in (0.5, 1.0, 0.3, 2.5) for fl in (None, FLOOR)]


@pytest.mark.parametrize('method,theta,floor,mutual', VARIANTS)
@pytest.mark.parametrize('k', [1, 7, 64])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 257])
def test_links_match_the_reference_byte_for_byte(n, k, method, theta, floor, mutual):
    _, C = _mods()
    scores, index, want, why = _link_case(n, k, method, theta, floor, mutual)
    if floor is not None and n > 2 and k > 1:
        assert (scores == FLOOR).any()                               # the `>=` edge is exercised
    keep = C.knn_links(torch.from_numpy(scores).cuda(), torch.from_numpy(index).cuda(), method, theta=theta, min_score=floor,
                       mutual=mutual)
    got = keep.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (why, np.argwhere(got != want)[:10].tolist())


def test_links_nan_scores_and_repeated_entries():
    """A NaN score compares false; an entry repeated in a row counts at its first position (the search never writes one)."""
    _, C = _mods()
    scores, index, _ = _lists_and_table(65, 7, 0)
    scores, index = scores.copy(), index.copy()
    rng = np.random.default_rng(5)
    scores[rng.random(scores.shape) < 0.1] = np.nan
    for a in range(0, 65, 4):
        index[a, 5] = index[a, 1]
        index[a, 6] = index[a, 0]
    s, i = torch.from_numpy(scores).cuda(), torch.from_numpy(index).cuda()
    for mutual in (False, True):
        assert C.knn_links(s, i, 'threshold', min_score=FLOOR, mutual=mutual).cpu().numpy().tobytes() == \
            cr.links_threshold(scores, index, FLOOR, mutual).tobytes()
    for theta, floor in ((1.0, None), (2.5, FLOOR), (0.5, -1.0)):
        want = cr.links_rank_order(scores, index, theta, -np.inf if floor is None else floor)
        assert C.knn_links(s, i, 'rank_order', theta=theta, min_score=floor).cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------ components, direct
def _path(order):
    """k = 1 lists: row order[j] points at order[j + 1]; the last row holds a hole"""
    n = len(order)
    index = np.full((n, 1), -1, np.int32)
    index[order[:-1], 0] = order[1:]
    return index, np.ones((n, 1), np.uint8)


def _star(leaves=3000, k=64):
    n, hub = leaves + 1, leaves // 2
    index = np.full((n, k), -1, np.int32)
    rows = np.asarray([r for r in range(n) if r != hub])
    index[rows, 0] = hub
    index[hub] = rows[::leaves // k][:k]
    keep = np.zeros((n, k), np.uint8)
    keep[rows, 0] = 1
    keep[hub] = 1
    return index, keep


def _two_cliques(size=8):
    n, k = 2 * size, size
    index = np.full((n, k), -1, np.int32)
    keep = np.zeros((n, k), np.uint8)
    for a in range(n):
        base = a // size * size
        index[a, :size - 1] = [j for j in range(base, base + size) if j != a]
        keep[a, :size - 1] = 1
        index[a, size - 1] = (a + size) % n                          # a slot into the other clique, kept by row 11 alone
    keep[11, size - 1] = 1
    return index, keep


@functools.lru_cache(maxsize=None)
def _random_graph(n=5000, k=8):
    rng = np.random.default_rng(17)
    index = np.stack([rng.choice(n - 1, k, replace=False) for _ in range(n)]).astype(np.int32)
    index += index >= np.arange(n)[:, None]                          # skip self
    index[rng.random((n, k)) < 0.02] = n
    for p in (0.04, 0.06, 0.08, 0.1, 0.14):
        keep = (np.random.default_rng(int(p * 1000)).random((n, k)) < p).astype(np.uint8)
        want = cr.components(index, keep)
        sizes = np.unique(want, return_counts=True)[1]
        if len(sizes) > 1 and sizes.max() > 100:
            return index, keep, want
    raise AssertionError('no keep probability gives several components with one above 100 rows')


def _graph(name):
    if name == 'path_ascending':
        return _path(np.arange(4097))
    if name == 'path_descending':
        return _path(np.arange(4097)[::-1].copy())
    if name == 'path_permuted':
        return _path(np.random.default_rng(3).permutation(4097))
    if name == 'star':
        return _star()
    if name == 'two_cliques':
        return _two_cliques()
    if name == 'all_zero':
        index = _random_graph()[0][:300, :8] % 300
        return index.astype(np.int32), np.zeros(index.shape, np.uint8)
    if name == 'single_row':
        return np.asarray([[0]], np.int32), np.ones((1, 1), np.uint8)
    return _random_graph()[:2]


@pytest.mark.parametrize('name', ['path_ascending', 'path_descending', 'path_permuted', 'star', 'two_cliques', 'all_zero', 'single_row',
                                  'random'])
def test_components_match_the_reference_and_repeat(name):
    _, C = _mods()
    index, keep = _graph(name)
    want = _random_graph()[2] if name == 'random' else cr.components(index, keep)
    n = len(index)
    if name.startswith('path') or name in ('star', 'two_cliques'):
        assert (want == 0).all()                                     # one component: every label is row 0
    if name in ('all_zero', 'single_row'):
        assert want.tolist() == list(range(n))
    i, kp = torch.from_numpy(index).cuda(), torch.from_numpy(keep).cuda()
    first = C.components(i, kp).cpu().numpy()
    assert first.dtype == np.int32 and first.tolist() == want.tolist()
    assert C.components(i, kp).cpu().numpy().tobytes() == first.tobytes()


def test_two_cliques_need_the_one_sided_slot():
    _, C = _mods()
    index, keep = _two_cliques()
    keep[11, 7] = 0
    got = C.components(torch.from_numpy(index).cuda(), torch.from_numpy(keep).cuda()).cpu().numpy()
    assert got.tolist() == [0] * 8 + [8] * 8


# ------------------------------------------------------------------ end to end
def _exact_rows(rng, n, d=64):
    """16 entries of +-0.25 per row: norm exactly 1, every dot product an exact multiple of 1/16 in fp32 (many ties)"""
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        x[i, rng.choice(d, 16, replace=False)] = rng.choice([-0.25, 0.25], 16)
    return x


@functools.lru_cache(maxsize=None)
def _exact_set(ids=40, per=12, d=64, k=10):
    """rows of `ids` identities that share most of their signs with a centre row, their float64 brute-force kNN lists and the
    reference's rank-order table"""
    rng = np.random.default_rng(11)
    c = _exact_rows(rng, ids, d)
    labels = np.repeat(np.arange(ids), per)
    x = c[labels].copy()
    for i in range(len(x)):
        nz = np.nonzero(x[i])[0]
        flip = rng.choice(nz, rng.integers(0, 5), replace=False)
        x[i, flip] *= -1
    scores, index = cr.topk(x, k)
    return x, labels, scores, index, cr.rank_order_table(index)


EXACT_METHODS = {'rank_order': dict(theta=1.0), 'rank_order_floor': dict(theta=2.5, min_score=0.5),
                 'threshold': dict(min_score=0.625), 'threshold_mutual': dict(min_score=0.5, mutual=True)}


def _exact_want(name, min_size=1):
    x, labels, scores, index, table = _exact_set()
    kw = EXACT_METHODS[name]
    if name.startswith('rank_order'):
        keep = cr.links_rank_order(scores, index, kw['theta'], kw.get('min_score', -np.inf), table)
    else:
        keep = cr.links_threshold(scores, index, kw['min_score'], kw.get('mutual', False))
    return cr.renumber(cr.components(index, keep), min_size)


@pytest.mark.parametrize('name', sorted(EXACT_METHODS))
def test_exact_rows_end_to_end_for_every_chunking(name):
    _, C = _mods()
    x, labels, scores, index, _ = _exact_set()
    want = _exact_want(name)
    assert 1 < want.max() + 1 < len(x)                               # neither one cluster nor all singletons
    xd = torch.from_numpy(x).cuda()
    gs, gi = C.knn_graph(xd, 10)
    assert gi.cpu().numpy().tolist() == index.tolist() and gs.cpu().numpy().tobytes() == scores.tobytes()
    method = name.split('_')[0] if name.startswith('threshold') else 'rank_order'
    for chunk_rows in (None, 50, 97):
        got = C.cluster(xd, 10, method, chunk_rows=chunk_rows, **EXACT_METHODS[name])
        assert got.dtype == np.int32 and got.tolist() == want.tolist(), chunk_rows
    sc = C.clustering_scores(want, labels)
    print('exact rows, %s: %s' % (name, json.dumps(sc)))


def test_knn_graph_pads_when_k_exceeds_the_set():
    _, C = _mods()
    x = _exact_set()[0][:5]
    gs, gi = C.knn_graph(torch.from_numpy(x).cuda(), 7)
    ws, wi = cr.topk(x, 7)
    assert gi.cpu().numpy().tolist() == wi.tolist() and gs.cpu().numpy().tobytes() == ws.tobytes()
    assert (wi[:, 4:] == -1).all()


def test_gaussian_rows_end_to_end():
    """n = 3,000, d = 128, 150 centres.  The reference consumes the GPU's own lists (the search has its own tests); labels exact;
    the scores against the planted labels are printed, not asserted: nobody has measured them."""
    _, C = _mods()
    rng = np.random.default_rng(23)
    n, d, ids, k = 3000, 128, 150, 16
    planted = rng.integers(0, ids, n)
    cen = rng.standard_normal((ids, d))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    x = (cen[planted] + rng.standard_normal((n, d)) * np.sqrt(0.6 / d)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    gs, gi = C.knn_graph(xd, k, chunk_rows=1100)
    scores, index = gs.cpu().numpy(), gi.cpu().numpy()
    assert ((index >= 0) & (index < n) & (index != np.arange(n)[:, None])).all() and (np.diff(scores, axis=1) <= 0).all()
    table = cr.rank_order_table(index)
    for method, kw in (('rank_order', dict(theta=1.0)), ('rank_order', dict(theta=2.0, min_score=0.5)),
                       ('threshold', dict(min_score=0.55)), ('threshold', dict(min_score=0.5, mutual=True))):
        if method == 'rank_order':
            want_keep = cr.links_rank_order(scores, index, kw['theta'], kw.get('min_score', -np.inf), table)
        else:
            want_keep = cr.links_threshold(scores, index, kw['min_score'], kw.get('mutual', False))
        keep = C.knn_links(gs, gi, method, **kw)
        assert keep.cpu().numpy().tobytes() == want_keep.tobytes()
        want = cr.renumber(cr.components(index, want_keep), 2)
        got = C.cluster(xd, k, method, min_size=2, chunk_rows=1100, **kw)
        assert got.tolist() == want.tolist()
        print('gaussian rows, %s %s: %s' % (method, kw, json.dumps(C.clustering_scores(got, planted))))


# ------------------------------------------------------------------ errors and CLI
def test_c_abi_error_codes():
    lib, _ = _mods()
    L = lib.load()
    s = torch.zeros(4, 4, dtype=torch.float32, device='cuda')
    i = torch.zeros(4, 4, dtype=torch.int32, device='cuda')
    kp = torch.zeros(4, 4, dtype=torch.uint8, device='cuda')
    par = torch.zeros(4, dtype=torch.int32, device='cuda')
    lab = torch.zeros(4, dtype=torch.int32, device='cuda')
    S, I, K, P, Lb = (t.data_ptr() for t in (s, i, kp, par, lab))
    EINVAL = -1
    ninf = float('-inf')
    assert L.fte_knn_links_threshold(S, I, 4, 4, 0.5, 0, K, None) == 0
    assert L.fte_knn_links_rank_order(S, I, 4, 4, 1.0, ninf, K, None) == 0
    assert L.fte_components(I, K, 4, 4, P, Lb, None) == 0
    for bad in ((None, I, K), (S, None, K), (S, I, None)):
        assert L.fte_knn_links_threshold(bad[0], bad[1], 4, 4, 0.5, 0, bad[2], None) == EINVAL
        assert L.fte_knn_links_rank_order(bad[0], bad[1], 4, 4, 1.0, ninf, bad[2], None) == EINVAL
    for bad in ((None, K, P, Lb), (I, None, P, Lb), (I, K, None, Lb), (I, K, P, None)):
        assert L.fte_components(bad[0], bad[1], 4, 4, bad[2], bad[3], None) == EINVAL
    for n, k in ((0, 4), (-3, 4), (4, 0), (4, 65), (4, -1), (1 << 23, 64), (1 << 28, 2)):       # the last two: n * k = 2^29
        assert L.fte_knn_links_threshold(S, I, n, k, 0.5, 1, K, None) == EINVAL, (n, k)
        assert L.fte_knn_links_rank_order(S, I, n, k, 1.0, ninf, K, None) == EINVAL, (n, k)
        assert L.fte_components(I, K, n, k, P, Lb, None) == EINVAL, (n, k)
    for theta in (0.0, -1.0, float('inf'), float('nan')):
        assert L.fte_knn_links_rank_order(S, I, 4, 4, theta, ninf, K, None) == EINVAL, theta
    torch.cuda.synchronize()
    _, C = _mods()
    with pytest.raises(ValueError):
        C.knn_links(s, i, 'rank_order')
    with pytest.raises(ValueError):
        C.knn_links(s, i, 'threshold')
    with pytest.raises(ValueError):
        C.knn_links(s, i, 'kmeans', theta=1.0)
    with pytest.raises(ValueError):
        C.knn_graph(s, 65)


def test_cluster_cli_end_to_end(tmp_path):
    import cluster as cli
    x, labels, _, _, _ = _exact_set()
    np.save(str(tmp_path / 'fea.npy'), x)
    paths = ['id%03d/img_%04d.jpg' % (l, r) for r, l in enumerate(labels)]
    with open(str(tmp_path / 'list.txt'), 'w') as f:
        f.writelines('%s %d\n' % (p, l) for p, l in zip(paths, labels))
    out, js = str(tmp_path / 'out' / 'clustered.txt'), str(tmp_path / 'out' / 'clusters.json')
    cli.main(['--feature_path', str(tmp_path / 'fea.npy'), '--data_list_path', str(tmp_path / 'list.txt'), '--k', '10', '--method',
              'threshold', '--min_score', '0.625', '--min_size', '3', '--chunk_rows', '97', '--out_list', out, '--output_json', js])
    want = _exact_want('threshold', 3)
    assert (want == -1).any() and want.max() > 0                     # some clusters are dropped, several are kept
    lines = [ln.split() for ln in open(out)]
    assert all(len(t) == 2 for t in lines)
    assert [t[0] for t in lines] == [p for p, c in zip(paths, want) if c >= 0]          # rows of dropped clusters are absent
    ids = [int(t[1]) for t in lines]
    assert ids == want[want >= 0].tolist()
    assert sorted(set(ids)) == list(range(max(ids) + 1))             # dense
    res = json.load(open(js))
    assert res['rows'] == len(x) and res['kept_rows'] == len(lines) and res['kept_clusters'] == max(ids) + 1
    _, C = _mods()
    sc = C.clustering_scores(want, labels)
    assert set(res['scores']) == set(sc)
    for key, v in sc.items():
        assert res['scores'][key] == pytest.approx(v, abs=1e-12), key
