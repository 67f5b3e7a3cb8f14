"""CPU: the host half of the clustering stage (tf_face_toolbox_amd/clustering.py renumber / clustering_scores, cluster.py flags and
list writer) against hand-computed answers and brute force, and the numpy restatement (cluster_ref.py) against itself: the
rank-order distance is symmetric, and the union-find labels equal a brute-force transitive closure."""
import numpy as np
import pytest

import cluster as cli
import cluster_ref as cr
from tf_face_toolbox_amd import clustering as C


def _random_lists(rng, n, k, holes=0.15):
    """kNN-like lists: per row a random permutation of the other rows cut to k, tails and planted bad entries as holes; scores
    are multiples of 1/16, descending along the row"""
    index = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), -np.inf, np.float32)
    for a in range(n):
        others = rng.permutation([j for j in range(n) if j != a])[:k]
        index[a, :len(others)] = others
        scores[a, :len(others)] = np.sort(rng.integers(-4, 17, len(others)))[::-1] / 16.0
    bad = rng.random((n, k)) < holes
    index[bad] = rng.choice([n, -7, n + 5], int(bad.sum()))
    for a in rng.choice(n, max(1, n // 8), replace=False):
        index[a, rng.integers(0, k)] = a                  # self
    return scores, index


def test_rank_order_distance_is_symmetric_in_the_reference():
    rng = np.random.default_rng(0)
    for n, k in ((12, 5), (40, 7), (30, 29)):
        scores, index = _random_lists(rng, n, k)
        for theta in (0.5, 1.0, 2.5):
            keep = cr.links_rank_order(scores, index, theta)
            assert 0 < keep.sum() < keep.size
            for a in range(n):
                for b in range(n):
                    if a != b:
                        assert cr.rank_order_parts(index, a, b) == cr.rank_order_parts(index, b, a)
            for a in range(n):                            # a pair listed from both sides gets one answer
                for t in range(k):
                    if not cr.valid(index, a, t):
                        continue
                    b = int(index[a, t])
                    for u in range(k):
                        if int(index[b, u]) == a:
                            first = [v for v in range(k) if int(index[b, v]) == a][0]
                            firsta = [v for v in range(k) if int(index[a, v]) == b][0]
                            assert keep[a, firsta] == keep[b, first]


def test_rank_order_hand_example():
    # rows 0, 1, 2 list each other first; row 3 lists 0, 1 and a hole.  k = 3.
    index = np.asarray([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, -1]], np.int32)
    scores = np.full((4, 3), 0.5, np.float32)
    # (0, 1): r = 1 both ways.  m(0,1): positions 0..1 of L_0 = (0, 1): both in L_1 = {1, 0, 2, 3} -> 0; m(1,0) likewise 0.
    assert cr.rank_order_parts(index, 0, 1) == (0, 1)
    # (0, 3): r(0,3) = 3, r(3,0) = 1.  m(0,3): positions 0..3 of L_0 = (0, 1, 2, 3); L_3 = {3, 0, 1}: only 2 is missing -> 1.
    # m(3,0): positions 0..1 of L_3 = (3, 0): both in L_0 -> 0.
    assert cr.rank_order_parts(index, 0, 3) == (1, 1)
    # (3, 2): 2 is not in L_3: r(3,2) = k + 1 = 4, r(2,3) = 3.  m(3,2): positions 0..3 of L_3 = (3, 0, 1, hole): all in L_2 -> 0;
    # m(2,3): positions 0..3 of L_2 = (2, 0, 1, 3): 2 is missing from L_3 -> 1.
    assert cr.rank_order_parts(index, 3, 2) == (1, 3)
    keep = cr.links_rank_order(scores, index, 1.0)
    # (1, 3): r(1,3) = 3, r(3,1) = 2; m(1,3) = 1 (2 is missing from L_3), m(3,1) = 0: 1 < 1.0 * 2 links, and so does (3, 1).
    assert cr.rank_order_parts(index, 1, 3) == (1, 2)
    # pairs among 0, 1, 2: distance 0.  (0,3) / (3,0): 1 < 1.0 * 1 fails.  (2,3): 1 < 1.0 * 3 links.
    assert keep.tolist() == [[1, 1, 0], [1, 1, 1], [1, 1, 1], [0, 1, 0]]
    assert cr.links_rank_order(scores, index, 1.0, min_score=0.5).tolist() == keep.tolist()       # >= keeps an equal score
    assert cr.links_rank_order(scores, index, 1.0, min_score=0.5625).sum() == 0


def test_threshold_reference_mutual():
    index = np.asarray([[1, 2], [2, 0], [0, 5]], np.int32)
    scores = np.asarray([[0.5, 0.25], [0.75, 0.5], [0.5, 0.9]], np.float32)
    assert cr.links_threshold(scores, index, 0.5, False).tolist() == [[1, 0], [1, 1], [1, 0]]
    # (0,1) back (1,0) 0.5 ok; (1,2): row 2 does not list 1; (1,0) ok; (2,0): row 0 lists 2 at 0.25 < 0.5
    assert cr.links_threshold(scores, index, 0.5, True).tolist() == [[1, 0], [0, 1], [0, 0]]


@pytest.mark.parametrize('n,k,p', [(1, 1, 1.0), (2, 1, 1.0), (17, 3, 0.3), (60, 4, 0.12), (60, 2, 0.5)])
def test_reference_labels_equal_a_transitive_closure(n, k, p):
    rng = np.random.default_rng(n * 100 + k)
    _, index = _random_lists(rng, n, k) if n > 1 else (None, np.asarray([[0]], np.int32))
    keep = (rng.random((n, k)) < p).astype(np.uint8)
    got = cr.components(index, keep)
    assert got.tolist() == cr.closure_labels(index, keep).tolist()
    assert all(got[i] <= i for i in range(n)) and all(got[got[i]] == got[i] for i in range(n))


def test_renumber_and_min_size():
    label = np.asarray([5, 5, 2, 9, 2, 5, 7], np.int32)
    assert C.renumber(label).tolist() == [0, 0, 1, 2, 1, 0, 3]
    assert C.renumber(label, 2).tolist() == [0, 0, 1, -1, 1, 0, -1]
    assert C.renumber(label, 3).tolist() == [0, 0, -1, -1, -1, 0, -1]
    assert C.renumber(label, 4).tolist() == [-1] * 7
    assert C.renumber(label, 2).dtype == np.int32
    with pytest.raises(ValueError):
        C.renumber(label, 0)
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 50, 400)
    for ms in (1, 2, 7, 12):
        assert C.renumber(lab, ms).tolist() == cr.renumber(lab, ms).tolist()


def test_scores_perfect_and_all_singletons():
    truth = np.asarray([0, 0, 0, 1, 1, 2])
    s = C.clustering_scores(np.asarray([4, 4, 4, 0, 0, 9]), truth)
    for key in ('pairwise_precision', 'pairwise_recall', 'pairwise_f', 'bcubed_precision', 'bcubed_recall', 'bcubed_f', 'nmi'):
        assert s[key] == pytest.approx(1.0, abs=1e-12), key
    assert (s['clusters'], s['singletons'], s['n']) == (3, 1, 6)
    for pred in (np.arange(6), np.full(6, -1)):           # every row alone
        s = C.clustering_scores(pred, truth)
        assert s['pairwise_precision'] == 1.0 and s['pairwise_recall'] == 0.0 and s['pairwise_f'] == 0.0       # 0 of 3 + 1 pairs
        assert s['bcubed_precision'] == 1.0
        assert s['bcubed_recall'] == pytest.approx((3 * (1 / 3) + 2 * (1 / 2) + 1) / 6, abs=1e-15)              # = 1/2
        assert (s['clusters'], s['singletons']) == (6, 6)
        # I = H(truth) (pred determines truth), H(pred) = ln 6
        ht = -(0.5 * np.log(0.5) + (1 / 3) * np.log(1 / 3) + (1 / 6) * np.log(1 / 6))
        assert s['nmi'] == pytest.approx(2 * ht / (ht + np.log(6)), abs=1e-12)


def test_scores_hand_computed_bcubed():
    # the textbook case: truth A A A A B B B, predicted {A A A B} {A B B}
    truth = np.asarray([0, 0, 0, 0, 1, 1, 1])
    pred = np.asarray([0, 0, 0, 1, 0, 1, 1])
    s = C.clustering_scores(pred, truth)
    # precision: rows of A in cluster 0: 3/4 each (3 rows), B in cluster 0: 1/4; A in cluster 1: 1/3, B in cluster 1: 2/3 each (2 rows)
    assert s['bcubed_precision'] == pytest.approx((3 * 3 / 4 + 1 / 4 + 1 / 3 + 2 * 2 / 3) / 7, abs=1e-15)
    # recall: A rows in cluster 0: 3/4 each, the A row in cluster 1: 1/4; B row in cluster 0: 1/3, B rows in cluster 1: 2/3 each
    assert s['bcubed_recall'] == pytest.approx((3 * 3 / 4 + 1 / 4 + 1 / 3 + 2 * 2 / 3) / 7, abs=1e-15)
    # pairs: together in both: C(3,2) + C(2,2) = 4; predicted C(4,2) + C(3,2) = 9; truth C(4,2) + C(3,2) = 9
    assert s['pairwise_precision'] == pytest.approx(4 / 9) and s['pairwise_recall'] == pytest.approx(4 / 9)
    assert (s['clusters'], s['singletons']) == (2, 0)


def test_scores_equal_brute_force():
    rng = np.random.default_rng(7)
    for n, npred, ntrue in ((40, 6, 5), (90, 30, 8), (25, 3, 25)):
        pred = rng.integers(0, npred, n)
        pred[rng.random(n) < 0.15] = -1
        truth = rng.integers(0, ntrue, n) * 3 - 4         # labels need not be dense or non-negative
        s = C.clustering_scores(pred, truth)
        both, inp, intr = cr.pair_counts(pred, truth)
        assert s['pairwise_precision'] == pytest.approx(both / inp if inp else 1.0, abs=1e-15)
        assert s['pairwise_recall'] == pytest.approx(both / intr if intr else 1.0, abs=1e-15)
        bp, br = cr.bcubed(pred, truth)
        assert s['bcubed_precision'] == pytest.approx(bp, abs=1e-12) and s['bcubed_recall'] == pytest.approx(br, abs=1e-12)
        sizes = np.unique(pred[pred >= 0], return_counts=True)[1]
        assert s['clusters'] == len(sizes) + int((pred < 0).sum())
        assert s['singletons'] == int((sizes == 1).sum()) + int((pred < 0).sum())
        assert 0.0 <= s['nmi'] <= 1.0
    with pytest.raises(ValueError):
        C.clustering_scores([0, 1], [0])


BASE = ['--feature_path', 'f.npy', '--data_list_path', 'l.txt', '--out_list', 'o.txt']


@pytest.mark.parametrize('extra', [['--method', 'rank_order'], ['--method', 'threshold'], ['--method', 'threshold', '--theta', '1.0'],
                                   ['--method', 'rank_order', '--theta', '1.0', '--k', '0'],
                                   ['--method', 'rank_order', '--theta', '1.0', '--k', '65'],
                                   ['--method', 'rank_order', '--theta', '-1.0'], ['--method', 'rank_order', '--theta', 'nan'],
                                   ['--method', 'rank_order', '--theta', '1.0', '--mutual', '1'],
                                   ['--method', 'threshold', '--min_score', '0.5', '--theta', '1.0'],
                                   ['--method', 'threshold', '--min_score', '0.5', '--min_size', '0'], ['--method', 'kmeans', '--theta', '1']])
def test_cli_refuses_bad_flags(extra):
    with pytest.raises(SystemExit) as e:
        cli.check_flags(cli.build_parser().parse_args(BASE + extra))
    assert e.value.code not in (0, None)


def test_cli_accepts_good_flags_and_says_why_there_is_no_default():
    f = cli.build_parser().parse_args(BASE + ['--method', 'rank_order', '--theta', '1.5'])
    cli.check_flags(f)
    assert f.k == 32 and f.min_size == 1 and f.min_score is None
    for k in ('1', '64'):
        cli.check_flags(cli.build_parser().parse_args(BASE + ['--method', 'threshold', '--min_score', '0.4', '--mutual', '1', '--k', k]))
    text = ' '.join(cli.build_parser().format_help().split())
    assert text.count('has not been measured') == 2 and 'no default' in text


def test_cli_list_reader_and_writer(tmp_path):
    src = tmp_path / 'l.txt'
    src.write_text('a/1.jpg 7\n\nb/2.jpg 7\nc/3.jpg 9\nd/4.jpg 9\n')
    paths, labels = cli.read_list(str(src))
    assert paths == ['a/1.jpg', 'b/2.jpg', 'c/3.jpg', 'd/4.jpg'] and labels.tolist() == [7, 7, 9, 9]
    src.write_text('a/1.jpg\nb/2.jpg\n')
    assert cli.read_list(str(src)) == (['a/1.jpg', 'b/2.jpg'], None)
    out = tmp_path / 'sub' / 'o.txt'
    assert cli.write_list(str(out), paths, np.asarray([1, -1, 0, 1], np.int32)) == 3
    assert out.read_text() == 'a/1.jpg 1\nc/3.jpg 0\nd/4.jpg 1\n'


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """The argument checks return before the first device call, so they run here too: every listed case is FTE_EINVAL."""
    import ctypes
    from tf_face_toolbox_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_char * 4096)()                        # host memory: never dereferenced on these paths
    p = ctypes.addressof(buf)
    ninf = float('-inf')
    for s, i, kp in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.fte_knn_links_threshold(s, i, 4, 4, 0.5, 0, kp, None) == -1
        assert L.fte_knn_links_rank_order(s, i, 4, 4, 1.0, ninf, kp, None) == -1
    for i, kp, par, lab in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.fte_components(i, kp, 4, 4, par, lab, None) == -1
    for n, k in ((0, 4), (-3, 4), (4, 0), (4, 65), (4, -1), (1 << 23, 64), (1 << 28, 2)):
        assert L.fte_knn_links_threshold(p, p, n, k, 0.5, 1, p, None) == -1, (n, k)
        assert L.fte_knn_links_rank_order(p, p, n, k, 1.0, ninf, p, None) == -1, (n, k)
        assert L.fte_components(p, p, n, k, p, p, None) == -1, (n, k)
    for theta in (0.0, -1.0, float('inf'), float('nan')):
        assert L.fte_knn_links_rank_order(p, p, 4, 4, theta, ninf, p, None) == -1, theta
