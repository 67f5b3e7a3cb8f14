"""CPU: the inputs and expectations of tests/search_cases.py justify the exact comparisons of tests/test_gpu_search_edges.py.
Every row set is exact (fp32 products equal float64 ones, scores are multiples of 1/16 and never sit inside a histogram bin's
rounding reach), every top-k case really has the ties it is there for, every case reaches the slice plan it claims at 256 CUs,
and a set score's fp32 sum does not depend on the order.  Also the expectations against verify_ref and hand-made examples."""
import numpy as np
import pytest

import search_cases as sc
import verify_ref as vr

_CACHE = {}


def _topk(case):
    if case['name'] not in _CACHE:
        P, G = sc.topk_inputs(case)
        _CACHE[case['name']] = (P, G) + sc.topk_expected_of(case)
    return _CACHE[case['name']]


def _assert_exact(P, G, unit=16.0):
    """fp32 products equal the float64 ones, every score is a multiple of 1 / unit, and lands on an integer bin coordinate"""
    s64 = P.astype(np.float64) @ G.astype(np.float64).T
    s32 = P @ G.T
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)
    assert np.array_equal(s64 * unit, np.round(s64 * unit))
    for nbins in (256, 8192):
        e = (s64 + 1.0) * nbins / 2
        assert np.array_equal(e, np.round(e))
        # the fp32 expression of fte.h lands on the same integer: no score is within rounding reach of a bin edge
        e32 = (s32 + np.float32(1.0)) * np.float32(0.5 * nbins)
        assert np.array_equal(e32.astype(np.float64), e)
    return s64


@pytest.mark.parametrize('case', sc.TOPK_CASES, ids=lambda c: c['name'])
def test_topk_case_rows_exact_and_tied(case):
    P, G, es, ei = _topk(case)
    m, n, k = case['m'], case['n'], case['k']
    assert P.shape == (m, case['d']) and G.shape == (n, case['d'])
    assert np.all((P * P).sum(1) == 1.0) and np.all((G * G).sum(1) == 1.0)
    s = _assert_exact(P, G)
    excl = bool(case.get('excl', 0))
    if excl:
        self_col = case['p0'] + np.arange(m) - case['g0']
        inside = (self_col >= 0) & (self_col < n)
        s[np.arange(m)[inside], self_col[inside]] = -np.inf     # not a candidate
    cand = np.isfinite(s).sum(1)
    assert np.array_equal((ei >= 0).sum(1), np.minimum(cand, k))
    if case['ties'] == 'overflow':
        assert np.all(cand > k)
        kth = es[:, k - 1]
        tied = (s == kth[:, None]).sum(1)                        # candidates at the k-th score
        places = k - (s > kth[:, None]).sum(1)                   # slots the tied rows compete for
        assert np.all(places >= 1)
        over = tied > places
        assert over.any(), 'no probe has more tied rows than places: the case does not test the tie rule'
        if case.get('every_probe'):
            assert over.all(), (tied[~over], places[~over])
    elif case['ties'] == 'order':
        assert np.all(cand <= k)
        real = ei >= 0
        eq = (es[:, :-1] == es[:, 1:]) & real[:, :-1] & real[:, 1:]
        assert eq.any(1).all(), 'a probe without two equal scores: nothing to order by index'
    else:
        assert n == 1


def test_topk_self_rows_fall_where_the_cases_say():
    by = {c['name']: c for c in sc.TOPK_CASES}

    def inside(c):
        col = c['p0'] + np.arange(c['m']) - c['g0']
        return (col >= 0) & (col < c['n']), col
    assert inside(by['X_self_inside'])[0].all() and inside(by['X_self_inside_offset'])[0].all()
    assert not inside(by['X_self_outside'])[0].any()
    some, col = inside(by['X_self_inside_for_some'])
    assert some.any() and not some.all()
    n = by['X_self_inside_for_some']['n']
    assert np.all((col[~some] >= n) & (col[~some] < (n + 63) // 64 * 64))     # on rows the last step reads through the clamp
    assert inside(by['X_k_eq_n_excl'])[0].all()


@pytest.mark.parametrize('case', sc.TOPK_CASES, ids=lambda c: c['name'])
def test_topk_slice_plan_at_256_cus(case):
    m, n = case['m'], case['n']
    assert sc.topk_slices(m, n, 256) == case['slices']
    assert sc.steps_per_slice(m, n, 256) == case['steps']
    assert sc.empty_slices(m, n, 256) == case['empty']
    assert case['slices'] <= 64 and case['slices'] * case['steps'] >= (n + 63) // 64


def test_slice_plan_restates_the_launcher():
    # hand-computed from s_topk_slices: want = 8 * CUs one-wave blocks over the 32-probe blocks, capped at 64 and at the steps
    assert sc.topk_slices(1, 1, 256) == 1
    assert sc.topk_slices(33, 16421, 256) == 64 and sc.steps_per_slice(33, 16421, 256) == 5
    assert sc.topk_slices(4101, 4133, 256) == 16              # ceil(2048 / 129)
    assert sc.topk_slices(100000, 100003, 256) == 1           # more probe blocks than wanted blocks
    assert sc.topk_slices(33, 16421, 8) == 32 and sc.steps_per_slice(33, 16421, 8) == 9


def test_dup_case_layout():
    case = next(c for c in sc.TOPK_CASES if c['rows'] == 'dups')
    P, G, es, ei = _topk(case)
    assert len(sc.DUP_POS) == 200 and sc.DUP_POS.max() < case['n']
    per_step = np.bincount(sc.DUP_POS // 64, minlength=16)
    assert per_step.min() >= 8                                 # every 64-row step (= slice) holds copies
    assert np.all(es[:sc.DUP_PROBES] == 1.0)
    assert np.array_equal(ei[:sc.DUP_PROBES], np.tile(sc.DUP_POS[:64], (sc.DUP_PROBES, 1)))


def test_topk_expected_against_verify_ref_and_by_hand():
    rng = np.random.default_rng(3)
    P, G = sc.exact_rows(rng, 7, 32), sc.exact_rows(rng, 40, 32)
    s, i = sc.topk_expected(P, G, 9)
    rs, ri = vr.topk(P, G, 9)
    assert np.array_equal(s, rs) and np.array_equal(i, ri)
    X = sc.exact_rows(rng, 12, 32)
    s, i = sc.topk_expected(X, X, 12, exclude_self=True)
    rs, ri = vr.topk(X, X, 12, exclude_self=True)
    assert np.array_equal(s, rs) and np.array_equal(i, ri) and np.all(i[:, -1] == -1)
    # bases: probes 5..8 against gallery rows 3..10 of one set
    s, i = sc.topk_expected(X[5:9], X[3:11], 8, gallery_base=3, probe_base=5, exclude_self=True)
    for r in range(4):
        assert 5 + r not in i[r] and i[r, -1] == -1 and sorted(i[r, :-1].tolist()) == [j for j in range(3, 11) if j != 5 + r]
    e = np.eye(4, 32, dtype=np.float32)
    G = np.stack([e[1], e[0], e[0], e[2], e[0]])
    s, i = sc.topk_expected(e[:1], G, 3, gallery_base=10)
    assert i.tolist() == [[11, 12, 14]] and s.tolist() == [[1.0, 1.0, 1.0]]


def test_merge_expected_by_hand_and_inputs_follow_the_contract():
    ninf = -np.inf
    in_s = np.array([[[0.5, 0.25, ninf], [0.5, 0.5, 0.0], [ninf, ninf, ninf]]])
    in_i = np.array([[[7, 1, -1], [3, 9, 2], [-1, -1, -1]]])
    s, i = sc.merge_expected(in_s, in_i, 3)
    assert i.tolist() == [[3, 7, 9]] and s.tolist() == [[0.5, 0.5, 0.5]]
    s, i = sc.merge_expected(in_s[:, 2:], in_i[:, 2:], 3)
    assert i.tolist() == [[-1, -1, -1]] and np.all(np.isneginf(s))
    rng = np.random.default_rng(4)
    short = empty = cross = 0
    for m in sc.MERGE_M:
        for lists in sc.MERGE_LISTS:
            for k in sc.MERGE_K:
                a, b = sc.merge_inputs(rng, m, lists, k)
                assert a.shape == (m, lists, k) and a.dtype == np.float32 and b.dtype == np.int32
                real = b >= 0
                assert np.all(np.isneginf(a[~real])) and np.all(real[..., :-1] >= real[..., 1:])     # empty slots last
                ok = (a[..., :-1] > a[..., 1:]) | ((a[..., :-1] == a[..., 1:]) & (b[..., :-1] < b[..., 1:]))
                assert np.all(ok | ~real[..., 1:])                                                 # each list in the order
                for r in range(m):
                    ids = b[r][real[r]]
                    assert len(set(ids.tolist())) == len(ids)                                      # disjoint indices
                fill = real.sum(2)
                short += int(((fill > 0) & (fill < k)).sum())
                empty += int((fill == 0).sum())
                if m > 1:
                    assert not real[-1].any()
                es, ei = sc.merge_expected(a, b, k)
                if lists > 1:
                    for r in range(m):
                        for t in range(k - 1):
                            if ei[r, t + 1] >= 0 and es[r, t] == es[r, t + 1]:
                                la = np.argwhere(b[r] == ei[r, t])[0][0]
                                lb = np.argwhere(b[r] == ei[r, t + 1])[0][0]
                                cross += la != lb
    assert short > 0 and empty > 0 and cross > 0


def test_hist_sets_exact_and_expected_against_verify_ref():
    x, lab = sc.hist_set()
    assert len(set(lab.tolist())) == 4
    _assert_exact(x, x)
    for n in (2, 33, 130):
        hg, hi = sc.hist_expected(x[:n], lab[:n], x[:n], lab[:n], 1, 256)
        rg, ri, _, _, _ = vr.histograms(x[:n], lab[:n], 256)
        assert np.array_equal(hg, rg.astype(np.uint64)) and np.array_equal(hi, ri.astype(np.uint64))
        assert int(hg.sum() + hi.sum()) == n * (n - 1) // 2
    hg, hi = sc.hist_expected(x[:130], lab[:130], x[:130], lab[:130], 1, 8192)
    assert hg.sum() > 0 and hi.sum() > 0 and np.count_nonzero(hg + hi) >= 8
    hg, hi = sc.hist_expected(x[:1], lab[:1], x[:1], lab[:1], 1, 256)
    assert hg.sum() == 0 and hi.sum() == 0
    hg, hi = sc.hist_expected(x[:65], lab[:65], x[100:101], lab[100:101], 0, 256)
    assert int(hg.sum() + hi.sum()) == 65
    # the clamps: s == 1.0f goes to the last bin (both histograms), scores of norm-2 rows beyond [-1, 1] to the first and last
    xd, ld = sc.hist_dup_set()
    _assert_exact(xd, xd)
    s = xd.astype(np.float64) @ xd.astype(np.float64).T
    iu = np.triu_indices(len(xd), 1)
    ones = s[iu] == 1.0
    same_lab = (ld[:, None] == ld[None, :])[iu]
    assert (ones & same_lab).sum() >= 10 and (ones & ~same_lab).sum() >= 10
    for nbins in sc.HIST_NBINS:
        hg, hi = sc.hist_expected(xd, ld, xd, ld, 1, nbins)
        assert hg[-1] == (ones & same_lab).sum() and hi[-1] == (ones & ~same_lab).sum()
    x2, l2 = sc.hist_set(97, 32, scale=0.5, seed=57)
    s2 = _assert_exact(x2, x2, unit=4.0)[np.triu_indices(97, 1)]
    assert (s2 < -1).sum() > 10 and (s2 >= 1).sum() > 10 and np.abs(s2).max() > 1.5
    hg, hi = sc.hist_expected(x2, l2, x2, l2, 1, 256)
    assert int(hg[0] + hi[0]) == (s2 <= -1 + 2 / 256 - 1e-9).sum() and int(hg[-1] + hi[-1]) == (s2 >= 1 - 2 / 256).sum()


@pytest.mark.parametrize('d', sc.SET_D)
def test_set_scores_do_not_depend_on_the_fp32_sum_order(d):
    x = sc.set_rows(d)
    _assert_exact(x, x)
    members, media_off, tmpl_off, rows = sc.set_lists()
    assert [len(r) for r in rows] == sc.SET_SIZES and len(members) == media_off[-1] == len(x)
    # every partial sum is a multiple of 1/16 of magnitude <= |A| |B| <= 48 * 48, an integer below 2^24 in units of 1/16
    assert 16 * max(sc.SET_SIZES) ** 2 < 2 ** 24
    rng = np.random.default_rng(d)
    for a in range(len(rows)):
        for b in range(len(rows)):
            s = (x[rows[a]] @ x[rows[b]].T).ravel()
            want = float(s.astype(np.float64).sum())
            assert sc.set_score_expected(x, rows[a], rows[b]) == want / s.size
            for order in (np.arange(s.size), np.arange(s.size)[::-1], rng.permutation(s.size), np.argsort(s), np.argsort(-s)):
                run = np.cumsum(s[order], dtype=np.float32)
                assert run.dtype == np.float32 and float(run[-1]) == want
            # pairwise (butterfly-like) order too
            assert float(np.sum(s.reshape(-1), dtype=np.float32)) == want
    # one element counted twice or dropped moves the mean by at least 1 / (16 * 48 * 48) unless that score is 0 ...
    assert 1.0 / (16 * 48 * 48) > 6 * sc.SET_TOL
    # ... so the cases must not be blind to it: every template pair has non-zero scores in its last (ragged) row and column
    for a in range(len(rows)):
        for b in range(len(rows)):
            s = x[rows[a]] @ x[rows[b]].T
            if d < 512:
                assert np.any(s[-1] != 0) or np.any(s[:, -1] != 0) or s.size == 1


def test_pool_exact_sums_are_fp32_exact():
    members, media_off, tmpl_off = sc.pool_exact_lists()
    rng = np.random.default_rng(9)
    x = rng.integers(-8, 9, (len(members), 65)).astype(np.float32)
    v = sc.pool_exact_sum(x, members, media_off, tmpl_off)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert np.array_equal(v * 4, np.round(v * 4))             # means over 1, 2 or 4 members of integers: quarters
    sizes = set(int(c) for c in np.diff(media_off))
    assert sizes == {1, 2, 4}
    # any fp32 evaluation order of a column's chain is exact: |partial| <= 5 media * 4 members * 8, in quarters far below 2^24
    m2, mo2, to2 = sc.pool_lists(5)
    assert sorted(set(np.diff(mo2).tolist())) == sorted(sc.POOL_MEDIA) and len(to2) == 6 and mo2[-1] == len(m2)


def test_megaface_sets_exact():
    for m in sc.MF_M:
        for n in sc.MF_N:
            P, labels, D = sc.mf_sets(m, n)
            assert P.shape == (m, sc.MF_D) and D.shape == (n, sc.MF_D) and len(labels) == m
            _assert_exact(P, D)
            _assert_exact(P, P)
