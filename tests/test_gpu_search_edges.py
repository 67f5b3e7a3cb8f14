"""-m gpu: the evaluation kernels of csrc/search.hip (include/fte.h "Evaluation", "Templates", "MegaFace") at the smallest shapes
that reach each branch of their code, on rows whose dot products are exact in fp32 (tests/search_cases.py; the CPU module
tests/test_search_cases_host.py proves that the expectations are unique).  Top-k lists, merged lists, histograms, pair scores
and MegaFace counts are compared bit for bit, with no allowance; every output buffer carries one extra row or element holding a
sentinel that must survive the call.  Calls go through _lib.call / _lib.query on the C ABI unless a case names a wrapper."""
import ctypes

import numpy as np
import pytest
import torch

import megaface_ref as mr
import search_cases as sc
import template_ref as tr
import verify_ref as vr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tf_face_toolbox_amd import _lib, verification as V

TOL = 2e-6                             # the fp32 allowance of test_gpu_verify.py / test_gpu_templates.py, for Gaussian rows only
SENT_F, SENT_I = -7.5, -77             # sentinels: no kernel here writes either value
_EXPECTED = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fbuf(*shape):
    return torch.full(shape, SENT_F, dtype=torch.float32, device='cuda')


def _ibuf(*shape, dtype=torch.int32):
    return torch.full(shape, SENT_I, dtype=dtype, device='cuda')


def _bits(a):
    """uint32 view of float32 values; an expected float64 goes through + 0.0 first (a kernel's sum starts at +0, never -0)"""
    a = np.asarray(a)
    if a.dtype != np.float32:
        a = (a + 0.0).astype(np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


def _q(name, *a):
    return _lib.query(name, *[t.data_ptr() if hasattr(t, 'data_ptr') else t for t in a])


def _topk_case(case):
    if case['name'] not in _EXPECTED:
        P, G = sc.topk_inputs(case)
        _EXPECTED[case['name']] = (P, G) + sc.topk_expected_of(case)
    return _EXPECTED[case['name']]


# ------------------------------------------------------------------ a. fte_l2_normalize_rows
@pytest.mark.parametrize('n,d', sc.NORMALIZE_SHAPES)
def test_normalize_rows_shapes(n, d):
    rng = np.random.default_rng(100 * n + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.01, 50, (n, 1))).astype(np.float32)
    y, norms = _fbuf(n + 1, d), _fbuf(n + 1)
    _lib.call('fte_l2_normalize_rows', _dev(x), y, norms, n, d, _stream())
    y, norms = y.cpu().numpy(), norms.cpu().numpy()
    assert np.all(y[n] == SENT_F) and norms[n] == SENT_F
    ref_n = np.linalg.norm(x.astype(np.float64), axis=1)
    assert np.abs(y[:n] - vr.normalize(x)).max() <= TOL
    assert np.abs(norms[:n] - ref_n).max() <= 1e-6 * ref_n.max()


def test_normalize_zero_row_tiny_row_alias_and_null_norms():
    n, d = 7, 65
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[2] = 0.0                                               # stays zero
    x[4] = np.float32(1e-25)                                 # the sum of squares underflows to 0: y = x / 1e-12f, norms = 0
    X = _dev(x)
    y, norms = _fbuf(n + 1, d), _fbuf(n + 1)
    _lib.call('fte_l2_normalize_rows', X, y, norms, n, d, _stream())
    yh, nh = y.cpu().numpy(), norms.cpu().numpy()
    assert np.all(yh[2] == 0) and nh[2] == 0
    assert nh[4] == 0 and np.array_equal(_bits(yh[4]), _bits(x[4] / np.float32(1e-12)))
    assert np.all(yh[n] == SENT_F) and nh[n] == SENT_F
    a = _fbuf(n + 1, d)
    a[:n] = X
    _lib.call('fte_l2_normalize_rows', a, a, None, n, d, _stream())          # aliased, norms == NULL
    assert torch.equal(a, y)                                                 # the sentinel row included
    b = _fbuf(n + 1, d)
    _lib.call('fte_l2_normalize_rows', X, b, None, n, d, _stream())          # separate, norms == NULL
    assert torch.equal(b, y)


# ------------------------------------------------------------------ b. fte_pair_scores
@pytest.mark.parametrize('npairs,d', sc.PAIR_SHAPES)
def test_pair_scores_shapes(npairs, d):
    rng = np.random.default_rng(1000 * npairs + d)
    n = 9
    x = sc.exact_rows(rng, n, d) if d >= 16 else rng.standard_normal((n, d)).astype(np.float32)
    ia, ib = rng.integers(0, n, npairs), rng.integers(0, n, npairs)
    ib[0] = ia[0]                                            # a row with itself
    out = _fbuf(npairs + 1)
    _lib.call('fte_pair_scores', _dev(x), _dev(ia.astype(np.int32)), _dev(ib.astype(np.int32)), out, n, d, npairs, _stream())
    got = out.cpu().numpy()
    assert got[npairs] == SENT_F
    ref = vr.pair_scores(x, ia, ib)
    if d >= 16:
        assert np.array_equal(_bits(got[:npairs]), _bits(ref))
        assert got[0] == 1.0
    else:
        assert np.abs(got[:npairs] - ref).max() <= TOL


def test_pair_scores_bad_index_is_nan_for_its_pair_only_and_error_codes():
    rng = np.random.default_rng(21)
    n, d, npairs = 9, 32, 12
    x = sc.exact_rows(rng, n, d)
    ia, ib = rng.integers(0, n, npairs).astype(np.int64), rng.integers(0, n, npairs).astype(np.int64)
    ia[1], ib[6], ia[9] = -1, n, 2 ** 31 - 1                 # each in the middle of a block of four pairs
    bad = np.zeros(npairs, bool)
    bad[[1, 6, 9]] = True
    X, A, B = _dev(x), _dev(ia.astype(np.int32)), _dev(ib.astype(np.int32))
    out = _fbuf(npairs + 1)
    _lib.call('fte_pair_scores', X, A, B, out, n, d, npairs, _stream())
    got = out.cpu().numpy()
    assert np.isnan(got[:npairs][bad]).all() and got[npairs] == SENT_F
    assert np.array_equal(_bits(got[:npairs][~bad]), _bits(vr.pair_scores(x, ia[~bad], ib[~bad])))
    S = _stream()
    assert _q('fte_pair_scores', X, A, B, out, n, d, npairs, S) == 0
    for args in ((None, A, B, out), (X, None, B, out), (X, A, None, out), (X, A, B, None)):
        assert _q('fte_pair_scores', *args, n, d, npairs, S) == -1
    assert _q('fte_pair_scores', X, A, B, out, 0, d, npairs, S) == -1
    assert _q('fte_pair_scores', X, A, B, out, n, 0, npairs, S) == -1
    assert _q('fte_pair_scores', X, A, B, out, n, d, 0, S) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ c. fte_topk_search
def _assert_topk(got_s, got_i, es, ei, what):
    gs, gi = got_s.cpu().numpy(), got_i.cpu().numpy()
    assert gi.dtype == np.int32 and gs.dtype == np.float32
    same_i = gi == ei.astype(np.int32)
    same_s = _bits(gs) == _bits(es)
    if not (same_i.all() and same_s.all()):
        r, t = np.argwhere(~(same_i & same_s))[0]
        raise AssertionError('%s: first difference at probe %d slot %d: got (%r, %d), expected (%r, %d); %d of %d slots differ'
                             % (what, r, t, gs[r, t], gi[r, t], es[r, t], ei[r, t], (~(same_i & same_s)).sum(), same_i.size))


@pytest.mark.parametrize('case', sc.TOPK_CASES, ids=lambda c: c['name'])
def test_topk_search_ties_slices_and_bases(case):
    P, G, es, ei = _topk_case(case)
    m, n, d, k = case['m'], case['n'], case['d'], case['k']
    p0, g0, excl = case.get('p0', 0), case.get('g0', 0), case.get('excl', 0)
    wsb = _lib.query('fte_topk_search_ws_bytes', m, n, d, k)
    S = wsb // (m * k * 8)
    # the launch this case is for: fail loudly, never test less, on a device with another slice plan
    assert wsb == S * m * k * 8 and S == case['slices'], (S, case['slices'])
    assert sc.steps_per_slice(m, n) == case['steps'] and sc.empty_slices(m, n) == case['empty']
    ws = torch.full((wsb + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    s, i = _fbuf(m + 1, k), _ibuf(m + 1, k)
    _lib.call('fte_topk_search', _dev(P), _dev(G), m, n, d, k, g0, excl, p0, s, i, ws, wsb, _stream())
    assert torch.all(s[m] == SENT_F) and torch.all(i[m] == SENT_I) and torch.all(ws[wsb:] == 0xA5)
    _assert_topk(s[:m], i[:m], es, ei, case['name'])
    if case['rows'] == 'dups':                               # more duplicates than k: the 64 smallest indices, in order
        assert np.array_equal(i[:sc.DUP_PROBES].cpu().numpy(), np.tile(sc.DUP_POS[:64], (sc.DUP_PROBES, 1)))
    if excl and k == n:
        assert torch.all(i[:m, k - 1] == -1) and torch.all(torch.isneginf(s[:m, k - 1]))


@pytest.mark.parametrize('name', ['slices64_compact', 'X_self_inside'])
def test_topk_wrapper_chunks_match_the_same_expectation(name):
    case = next(c for c in sc.TOPK_CASES if c['name'] == name)
    assert case.get('p0', 0) == 0 and case.get('g0', 0) == 0             # the wrapper searches from row 0 of both
    P, G, es, ei = _topk_case(case)
    Pd, Gd = _dev(P), _dev(G)
    for r in (case['k'], 97):
        s, i = V.topk_search(Pd, Gd, case['k'], exclude_self=bool(case.get('excl', 0)), chunk_rows=r)
        _assert_topk(s, i, es, ei, '%s chunk_rows=%d' % (name, r))


# ------------------------------------------------------------------ d. fte_topk_merge
@pytest.mark.parametrize('lists', sc.MERGE_LISTS)
def test_topk_merge_direct(lists):
    rng = np.random.default_rng(300 + lists)
    for m in sc.MERGE_M:
        for k in sc.MERGE_K:
            in_s, in_i = sc.merge_inputs(rng, m, lists, k)
            es, ei = sc.merge_expected(in_s, in_i, k)
            s, i = _fbuf(m + 1, k), _ibuf(m + 1, k)
            _lib.call('fte_topk_merge', _dev(in_s), _dev(in_i), m, lists, k, s, i, _stream())
            assert torch.all(s[m] == SENT_F) and torch.all(i[m] == SENT_I)
            _assert_topk(s[:m], i[:m], es, ei, 'merge m=%d lists=%d k=%d' % (m, lists, k))
            if m > 1:                                        # the row whose lists are all empty
                assert torch.all(i[m - 1] == -1) and torch.all(torch.isneginf(s[m - 1]))


def test_topk_merge_error_codes():
    in_s = torch.zeros(2, 64, 64, device='cuda')
    in_i = torch.zeros(2, 64, 64, dtype=torch.int32, device='cuda')
    s, i = _fbuf(3, 64), _ibuf(3, 64)
    S = _stream()
    assert _q('fte_topk_merge', in_s, in_i, 2, 64, 64, s, i, S) == 0
    assert _q('fte_topk_merge', in_s, in_i, 2, 1, 1, s, i, S) == 0
    for lists in (0, 65):
        assert _q('fte_topk_merge', in_s, in_i, 2, lists, 7, s, i, S) == -1
    for k in (0, 65):
        assert _q('fte_topk_merge', in_s, in_i, 2, 3, k, s, i, S) == -1
    assert _q('fte_topk_merge', in_s, in_i, 0, 3, 7, s, i, S) == -1
    for args in ((None, in_i, s, i), (in_s, None, s, i), (in_s, in_i, None, i), (in_s, in_i, s, None)):
        assert _q('fte_topk_merge', args[0], args[1], 2, 3, 7, args[2], args[3], S) == -1
    torch.cuda.synchronize()
    assert torch.all(s[2] == SENT_F) and torch.all(i[2] == SENT_I)


# ------------------------------------------------------------------ e. fte_score_histograms
def _hist(A, la, B, lb, same, nbins, calls=1, fill=None):
    """host (genuine, impostor) int64 [nbins] after `calls` calls into buffers pre-filled with `fill` ([nbins], default 0);
    the buffers' extra element keeps its sentinel"""
    bufs = []
    for _ in range(2):
        b = _ibuf(nbins + 1, dtype=torch.int64)
        b[:nbins] = 0 if fill is None else _dev(fill)
        bufs.append(b)
    Ad, Bd, lad, lbd = _dev(A), _dev(B), _dev(np.asarray(la, np.int32)), _dev(np.asarray(lb, np.int32))
    for _ in range(calls):
        _lib.call('fte_score_histograms', Ad, lad, len(A), Bd, lbd, len(B), A.shape[1], same, nbins, bufs[0], bufs[1], _stream())
    hg, hi = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    assert hg[nbins] == SENT_I and hi[nbins] == SENT_I
    return hg[:nbins], hi[:nbins]


def _assert_hist(got, want, what):
    for g, w, kind in zip(got, want, ('genuine', 'impostor')):
        assert np.array_equal(g.astype(np.uint64), w), (what, kind, np.nonzero(g.astype(np.uint64) != w)[0][:8])


@pytest.mark.parametrize('nbins', sc.HIST_NBINS)
def test_histograms_triangle_exact(nbins):
    x, lab = sc.hist_set()
    for n in sc.HIST_SAME_N:
        want = sc.hist_expected(x[:n], lab[:n], x[:n], lab[:n], 1, nbins)
        assert int(want[0].sum() + want[1].sum()) == n * (n - 1) // 2
        _assert_hist(_hist(x[:n], lab[:n], x[:n], lab[:n], 1, nbins), want, 'same n=%d' % n)


@pytest.mark.parametrize('nbins', sc.HIST_NBINS)
def test_histograms_rectangle_exact(nbins):
    a, la = sc.hist_set()
    b, lb = sc.hist_set(seed=sc.HIST_SEED + 3)
    for na, nb in sc.HIST_RECT:
        want = sc.hist_expected(a[:na], la[:na], b[:nb], lb[:nb], 0, nbins)
        assert int(want[0].sum() + want[1].sum()) == na * nb
        _assert_hist(_hist(a[:na], la[:na], b[:nb], lb[:nb], 0, nbins), want, 'rect %d x %d' % (na, nb))


@pytest.mark.parametrize('nbins', sc.HIST_NBINS)
def test_histograms_bin_clamps(nbins):
    x, lab = sc.hist_dup_set()                               # s == 1.0f: the last bin, of both histograms
    want = sc.hist_expected(x, lab, x, lab, 1, nbins)
    assert want[0][-1] > 0 and want[1][-1] > 0
    _assert_hist(_hist(x, lab, x, lab, 1, nbins), want, 'duplicated rows')
    x2, l2 = sc.hist_set(97, 32, scale=0.5, seed=57)         # norm-2 rows: scores in [-4, 4], clamped to the first and last bin
    for same in (1, 0):
        want = sc.hist_expected(x2, l2, x2, l2, same, nbins)
        assert want[0][0] + want[1][0] > 10 and want[0][-1] + want[1][-1] > 10
        _assert_hist(_hist(x2, l2, x2, l2, same, nbins), want, 'norm-2 rows same=%d' % same)


def test_histograms_accumulate_and_wrapper_chunks():
    x, lab = sc.hist_set()
    nbins = 256
    hg, hi = sc.hist_expected(x, lab, x, lab, 1, nbins)
    fill = (np.arange(nbins) % 5 + 1).astype(np.int64)
    got = _hist(x, lab, x, lab, 1, nbins, calls=2, fill=fill)
    _assert_hist(got, (fill.astype(np.uint64) + 2 * hg, fill.astype(np.uint64) + 2 * hi), 'pattern + 2 * counts')
    X = _dev(x)
    for r in sc.HIST_CHUNK_ROWS:
        _assert_hist(V.score_histograms(X, lab, nbins, chunk_rows=r), (hg, hi), 'chunk_rows=%d' % r)


# ------------------------------------------------------------------ f. fte_template_pool
def _pool(x, w, members, media_off, tmpl_off):
    nt, d = len(tmpl_off) - 1, x.shape[1]
    out = _fbuf(nt + 1, d)
    _lib.call('fte_template_pool', _dev(x), None if w is None else _dev(w), len(x), d, _dev(members), len(members), _dev(media_off),
              len(media_off) - 1, _dev(tmpl_off), nt, out, _stream())
    assert torch.all(out[nt] == SENT_F)
    return out[:nt]


@pytest.mark.parametrize('d', sc.POOL_D)
def test_template_pool_against_float64(d):
    for nt in sc.POOL_NT:
        members, media_off, tmpl_off = sc.pool_lists(nt)
        rng = np.random.default_rng(10 * d + nt)
        x = rng.standard_normal((len(members), d)).astype(np.float32)
        w = rng.uniform(0.5, 2.0, len(members)).astype(np.float32)
        for weights in (None, w):
            got = _pool(x, weights, members, media_off, tmpl_off).cpu().numpy()
            assert np.abs(got - tr.pool(x, members, media_off, tmpl_off, weights)).max() <= TOL, (d, nt, weights is None)


def _normalize_dev(v):
    n, d = v.shape
    y = _fbuf(n, d)
    _lib.call('fte_l2_normalize_rows', _dev(v), y, None, n, d, _stream())
    return y


@pytest.mark.parametrize('d', sc.POOL_BITWISE_D)
def test_template_pool_is_the_normalize_rule_bitwise(d):
    rng = np.random.default_rng(40 + d)
    x = rng.standard_normal((7, d)).astype(np.float32)       # single-member templates of weight 1: the pooled sum is the row
    ar = np.arange(8, dtype=np.int32)
    assert torch.equal(_pool(x, None, ar[:7], ar, ar), _normalize_dev(x))
    members, media_off, tmpl_off = sc.pool_exact_lists()     # media of 1, 2 or 4 small-integer rows: the pooled sum is exact
    xi = rng.integers(-8, 9, (len(members), d)).astype(np.float32)
    v = sc.pool_exact_sum(xi, members, media_off, tmpl_off)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    assert torch.equal(_pool(xi, None, members, media_off, tmpl_off), _normalize_dev(v32))


# ------------------------------------------------------------------ g. fte_set_pair_scores
def _set_scores(x, lists, ta, tb, betas):
    members, media_off, tmpl_off, _ = lists
    npairs = len(ta)
    b = np.asarray(betas, np.float32)
    out = _fbuf(npairs + 1)
    _lib.call('fte_set_pair_scores', _dev(x), len(x), x.shape[1], _dev(members), len(members), _dev(media_off), len(media_off) - 1,
              _dev(tmpl_off), len(tmpl_off) - 1, _dev(np.asarray(ta, np.int32)), _dev(np.asarray(tb, np.int32)), npairs,
              b.ctypes.data_as(ctypes.c_void_p), len(b), out, _stream())
    got = out.cpu().numpy()
    assert got[npairs] == SENT_F
    return got[:npairs]


@pytest.mark.parametrize('d', sc.SET_D)
def test_set_pair_scores_ragged_tiles_exact_mean(d):
    x = sc.set_rows(d)
    lists = sc.set_lists()
    rows = lists[3]
    nt = len(rows)
    ta, tb = [a.ravel() for a in np.meshgrid(np.arange(nt), np.arange(nt), indexing='ij')]
    perm = np.random.default_rng(d).permutation(nt * nt)
    ta, tb = ta[perm], tb[perm]                              # all 64 ordered pairs, shuffled
    want = np.array([sc.set_score_expected(x, rows[a], rows[b]) for a, b in zip(ta, tb)])
    for npairs in sc.SET_NPAIRS:
        got = _set_scores(x, lists, ta[:npairs], tb[:npairs], [0.0])
        err = np.abs(got.astype(np.float64) - want[:npairs])
        w = err.argmax()
        assert err.max() <= sc.SET_TOL, (npairs, err.max(), sc.SET_SIZES[ta[w]], sc.SET_SIZES[tb[w]])
    if d <= 64:
        got = _set_scores(x, lists, ta, tb, sc.SET_BETAS)
        ref = np.array([tr.softmax_score(x, rows[a], rows[b], sc.SET_BETAS) for a, b in zip(ta, tb)])
        assert np.abs(got - ref).max() <= 1e-5


# ------------------------------------------------------------------ h. MegaFace
@pytest.mark.parametrize('npairs', sc.MF_NPAIRS)
def test_megaface_pair_scores_wave_edges(npairs):
    rng = np.random.default_rng(500 + npairs)
    m, n, d = 9, 11, sc.MF_D
    P, R = sc.exact_rows(rng, m, d), sc.exact_rows(rng, n, d)
    ip, ig = rng.integers(0, m, npairs), rng.integers(0, n, npairs)
    out = _fbuf(npairs + 1)
    _lib.call('fte_megaface_pair_scores', _dev(P), m, _dev(R), n, d, _dev(ip.astype(np.int32)), _dev(ig.astype(np.int32)), npairs, out,
              _stream())
    got = out.cpu().numpy()
    ref = (P[ip].astype(np.float64) * R[ig]).sum(1)
    assert got[npairs] == SENT_F and np.array_equal(_bits(got[:npairs]), _bits(ref))
    bad = npairs // 2                                        # a bad index gives NaN for its pair only
    for which, val in ((ip, m), (ig, -1)):
        a, b = ip.copy(), ig.copy()
        (a if which is ip else b)[bad] = val
        out = _fbuf(npairs + 1)
        _lib.call('fte_megaface_pair_scores', _dev(P), m, _dev(R), n, d, _dev(a.astype(np.int32)), _dev(b.astype(np.int32)), npairs,
                  out, _stream())
        got = out.cpu().numpy()
        keep = np.arange(npairs) != bad
        assert np.isnan(got[bad]) and got[npairs] == SENT_F
        assert np.array_equal(_bits(got[:npairs][keep]), _bits(ref[keep]))


@pytest.mark.parametrize('m', sc.MF_M)
def test_megaface_scan_tile_edges(m):
    for n in sc.MF_N:
        P, labels, D = sc.mf_sets(m, n)
        Pd, Dd = _dev(P), _dev(D)
        ip, ig, off, _ = V.megaface_pairs(labels)
        rp, rg = mr.pairs(labels)
        assert ip.tolist() == rp.tolist() and ig.tolist() == rg.tolist()
        sg = V.megaface_pair_scores(Pd, ip, ig).cpu().numpy() if len(ip) else np.zeros(0, np.float32)
        assert np.array_equal(_bits(sg), _bits((P[ip].astype(np.float64) * P[ig]).sum(1)))
        thr, perm = V.megaface_thresholds(sg, off)
        counts, hist = V.megaface_scan(Pd, Dd, [n], off, thr, 256)
        rank = np.empty((1, len(ip)), np.int64)
        rank[:, perm] = counts.astype(np.int64) + 1
        assert np.array_equal(rank, mr.ranks(P, D, ip, ig, [n])), (m, n)
        assert np.array_equal(hist[0], mr.impostor_hist(P, D, n, 256)), (m, n)
        assert int(hist[0].sum()) == m * n
