"""-m gpu: the template path (include/fte.h "Templates", verification.py, verify.py --protocol templates / template_search)
against the float64 restatement (tests/template_ref.py): media-aware pooling, set-to-set softmax score fusion with 1 x 1,
1 x 300 and 300 x 300 pairs, the NaN rules and C-ABI error codes, bitwise determinism across calls, pair orders and npairs,
and both protocols end to end, including a two-split run."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import template_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from tf_face_toolbox_amd import _lib, verification as V

SIZES = [1, 1, 300, 300, 2, 5, 17, 33, 64, 150, 3, 1, 8, 250, 16, 32, 15, 47, 4, 120]


def _synth(seed, sizes=SIZES, d=512, subjects=8):
    """templates of the given sizes over shared rows: media of 1..6 frames, some rows reused by later templates, one media of
    template 4 with weight 0.  Returns x [n, d] float32, weights [n], members, media_off, tmpl_off, template subjects."""
    rng = np.random.default_rng(seed)
    members, media_off, tmpl_off, subj = [], [0], [0], []
    n = 0
    owner = []
    for t, s in enumerate(sizes):
        sub = int(rng.integers(subjects))
        subj.append(sub)
        rows = []
        for _ in range(s):
            reuse = [r for r in range(n) if owner[r] == sub]
            if reuse and rng.random() < 0.2:
                rows.append(int(rng.choice(reuse)))
            else:
                rows.append(n)
                owner.append(sub)
                n += 1
        i = 0
        while i < s:
            k = int(rng.integers(1, 7))
            members.extend(rows[i:i + k])
            media_off.append(len(members))
            i += k
        tmpl_off.append(len(media_off) - 1)
    centers = rng.standard_normal((subjects, d))
    x = (centers[np.asarray(owner)] + 1.5 * rng.standard_normal((n, d))).astype(np.float32)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32)
    if len(sizes) > 4:
        zm = tmpl_off[4]                                        # template 4's first media: weight 0
        for r in members[media_off[zm]:media_off[zm + 1]]:
            w[r] = 0.0
    return (x, w, np.asarray(members, np.int32), np.asarray(media_off, np.int32), np.asarray(tmpl_off, np.int32),
            np.asarray(subj))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('d', [512, 100, 1100])
def test_pool_against_float64(d):
    x, w, mem, mo, to, _ = _synth(1, d=d)
    X = torch.from_numpy(x).cuda()
    for weights in (None, w):
        got = V.template_pool(X, mem, mo, to, weights).cpu().numpy()
        ref = tr.pool(x, mem, mo, to, weights)
        assert got.shape == (len(SIZES), d)
        assert np.abs(got - ref).max() <= 2e-6, (d, weights is None)
    # a template whose only media has weight 0 is a zero row; so is one with no media
    to2 = np.concatenate([to, [to[-1]]]).astype(np.int32)       # an extra, empty template
    got = V.template_pool(X, mem, mo, to2, w).cpu().numpy()
    assert np.all(got[-1] == 0)
    one = np.asarray([0, 1], np.int32)
    got = V.template_pool(X, mem[mo[to[4]]:mo[to[4] + 1]], np.asarray([0, mo[to[4] + 1] - mo[to[4]]], np.int32), one, w)
    assert np.all(got.cpu().numpy() == 0)


def test_pool_is_the_normalize_rule_bitwise():
    """single-member templates of weight 1: the pooled sum is the row itself, so the pooled row is bitwise what
    fte_l2_normalize_rows gives on it (same reduction order, same rule)"""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((50, 512)).astype(np.float32)
    X = torch.from_numpy(x).cuda()
    ar = np.arange(51, dtype=np.int32)
    got = V.template_pool(X, ar[:50], ar, ar)
    ref = torch.empty_like(X)
    _lib.call('fte_l2_normalize_rows', X, ref, None, 50, 512, _stream())
    assert torch.equal(got, ref)


BETAS = list(range(0, 41, 2))


def test_set_pair_scores_against_float64():
    x, _, mem, mo, to, _ = _synth(2)
    X = V.normalize(torch.from_numpy(x).cuda())
    xn = X.cpu().numpy()
    nt = len(SIZES)
    ta, tb = np.meshgrid(np.arange(nt), np.arange(nt), indexing='ij')
    ta, tb = ta.ravel(), tb.ravel()
    rows = [tr.template_rows(mem, mo, to, t) for t in range(nt)]
    for betas, tol in ((BETAS, 1e-5), ([0], 2e-6), ([40], 1e-5), ([0, 10, 20, 30, 40], 1e-5)):
        got = V.set_pair_scores(X, mem, mo, to, ta, tb, betas).cpu().numpy()
        ref = np.array([tr.softmax_score(xn, rows[a], rows[b], betas) for a, b in zip(ta, tb)])
        err = np.abs(got - ref)
        assert err.max() <= tol, (betas, err.max(), ta[err.argmax()], tb[err.argmax()])
    # the 1 x 1, 1 x 300 and 300 x 300 pairs on their own
    assert SIZES[0] == 1 and SIZES[2] == 300 and SIZES[3] == 300
    for a, b in ((0, 1), (0, 2), (2, 0), (2, 3), (3, 3)):
        got = float(V.set_pair_scores(X, mem, mo, to, [a], [b], BETAS).cpu().numpy()[0])
        assert abs(got - tr.softmax_score(xn, rows[a], rows[b], BETAS)) <= 1e-5, (a, b)
    got = float(V.set_pair_scores(X, mem, mo, to, [0], [1], [0]).cpu().numpy()[0])
    assert abs(got - float(xn[rows[0][0]].astype(np.float64) @ xn[rows[1][0]])) <= 2e-6


def test_set_pair_scores_bitwise_deterministic():
    x, _, mem, mo, to, _ = _synth(3)
    X = V.normalize(torch.from_numpy(x).cuda())
    rng = np.random.default_rng(5)
    nt = len(SIZES)
    ta, tb = rng.integers(0, nt, 700), rng.integers(0, nt, 700)
    ref = V.set_pair_scores(X, mem, mo, to, ta, tb).cpu().numpy()
    assert np.array_equal(V.set_pair_scores(X, mem, mo, to, ta, tb).cpu().numpy().view(np.uint32), ref.view(np.uint32))
    perm = rng.permutation(700)
    got = V.set_pair_scores(X, mem, mo, to, ta[perm], tb[perm]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref[perm].view(np.uint32))
    # through the C ABI in the listed order (no reordering by the wrapper), and with a different npairs
    betas = np.arange(0, 21, dtype=np.float32)
    dev = lambda a: torch.as_tensor(np.asarray(a, np.int32)).cuda()
    for sel in (np.arange(700), np.arange(3, 10), np.arange(699, 700)):
        out = torch.empty(len(sel), device='cuda')
        _lib.call('fte_set_pair_scores', X, X.shape[0], 512, dev(mem), len(mem), dev(mo), len(mo) - 1, dev(to), nt, dev(ta[sel]),
                  dev(tb[sel]), len(sel), betas.ctypes.data_as(ctypes.c_void_p), 21, out, _stream())
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref[sel].view(np.uint32)), len(sel)
    P = V.template_pool(X, mem, mo, to)
    assert torch.equal(P, V.template_pool(X, mem, mo, to))


def test_nan_rules_and_error_codes():
    x, w, mem, mo, to, _ = _synth(6, sizes=[3, 4, 1])
    X = V.normalize(torch.from_numpy(x).cuda())
    n = X.shape[0]
    dev = lambda a: torch.as_tensor(np.asarray(a, np.int32)).cuda()
    # pooling: a bad member row gives a NaN row, the other templates are untouched
    bad = mem.copy()
    bad[mo[to[1]]] = n
    got = V.template_pool(X, bad, mo, to).cpu().numpy()
    ref = V.template_pool(X, mem, mo, to).cpu().numpy()
    assert np.all(np.isnan(got[1])) and np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    bad[mo[to[1]]] = -1
    assert np.all(np.isnan(V.template_pool(X, bad, mo, to).cpu().numpy()[1]))
    badoff = to.copy()
    badoff[2] = len(mo) + 5                                     # a template offset past the media list
    got = V.template_pool(X, mem, mo, badoff).cpu().numpy()
    assert np.all(np.isnan(got[1])) and np.all(np.isnan(got[2])) and np.array_equal(got[0], ref[0])
    # set scores: bad template id, empty template, bad member row -> NaN for that pair only
    to_e = np.concatenate([to, [to[-1]]]).astype(np.int32)      # template 3 is empty
    s = V.set_pair_scores(X, mem, mo, to_e, [0, -1, 0, 4, 3, 1], [1, 0, 9, 0, 0, 2]).cpu().numpy()
    assert np.isfinite(s[0]) and np.isfinite(s[5]) and np.all(np.isnan(s[1:5]))
    bad = mem.copy()
    bad[mo[to[2]]] = n + 100
    s = V.set_pair_scores(X, bad, mo, to, [0, 2, 1], [1, 0, 1]).cpu().numpy()
    assert np.isfinite(s[0]) and np.isnan(s[1]) and np.isfinite(s[2])
    # C-ABI codes
    out = torch.empty(8, 512, device='cuda')
    q = lambda *a: _lib.query('fte_template_pool', *[t.data_ptr() if hasattr(t, 'data_ptr') else t for t in a])
    m_, mo_, to_ = dev(mem), dev(mo), dev(to)
    assert q(X, None, n, 512, m_, len(mem), mo_, len(mo) - 1, to_, 3, out, _stream()) == 0
    assert q(None, None, n, 512, m_, len(mem), mo_, len(mo) - 1, to_, 3, out, _stream()) == -1
    assert q(X, None, n, 512, None, len(mem), mo_, len(mo) - 1, to_, 3, out, _stream()) == -1
    assert q(X, None, n, 0, m_, len(mem), mo_, len(mo) - 1, to_, 3, out, _stream()) == -1
    assert q(X, None, n, 512, m_, 0, mo_, len(mo) - 1, to_, 3, out, _stream()) == -1
    assert q(X, None, n, 512, m_, len(mem), mo_, 0, to_, 3, out, _stream()) == -1
    assert q(X, None, n, 512, m_, len(mem), mo_, len(mo) - 1, to_, 0, out, _stream()) == -1
    assert q(X, None, 1 << 21, 512, m_, len(mem), mo_, len(mo) - 1, to_, 3, out, _stream()) == -1      # x of 4 GiB
    ps = torch.empty(2, device='cuda')
    ta, tb = dev([0, 1]), dev([1, 2])

    def qs(d=512, nbetas=2, betas=(0.0, 10.0), np_=2, xx=X, nn=n, tt=ta):
        b = (ctypes.c_float * 32)(*betas)
        return _lib.query('fte_set_pair_scores', xx.data_ptr() if xx is not None else None, nn, d, m_.data_ptr(), len(mem),
                          mo_.data_ptr(), len(mo) - 1, to_.data_ptr(), 3, tt.data_ptr() if tt is not None else None, tb.data_ptr(),
                          np_, ctypes.cast(b, ctypes.c_void_p), nbetas, ps.data_ptr(), _stream())
    assert qs() == 0
    assert qs(d=500) == -1 and qs(d=16) == -1
    assert qs(nbetas=0) == -1 and qs(nbetas=33) == -1
    assert qs(betas=(0.0, 40.5)) == -1 and qs(betas=(-0.5, 1.0)) == -1 and qs(betas=(float('nan'), 1.0)) == -1
    assert qs(betas=(0.0, 40.0)) == 0
    assert qs(np_=0) == -1 and qs(xx=None) == -1 and qs(tt=None) == -1 and qs(nn=0) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='betas'):
        V.set_pair_scores(X, mem, mo, to, [0], [1], [50])
    with pytest.raises(ValueError, match='multiple of 32'):
        V.set_pair_scores(X[:, :48].contiguous(), mem, mo, to, [0], [1])


def test_two_gib_limit_of_the_wrappers():
    big = torch.empty(1 << 20, 512, device='cuda')              # exactly 2 GiB
    with pytest.raises(ValueError, match='below 2 GiB'):
        V.template_pool(big, [0], [0, 1], [0, 1])
    with pytest.raises(ValueError, match='below 2 GiB'):
        V.set_pair_scores(big, [0], [0, 1], [0, 1], [0], [0])
    del big
    fits = torch.zeros(1000000, 512, device='cuda')             # 1M x 512 fp32 still fits
    fits[999999, 3] = 2.0
    ar = np.asarray([0, 999999], np.int32)
    P = V.template_pool(fits, ar, np.asarray([0, 1, 2], np.int32), np.asarray([0, 2], np.int32))
    assert float(P[0, 3]) == 1.0
    s = V.set_pair_scores(fits, [999999], [0, 1], [0, 1], [0], [0], [0])
    assert float(s[0]) == 4.0
    del fits
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ verify.py end to end
def _write(tmp, tag, x, meta_rows, extra_col=True):
    """feature .mat, image list and metadata CSV of one template set (row i of each is metadata row i)"""
    from scipy.io import savemat
    savemat(str(tmp / ('%s.mat' % tag)), {'wfea': x})
    with open(str(tmp / ('%s.csv' % tag)), 'w') as f:
        f.write('TEMPLATE_ID,SUBJECT_ID,FILE,MEDIA_ID,FRAME\n')
        for t, s, fn, m in meta_rows:
            f.write('%d,%d,%s,%s,0\n' % (t, s, fn, m))
    with open(str(tmp / ('%s.txt' % tag)), 'w') as f:
        for t, s, fn, m in meta_rows:
            f.write('/data/ijb/%s %d\n' % (fn, s))
    return [str(tmp / ('%s.%s' % (tag, e))) for e in ('mat', 'txt', 'csv')]


def _set(seed, n_templates, subjects, tid0=1):
    """a synthetic template set as metadata rows + features: 1..12 images per template in media of 1..4 frames"""
    rng = np.random.default_rng(seed)
    centers = np.random.default_rng(99).standard_normal((subjects, 64))
    rows, feats = [], []
    for t in range(n_templates):
        sub = int(rng.integers(subjects))
        k = int(rng.integers(1, 13))
        media = 0
        left = k
        while left:
            f = min(left, int(rng.integers(1, 5)))
            media += 1
            for j in range(f):
                rows.append((tid0 + t, sub, 'frames/%d_%d_%d.jpg' % (tid0 + t, media, j), '%d_%d' % (tid0 + t, media)))
                feats.append(centers[sub] + 4.0 * rng.standard_normal(64))
            left -= f
    return np.asarray(feats, np.float32), rows


def _verify(args, tmp):
    out = str(tmp / 'res.json')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py')] + args + ['--output_json', out], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.load(open(out)), r.stdout


def _csr(rows):
    """the grouping build_templates is documented to make, restated: templates ascending, media by first appearance"""
    tids = sorted(set(r[0] for r in rows))
    members, mo, to, subj = [], [0], [0], []
    for t in tids:
        order = []
        for i, r in enumerate(rows):
            if r[0] == t and r[3] not in order:
                order.append(r[3])
        for m in order:
            members.extend(i for i, r in enumerate(rows) if r[0] == t and r[3] == m)
            mo.append(len(members))
        to.append(len(mo) - 1)
        subj.append([r[1] for r in rows if r[0] == t][0])
    return tids, members, mo, to, subj


def _check_tar(res_rows, ref_rows, ngen):
    for row, r in zip(res_rows, ref_rows):
        assert (r is None) == (row['tar'] == 'n/a'), (row, r)
        if r is not None:
            assert abs(row['tar'] - r[0]) <= 1.01 / ngen, (row, r)


FARS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)


def test_verify_cli_templates_and_search(tmp_path):
    x, rows = _set(31, 60, 12)
    fmat, flist, fcsv = _write(tmp_path, 'set', x, rows)
    tids, mem, mo, to, subj = _csr(rows)
    nt = len(tids)
    ia, ib = np.triu_indices(nt, 1)
    with open(str(tmp_path / 'pairs.txt'), 'w') as f:
        for a, b in zip(ia, ib):
            f.write('%d %d\n' % (tids[a], tids[b]))
    genuine = np.asarray(subj)[ia] == np.asarray(subj)[ib]
    base = ['--feature_path', fmat, '--data_list_path', flist, '--template_metadata', fcsv, '--template_pairs', str(tmp_path / 'pairs.txt')]
    xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    # pool
    res, text = _verify(['--protocol', 'templates'] + base, tmp_path)
    P = tr.pool(xn, mem, mo, to)
    ref = tr.tar_at_far((P[ia] * P[ib]).sum(1), genuine, FARS)
    assert res['templates'] == nt and res['pairs'] == len(ia) and res['genuine'] == int(genuine.sum()) and res['fusion'] == 'pool'
    _check_tar(res['tar_at_far'], ref, genuine.sum())
    assert 'n/a' in text
    # softmax
    res, _ = _verify(['--protocol', 'templates', '--fusion', 'softmax', '--betas', '0:20'] + base, tmp_path)
    rws = [np.asarray(mem[mo[to[t]]:mo[to[t + 1]]]) for t in range(nt)]
    sc = np.array([tr.softmax_score(xn, rws[a], rws[b], range(21)) for a, b in zip(ia, ib)])
    _check_tar(res['tar_at_far'], tr.tar_at_far(sc, genuine, FARS), genuine.sum())
    # a list that does not match the metadata stops with the first mismatch
    bad = open(flist).read().splitlines()
    bad[5] = '/data/ijb/frames/other.jpg 0'
    (tmp_path / 'bad.txt').write_text('\n'.join(bad) + '\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py'), '--protocol', 'templates'] + base[:2] +
                       ['--data_list_path', str(tmp_path / 'bad.txt')] + base[4:], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and 'row 5' in (r.stdout + r.stderr)

    # template_search: gallery = templates of subjects 0..7, probes = another set over subjects 0..11
    gx, grows = _set(32, 30, 8, tid0=1000)
    gmat, glist, gcsv = _write(tmp_path, 'gal', gx, grows)
    res, text = _verify(['--protocol', 'template_search', '--feature_path', fmat, '--data_list_path', flist, '--template_metadata', fcsv,
                         '--gallery_metadata', gcsv, '--gallery_feature_path', gmat, '--gallery_list_path', glist], tmp_path)
    gt, gmem, gmo, gto, gsubj = _csr(grows)
    gxn = gx.astype(np.float64) / np.linalg.norm(gx.astype(np.float64), axis=1, keepdims=True)
    G = tr.pool(gxn, gmem, gmo, gto)
    cmc, tp = tr.open_set(P @ G.T, subj, gsubj, range(1, 11), (0.01, 0.1))
    assert res['probe_templates'] == nt and res['gallery_templates'] == len(gt)
    assert res['mated'] == int(np.isin(subj, gsubj).sum()) and res['non_mated'] == nt - res['mated']
    for r in range(1, 11):
        assert abs(res['cmc'][str(r)] - cmc[r]) <= 1.01 / res['mated'], r
    for row, t in zip(res['tpir_at_fpir'], tp):
        assert (t is None) == (row['tpir'] == 'n/a')
        if t is not None:
            assert abs(row['tpir'] - t) <= 1.01 / res['mated']
    assert 'rank-1' in text and 'TPIR@FPIR' in text


def test_verify_cli_two_splits(tmp_path):
    singles = []
    for sp in (1, 2):
        x, rows = _set(40 + sp, 40, 10)
        _write(tmp_path, 'split%d' % sp, x, rows)
        tids, _, _, _, _ = _csr(rows)
        with open(str(tmp_path / ('pairs%d.txt' % sp)), 'w') as f:
            for a in range(len(tids)):
                for b in range(a + 1, len(tids)):
                    f.write('%d,%d\n' % (tids[a], tids[b]))
        singles.append(_verify(['--protocol', 'templates', '--fusion', 'softmax', '--feature_path', str(tmp_path / ('split%d.mat' % sp)),
                                '--data_list_path', str(tmp_path / ('split%d.txt' % sp)), '--template_metadata',
                                str(tmp_path / ('split%d.csv' % sp)), '--template_pairs', str(tmp_path / ('pairs%d.txt' % sp))],
                               tmp_path)[0])
    res, text = _verify(['--protocol', 'templates', '--fusion', 'softmax', '--splits', '1-2',
                         '--feature_path', str(tmp_path / 'split{split}.mat'), '--data_list_path', str(tmp_path / 'split{split}.txt'),
                         '--template_metadata', str(tmp_path / 'split{split}.csv'), '--template_pairs', str(tmp_path / 'pairs{split}.txt')],
                        tmp_path)
    assert sorted(res['splits']) == ['1', '2']
    for sp, single in zip(('1', '2'), singles):
        assert res['splits'][sp]['tar_at_far'] == single['tar_at_far']
    t1 = [r['tar'] for r in singles[0]['tar_at_far']]
    t2 = [r['tar'] for r in singles[1]['tar_at_far']]
    for far, a, b in zip(FARS, t1, t2):
        v = res['summary']['TAR@FAR=%g' % far]
        if 'n/a' in (a, b):
            assert v['mean'] == 'n/a'
        else:
            assert abs(v['mean'] - (a + b) / 2) < 1e-12 and abs(v['std'] - abs(a - b) / 2) < 1e-12
    assert 'mean +- std' in text
