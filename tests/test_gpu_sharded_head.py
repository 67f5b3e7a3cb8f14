"""-m gpu: the sharded margin head (include/fte.h fte_margin_shard_stats / fte_margin_shard_fwd_bwd) in ONE process -- a problem
[N, C] is cut into R shards by class, the statistics run per shard, are stacked in rank order and the gradient kernel runs per shard.
The shards side by side are held against fte_margin_softmax_fwd_bwd on the whole problem and against the float64 restatements
(tests/margin_ref.py through test_gpu_margin's own comparison, tests/sharded_head_ref.py per shard), bounds 2e-5 as there."""
import numpy as np
import pytest
import torch

import margin_ref as mr
import sharded_head_ref as shr
import test_gpu_margin as tgm

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from util_gpu import dev, host, check_maxabs, check_rell2, call, stream
    from tf_face_toolbox_amd import _lib, heads
    from tf_face_toolbox_amd.loss import additive_margin_loss, sharded_margin_loss

ARC, COS = tgm.ARC, tgm.COS
SENTINEL = 7.0
# (N, C, R): shards of 4 / 4 / 2 classes; Cs = 251 (boundaries inside a 16-byte chunk, ld > c); a one-column tail behind 64 whole
# chunks; Cs = 2 with a last shard of one class (R = 8 over these 9 classes is the host's refusal); more rows than one block
CASES = [(7, 10, 3), (8, 1001, 4), (5, 513, 2), (4, 9, 5), (130, 640, 2)]


def _ld(c, layout):
    """'pad': c rounded up to 128, the nets' layout (vector path); 'odd': the next odd width (ld % 4 != 0: scalar path)"""
    return (c + 127) // 128 * 128 if layout == 'pad' else c | 1


def _problem(N, C, R, seed):
    """test_gpu_margin's problem with labels on the first and the last shard, on the last column of shard 0 and the first of shard 1"""
    s, xn, wn, labels = tgm._raw(N, C, seed)
    (lo0, hi0), (lo1, _) = shr.shard_ranges(C, R)[:2]
    labels[1], labels[2] = hi0 - 1, lo1
    return s, xn, wn, labels


def _cut(s, wn, C, R, layout):
    """[(lo, c, ld, s_r [N, ld], wn_r [ld])]: the columns of every shard, zero padded, in buffers of their own"""
    out = []
    for lo, hi in shr.shard_ranges(C, R):
        c = hi - lo
        ld = _ld(c, layout)
        sr = torch.zeros(s.shape[0], ld, device='cuda')
        sr[:, :c] = s[:, lo:hi]
        wr = torch.zeros(ld, device='cuda')
        wr[:c] = wn[lo:hi]
        out.append((lo, c, ld, sr, wr))
    return out


def _stats(shards, xn, labels, C, S, m, m3):
    N = xn.shape[0]
    all_stats = torch.full((len(shards), 3, N), SENTINEL, device='cuda')
    for r, (lo, c, ld, sr, wr) in enumerate(shards):
        call('fte_margin_shard_stats', sr, xn, wr, labels, lo, C, S, m, m3, all_stats[r], N, c, ld, stream())
    torch.cuda.synchronize()
    return all_stats


def _grads(shards, xn, labels, C, S, m, m3, all_stats, gs, with_f=True):
    """[(f, loss_rows, G, rowcoef_part)] per shard"""
    N, out = xn.shape[0], []
    for lo, c, ld, sr, wr in shards:
        f = torch.full((N, ld), SENTINEL, device='cuda') if with_f else None
        G = torch.full((N, ld), SENTINEL, device='cuda')
        rows, rc = torch.full((N,), SENTINEL, device='cuda'), torch.full((N,), SENTINEL, device='cuda')
        call('fte_margin_shard_fwd_bwd', sr, xn, wr, labels, lo, C, S, m, m3, all_stats, len(shards), f, rows, G, rc, N, c, ld, gs, stream())
        out.append((f, rows, G, rc))
    torch.cuda.synchronize()
    return out


def _side_by_side(shards, got, like):
    """the shards' f / G blocks in the whole problem's [N, ldp] layout, the common loss rows and the sum of the rowcoef shares"""
    f, G = torch.zeros_like(like), torch.zeros_like(like)
    for (lo, c, ld, _, _), (fr, _, Gr, _) in zip(shards, got):
        G[:, lo:lo + c] = Gr[:, :c]
        assert (Gr[:, c:] == 0).all(), 'G pads of the shard at %d' % lo
        if fr is not None:
            f[:, lo:lo + c] = fr[:, :c]
            assert (fr[:, c:] == 0).all(), 'f pads of the shard at %d' % lo
    rc = torch.tensor(sum(host(g[3]) for g in got))
    return (f if got[0][0] is not None else None), got[0][1], G, rc


def _rowcoef_mag(s, xn, wn, labels, c, S, m, m3, gs):
    """the sum of the magnitudes of rowcoef's terms, as test_gpu_margin._check_head judges its error"""
    sh, xv = host(s), np.maximum(host(xn), 1e-12)
    idx, y = np.arange(sh.shape[0]), np.clip(host(labels).astype(int), 0, c - 1)
    cos = np.clip(sh[:, :c] / (xv[:, None] * host(wn)[None, :c]), -1, 1)
    t, tp = mr.target(cos[idx, y], m, m3)
    z = S * cos
    z[idx, y] = S * t
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    wgt = p.copy()
    wgt[idx, y] = (p[idx, y] + 1) * tp
    return abs(gs) * S * (wgt * np.abs(cos)).sum(1) / xv ** 2


def _check(s, xn, wn, labels, C, R, preset, layout, what, gs=None):
    """the three checks of the module docstring on one problem; -> the per-shard outputs"""
    S, m, m3 = preset
    N = s.shape[0]
    gs = 1.0 / N if gs is None else gs
    shards = _cut(s, wn, C, R, layout)
    all_stats = _stats(shards, xn, labels, C, S, m, m3)
    got = _grads(shards, xn, labels, C, S, m, m3, all_stats, gs)
    lab = host(labels).astype(int)
    # 1. the loss of a row is the same bits on every shard
    for g in got[1:]:
        assert torch.equal(g[1], got[0][1]) or (torch.isnan(g[1]) == torch.isnan(got[0][1])).all() and \
            torch.equal(torch.nan_to_num(g[1]), torch.nan_to_num(got[0][1])), what + ': loss_rows differ between shards'
    # per shard against the sharded restatement: the statistics and the gradient.  The restatement merges ITS OWN float64 statistics:
    # fed the kernel's fp32 ones, its p = exp(z - M) / Z would pair an exact z with a rounded Z, an error the kernel does not have
    # (there the rounding of the row's largest logit enters z and Z alike and cancels)
    ref_stats = np.stack([shr.stats_ref(host(sr), host(xn), host(wr), lab, lo, C, S, m, m3, c) for lo, c, ld, sr, wr in shards])
    for r, ((lo, c, ld, sr, wr), (f, rows, G, rc)) in enumerate(zip(shards, got)):
        ref = ref_stats[r]
        ok = np.isfinite(ref[0])
        st = host(all_stats[r])
        assert np.isnan(st[:, ~ok]).all(), what
        assert np.all(np.abs(st[0, ok] - ref[0, ok]) <= 2e-5 * S), (what, r, 'max')
        # the sum is held through the shard's logsumexp, by the bound of the dense loss: the sum alone moves by exp(d) when two
        # near-equal logits swap the role of the maximum d apart, the logsumexp does not
        lse, lse_ref = st[0, ok] + np.log(st[1, ok]), ref[0, ok] + np.log(ref[1, ok])
        assert np.all(st[1, ok] >= 1) and np.all(np.abs(lse - lse_ref) <= 2e-5 * np.maximum(1.0, np.abs(lse_ref))), (what, r, 'sum of exp')
        assert np.all(np.abs(st[2, ok] - ref[2, ok]) <= 2e-5 * S), (what, r, 'target logit')
        assert np.all(st[2, ok][~((lab[ok] >= lo) & (lab[ok] < lo + c))] == 0), (what, r, 'target logit of a row another shard owns')
        fr, lr, Gr, rcr = shr.fwd_bwd_ref(host(sr), host(xn), host(wr), lab, lo, C, S, m, m3, ref_stats, gs, c)
        check_maxabs(host(f)[ok], fr[ok], what='%s shard %d f' % (what, r))      # (G is judged below, on the whole row: its bound is the row's)
        assert np.all(np.abs(host(rows)[ok] - lr[ok]) <= 2e-5 * np.maximum(1.0, np.abs(lr[ok]))), (what, r, 'loss')
    whole = _side_by_side(shards, got, s)
    # 2. the shards side by side against the float64 restatement of the WHOLE problem, by test_gpu_margin's comparison
    tgm._check_head(whole, s, xn, wn, labels, C, S, m, m3, gs, what + ' (restatement)')
    # 3. ... and against the dense kernel on the whole problem
    fd, rowsd, Gd, rcd = tgm._kernel(s, xn, wn, labels, C, S, m, m3, gs)
    ok = np.isfinite(host(rowsd))
    assert (np.isfinite(host(whole[1])) == ok).all(), what
    check_maxabs(host(whole[2])[ok], host(Gd)[ok], what=what + ' G against the dense kernel')
    check_rell2(host(whole[2])[ok], host(Gd)[ok], what=what + ' G against the dense kernel')
    check_maxabs(host(whole[0])[ok], host(fd)[ok], what=what + ' f against the dense kernel')
    ld_, lg = host(rowsd)[ok], host(whole[1])[ok]
    assert np.all(np.abs(lg - ld_) <= 2e-5 * np.maximum(1.0, np.abs(ld_))), (what, 'loss against the dense kernel', np.abs(lg - ld_).max())
    mag = _rowcoef_mag(s, xn, wn, labels, C, S, m, m3, gs)
    assert np.all(np.abs(host(whole[3])[ok] - host(rcd)[ok]) <= 2e-5 * mag[ok]), (what, 'rowcoef against the dense kernel')
    return shards, all_stats, got


@pytest.mark.parametrize('layout', ['pad', 'odd'])
@pytest.mark.parametrize('preset', [ARC, COS], ids=['arcface', 'cosface'])
@pytest.mark.parametrize('N,C,R', CASES)
def test_shards_against_the_dense_kernel_and_the_restatement(N, C, R, preset, layout):
    s, xn, wn, labels = _problem(N, C, R, seed=N * 7 + C)
    _check(s, xn, wn, labels, C, R, preset, layout, 'N=%d C=%d R=%d %s' % (N, C, R, layout))


def test_a_split_with_an_empty_rank_is_refused_on_the_host():
    """(N, C, R) = (4, 9, 8): Cs = 2, ranks 5..7 would own nothing"""
    for r in range(8):
        with pytest.raises(ValueError, match='without a class'):
            heads.shard_range(9, 8, r)
    assert [heads.shard_range(9, 5, r) for r in range(5)] == shr.shard_ranges(9, 5) and shr.shard_ranges(9, 5)[-1] == (8, 9)


@pytest.mark.parametrize('layout', ['pad', 'odd'])
def test_fallback_branch_is_taken(layout):
    """every target cosine below cos(pi - m), as test_gpu_margin.test_fallback_branch_is_taken constructs it"""
    N, C, R = 8, 1001, 4
    s, xn, wn, labels = _problem(N, C, R, seed=5)
    sh = host(s)
    rows, y = np.arange(N), host(labels).astype(int)
    den = host(xn) * host(wn)[y]
    sh[rows, y] = -0.99 * den
    s = dev(sh)
    assert (host(s)[rows, y] / den < np.cos(np.pi - ARC[1])).all()
    _check(s, xn, wn, labels, C, R, ARC, layout, 'fallback ' + layout)


@pytest.mark.parametrize('preset', [ARC, COS], ids=['arcface', 'cosface'])
def test_shard_maxima_more_than_88_apart(preset):
    """S = 64, cosines near -1 on one shard and one near +1 on the other: expf(m_r - M) underflows to 0 for the low shard.  Row 0's
    label sits on the low shard, the last row's on the high one.  Loss and G stay finite and within bound."""
    N, C, R = 4, 256, 2
    s, xn, wn, labels = _problem(N, C, R, seed=23)
    sh, x_, w_ = host(s), host(xn), host(wn)
    sh[0, :128] = -0.95 * x_[0] * w_[:128]                      # label 0: shard 0 holds only low logits ...
    sh[0, 200] = 0.95 * x_[0] * w_[200]                         # ... and shard 1 the row's maximum
    sh[-1, 128:C] = -0.95 * x_[-1] * w_[128:C]                  # label C - 1 on shard 1, the maximum on shard 0
    sh[-1, 5] = 0.95 * x_[-1] * w_[5]
    s = dev(sh)
    shards, all_stats, got = _check(s, xn, wn, labels, C, R, preset, 'pad', 'maxima apart')
    st = host(all_stats)
    for i, low in ((0, 0), (N - 1, 1)):
        gap = st[1 - low, 0, i] - st[low, 0, i]
        assert gap > 88, (i, gap)
        assert np.exp(np.float32(-gap), dtype=np.float32) == 0
    for f, rows, G, rc in got:
        assert torch.isfinite(rows).all() and torch.isfinite(G).all() and torch.isfinite(rc).all()


@pytest.mark.parametrize('layout', ['pad', 'odd'])
def test_out_of_range_label_gives_a_nan_row_on_every_shard(layout):
    N, C, R = 8, 1001, 4
    s, xn, wn, labels = _problem(N, C, R, seed=11)
    S, m, m3 = ARC
    shards = _cut(s, wn, C, R, layout)
    clean_stats = _stats(shards, xn, labels, C, S, m, m3)
    clean = _grads(shards, xn, labels, C, S, m, m3, clean_stats, 1.0 / N)
    bad = labels.clone()
    bad[3], bad[5] = C, -1
    all_stats = _stats(shards, xn, bad, C, S, m, m3)
    got = _grads(shards, xn, bad, C, S, m, m3, all_stats, 1.0 / N)
    good = [0, 1, 2, 4, 6, 7]
    assert torch.isnan(all_stats[:, :, [3, 5]]).all() and torch.equal(all_stats[:, :, good], clean_stats[:, :, good])
    for (lo, c, ld, _, _), (f, rows, G, rc), (f0, rows0, G0, rc0) in zip(shards, got, clean):
        for i in (3, 5):
            assert np.isnan(float(rows[i])) and np.isnan(float(rc[i]))
            assert torch.isnan(G[i, :c]).all() and torch.isnan(f[i, :c]).all()
        assert (G[:, c:] == 0).all() and (f[:, c:] == 0).all()
        for a, b in ((f, f0), (rows, rows0), (G, G0), (rc, rc0)):
            assert torch.equal(a[good], b[good]), 'the other rows are bitwise unaffected'


def test_a_nan_statistic_gives_a_nan_row():
    N, C, R = 8, 1001, 4
    s, xn, wn, labels = _problem(N, C, R, seed=12)
    S, m, m3 = COS
    shards = _cut(s, wn, C, R, 'pad')
    all_stats = _stats(shards, xn, labels, C, S, m, m3)
    clean = _grads(shards, xn, labels, C, S, m, m3, all_stats, 1.0 / N)
    for which, (r, k, i) in enumerate(((2, 0, 1), (0, 1, 4), (3, 2, 6))):      # a NaN max, sum and target logit, each on another shard
        hurt = all_stats.clone()
        hurt[r, k, i] = float('nan')
        got = _grads(shards, xn, labels, C, S, m, m3, hurt, 1.0 / N)
        good = [j for j in range(N) if j != i]
        for (lo, c, ld, _, _), (f, rows, G, rc), (f0, rows0, G0, rc0) in zip(shards, got, clean):
            assert np.isnan(float(rows[i])) and np.isnan(float(rc[i])) and torch.isnan(G[i, :c]).all() and torch.isnan(f[i, :c]).all()
            assert (G[:, c:] == 0).all() and (f[:, c:] == 0).all()
            for a, b in ((f, f0), (rows, rows0), (G, G0), (rc, rc0)):
                assert torch.equal(a[good], b[good]), which


@pytest.mark.parametrize('layout', ['pad', 'odd'])
def test_f_null_gives_the_same_G_and_repeats_bit_for_bit(layout):
    N, C, R = 8, 1001, 4
    s, xn, wn, labels = _problem(N, C, R, seed=13)
    S, m, m3 = ARC
    shards = _cut(s, wn, C, R, layout)
    st1, st2 = _stats(shards, xn, labels, C, S, m, m3), _stats(shards, xn, labels, C, S, m, m3)
    assert torch.equal(st1, st2)
    a = _grads(shards, xn, labels, C, S, m, m3, st1, 1.0 / N, with_f=True)
    b = _grads(shards, xn, labels, C, S, m, m3, st1, 1.0 / N, with_f=False)
    c2 = _grads(shards, xn, labels, C, S, m, m3, st1, 1.0 / N, with_f=False)
    a2 = _grads(shards, xn, labels, C, S, m, m3, st1, 1.0 / N, with_f=True)
    for r in range(R):
        assert torch.equal(a[r][0], a2[r][0])
        for i in (1, 2, 3):
            assert torch.equal(a[r][i], b[r][i]) and torch.equal(b[r][i], c2[r][i])


def test_invalid_arguments_launch_nothing():
    N, C, R = 4, 10, 3
    s, xn, wn, labels = _problem(N, C, R, seed=1)
    lo, c, ld, sr, wr = _cut(s, wn, C, R, 'pad')[1]            # classes 4..7
    stats = torch.full((3, N), SENTINEL, device='cuda')
    all_stats = torch.zeros(R, 3, N, device='cuda')
    f, G = torch.full((N, ld), SENTINEL, device='cuda'), torch.full((N, ld), SENTINEL, device='cuda')
    rows, rc = torch.full((N,), SENTINEL, device='cuda'), torch.full((N,), SENTINEL, device='cuda')
    # (scale, m, class_lo, num_classes, n, c, ld, R)
    good = (64.0, 0.5, lo, C, N, c, ld, R)
    cases = [(0.0,) + good[1:], (float('nan'),) + good[1:], (64.0, -0.1) + good[2:], (64.0, float('nan')) + good[2:],
             good[:2] + (-1,) + good[3:], good[:2] + (C - c + 1,) + good[3:], good[:3] + (lo + c - 1,) + good[4:],
             good[:2] + (2 ** 31 - 2,) + good[3:], good[:4] + (0,) + good[5:], good[:5] + (0,) + good[6:], good[:6] + (c - 1,) + good[7:]]
    for S, m, lo_, C_, n_, c_, ld_, R_ in cases:
        with pytest.raises(_lib.FteError):
            call('fte_margin_shard_stats', sr, xn, wr, labels, lo_, C_, S, m, 0.0, stats, n_, c_, ld_, stream())
        with pytest.raises(_lib.FteError):
            call('fte_margin_shard_fwd_bwd', sr, xn, wr, labels, lo_, C_, S, m, 0.0, all_stats, R_, f, rows, G, rc, n_, c_, ld_, 0.25, stream())
    for R_ in (0, -1):
        with pytest.raises(_lib.FteError):
            call('fte_margin_shard_fwd_bwd', sr, xn, wr, labels, lo, C, 64.0, 0.5, 0.0, all_stats, R_, f, rows, G, rc, N, c, ld, 0.25, stream())
    ptrs = [sr, xn, wr, labels]
    for k in range(4):                                          # a null input, a null output
        p = list(ptrs)
        p[k] = None
        with pytest.raises(_lib.FteError):
            call('fte_margin_shard_stats', p[0], p[1], p[2], p[3], lo, C, 64.0, 0.5, 0.0, stats, N, c, ld, stream())
        with pytest.raises(_lib.FteError):
            call('fte_margin_shard_fwd_bwd', p[0], p[1], p[2], p[3], lo, C, 64.0, 0.5, 0.0, all_stats, R, f, rows, G, rc, N, c, ld, 0.25, stream())
    with pytest.raises(_lib.FteError):
        call('fte_margin_shard_stats', sr, xn, wr, labels, lo, C, 64.0, 0.5, 0.0, None, N, c, ld, stream())
    for out in ((None, rows, G, rc), (all_stats, None, G, rc), (all_stats, rows, None, rc), (all_stats, rows, G, None)):
        with pytest.raises(_lib.FteError):
            call('fte_margin_shard_fwd_bwd', sr, xn, wr, labels, lo, C, 64.0, 0.5, 0.0, out[0], R, f, out[1], out[2], out[3], N, c, ld, 0.25, stream())
    torch.cuda.synchronize()
    for t in (stats, f, G, rows, rc):
        assert (t == SENTINEL).all(), 'a refused call wrote to an output'
    # ... and the same arguments, valid, do launch
    call('fte_margin_shard_stats', sr, xn, wr, labels, lo, C, 64.0, 0.5, 0.0, stats, N, c, ld, stream())
    torch.cuda.synchronize()
    assert (stats != SENTINEL).any()


class _OneRank(object):
    """the collective layer of sharded_margin_loss for a world of one rank"""

    def world_size(self):
        return 1

    def rank(self):
        return 0

    def all_gather(self, out, t):
        out.view(-1).copy_(t.reshape(-1))

    def reduce_scatter_sum(self, out, inp):
        out.copy_(inp)


@pytest.mark.parametrize('preset', [ARC, COS], ids=['arcface', 'cosface'])
def test_public_loss_function_on_one_rank(preset):
    """sharded_margin_loss over a world of one rank is the dense head: against the restatement by test_gpu_margin's bounds, and
    against additive_margin_loss"""
    rng = np.random.default_rng(17)
    n, c, ld = 64, 1000, 1024
    W = np.zeros((tgm.D, ld), np.float32)
    W[:, :c] = rng.standard_normal((tgm.D, c))
    y = rng.integers(0, c, n)
    x = tgm._features(rng, W, y, n)
    loss, dx, dW = sharded_margin_loss(dev(x), dev(W), dev(y, torch.int32), 0, c, _OneRank(), *preset)
    dense = additive_margin_loss(dev(x), dev(W), dev(y, torch.int32), *preset, num_classes=c)
    torch.cuda.synchronize()
    lr, _, dxr, dWr = mr.head_fwd_bwd(x.astype(np.float64), W[:, :c].astype(np.float64), y, *preset)
    assert abs(float(loss) - lr) <= 2e-5 * max(1.0, abs(lr)), (float(loss), lr)
    check_rell2(host(dx), dxr, what='dfeatures')
    check_rell2(host(dW)[:, :c], dWr, what='dweights')
    assert (host(dW)[:, c:] == 0).all()
    assert abs(float(loss) - float(dense[0])) <= 2e-5 * max(1.0, abs(lr))
    check_rell2(host(dx), host(dense[1]), what='dfeatures against additive_margin_loss')
    with pytest.raises(ValueError, match='not a shard that starts at'):
        sharded_margin_loss(dev(x), dev(W), dev(y, torch.int32), 5, c, _OneRank(), *preset)
