"""The launch arithmetic of the bf16 conv kernels (csrc/igemm16.hip, csrc/wgrad16.hip) restated in Python: the padded-slot window of
igemm16rw_kernel and its admission, the selection ladder of igemm16_launch for a bf16-STORAGE launch without BN, the plans of the two
resident filter-gradient kernels and their block maps, and -- for the exact-placement kinds of tests/tile_worker.py -- what a 3x3 conv of a
one-non-zero-per-channel filter must store.  It says WHICH kernel, window and slot range a shape gets and which element lands where, so
that the tests can pin a case to the branch it is there for; tests/test_gpu_bf16_conv_edges.py ties it to the C++ (recorded symbol ==
prediction for every case).  No GPU, no torch.

Restated from (line numbers of the files as of this module's commit):
  slot_of, window            igemm16.hip 1087-1093 (slot_of), 1107-1112 (setup_w: lo, hi, npc), comment 1027-1031
  launch16rw_ok              igemm16.hip 1535-1545
  launch16p_ok               igemm16.hip 1630-1640
  igemm16_handles            igemm16.hip 1693-1701
  igemm16_launch (no BN)     igemm16.hip 1741-1807; recorded names: launch16p 967, launch16rw 1558, launch16 1650
  pick_tile / plan_rows      conv_plan.h 136-145, 208-303 (only the single-launch outcomes the edge cases use)
  wgrad16_plan               wgrad16.hip 517-559; TABCAP: 315-316; block map: 85-94
  wgrad16p_plan              wgrad16.hip 566-598; block map: 382-390
  magic division             wgrad16.hip 153 (use), 554-556 (making)"""
import numpy as np

EPI_FWD, EPI_DGRAD = 0, 1
T128, T256x64, T128x64, T64 = 0, 1, 2, 3          # csrc/igemm.h TILE_*, as tests/conv_plan_cases.py
BK16, KP, BM_RW = 64, 64, 256
SLOTS = 1536


def _up(a, b):
    return (a + b - 1) // b


# ---- window geometry ----------------------------------------------------------------------------------------------------------------
def slot_of(m, H, W):
    """pixel index -> padded slot: one zero slot ahead of every image row, one zero row ahead of every image"""
    n, rem = divmod(m, H * W)
    y, x = divmod(rem, W)
    return n * (H + 1) * (W + 1) + (y + 1) * (W + 1) + x + 1


def window(m0, mlast, H, W):
    """(lo, hi, pieces) of the tile of pixels m0 .. mlast: slots [slot(m0) - W - 2, slot(mlast) + W + 2] in 8-slot pieces"""
    lo, hi = slot_of(m0, H, W) - W - 2, slot_of(mlast, H, W) + W + 2
    return lo, hi, (hi - lo + 8) >> 3


def pieces_needed(H, W, BM=BM_RW, starts=None):
    """the most pieces a FULL tile of BM pixels needs over the tile starts m0 (default: every start of a period, 0 .. H W - 1, which
    contains every multiple of BM modulo H W); a ragged last tile needs no more than the full tile at its start"""
    hw = H * W
    m0 = np.arange(hw, dtype=np.int64) if starts is None else np.asarray(starts, np.int64)
    m1 = m0 + BM - 1

    def slot(m):
        n, rem = m // hw, m % hw
        return n * (H + 1) * (W + 1) + (rem // W + 1) * (W + 1) + rem % W + 1
    return int((((slot(m1) + W + 2) - (slot(m0) - W - 2) + 8) >> 3).max())


def pieces_needed_launch(H, W, BM=BM_RW):
    """... over the tile starts a launch really has (multiples of BM, one period of them)"""
    hw = H * W
    return pieces_needed(H, W, BM, starts=[(BM * t) % hw for t in range(hw)])


def span_bound(H, W, BM=BM_RW):
    """launch16rw_ok's worst-case window in slots, and in pieces"""
    hw = H * W
    imgx, rowx = (BM + hw - 1) // hw, (BM - 1) // W + 1
    span = (BM - 1) + rowx + imgx * (W + 1) + 2 * (W + 1) + 3
    return span, (span + 7) // 8


def launch16rw_ok(H, W, a_KC, K, a_NT, stride, wcap, BM=BM_RW):
    """(the tap shifts of a 3x3 TF-SAME conv are within +-1, m_base = 0, c_OH = 0 and c_ld = N for the stride-1 storage launches)"""
    if a_NT != 9 or stride != 1 or a_KC % BK16 or K != 9 * a_KC:
        return False
    return span_bound(H, W, BM)[1] <= wcap


def launch16p_ok(tile, a_KC, K, a_NT):
    """a whole-K storage launch (splits = 1, no split-K slab, one parity class, amod = channels: a multiple of 8)"""
    if tile not in (T128, T128x64):
        return False
    return not (K % BK16 or K // BK16 < 4 or a_KC % BK16 or a_NT > 9)


def symbol16(epi, tile, H, W, a_KC, K, a_NT, stride, ntiles, deep_tiles=256):
    """igemm16_launch of a storage launch without BN -> the symbol as fte_prof_get_name records it; None where igemm16_handles refuses (the
    register-staged kernels of igemm.hip run).  ntiles = ceil(M / 128) * (N / the tile's width)."""
    if a_KC % BK16 or K % BK16 or tile not in (T128, T128x64):
        return None
    bn = 128 if tile == T128 else 64
    if a_NT == 1 and ntiles <= deep_tiles and K // BK16 >= 6:                      # the three-stage ring of the per-tile kernel
        return 'igemm16_kernel<128,%d,4,2,%d,3,%d,0,0>' % (bn, epi, 2 if tile == T128 else 4)
    if launch16p_ok(tile, a_KC, K, a_NT):
        if tile == T128:
            if (K // BK16) % 2 == 0 and launch16rw_ok(H, W, a_KC, K, a_NT, stride, 45):
                return 'igemm16rw_kernel<256,128,4,2,%d,4,1,45,2,0,0>' % epi
            if launch16rw_ok(H, W, a_KC, K, a_NT, stride, 48):
                return 'igemm16rw_kernel<256,128,4,2,%d,4,2,48,1,0,0>' % epi
            if epi == EPI_FWD:
                return 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>'
        else:
            if launch16rw_ok(H, W, a_KC, K, a_NT, stride, 56):
                return 'igemm16rw_kernel<256,64,8,1,%d,4,2,56,1,8,0>' % epi
            return 'igemm16p_kernel<128,64,4,2,%d,2,6,1,0>' % epi
    return 'igemm16_kernel<128,%d,4,2,%d,2,%d,0,0>' % (bn, epi, 4 if tile == T128 else 6)


def wcap_of(symbol):
    """window capacity (pieces) of an igemm16rw symbol, else None"""
    if not symbol or not symbol.startswith('igemm16rw_kernel<'):
        return None
    return int(symbol[symbol.index('<') + 1:-1].split(',')[7])


# ---- the planner's tile for the small storage launches of the edge tests ------------------------------------------------------------
def tiles_of(tile, M, N):
    bm, bn = {T128: (128, 128), T256x64: (256, 64), T128x64: (128, 64), T64: (64, 64)}[tile]
    return _up(M, bm) * (N // bn)


def pick_tile16(M, N, want16=120):
    cands = [T128 if N % 128 == 0 else T256x64, T128x64, T64]
    for c in cands:
        if tiles_of(c, M, N) >= want16:
            return c
    return cands[2]


def plan_tile16(M, N, want16=120, fills16=384):
    """plan_rows of a bf16-storage launch that stays ONE launch below a round of 64x64 tiles -> the tile.  (Every edge case is one; the host
    test compares with the planner itself, tests/conv_plan_dump.cpp.)"""
    n16 = _up(M, 128) * (N // (128 if N % 128 == 0 else 64))
    if 512 <= n16 < SLOTS:                                  # plan_unsplit16
        return T128 if N % 128 == 0 else T128x64
    big = (T128 if N % 128 == 0 else T128x64) if n16 >= fills16 else T64
    assert tiles_of(big, M, N) < SLOTS, 'not a small launch'
    return pick_tile16(M, N, want16)


def conv_launch(kind, n, h, w, cin, cout, ksize, want16=120):
    """(symbol | None, tile, M, N, K) of fte_conv2d_{fwd,dgrad}_s16 for a stride-1 conv; kind 'fwd' | 'dgrad'"""
    M = n * h * w
    N, kc = (cout, cin) if kind == 'fwd' else (cin, cout)
    K = ksize * ksize * kc
    tile = plan_tile16(M, N, want16)
    ntiles = _up(M, 128) * (N // (128 if tile == T128 else 64)) if tile in (T128, T128x64) else 0
    sym = symbol16(EPI_FWD if kind == 'fwd' else EPI_DGRAD, tile, h, w, kc, K, ksize * ksize, 1, ntiles)
    return sym, tile, M, N, K


# ---- filter-gradient plans ----------------------------------------------------------------------------------------------------------
WGRAD16_CFG = [(32, 256, 128, 'wgrad16_kernel<32,256,3,128>'), (64, 128, 128, 'wgrad16_kernel<64,128,3,128>'),
               (64, 64, 192, 'wgrad16_kernel<64,64,3,192>')]                   # (CT, BN, XCAP, symbol) per cfg
WGRAD16P_CFG = [(128, 256, 'wgrad16p_kernel<128,256,2,4>'), (256, 128, 'wgrad16p_kernel<256,128,4,2>'), (128, 128, 'wgrad16p_kernel<128,128,2,4>'),
                (64, 256, 'wgrad16p_kernel<64,256,1,8>'), (256, 64, 'wgrad16p_kernel<256,64,8,1>'), (64, 128, 'wgrad16p_kernel<64,128,2,4>'),
                (128, 64, 'wgrad16p_kernel<128,64,4,2>')]


def _round_s(S):
    return S & ~7 if S >= 8 else 4 if S >= 4 else 2 if S >= 2 else 1


def tabcap(cfg):
    """slots of an image the kernel's LDS table holds"""
    return 57 * 57 if cfg == 2 else 31 * 31


def wgrad16_plan(n, h, w, cin, cout, cus=256, minp=8):
    """-> dict(cfg, ct, bn, xcap, symbol, npairs, S, kper, pieces, KT, magic_is, magic_pw1), or None where the plan refuses"""
    if w > 62 or w < 7 or h < 7:
        return None
    if w <= 30 and cout % 256 == 0 and cin % 32 == 0:
        cfg = 0
    elif w <= 30 and cout % 128 == 0 and cin % 64 == 0:
        cfg = 1
    elif cout % 64 == 0 and cin % 64 == 0:
        cfg = 2
    else:
        return None
    ct, bn, xcap, sym = WGRAD16_CFG[cfg]
    if (h + 1) * (w + 1) > tabcap(cfg):
        return None
    npairs = (cin // ct) * (cout // bn)
    S = _round_s(cus // npairs)
    KT = n * (h + 1) * (w + 1)
    pieces = _up(KT, KP)
    if KT >= 1 << 24:
        return None
    if pieces < minp * S:
        S = _round_s(pieces // minp)
        if pieces < 2:
            return None
    return dict(cfg=cfg, ct=ct, bn=bn, xcap=xcap, symbol=sym, npairs=npairs, S=S, kper=_up(pieces, S) * KP, pieces=pieces, KT=KT,
                magic_is=(1 << 40) // ((h + 1) * (w + 1)) + 1, magic_pw1=(1 << 40) // (w + 1) + 1)


def wgrad16p_plan(n, h, w, cin, cout, cus=256):
    for cfg, (c, o) in enumerate([(128, 256), (256, 128), (128, 128), (64, 256), (256, 64), (64, 128), (128, 64)]):
        if cin % c == 0 and cout % o == 0:
            break
    else:
        return None
    ct, bn, sym = WGRAD16P_CFG[cfg]
    npairs = (cin // ct) * (cout // bn)
    KT = n * h * w
    pieces = _up(KT, KP)
    S = _round_s(cus // npairs)
    while S > 1 and pieces < 4 * S:
        S >>= 1
    if pieces < 4 or KT * max(cin, cout) * 2 >= 1 << 31:
        return None
    return dict(cfg=cfg, ct=ct, bn=bn, symbol=sym, npairs=npairs, S=S, kper=_up(pieces, S) * KP, pieces=pieces, KT=KT)


def slot_ranges(plan):
    """per split: (first piece, pieces) as the kernels derive them -- kend = min(kbeg + kper, pieces * 64); a range that starts at or behind
    the end is EMPTY (0 pieces: the block stores a zero slab)"""
    end = plan['pieces'] * KP
    out = []
    for split in range(plan['S']):
        kbeg = split * plan['kper']
        kend = min(kbeg + plan['kper'], end)
        out.append((kbeg // KP, max((kend - kbeg) // KP, 0) if kend > kbeg else 0))
    return out


def block_map(bid, S, npairs):
    """block id -> (pair, split): the blocks of one slot range share an XCD (id & 7) where S allows"""
    if S >= 8:
        return (bid >> 3) % npairs, (bid & 7) + 8 * ((bid >> 3) // npairs)
    return bid // S, bid % S


def magic_div(s, magic):
    return (s * magic) >> 40


# ---- exact placement (tests/tile_worker.py 's16fwdx' / 's16dgradx') -----------------------------------------------------------------
def placement_filter(C, N, a=5, b=3):
    """one non-zero per GEMM output channel n: tap(n) = n mod 9, k(n) = (a n + b) mod C (a odd), weight 2^e, e = n mod 5 - 2 (as
    tile_worker.selection_filter) -> (tap [N], k [N], g [N])"""
    n = np.arange(N)
    return n % 9, (a * n + b) % C, 2.0 ** ((n % 5) - 2)


def hwio_filter(kind, cin, cout):
    """the HWIO [3, 3, cin, cout] filter of the placement check.  Forward: output channel n = cout index, k(n) a cin index.  Data gradient:
    output channel n = cin index, k(n) a cout index."""
    wt = np.zeros((3, 3, cin, cout))
    if kind == 'fwd':
        tap, k, g = placement_filter(cin, cout)
        wt[tap // 3, tap % 3, k, np.arange(cout)] = g
    else:
        tap, k, g = placement_filter(cout, cin)
        wt[tap // 3, tap % 3, np.arange(cin), k] = g
    return wt


def placement_expected(kind, src, N):
    """src [n, h, w, C] (x, or dz) -> the [n, h, w, N] tensor a 3x3 / stride-1 TF-SAME conv ('fwd') or its data gradient ('dgrad') of
    hwio_filter must give: the input element one tap away times a power of two, exact zero where the tap leaves the image.
    forward: z[y, x, n] = x[y + r - 1, x + s - 1, k(n)] g(n); data gradient: dx[y, x, n] = dz[y - (r - 1), x - (s - 1), k(n)] g(n), tap = 3 r + s"""
    nimg, h, w, C = src.shape
    tap, k, g = placement_filter(C, N)
    pad = np.zeros((nimg, h + 2, w + 2, C))
    pad[:, 1:-1, 1:-1] = src
    out = np.zeros((nimg, h, w, N))
    sign = 1 if kind == 'fwd' else -1
    for t in range(9):
        dh, dw = sign * (t // 3 - 1), sign * (t % 3 - 1)
        ch = np.flatnonzero(tap == t)
        out[..., ch] = pad[:, 1 + dh:1 + dh + h, 1 + dw:1 + dw + w][..., k[ch]] * g[ch]
    return out


def placement_check(got, want):
    """-> (number of wrong elements, (image, y, x, channel) of the first in memory order | None); got / want [n, h, w, N], compared as
    given (the worker passes bf16 BIT patterns, the host tests values)"""
    bad = np.asarray(got) != np.asarray(want)
    cnt = int(bad.sum())
    if not cnt:
        return 0, None
    return cnt, tuple(int(v) for v in np.unravel_index(int(np.flatnonzero(bad.reshape(-1))[0]), bad.shape))


def placement_by_slots(kind, src, N, pad_wrap=False, image_shift=0):
    """the SAME result the way the window kernel forms it: pixels at their padded slots in one flat array (pad slots zero), output pixel m
    reads slot(m) + dh (W + 1) + dw.  The two flags build WRONG kernels for the checker's sensitivity tests: `pad_wrap` drops the zero
    slot ahead of every image row (a tap across a row end reads the neighbouring row's pixel), `image_shift` moves the read by that many
    slots for every pixel behind the first image."""
    nimg, h, w, C = src.shape
    tap, k, g = placement_filter(C, N)
    M = nimg * h * w
    flat = src.reshape(M, C)
    m = np.arange(M)
    pw1 = w if pad_wrap else w + 1
    img, rem = m // (h * w), m % (h * w)
    slots = img * (h + 1) * pw1 + (rem // w + 1) * pw1 + rem % w + (0 if pad_wrap else 1)
    assert pad_wrap or all(int(s) == slot_of(int(i), h, w) for i, s in zip(m[:: max(M // 64, 1)], slots[:: max(M // 64, 1)]))
    lds = np.zeros((nimg * (h + 1) * pw1 + 2 * pw1 + 4, C))
    lds[slots] = flat
    out = np.zeros((M, N))
    sign = 1 if kind == 'fwd' else -1
    for t in range(9):
        dh, dw = sign * (t // 3 - 1), sign * (t % 3 - 1)
        ch = np.flatnonzero(tap == t)
        s = slots + dh * pw1 + dw + np.where(img > 0, image_shift, 0)
        ok = s >= 0
        out[np.ix_(ok, ch)] = lds[s[ok]][:, k[ch]] * g[ch]
    return out.reshape(nimg, h, w, N)
