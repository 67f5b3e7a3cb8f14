"""The streaming pointwise kernel's launch arithmetic (csrc/pw16.hip: nb_for, pw16_plan, pw16_waves, the kernel's block -> (rb, ct) decode
and its tile loop `t = rb * NW + wv; t += nrb * NW`) restated in Python for the statistics form (EPI = PW_EPI_STATS) that
fte_conv2d_bn_fwd launches.  It only says WHICH instantiation, grid and tile walk a shape gets, so that the tests can pin a case to the
class it is there for and the launch record to a symbol; it never checks a value.  No GPU, no torch.

The two hooks pw16_plan reads once per process are arguments here: `blocks` = FTE_PW16_BLOCKS (default 256), `k256` = FTE_PW16_K256
(default 1; 0 = the four-wave K = 256 forms)."""

PRO_NONE, PRO_FWD = 0, 1
EPI_STATS = 1


def nb_for(K, N):
    nb = 256 if K == 64 else 128
    while nb > 64 and N % nb:
        nb >>= 1
    return nb


def plan(M, K, N, blocks=256, k256=1):
    """pw16_plan(M, K, N, PW_EPI_STATS) -> dict(nb, nct, nw, nrb), or None where the planner refuses the shape (the tile kernels run)"""
    if K not in (64, 128, 256) or N < 64 or N % 64 or M < 32 or M * max(K, N) * 2 >= 1 << 31:
        return None
    wide = k256 == 0
    nb = nb_for(K, N)
    eight256 = K == 256 and not wide
    if eight256:
        nb = 64
    if N % nb:
        return None
    nw = 4 if (K == 256 and not eight256) else 8
    nct = N // nb
    tiles = (M + 31) // 32
    nrb = (tiles + nw - 1) // nw
    want = blocks // nct if blocks // nct > 0 else 1
    nrb = min(nrb, want, 512)
    # pw16_waves: what the launch record spells (the same value as the planner's nw for the statistics form)
    waves = 8 if K != 256 else (8 if (nb == 64 and not wide) else 4)
    assert waves == nw, (M, K, N, blocks, k256)
    return dict(nb=nb, nct=nct, nw=nw, nrb=nrb)


def symbol(K, nb, nw, fold):
    """as csrc/api.hip spells it into the launch record"""
    return 'pw16_kernel<%d,%d,%d,%d,%d>' % (K, nb, nw, PRO_FWD if fold else PRO_NONE, EPI_STATS)


def decode(bid, nrb, nct):
    """block id -> (rb, ct): the column tiles of one row block sit on one XCD (ids 8 apart); rb >= nrb is a dead block"""
    xcd, j = bid & 7, bid >> 3
    per = (nrb + 7) // 8
    return j // nct + xcd * per, j % nct


def wave_tiles(rb, wv, nrb, nw, ntile):
    """the 32-row tiles wave `wv` of row block `rb` walks, in order"""
    return list(range(rb * nw + wv, ntile, nrb * nw))


def launch(M, K, N, fold=False, blocks=256, k256=1):
    """What fte_conv2d_bn_fwd launches for a 1x1 / stride-1 conv of M pixels, K -> N channels, under bf16 storage.  None where pw16_plan
    refuses.  Keys: symbol, nb, nct, nw, nrb, grid, dead_blocks, tiles (32-row tiles), tiles_min / tiles_max (tiles per wave over every
    wave of the live blocks: an idle wave counts 0), idle_waves (waves of live blocks without a tile), last_rows (rows of the last tile).
    The enumeration also PROVES the map: every (tile, column tile) is visited exactly once and every rb < nrb has a block per column tile."""
    p = plan(M, K, N, blocks, k256)
    if p is None:
        return None
    nb, nct, nw, nrb = p['nb'], p['nct'], p['nw'], p['nrb']
    ntile = (M + 31) // 32
    grid = (nrb + 7) // 8 * 8 * nct
    seen, live, dead, per_wave = {}, set(), 0, []
    for bid in range(grid):
        rb, ct = decode(bid, nrb, nct)
        assert 0 <= ct < nct
        if rb >= nrb:
            dead += 1
            continue
        assert (rb, ct) not in live, 'two blocks decode to (%d, %d)' % (rb, ct)
        live.add((rb, ct))
        for wv in range(nw):
            ts = wave_tiles(rb, wv, nrb, nw, ntile)
            if ct == 0:
                per_wave.append(len(ts))
            for t in ts:
                seen[(t, ct)] = seen.get((t, ct), 0) + 1
    assert live == {(rb, ct) for rb in range(nrb) for ct in range(nct)}, 'a row block below nrb has no block'
    assert sorted(seen) == [(t, ct) for t in range(ntile) for ct in range(nct)], 'a tile is never visited'
    assert set(seen.values()) == {1}, 'a tile is visited twice'
    assert dead == grid - nrb * nct
    return dict(symbol=symbol(K, nb, nw, fold), nb=nb, nct=nct, nw=nw, nrb=nrb, grid=grid, dead_blocks=dead, tiles=ntile,
                tiles_min=min(per_wave), tiles_max=max(per_wave), idle_waves=sum(1 for c in per_wave if c == 0),
                last_rows=M - 32 * (ntile - 1))


def ws_rows(M):
    """partial rows fte_conv2d_bn_fwd_ws_bytes grants ([rows][3][cout] floats): one per 64 output rows, and two"""
    return (M + 63) // 64 + 2


def reachable(blocks=256, k256=1, max_n=1024):
    """every (K, NB, NW) the statistics form reaches under the given hooks, over N = 64 .. max_n"""
    out = set()
    for K in (64, 128, 256):
        for N in range(64, max_n + 1, 64):
            p = plan(4096, K, N, blocks, k256)
            if p:
                out.add((K, p['nb'], p['nw']))
    return out
