"""CPU: the host model of the bf16 conv kernels' windows and plans (tests/win16_map.py) -- the window kernel's capacity bound against a
brute force over every tile start, the filter-gradient plans' capacity / coverage / magic-division / block-map properties, the case table
of tests/test_gpu_bf16_conv_edges.py against the host planner (tests/conv_plan_dump.cpp) and against what the issue's table names, and the
exact-placement checker against two deliberately wrong 'kernels' built in numpy."""
import numpy as np
import pytest

import bf16_edge_cases as E
import conv_plan_cases as C
import win16_map as W
from test_conv_plan_host import dump, run_dump      # noqa: F401  (the compiled planner: a module-scoped fixture and its driver)

ALL_CASES = [(g, env, c) for g, env, cases in E.GROUPS for c in cases]


# ---- the window ---------------------------------------------------------------------------------------------------------------------
def test_slot_of_is_the_padded_layout():
    """one zero slot ahead of every image row, one zero row ahead of every image: distinct, increasing, and the eight neighbours of a
    pixel are its slot + dh (W + 1) + dw -- a pad slot (no pixel maps to it) exactly where the tap leaves the image"""
    for H, Wd in ((7, 6), (4, 4), (5, 9), (1, 3), (3, 1)):
        n = 3
        slots = {W.slot_of(m, H, Wd): m for m in range(n * H * Wd)}
        assert len(slots) == n * H * Wd and sorted(slots.values()) == sorted(slots.values(), key=lambda m: W.slot_of(m, H, Wd))
        for m in range(n * H * Wd):
            img, rem = divmod(m, H * Wd)
            y, x = divmod(rem, Wd)
            for dh in (-1, 0, 1):
                for dw in (-1, 0, 1):
                    s = W.slot_of(m, H, Wd) + dh * (Wd + 1) + dw
                    inside = 0 <= y + dh < H and 0 <= x + dw < Wd
                    assert (slots.get(s) == m + dh * Wd + dw) if inside else (s not in slots), (H, Wd, m, dh, dw)
        lo, hi, npc = W.window(0, n * H * Wd - 1, H, Wd)
        assert lo == W.slot_of(0, H, Wd) - Wd - 2 and hi == max(slots) + Wd + 2 and npc == (hi - lo + 8) // 8


def test_the_window_bound_covers_every_tile_start_and_is_attained():
    """launch16rw_ok's hand-derived span, in 8-slot pieces, is never below what a 256-pixel tile needs at ANY start of a period, for every
    H, W in 1..64; it is attained (not slack everywhere); and every shape the ladder sends to a WCAP variant needs at most that WCAP"""
    attained = []
    for H in range(1, 65):
        for Wd in range(1, 65):
            need, bound = W.pieces_needed(H, Wd), W.span_bound(H, Wd)[1]
            assert need <= bound, (H, Wd, need, bound)
            assert W.pieces_needed_launch(H, Wd) <= need
            if need == bound:
                attained.append((H, Wd))
            for epi in (W.EPI_FWD, W.EPI_DGRAD):
                for tile, kc in ((W.T128, 128), (W.T128, 192), (W.T128x64, 64)):
                    cap = W.wcap_of(W.symbol16(epi, tile, H, Wd, kc, 9 * kc, 9, 1, 1000))
                    assert cap is None or need <= cap, (H, Wd, tile, kc, need, cap)
    assert len(attained) > 1000 and (7, 7) in attained and (56, 56) in attained, len(attained)


def test_the_pieces_of_the_issues_table():
    for (H, Wd), want in {(7, 7): 45, (7, 6): 46, (8, 5): 46, (14, 12): 42, (28, 24): 43, (28, 28): 45, (56, 48): 52, (56, 56): 55, (4, 4): 52}.items():
        assert W.span_bound(H, Wd)[1] == want, (H, Wd)
    assert W.span_bound(7, 7)[0] == 359


def test_the_ladder_of_igemm16_launch():
    s = W.symbol16
    # 3x3: the three window instantiations, igemm16p where the window is too wide, the per-tile data gradient
    assert s(0, W.T128, 7, 7, 128, 1152, 9, 1, 3) == 'igemm16rw_kernel<256,128,4,2,0,4,1,45,2,0,0>'
    assert s(1, W.T128, 7, 6, 128, 1152, 9, 1, 1) == 'igemm16rw_kernel<256,128,4,2,1,4,2,48,1,0,0>'      # 46 pieces
    assert s(0, W.T128, 7, 7, 64, 576, 9, 1, 2) == 'igemm16rw_kernel<256,128,4,2,0,4,2,48,1,0,0>'        # odd K-steps
    assert s(0, W.T128, 4, 4, 128, 1152, 9, 1, 1) == 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>'
    assert s(1, W.T128, 4, 4, 128, 1152, 9, 1, 1) == 'igemm16_kernel<128,128,4,2,1,2,4,0,0>'
    assert s(0, W.T128x64, 56, 56, 64, 576, 9, 1, 25) == 'igemm16rw_kernel<256,64,8,1,0,4,2,56,1,8,0>'
    assert s(1, W.T128x64, 64, 64, 64, 576, 9, 1, 32) == 'igemm16p_kernel<128,64,4,2,1,2,6,1,0>'         # 57 pieces > 56
    assert s(0, W.T128, 28, 28, 128, 1152, 9, 2, 9) == 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>'          # stride 2: no window
    # 1x1: K/64 >= 6 three-stage ring (at most 256 tiles), >= 4 igemm16p, else the two-stage per-tile kernel
    for k64, want in ((8, 'igemm16_kernel<128,128,4,2,0,3,2,0,0>'), (6, 'igemm16_kernel<128,128,4,2,0,3,2,0,0>'), (5, 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>'),
                      (4, 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>'), (3, 'igemm16_kernel<128,128,4,2,0,2,4,0,0>')):
        assert s(0, W.T128, 7, 6, 64 * k64, 64 * k64, 1, 1, 1) == want, k64
    assert s(0, W.T128, 7, 6, 512, 512, 1, 1, 257) == 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>'           # more than a tile per CU
    assert s(1, W.T128, 7, 6, 384, 384, 1, 1, 1) == 'igemm16_kernel<128,128,4,2,1,3,2,0,0>'
    assert s(1, W.T128, 7, 6, 256, 256, 1, 1, 1) == 'igemm16_kernel<128,128,4,2,1,2,4,0,0>'              # a 128 x 128 data gradient never on igemm16p
    assert s(0, W.T128x64, 7, 6, 512, 512, 1, 1, 2) == 'igemm16_kernel<128,64,4,2,0,3,4,0,0>'
    assert s(1, W.T128x64, 7, 6, 256, 256, 1, 1, 2) == 'igemm16p_kernel<128,64,4,2,1,2,6,1,0>'
    assert s(0, W.T128x64, 7, 6, 192, 192, 1, 1, 2) == 'igemm16_kernel<128,64,4,2,0,2,6,0,0>'
    assert s(0, W.T128, 7, 6, 96, 96, 1, 1, 1) is None and s(0, W.T64, 7, 6, 128, 128, 1, 1, 1) is None and s(0, W.T256x64, 7, 6, 128, 128, 1, 1, 1) is None


# ---- the case table of the GPU module -----------------------------------------------------------------------------------------------
# what the issue's table names per case id ('' = no igemm16 / no resident symbol); the model must agree, or the case is listed in
# CORRECTED with what the code does instead
NAMED = {
    '3x7x6x128': 'igemm16rw_kernel<256,128,4,2,{e},4,2,48,1,0,0>', '6x7x7x128': 'igemm16rw_kernel<256,128,4,2,{e},4,1,45,2,0,0>',
    '2x14x12x128': 'igemm16rw_kernel<256,128,4,2,{e},4,1,45,2,0,0>', '1x28x24x128': 'igemm16rw_kernel<256,128,4,2,{e},4,1,45,2,0,0>',
    '5x7x7x64to128-fwd': 'igemm16rw_kernel<256,128,4,2,0,4,2,48,1,0,0>', '5x9x7x192-fwd': 'igemm16rw_kernel<256,128,4,2,0,4,2,48,1,0,0>',
    '3x7x7x384': 'igemm16rw_kernel<256,128,4,2,{e},4,1,45,2,0,0>', '800x7x6x128to256': 'igemm16rw_kernel<256,128,4,2,{e},4,2,48,1,0,0>',
    '1x56x56x64': 'igemm16rw_kernel<256,64,8,1,{e},4,2,56,1,8,0>', '1x56x48x64': 'igemm16rw_kernel<256,64,8,1,{e},4,2,56,1,8,0>',
    '12x4x4x64': 'igemm16rw_kernel<256,64,8,1,{e},4,2,56,1,8,0>',
    '5x7x7x64to128-dgrad': 'igemm16rw_kernel<256,64,8,1,1,4,2,56,1,8,0>', '5x9x7x192-dgrad': 'igemm16rw_kernel<256,64,8,1,1,4,2,56,1,8,0>',
    '8x4x4x128-fwd': 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>', '8x4x4x128-dgrad': 'igemm16_kernel<128,128,4,2,1,2,4,0,0>',
    '1x56x48x64to128-fwd': 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>',
    'pw-k8': 'igemm16_kernel<128,128,4,2,0,3,2,0,0>', 'pw-k6': 'igemm16_kernel<128,128,4,2,0,3,2,0,0>', 'pw-k5': 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>',
    'pw-k4': 'igemm16p_kernel<128,128,4,2,0,2,4,1,0>', 'pw-k3': 'igemm16_kernel<128,128,4,2,0,2,4,0,0>', 'pw-k96': '',
    'pw-dgrad-k6': 'igemm16_kernel<128,128,4,2,1,3,2,0,0>', 'pw-n64-k8': 'igemm16_kernel<128,64,4,2,0,3,4,0,0>',
    'wg-30x30-cfg1': 'wgrad16_kernel<64,128,3,128>', 'wg-30x30-cfg0': 'wgrad16_kernel<32,256,3,128>', 'wg-31x31': 'wgrad16_kernel<64,64,3,192>',
    'wg-50x62': 'wgrad16_kernel<64,64,3,192>', 'wg-51x62': '', 'wg-14x12': 'wgrad16_kernel<64,128,3,128>', 'wg-28x24': 'wgrad16_kernel<64,128,3,128>',
    'wg-56x48': 'wgrad16_kernel<64,64,3,192>', 'wg-7x6': '', 'wg-6x9': '', 'wg-7x7-s1': 'wgrad16_kernel<32,256,3,128>',
    'wg-5x30x30-s8': 'wgrad16_kernel<64,128,3,128>', 'wg-38x8x8-empty': 'wgrad16_kernel<64,128,3,128>',
    'wgp-4pieces': 'wgrad16p_kernel<128,128,2,4>', 'wgp-3pieces': '', 'wgp-253px': 'wgrad16p_kernel<64,128,2,4>',
}
# the issue's table expected the 128 x 64 forms / wgrad16p here; the code decides otherwise (tests/bf16_edge_cases.py says why), and the
# nearest shapes that do reach them are the cases pw-n64-k8 and wgp-253px
CORRECTED = {'pw-n64-k8-m84': '', 'wgp-189px': ''}


def _named(cid):
    for key in (cid, cid.rsplit('-', 1)[0]):
        for table in (NAMED, CORRECTED):
            if key in table:
                return table[key].format(e=1 if cid.endswith('-dgrad') else 0)
    raise KeyError(cid)


def test_every_case_reaches_the_kernel_it_is_there_for():
    ids = [c[0] for _, _, c in ALL_CASES]
    assert len(set(ids)) == len(ids)
    for _, env, case in ALL_CASES:
        what, val = E.expected(case, env)
        got = (val or '') if what == 'symbol' else (val['symbol'] if val else '')
        assert got == _named(case[0]), (case[0], got)
        if case[1][0].startswith('s16wgrad'):
            assert case[4] == what, case[0]
    p = lambda cid: E.expected(next(c for _, _, c in ALL_CASES if c[0] == cid), next(e for _, e, c in ALL_CASES if c[0] == cid))[1]
    assert (p('wg-7x7-s1')['S'], p('wg-7x7-s1')['npairs']) == (1, 4)
    assert (p('wg-5x30x30-s8')['S'], p('wg-5x30x30-s8')['pieces']) == (8, 76) and W.slot_ranges(p('wg-5x30x30-s8'))[-1] == (70, 6)
    e = p('wg-38x8x8-empty')
    assert (e['S'], e['pieces'], e['kper']) == (48, 49, 128)
    assert [n for _, n in W.slot_ranges(e)] == [2] * 24 + [1] + [0] * 23
    assert (p('wgp-4pieces')['S'], p('wgp-4pieces')['pieces']) == (1, 4) and p('wgp-253px')['KT'] % 64 == 61
    for cid in ('wg-30x30-cfg1', 'wg-30x30-cfg0', 'wg-50x62'):              # XCAP exactly full; the slot table too at 30x30
        _, _, dims, _, _, _ = next(c for _, _, c in ALL_CASES if c[0] == cid)
        assert p(cid)['xcap'] == 64 + 2 * (dims[2] + 1) + 2
    assert 31 * 31 == W.tabcap(1) == W.tabcap(0) and 57 * 57 == W.tabcap(2)


def test_every_conv_case_has_the_models_tile_under_the_host_planner(dump, tmp_path):       # noqa: F811
    """the planner itself (csrc/conv_plan.h through tests/conv_plan_dump.cpp), under each group's environment: the bf16-storage context
    plans every case as ONE unsplit launch of the tile the model derives"""
    for gi, (name, env, cases) in enumerate(E.GROUPS):
        convs = [c for c in cases if not c[1][0].startswith('s16wgrad')]
        if not convs:
            continue
        shapes = sorted({('conv',) + tuple(c[2]) + (c[3], 1) for c in convs})
        d = tmp_path / ('g%d' % gi)
        d.mkdir()
        recs = dict(zip(shapes, run_dump(dump, d, env, shapes)))
        for cid, kinds, dims, ksize, _, _ in convs:
            kind = 'fwd' if 'fwd' in kinds[0] else 'dgrad'
            _, tile, M, N, K = W.conv_launch(kind, *dims, ksize, want16=E.want16(env))
            ctx = recs[('conv',) + tuple(dims) + (ksize, 1)]['ctx']['s16']
            if kind == 'fwd':
                rp = ctx['fwd']
            else:
                assert len(ctx['cls']) == 1 and not ctx['merged'][0], cid
                rp = ctx['cls'][0][4]
            bm = {W.T128: 128, W.T256x64: 256, W.T128x64: 128, W.T64: 64}[tile]
            assert rp[C.MAIN_TILE] == tile and rp[C.MAIN_ROWS] == M and rp[C.MAIN_MT] == -(-M // bm), (name, cid, rp)
            assert rp[C.TAIL_MODE] == 0 and rp[C.PW_BYTES] == 0, (name, cid, rp)


# ---- filter-gradient plans ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cus', [256, 104, 304])
def test_wgrad16_admission_capacity_and_coverage(cus):
    chans = ((64, 64), (64, 128), (32, 256), (128, 128), (128, 256), (256, 256), (192, 64), (96, 128), (64, 192))
    seen = set()
    for h in range(1, 66):
        for w in range(1, 66):
            for cin, cout in chans:
                for n, minp in ((1, 8), (5, 8), (38, 1), (128, 8)):
                    p = W.wgrad16_plan(n, h, w, cin, cout, cus=cus, minp=minp)
                    if p is None:
                        continue
                    what = (n, h, w, cin, cout, minp, p)
                    assert p['xcap'] >= 64 + 2 * (w + 1) + 2, what
                    assert (h + 1) * (w + 1) <= W.tabcap(p['cfg']), what
                    assert cin % p['ct'] == 0 and cout % p['bn'] == 0 and p['S'] >= 1 and (p['S'] < 8 or p['S'] % 8 == 0), what
                    assert p['S'] * p['npairs'] <= max(cus, p['npairs']), what
                    r = W.slot_ranges(p)
                    pos = 0
                    for first, cnt in r:                      # no gap, no overlap; an empty range is reported as one
                        if cnt:
                            assert first == pos, what
                            pos += cnt
                    assert pos == p['pieces'] and len(r) == p['S'], what
                    assert all(cnt == 0 for first, cnt in r if first >= p['pieces']), what
                    seen.add((p['cfg'], p['S'] >= 8, any(c == 0 for _, c in r)))
    assert {c for c, _, _ in seen} == {0, 1, 2} and {b for _, b, _ in seen} == {True, False} and any(e for _, _, e in seen), seen
    assert W.wgrad16_plan(1, 7, 6, 128, 128) is None and W.wgrad16_plan(1, 6, 9, 64, 128) is None and W.wgrad16_plan(1, 7, 63, 64, 64) is None
    assert W.wgrad16_plan(1, 51, 62, 64, 64) is None and W.wgrad16_plan(1, 50, 62, 64, 64)['cfg'] == 2
    # w <= 30 but 32 x 31 slots: the rule picks cfg 1 / cfg 0 by w alone, their table is 31 x 31, and the plan refuses (it does not go on to cfg 2)
    assert W.wgrad16_plan(1, 31, 30, 64, 128) is None and W.wgrad16_plan(1, 31, 30, 32, 256) is None and W.wgrad16_plan(1, 31, 31, 64, 128)['cfg'] == 2


@pytest.mark.parametrize('cus', [256, 104])
def test_wgrad16p_plan_coverage(cus):
    for cin, cout in ((128, 256), (256, 128), (128, 128), (64, 256), (256, 64), (64, 128), (128, 64), (64, 64), (1024, 2048)):
        for KT in list(range(1, 700)) + [64 * 1000 + 1, 64 * 4096]:
            p = W.wgrad16p_plan(1, 1, KT, cin, cout, cus=cus)
            if p is None:
                assert cin == cout == 64 or KT <= 3 * 64, (cin, cout, KT)
                continue
            r = W.slot_ranges(p)
            assert p['pieces'] >= 4 * p['S'] or p['S'] == 1, p
            pos = 0
            for first, cnt in r:
                if cnt:
                    assert first == pos
                    pos += cnt
            assert pos == p['pieces'], (KT, p)


def test_the_magic_divisions():
    """(s * magic) >> 40 == s // d for the plan's two divisors: at every slot the kernel can divide in the GPU cases (a window reaches one
    image's slots past the tensor), and around every multiple of d sampled up to the plan's own cut-off KT < 2^24"""
    rng = np.random.default_rng(5)
    for _, env, case in ALL_CASES:
        if case[1][0] != 's16wgrad':
            continue
        n, h, w = case[2][:3]
        p = W.wgrad16_plan(*case[2], minp=E.minp(env))
        if p is None:
            continue
        for d, magic in (((h + 1) * (w + 1), p['magic_is']), (w + 1, p['magic_pw1'])):
            s = np.arange(p['KT'] + (h + 1) * (w + 1) + 64, dtype=np.uint64)
            assert ((s * np.uint64(magic)) >> np.uint64(40) == s // np.uint64(d)).all(), case[0]          # (s * magic < 2^64: s < 2^24, magic <= 2^40)
    for h, w in ((7, 7), (30, 30), (50, 62), (56, 56), (14, 12), (7, 62), (62, 7)):
        for d in ((h + 1) * (w + 1), w + 1):
            magic = (1 << 40) // d + 1
            ks = np.unique(np.concatenate([np.arange(1, 64), rng.integers(1, (1 << 24) // d, 4000), [(1 << 24) // d]]))
            for k in ks:
                for s in (int(k) * d - 1, int(k) * d, int(k) * d + 1):
                    if s < 1 << 24:
                        assert W.magic_div(s, magic) == s // d, (h, w, d, s)


def test_the_block_maps_own_every_pair_and_split_once():
    for S in (1, 2, 4, 8, 16, 48, 64, 256):
        for npairs in (1, 2, 4, 8, 3):
            got = sorted(W.block_map(b, S, npairs) for b in range(S * npairs))
            assert got == [(p, s) for p in range(npairs) for s in range(S)], (S, npairs)
            if S >= 8:            # the blocks of one slot range share an XCD
                assert all(W.block_map(b, S, npairs)[1] % 8 == b % 8 for b in range(S * npairs))


# ---- the canary checker of the worker -----------------------------------------------------------------------------------------------
def test_the_canary_checker_flags_each_kind_of_stray_or_missing_write():
    """tests/tile_worker.py _canary_fails on host tensors: a clean run passes; an unwritten element, a written guard row, a changed
    workspace tail and an unwritten fp32 result are each flagged, and only they"""
    import torch
    import tile_worker as T
    M, c, nbytes = 10, 8, 4096

    def fresh():
        buf = torch.full((M + T.GUARD, c), T.CANARY16, dtype=torch.int16)
        buf[:M] = 0x3f80                                        # "the kernel wrote every element"
        wsb = torch.full((nbytes // 4 + 1024,), float('nan'))
        wsb[:nbytes // 4] = 1.0
        return buf, wsb, torch.zeros(c)
    buf, wsb, dw = fresh()
    assert T._canary_fails({'z16': buf}, wsb, nbytes, {'dw': dw}) == []
    buf, wsb, dw = fresh()
    buf[M - 1, c - 1] = T.CANARY16
    f = T._canary_fails({'z16': buf}, wsb, nbytes, {'dw': dw})
    assert len(f) == 1 and 'z16: 1 elements never written' in f[0]
    buf, wsb, dw = fresh()
    buf[M, 0] = 0
    f = T._canary_fails({'z16': buf}, wsb, nbytes, {'dw': dw})
    assert len(f) == 1 and 'guard row' in f[0]
    buf, wsb, dw = fresh()
    wsb[nbytes // 4] = 0.0
    f = T._canary_fails({'z16': buf}, wsb, nbytes, {'dw': dw})
    assert len(f) == 1 and 'workspace' in f[0]
    buf, wsb, dw = fresh()
    dw[3] = float('nan')
    f = T._canary_fails({'z16': buf}, wsb, nbytes, {'dw': dw})
    assert len(f) == 1 and 'dw: 1 elements not finite' in f[0]
    assert T.CANARY16 == 0x7fc1 and torch.isnan(torch.tensor([T.CANARY16], dtype=torch.int16).view(torch.bfloat16).float()).all()


# ---- the exact-placement checker ----------------------------------------------------------------------------------------------------
def _coded(n, h, w, c):
    m, k = np.arange(n * h * w, dtype=np.int64)[:, None], np.arange(c, dtype=np.int64)[None, :]
    return ((((7 * m + 13 * k) % 251) - 125) / 64.0).reshape(n, h, w, c)


@pytest.mark.parametrize('kind', ['fwd', 'dgrad'])
def test_the_placement_reference_is_the_oracles_conv(kind):
    """the expected tensor of the exact-placement kinds == the float64 oracle's conv / data gradient of the same filter (exact: one product
    per output), == the padded-slot walk of the window kernel"""
    from oracle import ops
    n, h, w, cin, cout = 3, 5, 4, 16, 24
    wt = W.hwio_filter(kind, cin, cout)
    assert (np.count_nonzero(wt, axis=(0, 1, 2) if kind == 'fwd' else (0, 1, 3)) == 1).all()
    if kind == 'fwd':
        src = _coded(n, h, w, cin)
        ref = ops.conv2d_fwd(src, wt, 1)
        N = cout
    else:
        src = _coded(n, h, w, cout)
        ref, _ = ops.conv2d_bwd(np.zeros((n, h, w, cin)), wt, src, 1, need_dw=False)
        N = cin
    want = W.placement_expected(kind, src, N)
    assert W.placement_check(ref, want) == (0, None)
    assert (want == 0).sum() > 0 and len(np.unique(want)) > 100
    assert W.placement_check(W.placement_by_slots(kind, src, N), want) == (0, None)


@pytest.mark.parametrize('kind', ['fwd', 'dgrad'])
def test_the_checker_flags_a_neighbour_read_across_a_row_end(kind):
    """a 'kernel' without the zero slot ahead of every image row: a tap that leaves the image sideways reads the neighbouring row's pixel.
    First wrong element: image 0, row 0, the first column whose tap goes left / right out of the row"""
    n, h, w, c = 2, 4, 4, 16
    src = _coded(n, h, w, c)
    want = W.placement_expected(kind, src, c)
    got = W.placement_by_slots(kind, src, c, pad_wrap=True)
    cnt, first = W.placement_check(got, want)
    assert cnt > 0 and first is not None
    tap = W.placement_filter(c, c)[0]
    sign = 1 if kind == 'fwd' else -1
    bad = np.argwhere(got != want)                                      # memory order, as the checker reports
    assert first == tuple(int(v) for v in bad[0]) and cnt == len(bad)
    img, y, x, ch = first
    dw = sign * (tap[ch] % 3 - 1)
    assert img == 0 and (x + dw < 0 or x + dw >= w), first              # a sideways tap out of the row, nothing else
    assert all((xx + sign * (tap[cc] % 3 - 1)) in (-1, w) for _, _, xx, cc in bad)


@pytest.mark.parametrize('kind', ['fwd', 'dgrad'])
def test_the_checker_flags_a_shift_of_one_slot_behind_an_image_boundary(kind):
    n, h, w, c = 3, 4, 5, 16
    src = _coded(n, h, w, c)
    want = W.placement_expected(kind, src, c)
    got = W.placement_by_slots(kind, src, c, image_shift=1)
    cnt, first = W.placement_check(got, want)
    assert (got[0] == want[0]).all() and cnt > 0
    assert first[0] == 1 and first[:3] == (1, 0, 0), first                   # the first pixel of the second image
    assert cnt == int((got != want).sum()) and cnt > (n - 1) * h * w * c // 2
