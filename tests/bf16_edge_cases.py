"""The case table of tests/test_gpu_bf16_conv_edges.py, shared with tests/test_win16_map_host.py (which confirms every case's tile with the
host planner and every expectation with tests/win16_map.py on the CPU).  No GPU, no torch.

GROUPS: one worker process per environment (the planner's switches are read once per process).  A case is
(id, worker kinds, (n, h, w, cin, cout), ksize, expectation, why): the worker kinds all run on the same launch; the expectation is
'model' (the symbol tests/win16_map.py predicts -- None there means NO igemm16 symbol may run), or for the filter gradient 'plan'
(the resident kernel of the model's plan, S splits) / 'refused' (no wgrad16 symbol: the per-tile kernel, whose result must be right)."""
import win16_map as W

FWD3, DG3 = ['s16fwd', 's16fwdx'], ['s16dgrad', 's16dgradx']


def _conv(name, dims, why, kinds=('fwd', 'dgrad')):
    out = []
    if 'fwd' in kinds:
        out.append((name + '-fwd', FWD3, dims, 3, 'model', why))
    if 'dgrad' in kinds:
        out.append((name + '-dgrad', DG3, dims, 3, 'model', why))
    return out


def _pw(name, dims, why, kind='s16fwd1'):
    return [(name, [kind], dims, 1, 'model', why)]


def _wg(name, dims, expect, why, ksize=3):
    return [(name, ['s16wgrad' if ksize == 3 else 's16wgrad1'], dims, ksize, expect, why)]


GROUPS = [
    # FTE_PICK_WANT16=1: pick_tile takes the 128 x 128 tile for every N % 128 == 0 launch
    ('want1', {'FTE_PICK_WANT16': '1'},
     _conv('3x7x6x128', (3, 7, 6, 128, 128), 'M = 126: one tile shorter than BM, 7 of 8 XCDs idle; 46 pieces -> WCAP 48, KS 1 although K/64 is even')
     + _conv('6x7x7x128', (6, 7, 7, 128, 128), 'the tightest window (45 pieces, span 359 of 360) -> KS 2; second tile has 38 rows')
     + _conv('2x14x12x128', (2, 14, 12, 128, 128), '112x96 stage 3, ragged last tile')
     + _conv('1x28x24x128', (1, 28, 24, 128, 128), '112x96 stage 2, ragged last tile')
     + _conv('5x9x7x192', (5, 9, 7, 192, 128), 'three chunks, odd K-steps, H != W (the data gradient has N = 192: group want8)', kinds=('fwd',))
     + _conv('3x7x7x384', (3, 7, 7, 384, 128), 'six chunks at KS 2: chunk boundaries at both interval parities')
     + _conv('8x4x4x128', (8, 4, 4, 128, 128), '52 pieces > 48: forward on igemm16p<128,128>, data gradient on the two-stage per-tile kernel')
     + _conv('1x56x48x64to128', (1, 56, 48, 64, 128), '52 pieces, N % 128 == 0 -> igemm16p', kinds=('fwd',))
     + _pw('pw-k8', (2, 7, 6, 512, 128), 'K/64 = 8 -> three-stage ring')
     + _pw('pw-k6', (2, 7, 6, 384, 128), 'K/64 = 6, the edge -> three-stage ring')
     + _pw('pw-k5', (2, 7, 6, 320, 128), 'K/64 = 5 -> igemm16p')
     + _pw('pw-k4', (2, 7, 6, 256, 128), 'K/64 = 4, the edge -> igemm16p')
     + _pw('pw-k3', (2, 7, 6, 192, 128), 'K/64 = 3 -> two-stage per-tile kernel')
     + _pw('pw-k96', (2, 7, 6, 96, 128), 'a_KC % 64 != 0 -> not igemm16 at all')
     + _pw('pw-dgrad-k6', (2, 7, 6, 128, 384), 'data-gradient twin of the K/64 = 6 edge (N = cin = 128, K = cout = 384)', kind='s16dgrad1')),
    # N = 64: pick_tile's first candidate is 256 x 64; want must satisfy ceil(M / 256) * (N / 64) < want <= ceil(M / 128) * (N / 64)
    ('want2', {'FTE_PICK_WANT16': '2'},
     _conv('12x4x4x64', (12, 4, 4, 64, 64), 'M = 192, one tile spanning 12 images: an image boundary every 16 rows')
     + _conv('5x7x7x64to128', (5, 7, 7, 64, 128), 'one chunk forward (K/64 = 9, odd -> KS 1): no next-chunk prefetch; data gradient N = 64, one tile of 245 rows')
     + _pw('pw-n64-k8-m84', (2, 7, 6, 512, 64), 'M = 84 has one tile of either height: no value of the switch reaches the 128 x 64 forms (64 x 64 tile, not igemm16)')
     + _pw('pw-n64-k8', (4, 7, 6, 512, 64), 'the nearest shape that does: M = 168 -> the 128 x 64 three-stage ring')),
    ('want16', {'FTE_PICK_WANT16': '16'},
     _conv('1x56x56x64', (1, 56, 56, 64, 64), '55 pieces, one under the cap; last tile 64 rows')
     + _conv('1x56x48x64', (1, 56, 48, 64, 64), '112x96 stage 1')),
    ('want8', {'FTE_PICK_WANT16': '8'},
     _conv('5x9x7x192', (5, 9, 7, 192, 128), 'N = 192: three column tiles of the 256 x 64 window kernel, K = 9 x 128', kinds=('dgrad',))),
    ('default', {},
     _conv('800x7x6x128to256', (800, 7, 6, 128, 256), '264 tiles > 256 CUs under the natural plan: some blocks walk two tiles, two column tiles, non-square')
     + _wg('wg-30x30-cfg1', (1, 30, 30, 64, 128), 'plan', 'cfg 1: XCAP and slot table both exactly full')
     + _wg('wg-30x30-cfg0', (1, 30, 30, 32, 256), 'plan', 'cfg 0: XCAP and slot table both exactly full')
     + _wg('wg-31x31', (1, 31, 31, 64, 128), 'plan', 'w = 31 -> the 64 x 64 instantiation with XCAP 192')
     + _wg('wg-50x62', (1, 50, 62, 64, 64), 'plan', 'XCAP 192 exactly full, H != W')
     + _wg('wg-51x62', (1, 51, 62, 64, 64), 'refused', 'slot table exceeded')
     + _wg('wg-14x12', (3, 14, 12, 128, 128), 'plan', '112x96 stage 3')
     + _wg('wg-28x24', (2, 28, 24, 128, 128), 'plan', '112x96 stage 2')
     + _wg('wg-56x48', (1, 56, 48, 64, 64), 'plan', '112x96 stage 1')
     + _wg('wg-7x6', (4, 7, 6, 128, 128), 'refused', 'w < 7')
     + _wg('wg-6x9', (2, 6, 9, 64, 128), 'refused', 'h < 7')
     + _wg('wg-7x7-s1', (2, 7, 7, 128, 256), 'plan', 'smallest admitted image, four channel pairs, S lowered to 1')
     + _wg('wg-5x30x30-s8', (5, 30, 30, 64, 128), 'plan', '76 pieces -> S = 8: the S >= 8 block map, short last range')
     + _wg('wgp-4pieces', (1, 16, 16, 128, 128), 'plan', 'wgrad16p at exactly four pieces', ksize=1)
     + _wg('wgp-3pieces', (1, 16, 12, 128, 128), 'refused', 'three pieces', ksize=1)
     + _wg('wgp-189px', (3, 9, 7, 64, 128), 'refused', '189 pixels are three pieces (two whole and 61 rows): refused as well', ksize=1)
     + _wg('wgp-253px', (1, 23, 11, 64, 128), 'plan', 'the nearest admitted shape with a ragged last piece of 61 rows: 253 pixels, four pieces', ksize=1)),
    ('minp1', {'FTE_WGRAD16_MINP': '1'},
     _wg('wg-38x8x8-empty', (38, 8, 8, 64, 128), 'plan', '49 pieces, S = 48, kper = 2 pieces: ranges 25..47 are empty and must leave zero slabs')),
]
CUS = 256          # MI355X; the plans of wgrad16.hip depend on it


def want16(env):
    return int(env.get('FTE_PICK_WANT16', 120))


def minp(env):
    return int(env.get('FTE_WGRAD16_MINP', 8))


def worker_cases(cases):
    """the worker's case list: [kind, n, h, w, cin, cout, stride] per kind of every case, and the index range of each case in it"""
    flat, where = [], []
    for _, kinds, dims, _, _, _ in cases:
        where.append((len(flat), len(flat) + len(kinds)))
        flat += [[k] + list(dims) + [1] for k in kinds]
    return flat, where


def expected(case, env, cus=CUS):
    """-> ('symbol', str | None) for a conv case; ('plan', plan dict) / ('refused', None) for a filter gradient, from the model"""
    _, kinds, dims, ksize, expect, _ = case
    if kinds[0].startswith('s16wgrad'):
        p = W.wgrad16_plan(*dims, cus=cus, minp=minp(env)) if ksize == 3 else W.wgrad16p_plan(*dims, cus=cus)
        return ('plan', p) if p else ('refused', None)
    kind = 'fwd' if 'fwd' in kinds[0] else 'dgrad'
    return 'symbol', W.conv_launch(kind, *dims, ksize, want16=want16(env))[0]
