"""Host-only (numpy) case tables, float64 references and host mirrors of the branch predicates for the dense products (fte_gemm_nn,
fte_gemm_nn_act, fte_gemm_nt, fte_gemm_tn) and the first conv (fte_conv3x3_first_*).  tests/test_gpu_dense_edges.py and
tests/test_gpu_first_conv_edges.py run the cases on the GPU; tests/test_dense_cases_host.py proves on the CPU that every case sits on the
branch it names: the plan columns against the planner header (tests/conv_plan_dump.cpp), everything else against the mirrors below.

The mirrors follow the launchers as written in csrc/api.hip (the three products' GEMM dimensions), csrc/igemm.hip (the `kmf` condition of
the m-contiguous A gather) and csrc/kernels.hip (k_reduce_rows2, k_conv_first_fwd, k_conv_first_wgrad, k_conv_first_wgrad_blocks); they
are written from those conditions, not copied from them, and the plan columns are stated for 256 CUs with every FTE_* switch unset."""
import collections

import numpy as np

from oracle import ops

# tile ids of csrc/conv_plan.h
T128, T256x64, T128x64, T64, T192 = 0, 1, 2, 3, 4
TILE_DIMS = {T128: (128, 128), T256x64: (256, 64), T128x64: (128, 64), T64: (64, 64), T192: (192, 64)}
REDUCE_SCRATCH_FLOATS = 1 << 18          # conv_plan.h (the host test reads the header to confirm it)
SCRATCH_BYTES = 4 * REDUCE_SCRATCH_FLOATS
U = 2.0 ** -24                           # unit roundoff of fp32


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def up(a, b):
    return -(-a // b)


def align_up(v):
    return (v + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------------------------------
# dense products
# ------------------------------------------------------------------------------------------------------------------------
# product, (m, n, k) as the API takes them, the plan at 256 CUs in the fp32 mode (tile, splits, kchunk), and the facts the case is in the
# table for (keys of dense_facts below)
DenseCase = collections.namedtuple('DenseCase', 'name product m n k tile splits kchunk facts')
DUMP_COLUMN = {'nn': 0, 'nt': 1, 'tn': 2}          # position of a product in a `dense` line of conv_plan_dump

NN_CASES = [
    DenseCase('nn_256x64', 'nn', 19500, 320, 64, T256x64, 1, 64, dict(tiles=385, row_tiles=77, last_tile_rows=44)),
    DenseCase('nn_128x64', 'nn', 16300, 192, 64, T128x64, 1, 64, dict(tiles=384, row_tiles=128, last_tile_rows=44)),
    DenseCase('nn_split4_bias_act', 'nn', 130, 320, 1056, T64, 4, 288, dict(last_range=192, last_tile_rows=2, reduce_bias='rows1', reduce_plain='slabs64')),
    DenseCase('nn_split3_one_row', 'nn', 257, 256, 800, T64, 3, 288, dict(last_range=224, row_tiles=5, last_tile_rows=1, reduce_plain='slabs64')),
    DenseCase('nn_split32_short', 'nn', 9, 64, 8192, T64, 32, 256, dict(row_tiles=1, last_tile_rows=9, last_range=256, reduce_plain='rows1')),
    DenseCase('nn_unsplit_act', 'nn', 33, 64, 64, T64, 1, 64, dict(row_tiles=1, last_tile_rows=33)),
]
NT_CASES = [
    DenseCase('nt_256x64', 'nt', 300, 64, 12352, T256x64, 1, 64, dict(tiles=386, row_tiles=2, last_tile_rows=44)),
    DenseCase('nt_split2', 'nt', 61, 640, 1024, T64, 2, 320, dict(last_range=320, row_tiles=1, last_tile_rows=61, reduce_plain='slabs64')),
    DenseCase('nt_small', 'nt', 33, 64, 64, T64, 1, 64, dict(row_tiles=1, last_tile_rows=33)),
]
TN_CASES = [
    DenseCase('tn_slow_gather', 'tn', 1000, 64, 100, T128x64, 3, 352, dict(last_range=296, row_tiles=1, last_tile_rows=100, kmf=[False, False, False], reduce_plain='slabs64')),
    DenseCase('tn_fast_then_slow', 'tn', 2050, 64, 64, T128x64, 8, 288, dict(last_range=34, kmf=[True] * 7 + [False], reduce_plain='slabs64')),
    DenseCase('tn_ragged_rows', 'tn', 515, 128, 2080, T128x64, 2, 288, dict(last_range=227, row_tiles=17, last_tile_rows=32, kmf=[True, False], reduce_plain='slabs64')),
    DenseCase('tn_short', 'tn', 5, 64, 68, T128x64, 1, 32, dict(last_range=5, row_tiles=1, last_tile_rows=68, kmf=[False])),
]
DENSE_CASES = NN_CASES + NT_CASES + TN_CASES
# the fused PReLU backward of fte_gemm_nt runs unsplit on pick_tile's tile whatever the reduction length: (tile, partial rows of dalpha)
NT_FUSED = {'nt_256x64': (T256x64, 2), 'nt_split2': (T64, 1), 'nt_small': (T64, 1)}
BF16_CASES = ['nn_256x64', 'nn_split4_bias_act', 'nt_256x64', 'tn_slow_gather']          # run again with bf16 MFMA operands
# (tile, splits) of those cases in the bf16 plan (pick_tile asks for fewer tiles there: the table's cases happen to keep their plan)
BF16_PLANS = {'nn_256x64': (T256x64, 1), 'nn_split4_bias_act': (T64, 4), 'nt_256x64': (T256x64, 1), 'tn_slow_gather': (T128x64, 3)}


def gemm_dims(c):
    """(rows, cols, reduction) of the GEMM behind a product (api.hip)"""
    return {'nn': (c.m, c.n, c.k), 'nt': (c.m, c.k, c.n), 'tn': (c.k, c.n, c.m)}[c.product]


def split_ranges(red, splits, kchunk):
    return [(s * kchunk, min(red, (s + 1) * kchunk)) for s in range(splits)]


def kmf(a_kc, rows, kbeg, kend):
    """the fast gather of the m-contiguous A operand (igemm_kernel, AL_KM, fp32 operands, a dense product: one pixel per row)"""
    return a_kc % 32 == 0 and rows % 32 == 0 and (kend - kbeg) % 32 == 0 and kend > kbeg


def reduce_rows2_plan(rows, cols, fold=1, scratch=True, bias=False, act=False, scale_one=True, two=False, aligned=True):
    """k_reduce_rows2's choice -> (kernel plan, row splits): 'slabs64' / 'slabs16' (reduce_slabs_kernel<QB>), 'q1' / 'q2'
    (reduce_rows_q_kernel in one launch / two passes), 'rows1' / 'rows2' (reduce_rows_kernel)"""
    rows, cols = rows * fold, cols // fold
    if not act and not two and not bias and scale_one and 2 <= rows < (1 << 20) and cols >= 4096 and cols % 4 == 0 and aligned:
        quads = cols // 4
        return ('slabs64' if quads // 64 >= 1024 or rows < 32 else 'slabs16'), 1
    nz = 2 if two else 1
    if not act and scratch and not bias and scale_one and rows >= 32 and cols % 4 == 0 and cols <= 1024 and aligned:
        quads = cols // 4
        qb_ = 64 if quads >= 64 else 16
        lanes = 256 // qb_
        qb = up(quads, qb_)
        rs = min(1024 // (qb * nz), rows // (8 * lanes))
        if rs * cols * nz > REDUCE_SCRATCH_FLOATS:
            rs = REDUCE_SCRATCH_FLOATS // (cols * nz)
        if rs < 1 or rows < 256:
            rs = 1
        rs = up(rows, up(rows, rs))
        return ('q1', 1) if rs == 1 else ('q2', rs)
    cb = up(cols, 64)
    rs = 1
    if scratch and cb < 512 and rows >= 64:
        while rs * rs < rows:
            rs += 1
        rs = max(rs, 256 // cb)
        rs = min(rs, 1024 // cb, rows // 16)
        if rs * cols * nz > REDUCE_SCRATCH_FLOATS:
            rs = REDUCE_SCRATCH_FLOATS // (cols * nz)
        rs = max(rs, 1)
    if rs == 1:
        return 'rows1', 1
    return 'rows2', up(rows, up(rows, rs))


def dense_facts(c):
    rows, cols, red = gemm_dims(c)
    bm, bn = TILE_DIMS[c.tile]
    ranges = split_ranges(red, c.splits, c.kchunk)
    f = dict(row_tiles=up(rows, bm), tiles=up(rows, bm) * (cols // bn), last_tile_rows=rows - (up(rows, bm) - 1) * bm,
             last_range=ranges[-1][1] - ranges[-1][0])
    if c.product == 'tn':
        f['kmf'] = [kmf(c.k, rows, a, b) for a, b in ranges]
    if c.splits > 1:          # launch_dense: the slabs go through k_reduce_rows WITHOUT scratch
        f['reduce_plain'] = reduce_rows2_plan(c.splits, rows * cols, scratch=False)[0]
        f['reduce_bias'] = reduce_rows2_plan(c.splits, rows * cols, scratch=False, bias=True)[0]
    return f


def dense_need_bytes(c):
    """workspace bytes the product's own launch touches (the query answers the maximum over the products of a layer)"""
    rows, cols, _ = gemm_dims(c)
    return c.splits * rows * cols * 4 if c.splits > 1 else 0


def nt_fused_need_bytes(c):
    tile, part_rows = NT_FUSED[c.name]
    return align_up(part_rows * c.k * 4) + SCRATCH_BYTES


def nt_dalpha_reduce_plan(c, amod):
    return reduce_rows2_plan(NT_FUSED[c.name][1], c.k, fold=c.k // amod, scratch=True)


def gemm_ws_bytes(m, n, k, slabs):
    """fte_gemm_ws_bytes from the three products' slab bytes (a `dense` line of the dump): the maximum over nn, nt, the dalpha partial
    rows of the fused nt, and tn -- each where its divisibility rule holds"""
    need = 0
    if n % 64 == 0:
        need = max(need, slabs[0], slabs[2])
    if k % 64 == 0:
        need = max(need, slabs[1], align_up(up(m, 64) * k * 4) + SCRATCH_BYTES)
    return need


def dense_inputs(c, seed=0):
    """float32 operands without heavy cancellation in the products: standard normal activations / gradients, weights scaled by 0.05"""
    r = np.random.default_rng(1000 + seed + 7 * DENSE_CASES.index(c))
    if c.product == 'nn':
        return dict(x=f32(r.standard_normal((c.m, c.k))), w=f32(r.standard_normal((c.k, c.n)) * 0.05), b=f32(r.standard_normal(c.n)))
    if c.product == 'nt':
        zp = f32(r.standard_normal((c.m, c.k)))
        zp[0, :4] = 0.0                       # the z == 0 sub-gradient
        zp[c.m - 1, c.k - 1] = 0.0            # ... in the last row tile's last column too
        return dict(dy=f32(r.standard_normal((c.m, c.n))), w=f32(r.standard_normal((c.k, c.n)) * 0.05), zp=zp,
                    al=f32(0.25 + 0.1 * r.standard_normal(c.k)))
    return dict(x=f32(r.standard_normal((c.m, c.k))), dy=f32(r.standard_normal((c.m, c.n))))


def act_ref(lin, act):
    return lin if act == 0 else (np.maximum(lin, 0.0) if act == 1 else 1.0 / (1.0 + np.exp(-lin)))


def sum_bound(terms, sum_abs):
    """order-free first-order bound of an fp32 sum of `terms` fp32 products: every product passes one rounding of its own and at most
    terms - 1 additions, whatever the order or the grouping (tiles, splits, slabs); + 3 for the epilogue's roundings and the second-order
    terms (the form tests/test_gpu_iresnet_kernels.py uses)"""
    return (terms + 3) * U * sum_abs


def dalpha_bound(dy, w, zp, amod):
    """dalpha[a] = sum over rows i and columns c = a mod amod with zp <= 0 of zp[i, c] * (sum_j dy[i, j] w[c, j]): a leaf product
    dy w zp passes at most n roundings inside the dot product, one for the multiplication by zp and R - 1 additions of the outer sum
    (R = m * k / amod terms) -> (n + R + 3) * 2^-24 * sum |dy| |w| |zp|"""
    m, n = dy.shape
    k = w.shape[0]
    gabs = np.abs(dy.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    zneg = np.where(zp <= 0, np.abs(zp.astype(np.float64)), 0.0)
    sabs = (gabs * zneg).reshape(m, k // amod, amod).sum(axis=(0, 1))
    return sum_bound(n + m * (k // amod), sabs)


# ------------------------------------------------------------------------------------------------------------------------
# first conv
# ------------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout, stride)
FIRST_FWD_CASES = [
    (2, 3, 32, 1, 64, 1),        # width exactly one 32-pixel group
    (1, 5, 33, 3, 64, 1),        # second group with one valid pixel; cin = 3 at stride 1
    (1, 2, 130, 3, 32, 2),       # three groups, even sizes at stride 2 (pads 0 / 1)
    (2, 7, 9, 1, 64, 2),         # odd sizes at stride 2 (pads 1 / 1)
    (1, 1, 1, 3, 64, 1),         # a single pixel: every tap but the centre is padding
    (1, 1, 1, 1, 32, 2),
    (1, 3, 112, 3, 64, 1),       # four groups per row, fewer waves' worth of rows than a block
    (2, 6, 9, 3, 64, 2),         # even height, odd width at stride 2: the row pad (0) differs from the column pad (1)
    (1, 1, 17, 3, 32, 1),        # filter gradient: one wave with three trips, the last with one valid pixel
]
FIRST_S16_FWD = FIRST_FWD_CASES[:4]
FIRST_COMBO_CASE = (2, 7, 9, 1, 64, 2)
FIRST_WGRAD_BIG = [
    (3, 112, 112, 3, 64, 1),     # 74 partial rows, six blocks without a row, 1728 columns: reduce_rows_kernel in two passes
    (3, 112, 112, 3, 32, 1),     # 74 partial rows of 864 columns: reduce_rows_q_kernel in one launch
    (11, 112, 112, 1, 32, 1),    # 270 partial rows of 288 columns: reduce_rows_q_kernel in two passes
]
FIRST_WGRAD_CAP = (21, 224, 224, 1, 32, 1)          # 1.05 M output pixels: the block count at its cap, as in every headline step
FIRST_WGRAD_CASES = FIRST_FWD_CASES + FIRST_WGRAD_BIG + [FIRST_WGRAD_CAP]
FIRST_S16_WGRAD = [(1, 5, 33, 3, 64, 1), (2, 6, 9, 3, 64, 2), (3, 112, 112, 3, 32, 1)]
FIRST_WGRAD_BLOCK_CAP = 2048


def same_pads(size, stride):
    """(output size, padding in front) of a 3-wide SAME window"""
    out = up(size, stride)
    return out, max((out - 1) * stride + 3 - size, 0) // 2


def first_fwd_geometry(case):
    n, h, w, cin, cout, stride = case
    (ho, pt), (wo, pl) = same_pads(h, stride), same_pads(w, stride)
    gpr = up(wo, 32)
    ngrp = n * ho * gpr
    blocks = min(4096, up(ngrp, 4))
    return dict(ho=ho, wo=wo, pt=pt, pl=pl, groups_per_row=gpr, groups=ngrp, blocks=blocks, last_group_pixels=wo - (gpr - 1) * 32,
                idle_waves=max(0, 4 * blocks - ngrp))


def first_wgrad_blocks(npix):
    return min(FIRST_WGRAD_BLOCK_CAP, max(1, up(npix, 512)))


def first_wgrad_geometry(case):
    """blocks, output rows per block, trips per output row (four pixel pairs each), and over all blocks: the trip counts of the waves,
    blocks / waves without a row, the valid pixels of a row's last trip, the plan of the partial rows' reduction"""
    n, h, w, cin, cout, stride = case
    (ho, pt), (wo, pl) = same_pads(h, stride), same_pads(w, stride)
    blocks = first_wgrad_blocks(n * ho * wo)
    nrows = n * ho
    rpb = up(nrows, blocks)
    tpr = up(wo, 8)
    trips, empty, idle = set(), 0, 0
    for b in range(blocks):
        r0, r1 = b * rpb, min(nrows, (b + 1) * rpb)
        if r1 <= r0:
            empty += 1
            continue
        for wv in range(4):
            my = (r1 - r0 - wv + 3) // 4 if r1 > r0 + wv else 0
            trips.add(my * tpr)
            idle += my == 0
    return dict(ho=ho, wo=wo, pt=pt, pl=pl, blocks=blocks, rows_per_block=rpb, trips_per_row=tpr, wave_trips=trips, empty_blocks=empty,
                idle_waves=idle, last_trip_pixels=wo - (tpr - 1) * 8, cols=9 * cin * cout,
                reduce=reduce_rows2_plan(blocks, 9 * cin * cout, scratch=True))


def first_wgrad_ws_bytes(case):
    n, h, w, cin, cout, stride = case
    g = first_wgrad_geometry(case)
    return align_up(g['blocks'] * 9 * cin * cout * 4) + SCRATCH_BYTES


def first_inputs(case, seed=0):
    """images in [-1, 1], filters scaled by 0.2, a quarter of the PReLU slopes negative; where the image is larger than one window the
    3 x 3 corner of image 0 is zero, so that output pixel (0, 0) is exactly zero without a bias (the z == 0 side of the PReLU)"""
    n, h, w, cin, cout, stride = case
    r = np.random.default_rng(2000 + seed + sum(v * 31 ** i for i, v in enumerate(case)) % 100000)
    x = f32(r.uniform(-1, 1, (n, h, w, cin)))
    if h * w > 9:
        x[0, :3, :3, :] = 0.0
    al = f32(0.25 + 0.1 * r.standard_normal(cout))
    al[::4] = -al[::4]
    return dict(x=x, w=f32(r.standard_normal((3, 3, cin, cout)) * 0.2), b=f32(r.standard_normal(cout)), al=al)


def first_dz(case, seed=0, bf16_exact=False):
    n, h, w, cin, cout, stride = case
    r = np.random.default_rng(3000 + seed)
    dz = r.standard_normal((n, same_pads(h, stride)[0], same_pads(w, stride)[0], cout), dtype=np.float32)
    return ops.bf16_round(dz) if bf16_exact else dz


def first_wgrad_ref(x, dz, stride, block=8):
    """float64 filter gradient and the sum of |term| of every element, image block by image block"""
    cin, cout = x.shape[3], dz.shape[3]
    wz = np.zeros((3, 3, cin, cout))
    ref, sabs = np.zeros_like(wz), np.zeros_like(wz)
    for i in range(0, x.shape[0], block):
        xb, db = x[i:i + block].astype(np.float64), dz[i:i + block].astype(np.float64)
        ref += ops.conv2d_bwd(xb, wz, db, stride, need_dx=False)[1]
        sabs += ops.conv2d_bwd(np.abs(xb), wz, np.abs(db), stride, need_dx=False)[1]
    return ref, sabs
