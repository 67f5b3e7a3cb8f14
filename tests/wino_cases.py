"""The case table of tests/test_gpu_wino_edges.py: shapes (n, h, w, cin, cout) of the stride-1 3x3 convolution under FTE_CONV_WINOGRAD, each
with the launcher classes (names of tests/test_wino_map_host.py CLASSES) it is in the table for.  test_wino_map_host.py proves with
tests/wino_map.py, at the MI355X's 256 CUs, that every case reaches its classes; the GPU module asserts the symbols that really ran.  The
forward product of a case is N = cout, K = cin; the data gradient runs on the SWAPPED pair (cin' = cout, cout' = cin: again N = cout,
K = cin -- the large channel counts stay on the N side, the reduction at K <= 512), and as given too where cin > cout."""

# products: every case runs forward, data gradient and filter gradient
MM_CASES = [
    ((5, 29, 27, 64, 1024), ['grp8', 'two_rounds', 'whole', 'two_tiles_per_block', 'k64', 'odd', 'ragged']),
    ((1, 6, 6, 64, 1024), ['grp8', 'half']),
    ((22, 31, 31, 64, 192), ['plain', 'two_rounds', 'whole', 'two_tiles_per_block', 'odd', 'wgrad_direct']),
    ((1, 9, 7, 64, 192), ['plain', 'half', 'n192', 'wgrad_direct']),
    ((6, 15, 13, 64, 384), ['plain', 'half', 'n384', 'wgrad_direct']),
    ((3, 9, 9, 64, 2048), ['plain', 'half', 'n2048']),
    ((5, 29, 27, 64, 512), ['whole', 'one_round', 'empty_blocks', 'odd', 'ragged', 'n512']),
    ((66, 31, 29, 64, 64), ['whole', 'n64', 'odd', 'ragged', 'k64']),
    ((33, 31, 29, 64, 128), ['whole', 'n128', 'odd', 'ragged', 'k64']),
    ((17, 29, 27, 64, 256), ['whole', 'n256', 'k64', 'odd', 'ragged']),
    ((34, 31, 29, 64, 64), ['half', 'tiles128']),
    ((35, 31, 29, 64, 64), ['whole', 'smallest_whole', 'empty_blocks']),
    ((1, 2, 2, 64, 64), ['half', 'one_tile', 'm_lt_64', 'tw1', 'empty_shares255']),
    ((1, 3, 2, 128, 64), ['half', 'two_tiles', 'm_lt_64', 'cin_gt_cout', 'tw1']),
    ((1, 2, 3, 64, 128), ['half', 'two_tiles', 'm_lt_64', 'tw2']),
    ((1, 4, 4, 64, 64), ['half', 'm_lt_64', 'tw2', 'empty_shares255']),
    ((2, 5, 3, 64, 64), ['half', 'm_lt_64', 'odd', 'tw2']),
    ((2, 7, 5, 512, 64), ['half', 'cin_gt_cout', 'k512', 'odd']),
    ((2, 7, 5, 512, 192), ['plain', 'half', 'cin_gt_cout', 'k512', 'odd', 'wgrad_direct']),
]

# filter gradient only
WGRAD_CASES = [
    ((3, 9, 7, 64, 512), ['p8']),
    ((3, 9, 7, 512, 64), ['p8', 'cin_gt_cout']),
    ((2, 7, 7, 256, 512), ['p32']),
    ((1, 6, 6, 512, 1024), ['p128']),
    ((1, 6, 6, 1024, 1024), ['p256']),
    ((9, 6, 2, 64, 64), ['tw1']),
    ((9, 2, 6, 64, 64), ['tw3', 'step_spans_images']),
    ((5, 4, 3, 128, 64), ['tw2', 'cin_gt_cout', 'step_spans_images']),
    ((4, 5, 5, 64, 128), ['tw3']),
    ((19, 2, 2, 64, 64), ['tw1', 'step_spans_images', 'carry_twice']),
    ((11, 3, 3, 64, 64), ['tw2', 'step_spans_images', 'carry_twice']),
    ((1, 4, 4, 64, 64), ['empty_shares255']),
]

# no split count (wino_wgrad_splits = 0): forward and data gradient Winograd, the filter gradient direct
NOSPLIT_CASES = [
    ((2, 9, 7, 192, 64), ['wgrad_direct', 'p_not_dividing_256']),
    ((1, 5, 5, 2048, 1024), ['wgrad_direct', 'p_above_256']),
]

# fte_conv3x3_fwd_keep + fte_conv3x3_wgrad_kept against the self-contained calls (256- against 512-thread tile transform)
KEPT_CASES = [(1, 3, 2, 128, 64), (3, 9, 7, 64, 128), (5, 29, 27, 64, 512)]
