"""The case table of tests/test_gpu_pw16_edges.py: 1x1 / stride-1 convolutions (M pixels, K -> N channels) under bf16 storage through
fte_conv2d_bn_fwd, each with the classes (names of tests/test_pw16_map_host.py CLASSES) it is in the table for.  test_pw16_map_host.py
proves with tests/pw16_map.py that every case reaches its classes; the GPU module asserts the symbol that really ran.  Every case runs
plain (PRO = 0) and folded (PRO = 1: the BN in front of the conv in the loader, y side-stored)."""

# (M, K, N), classes -- the default environment: run in-process
CASES = [
    ((32, 64, 128), ['k64_nb128', 'one_tile', 'idle7', 'dead7', 'nct1', 'no_tail']),
    ((35, 64, 192), ['k64_nb64', 'nct3', 'tail3']),
    ((36, 256, 64), ['k256_nb64_w8', 'nct1', 'tail4']),
    ((805, 64, 512), ['k64_nb256', 'nct2', 'nrb4', 'dead_blocks', 'idle_waves', 'tail5', 'm_not_32']),
    ((805, 128, 192), ['k128_nb64', 'nct3', 'tail5', 'm_not_32']),
    ((805, 128, 384), ['k128_nb128', 'nct3', 'tail5', 'm_not_32']),
    ((805, 256, 320), ['k256_nb64_w8', 'nct5', 'tail5', 'm_not_32']),
    ((2048, 128, 64), ['k128_nb64', 'nct1', 'nrb8', 'no_dead', 'no_idle', 'no_tail', 'one_tile_per_wave']),
    ((3256, 64, 256), ['k64_nb256', 'nct1', 'nrb13', 'two_rb_per_xcd', 'dead3']),
    ((16422, 256, 512), ['k256_nb64_w8', 'nct8', 'nrb32_capped', 'tiles_2_3', 'tail6', 'm_not_32']),
    ((66049, 128, 256), ['k128_nb128', 'nct2', 'nrb128_capped', 'tiles_2_3', 'tail1', 'm_not_32']),
]

# below pw16_plan's floor of 32 rows: the tile kernels run, no pw16 symbol, no fold; results still right
BELOW_FLOOR = (31, 64, 128)

# (M, K, N), environment, classes -- the hooks are read once per process: these go through tests/tile_worker.py
HOOKED = [
    ((10248, 64, 64), {'FTE_PW16_BLOCKS': '8'}, ['k64_nb64', 'nct1', 'nrb8', 'tiles_5_6', 'tail8']),
    ((10248, 128, 256), {'FTE_PW16_BLOCKS': '8'}, ['k128_nb128', 'nct2', 'nrb4', 'tiles_10_11', 'tail8']),
    ((131406, 64, 64), {'FTE_PW16_BLOCKS': '100000'}, ['k64_nb64', 'nct1', 'nrb512_capped', 'tiles_1_2', 'tail14']),
    ((805, 256, 128), {'FTE_PW16_K256': '0'}, ['k256_nb128_w4', 'nct1', 'tail5']),
    ((805, 256, 192), {'FTE_PW16_K256': '0'}, ['k256_nb64_w4', 'nct3', 'tail5']),
]

# hard statistics (plain form, default environment): one column tile | three column tiles, >= 3 tiles per wave, ragged tail
HARD_STATS = [
    ((66049, 64, 64), ['nct1', 'tiles_1_2', 'tail1']),
    ((66049, 64, 192), ['nct3', 'tiles_3_4', 'tail1']),
]


def hooks(env):
    """environment of a case -> the keyword arguments of pw16_map.plan / launch"""
    return dict(blocks=int(env.get('FTE_PW16_BLOCKS', 256)), k256=int(env.get('FTE_PW16_K256', 1)))
