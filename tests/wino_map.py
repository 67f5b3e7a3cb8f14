"""The Winograd launchers' arithmetic (csrc/wino.hip: wino_geom, wino_mm, wino_wgrad_splits, the kernels' id -> block decode) restated in
Python.  It only says WHICH branch a shape reaches -- block order, kernel form, rounds, empty blocks, filter-gradient shares -- so that the
tests can pin a case to the class it is there for; it never checks a value.  No GPU, no torch."""


def geom(n, h, w):
    """-> M (2x2 output tiles), MB (64-tile row blocks), th, tw (tiles per image column / row)"""
    th, tw = (h + 1) // 2, (w + 1) // 2
    M = n * th * tw
    return M, (M + 63) // 64, th, tw


def launch_cus(multi_processor_count):
    """resident blocks of a whole-tile launch: the device's CUs rounded down to a multiple of 8 (a block keeps its XCD every round)"""
    return multi_processor_count // 8 * 8 if multi_processor_count > 8 else 8


def _order(MB, N):
    NB = N // 64
    NBX = NB if NB < 2 else 2
    GRP = NB // NBX
    if NB % NBX or 8 % GRP:
        return NB, NBX, 0, MB * NB
    C = 8 // GRP
    return NB, NBX, GRP, 8 * ((MB + C - 1) // C) * NBX


def decode(vid, MB, N):
    """virtual block id -> (mb, nb), or None for an id without a row block (the kernel's decode(), the launcher's valid())"""
    NB, NBX, GRP, _ = _order(MB, N)
    if GRP > 0:
        xcd, slot = vid & 7, vid >> 3
        grp, cls, C = xcd % GRP, xcd // GRP, 8 // GRP
        mb, nb = (slot // NBX) * C + cls, grp * NBX + slot % NBX
    else:
        mb, nb = vid // NB, vid % NB
    return (mb, nb) if mb < MB else None


def mm_plan(MB, N, cus, epi=0):
    """wino_mm()'s plan for MB row blocks x N output channels on a device of `cus` CUs (multi_processor_count).  epi: 0 forward, 1 data
    gradient.  Keys: order ('plain' or GRP), nvirt, grid, rounds, last_valid (valid ids of the last round), symbols (the launches, in
    order), max_tiles (most tiles one resident block takes), empty_blocks (blocks of the grid without a valid id), tiles (MB * NB)."""
    cus = launch_cus(cus)
    NB, NBX, GRP, nvirt = _order(MB, N)
    grid = (nvirt + 7) // 8 * 8 if nvirt < cus else cus
    rounds = (nvirt + grid - 1) // grid
    last = grid * (rounds - 1)
    L = sum(1 for v in range(last, nvirt) if decode(v, MB, N) is not None)
    tail_base = last if (L > 0 and 2 * L <= cus and rounds == 1) else nvirt
    symbols, max_tiles, empty = [], 0, 0
    if tail_base > 0:
        symbols.append('wino_mm_kernel<%d,2>' % epi)
        per_block = [sum(1 for v in range(b, tail_base, grid) if decode(v, MB, N) is not None) for b in range(grid)]
        max_tiles, empty = max(per_block), sum(1 for c in per_block if c == 0)
    if tail_base < nvirt:
        symbols.append('wino_mm_kernel<%d,1>' % epi)
        max_tiles = max(max_tiles, 1)
    return dict(order=GRP if GRP else 'plain', nvirt=nvirt, grid=grid, rounds=rounds, last_valid=L, symbols=symbols, max_tiles=max_tiles,
                empty_blocks=empty, tiles=MB * NB)


def wgrad_splits(cin, cout):
    """wino_wgrad_splits: shares of the tiles per (64 cin x 64 cout) block of the filter gradient; 0 = no Winograd filter gradient"""
    if cin % 64 or cout % 64:
        return 0
    P = (cin // 64) * (cout // 64)
    return 0 if (P > 256 or 256 % P) else 256 // P


def wgrad_shares(MB, S):
    """row blocks of each of the S shares (the kernel's mb0 / mb1)"""
    return [(s + 1) * MB // S - s * MB // S for s in range(S)]


def block_of(pixel, channel, n, h, w):
    """(n, y, x) of an output element and its channel -> the (mb, nb) of the product block that writes it"""
    _, _, th, tw = geom(n, h, w)
    i, y, x = pixel
    return ((i * th + y // 2) * tw + x // 2) // 64, channel // 64
