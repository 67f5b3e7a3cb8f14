"""Planning for SphereNet (nets/sphere.py): what is decided before a buffer exists or a kernel runs.  Plain functions of the conv
list, the shard size, the options record (sphere.read_options) and `algo`, a callable with the signature of
_lib.query('fte_conv3x3_algo', n, h, w, cin, cout, stride, op) (op 0: forward, 2: filter gradient; 1 = Winograd); no device tensor is
made here and nothing of libfte.so is called, so a plan can be made and compared on any machine.

  wino_plan     which layers keep a V pack for their filter gradient, which residual blocks are lean
  split_point   the part-shard split of the forward walk
  StageRing     the dz / skip-gradient buffers of one stage and their rotation in the backward walk"""
import math


def wino_plan(convs, n, algo, options, s16):
    """-> (keep, lean), one flag per layer.  keep[l]: the forward pass leaves V = B^T d B of layer l's input for the layer's filter
    gradient (Winograd forward AND filter gradient at this shard size; never the stem, never under bf16 storage, FTE_WINO_KEEP=0: none).
    lean[l], l = a block's second conv: both convs of the block keep a pack, so the first conv's y need not be written."""
    keep = [False] * len(convs)
    if not s16 and options.wino_keep:
        for l, c in enumerate(convs):
            keep[l] = l > 0 and c.stride == 1 and algo(n, c.hin, c.win, c.cin, c.cout, 1, 0) == 1 \
                and algo(n, c.hin, c.win, c.cin, c.cout, 1, 2) == 1
    return keep, [c.second == 1 and keep[l] and keep[l - 1] for l, c in enumerate(convs)]


def split_point(convs, kept, n, algo, options):
    """Size of the first part of the forward walk as two part shards, or 0 (one chain).  The first part must end on a whole 64-tile row
    block of every kept V pack (the second part's pack is the rest of the shard's): the split point is the multiple of that granule
    nearest below the middle (112 x 112: 64 images), and both parts must plan the same algorithm per layer as the whole shard.
    FTE_FWD_HALVES=0 / 1 forces it off / on where it is possible, otherwise it is on from FTE_FWD_HALVES_MIN images;
    FTE_FWD_SPLIT=<images> moves the split point (exploration)."""
    if options.fwd_halves == 'off' or n < 2:
        return 0
    gran = 1
    for c, k in zip(convs, kept):
        if k:
            gran = max(gran, 64 // math.gcd(64, c.tiles))      # (powers of two: the largest is their common multiple)
    a = (n // 2) // gran * gran if options.fwd_split is None else options.fwd_split
    ok, any_w = 0 < a < n, False
    for l, c in enumerate(convs):
        if l == 0 or c.stride != 1 or not ok:
            continue
        whole, first, rest = [algo(m, c.hin, c.win, c.cin, c.cout, 1, 0) for m in (n, a, n - a)]
        any_w = any_w or whole == 1
        ok = first == whole and rest == whole and not (kept[l] and (a * c.tiles) % 64)
    if not (ok and any_w):
        return 0
    return a if options.fwd_halves == 'forced' or n >= options.fwd_halves_min else 0


class StageRing(object):
    """The buffers one stage's backward walk writes: `dz` (2 or 3, FTE_DZ_BUFFERS) and the two skip-path gradients `raw`, in the
    precision the mode stores them in (bf16 under bf16 storage, fp32 otherwise).  `dz16`: the bf16 copies that ride along with `dz`
    when the convs read copies (under bf16 storage `dz` itself); `f32`: under bf16 storage the last stage's one fp32 (dz, raw) pair
    that the dense layer's backward epilogue writes, else None.
    reset() (the walk enters the stage) and advance() (next layer of the stage) hand out the buffers the next data gradient writes:
    never the current dz, which that launch and the layer's filter gradient read, nor the current skip gradient; the skip buffer
    becomes the current one only when the layer has a shortcut to feed (take_raw)."""
    __slots__ = ('dz', 'raw', 'dz16', 'f32', 'i', 'j', 'k')       # i: dz handed out last; j: current skip gradient; k: the one on offer

    def __init__(self, dz, raw, dz16=None, f32=None):
        self.dz, self.raw, self.dz16, self.f32 = dz, raw, dz16, f32
        self.i = self.j = self.k = 0

    def reset(self):
        self.i = self.j = self.k = 0
        return self.dz[0], self.raw[0]

    def advance(self):
        self.i, self.k = (self.i + 1) % len(self.dz), self.j ^ 1
        return self.dz[self.i], self.raw[self.k]

    def take_raw(self):
        self.j = self.k

    def copy16(self):
        """the bf16 copy of the dz buffer handed out last"""
        return self.dz16[self.i]
