"""One rank's share of the sharded margin head next to the dense head, on ONE GPU, fp32, D = 512.

    python scripts/bench_sharded_head.py [--classes 85742,1000000] [--ranks 1,2,4,8] [--steps 10] [--repeats 7]

Sharded: what rank 0 of R runs per step without the collectives -- row / column norms, s = X W_r over the N = R * 512 gathered rows
and its C / R columns, fte_margin_shard_stats, fte_margin_shard_fwd_bwd (its all_stats block filled with the shard's own
statistics R times: the kernel's work does not depend on the values), colcoef, dW_r = X^T G + colcoef (.) W_r and
dX_part = G W_r^T + rowcoef_part (.) X.  Dense: the calls of loss.additive_margin_loss at n = 512 over all C classes.  The two run in
the same process in alternating windows (A B A B ...: HIP events around --steps back-to-back steps after warm-up); median and
min..max of --repeats windows each.  Per-rank FLOPs equal the dense head's (R x the rows, 1 / R of the columns), so the times are
printed side by side and no ratio is claimed.  Then each new kernel alone with its rate on the bytes it has to move (stats: s read
once; fwd_bwd: s read, G written), and the analytic wire bytes per step and rank: 2 N D 4 (features gathered, dX reduce-scattered) +
R 3 N 4 (statistics) against the D cpad 4 of the dense classifier gradient's all-reduce.
The multi-GPU step time is NOT measured here (one GPU has no wire) and is not projected."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_face_toolbox_amd import _lib, heads  # noqa: E402

NLOC, D = 512, 512
PRESET = (64.0, 0.5, 0.0)


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def timed_ab(fns, steps, repeats, warm=3):
    """the callables' windows alternating A B A B ...: -> [(median, min, max) us]"""
    for fn in fns:
        for _ in range(warm):
            fn()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            out[k].append(window(fn, steps))
    return [(float(np.median(o)), float(min(o)), float(max(o))) for o in out]


def run(C, R, steps, repeats):
    call, q = _lib.call, _lib.query
    st = torch.cuda.current_stream().cuda_stream
    f32, i32 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int32, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    cpad = (C + 127) // 128 * 128
    lo, hi = heads.shard_range(C, R, 0)
    c, ld, N = hi - lo, heads.shard_ld(C, R), R * NLOC
    wsb = max(q('fte_gemm_ws_bytes', NLOC, cpad, D), q('fte_gemm_ws_bytes', N, ld, D), 4096)
    ws = torch.empty(wsb // 4 + 1024, **f32)
    wsb = ws.numel() * 4
    # ---- dense, n = 512 over all C
    W = torch.randn(D, cpad, generator=g, **f32)
    W[:, C:] = 0
    x = torch.randn(NLOC, D, generator=g, **f32) * 4
    y = torch.randint(0, C, (NLOC,), generator=g, **i32)
    s, G, dW = torch.empty(NLOC, cpad, **f32), torch.empty(NLOC, cpad, **f32), torch.empty(D, cpad, **f32)
    xn, rc, rows, dx = torch.empty(NLOC, **f32), torch.empty(NLOC, **f32), torch.empty(NLOC, **f32), torch.empty(NLOC, D, **f32)
    wn, cc = torch.empty(cpad, **f32), torch.empty(cpad, **f32)

    def dense():
        call('fte_gemm_nn', x, W, None, s, NLOC, cpad, D, ws, wsb, st)
        call('fte_row_norms', x, xn, NLOC, D, D, st)
        call('fte_col_norms', W, wn, D, C, cpad, st)
        call('fte_margin_softmax_fwd_bwd', s, xn, wn, y, *PRESET, None, rows, G, rc, NLOC, C, cpad, 1.0 / NLOC, st)
        call('fte_asoftmax_colcoef', G, s, wn, cc, NLOC, C, cpad, st)
        call('fte_gemm_tn', x, G, dW, NLOC, cpad, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dW, W, None, cc, D, cpad, cpad, st)
        call('fte_gemm_nt', G, W, None, None, 0, None, dx, None, NLOC, cpad, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dx, x, rc, None, NLOC, D, D, st)

    # ---- rank 0 of R: N rows, its c columns
    Wr = torch.zeros(D, ld, **f32)
    Wr[:, :c] = W[:, lo:hi]
    X = torch.randn(N, D, generator=g, **f32) * 4
    Y = torch.randint(0, C, (N,), generator=g, **i32)
    sr, Gr, dWr = torch.empty(N, ld, **f32), torch.empty(N, ld, **f32), torch.empty(D, ld, **f32)
    xnr, rcr, rowsr, dXp = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, D, **f32)
    wnr, ccr = torch.empty(ld, **f32), torch.empty(ld, **f32)
    stats, all_stats = torch.empty(3, N, **f32), torch.empty(R, 3, N, **f32)

    def k_stats():
        call('fte_margin_shard_stats', sr, xnr, wnr, Y, lo, C, *PRESET, stats, N, c, ld, st)

    def k_grad():
        call('fte_margin_shard_fwd_bwd', sr, xnr, wnr, Y, lo, C, *PRESET, all_stats, R, None, rowsr, Gr, rcr, N, c, ld, 1.0 / N, st)

    def sharded():
        call('fte_row_norms', X, xnr, N, D, D, st)
        call('fte_col_norms', Wr, wnr, D, c, ld, st)
        call('fte_gemm_nn', X, Wr, None, sr, N, ld, D, ws, wsb, st)
        k_stats()
        k_grad()
        call('fte_asoftmax_colcoef', Gr, sr, wnr, ccr, N, c, ld, st)
        call('fte_gemm_tn', X, Gr, dWr, N, ld, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dWr, Wr, None, ccr, D, ld, ld, st)
        call('fte_gemm_nt', Gr, Wr, None, None, 0, None, dXp, None, N, ld, D, ws, wsb, st)
        call('fte_add_scaled_rows_cols', dXp, X, rcr, None, N, D, D, st)

    sharded()
    all_stats.copy_(stats.unsqueeze(0).expand(R, 3, N))
    td, ts = timed_ab([dense, sharded], steps, repeats)
    tk = timed_ab([k_stats, k_grad], steps, repeats)
    sbytes = N * ld * 4.0
    print('C=%d R=%d: rank 0 holds %d classes (ld %d), N = %d rows; dense n = %d, cpad %d; %d steps per window, median [min, max] of %d windows'
          % (C, R, c, ld, N, NLOC, cpad, steps, repeats))
    print('  dense head          %9.1f us [%.1f, %.1f]' % td)
    print("  one rank's share    %9.1f us [%.1f, %.1f]" % ts)
    print('  fte_margin_shard_stats   %8.1f us [%.1f, %.1f]  %.3f GB -> %.0f GB/s' % (tk[0] + (sbytes / 1e9, sbytes / tk[0][0] / 1e3)))
    print('  fte_margin_shard_fwd_bwd %8.1f us [%.1f, %.1f]  %.3f GB -> %.0f GB/s' % (tk[1] + (2 * sbytes / 1e9, 2 * sbytes / tk[1][0] / 1e3)))
    wire, dense_wire = 2.0 * N * D * 4 + R * 3.0 * N * 4, D * cpad * 4.0
    print('  wire bytes per step and rank (analytic): sharded %.2f MB, dense classifier gradient %.2f MB' % (wire / 1e6, dense_wire / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', default='85742,1000000')
    ap.add_argument('--ranks', default='1,2,4,8')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    a = ap.parse_args()
    print(_lib.version())
    for C in (int(v) for v in a.classes.split(',')):
        for R in (int(v) for v in a.ranks.split(',')):
            run(C, R, a.steps, a.repeats)
            torch.cuda.empty_cache()
    print('the multi-GPU step time is not measured on one GPU and is not projected')


if __name__ == '__main__':
    main()
