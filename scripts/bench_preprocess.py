"""The loader's three GPU transforms on the same slots, for a kernel trace: fte_preprocess_u8, fte_preprocess_u8_aug (every image with
all three colour bits set: brightness, hue and saturation) and fte_preprocess_u8_geo (both geometric bits as well: a zoom to
--zoom x --zoom, default 56, and a random row of the affine table; the two older entries ignore those words) on N slots of
src x src x 3 decoded pixels -> 128 x 128 -> crop 112 x 112.

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_preprocess.py [--n 512] [--src 250] [--reps 20]

Prints the bytes one launch moves (slot bytes read + float32 crop written) and, from HIP events, the mean time per launch; the
kernel times proper are the trace's."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--src', type=int, default=250)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--zoom', type=int, default=56, help='th = tw of the zoom in every header')
    a = ap.parse_args()
    import torch
    from tf_face_toolbox_amd import _lib
    from tf_face_toolbox_amd._decode_worker import HEADER_BYTES
    from tf_face_toolbox_amd.preprocessing import AFFINE, AFFINE_TABLE, ZOOM
    rng = np.random.default_rng(0)
    slot = (HEADER_BYTES + 256 * 256 * 3 + 63) // 64 * 64
    buf = np.zeros((a.n, slot), dtype=np.uint8)
    hd = buf[:, :HEADER_BYTES].view(np.int32)
    hd[:, 0], hd[:, 1], hd[:, 2] = 0, a.src, a.src
    hd[:, 3], hd[:, 4], hd[:, 5] = rng.integers(0, 17, a.n), rng.integers(0, 17, a.n), rng.integers(0, 2, a.n)
    hd[:, 6] = 7 | ZOOM | AFFINE
    hd[:, 10], hd[:, 11], hd[:, 12] = a.zoom, a.zoom, rng.integers(0, 729, a.n)
    hd[:, 7:10].view(np.float32)[:] = np.stack([rng.uniform(0, 0.1, a.n), rng.uniform(0, 0.2, a.n), rng.uniform(0.6, 1.0, a.n)], 1)
    buf[:, HEADER_BYTES:HEADER_BYTES + a.src * a.src * 3] = rng.integers(0, 256, (a.n, a.src * a.src * 3), dtype=np.uint8)
    raw = torch.from_numpy(buf).cuda()
    out = torch.empty((a.n, 112, 112, 3), dtype=torch.float32, device='cuda')
    moved = a.n * (HEADER_BYTES + a.src * a.src * 3) + out.numel() * 4
    st = torch.cuda.current_stream().cuda_stream
    table = torch.from_numpy(AFFINE_TABLE).cuda()
    ws_bytes = _lib.query('fte_preprocess_u8_geo_ws_bytes', a.n, 3, 112, 112)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device='cuda')
    for entry in ('fte_preprocess_u8', 'fte_preprocess_u8_aug', 'fte_preprocess_u8_geo'):
        extra = (table, ws, ws_bytes) if entry.endswith('_geo') else ()
        for _ in range(3):
            _lib.call(entry, raw.data_ptr(), out.data_ptr(), a.n, slot, 3, 128, 128, 112, 112, *extra, st)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            _lib.call(entry, raw.data_ptr(), out.data_ptr(), a.n, slot, 3, 128, 128, 112, 112, *extra, st)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / a.reps
        print('%s: %d x %dx%dx3 -> 112x112x3, %.1f us per launch back to back (events), %.2f MB moved, %.0f GB/s'
              % (entry, a.n, a.src, a.src, us, moved / 1e6, moved / us / 1e3))


if __name__ == '__main__':
    main()
