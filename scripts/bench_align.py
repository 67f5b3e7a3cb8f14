"""fte_preprocess_u8_align against fte_preprocess_u8 on slots of the same decoded pixels: N x (src x src x 3 -> 112 x 112), the
aligning entry with a rotation by --angle degrees at the scale that maps the 112 x 112 crop onto --cover of the source's side.

    python scripts/bench_align.py [--n 512] [--src 250] [--reps 50] [--angle 15] [--cover 0.8]

Prints, from in-stream HIP events around --reps back-to-back launches, the mean time per launch, and the bytes one launch
touches AT MOST (every slot byte + the float32 crop written): neither kernel reads every slot byte, so no rate is derived from
that count.  scripts/bench_preprocess.py is the model."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--src', type=int, default=250)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--angle', type=float, default=15.0)
    ap.add_argument('--cover', type=float, default=0.8)
    a = ap.parse_args()
    import torch
    from tf_face_toolbox_amd import _lib
    from tf_face_toolbox_amd._decode_worker import ALIGN_HEADER_BYTES, HEADER_BYTES
    rng = np.random.default_rng(0)
    pixels = rng.integers(0, 256, (a.n, a.src * a.src * 3), dtype=np.uint8)
    flips = rng.integers(0, 2, a.n)
    out = torch.empty((a.n, 112, 112, 3), dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    s = a.cover * a.src / 112.0
    c, sn = s * np.cos(np.deg2rad(a.angle)), s * np.sin(np.deg2rad(a.angle))
    m6 = np.asarray([c, -sn, (a.src - 1) / 2.0 - (c - sn) * 55.5, sn, c, (a.src - 1) / 2.0 - (sn + c) * 55.5], dtype=np.float32)
    for entry, header in (('fte_preprocess_u8', HEADER_BYTES), ('fte_preprocess_u8_align', ALIGN_HEADER_BYTES)):
        slot = (header + 256 * 256 * 3 + 63) // 64 * 64
        buf = np.zeros((a.n, slot), dtype=np.uint8)
        hd = buf[:, :header].view(np.int32)
        hd[:, 1], hd[:, 2], hd[:, 5] = a.src, a.src, flips
        if header == ALIGN_HEADER_BYTES:
            hd[:, 16:22].view(np.float32)[:] = m6
        buf[:, header:header + a.src * a.src * 3] = pixels
        raw = torch.from_numpy(buf).cuda()
        moved = a.n * (header + a.src * a.src * 3) + out.numel() * 4
        for _ in range(3):
            _lib.call(entry, raw.data_ptr(), out.data_ptr(), a.n, slot, 3, 112, 112, 112, 112, st)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            _lib.call(entry, raw.data_ptr(), out.data_ptr(), a.n, slot, 3, 112, 112, 112, 112, st)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / a.reps
        print('%s: %d x %dx%dx3 -> 112x112x3, %.1f us per launch back to back (events, %d launches), at most %.2f MB touched, output mean %.4f'
              % (entry, a.n, a.src, a.src, us, a.reps, moved / 1e6, float(out.mean())))


if __name__ == '__main__':
    main()
