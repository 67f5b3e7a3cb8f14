"""fte_pack_gather_slots alone, for a kernel trace: N slots of one h x w x 3 row each out of a resident pack of R rows, random rows.

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_pack_gather.py [--n 512] [--h 112] [--w 112] [--rows 8192] [--reps 50]

Prints the bytes one launch moves (headers + rows read, slots written) and, from HIP events, the mean time per launch back to back;
the kernel times proper are the trace's."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--h', type=int, default=112)
    ap.add_argument('--w', type=int, default=112)
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    import torch
    from tf_face_toolbox_amd import _lib
    from tf_face_toolbox_amd.packs import row_stride_of
    stride = row_stride_of(a.h, a.w, 3)
    slot = 64 + stride
    g = torch.Generator().manual_seed(0)
    rows = torch.randint(0, 256, (a.rows, stride), dtype=torch.uint8, generator=g).cuda()
    headers = torch.zeros((a.n, 64), dtype=torch.uint8, device='cuda')
    index = torch.randint(0, a.rows, (a.n,), dtype=torch.int64, generator=g).cuda()
    slots = torch.empty((a.n, slot), dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    args = (rows, a.rows, stride, index, headers, slots, a.n, slot, st)
    for _ in range(3):
        _lib.call('fte_pack_gather_slots', *args)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        _lib.call('fte_pack_gather_slots', *args)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / a.reps
    moved = 2 * a.n * slot
    print('fte_pack_gather_slots: %d x %dx%dx3 (row stride %d) out of %d rows, %.1f us per launch back to back (events), %.2f MB read + '
          'written, %.0f GB/s' % (a.n, a.h, a.w, stride, a.rows, us, moved / 1e6, moved / us / 1e3))


if __name__ == '__main__':
    main()
