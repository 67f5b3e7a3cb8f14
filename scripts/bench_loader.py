"""Throughput of the host input pipeline (tf_face_toolbox_amd/data.py: list reader -> JPEG decode -> TF-1.x bilinear resize ->
crop / flip -> normalise -> NHWC float32 batch) in images/s at 112x112, on this host's cores -- to be read against the
rate the GPU step consumes (~10 k images/s per MI355X in fp32, ~30 k in the bf16 mode).

    python scripts/bench_loader.py [--images 2048] [--batch 512] [--batches 60] [--warmup 24] [--src 250] [--device cpu|cuda]
                                   [--augmentation 0|1|2|3] [--landmark_list_path P]
                                   [--data_dir D] [--packed_data_path P.fpk [--pack_on_gpu 0|1]]

Writes N synthetic JPEGs of src x src pixels (CASIA-WebFace crops are 250 x 250) to a temporary directory, then times
`data.train_inputs(...)` batches (resize to 128 x 128, random crop 112 x 112, flip; --augmentation 1: the colour augmentation of
train.py --augmentation 1 as well): the same call train.py makes.  --landmark_list_path P: made-up landmarks for the generated
images (a face of 0.7 of the side, rotated by -30 .. 30 degrees, the angle changing from image to image) are written to P and
the call gets landmark_list_path=P -- five-point alignment to 128 x 128 in place of the resize (train.py --landmark_list_path),
the rest as before; FTE_LOADER_GPU=0 keeps the transform in the workers.
--data_dir D: the JPEGs and their list are written under D and kept, and found there by the next run (several loaders timed on ONE
set, in turn).  --packed_data_path P: the loader is fed from that image pack (train.py --packed_data_path; --pack_on_gpu 1: from
its copy in device memory); a pack that does not exist yet is made from the list first, with pack_list.py, and the time is printed."""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np          # noqa: E402
from PIL import Image       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--batches', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=24, help='untimed batches first: more than the pipeline holds prefetched (2 per group of 16 workers), so that the timed batches are decoded at the sustained rate')
    ap.add_argument('--src', type=int, default=250)
    ap.add_argument('--device', default=None, help="default: cuda when a GPU is present (the training path: pinned staging ring + async copy), else cpu")
    ap.add_argument('--workers', type=int, default=None, help='decode worker processes (default: data.train_inputs picks; 0 = threads)')
    ap.add_argument('--augmentation', type=int, choices=[0, 1, 2, 3], default=0,
                    help='1: flip + brightness / hue / saturation; 2: zoom + affine warp + flip; 3: both (train.py --augmentation)')
    ap.add_argument('--landmark_list_path', default=None,
                    help='write made-up landmarks for the generated images here and align (128 x 128) instead of resizing; --augmentation 0 | 1')
    ap.add_argument('--data_dir', default=None, help='keep the generated JPEGs and their list here and reuse them (default: a temporary directory)')
    ap.add_argument('--packed_data_path', default=None, help='feed from this image pack; made from the list with pack_list.py when it does not exist')
    ap.add_argument('--pack_on_gpu', type=int, default=0, help='1: the pack resident in device memory')
    args = ap.parse_args()
    from tf_face_toolbox_amd import data
    if args.device is None:
        import torch
        args.device = 'cuda' if torch.cuda.is_available() else 'cpu'
    rng = np.random.default_rng(0)
    import contextlib
    if args.data_dir is not None:
        os.makedirs(args.data_dir, exist_ok=True)
    with (tempfile.TemporaryDirectory() if args.data_dir is None else contextlib.nullcontext(os.path.abspath(args.data_dir))) as d:
        lst = os.path.join(d, 'list_%d_%d.txt' % (args.images, args.src))
        lines = ['%s %d' % (os.path.join(d, '%d_%06d.jpg' % (args.src, i)), i % 100) for i in range(args.images)]
        if not os.path.exists(lst):
            base = rng.integers(0, 255, (args.src, args.src, 3), dtype=np.uint8)
            for i, ln in enumerate(lines):
                Image.fromarray(np.roll(base, i * 7, axis=1)).save(ln.split()[0], quality=90)
            open(lst, 'w').write('\n'.join(lines) + '\n')
        more = {}
        if args.packed_data_path is not None:
            if args.landmark_list_path is not None:
                ap.error('--packed_data_path with --landmark_list_path: a pack is aligned when it is made')
            if not os.path.exists(args.packed_data_path):
                import pack_list
                t0 = time.time()
                pack_list.main(['--data_list_path', lst, '--out', args.packed_data_path])
                print('pack_list.py: %.1f s, %d bytes' % (time.time() - t0, os.path.getsize(args.packed_data_path)))
            more = {'packed_data_path': args.packed_data_path, 'pack_on_gpu': bool(args.pack_on_gpu)}
        if args.landmark_list_path is not None:
            from tf_face_toolbox_amd.preprocessing import ALIGN_TEMPLATE_112
            centred = (ALIGN_TEMPLATE_112 - 55.5) * (0.7 * args.src / 112.0)
            with open(args.landmark_list_path, 'w') as f:
                for i, ln in enumerate(lines):
                    t = np.deg2rad((i * 7) % 61 - 30)
                    pts = centred @ np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]]) + (args.src - 1) / 2.0
                    f.write('%s %s\n' % (ln.split()[0], ' '.join('%.2f' % v for v in pts.reshape(-1))))
            more['landmark_list_path'] = args.landmark_list_path
        inp = data.train_inputs(None if args.packed_data_path else lst, 128, 128, 112, 112, is_color=1, augmentation=args.augmentation, batch_size=args.batch, device=args.device, seed=0, num_workers=args.workers, **more)
        for _ in range(max(1, args.warmup)):             # warm-up: worker start, page cache -- and the prefetched batches (a short run
            inp['images'](); inp['labels']()             # timed right after start-up is served out of the filled pipe and reads 1.5-4x high)
        t0 = time.time()
        for _ in range(args.batches):
            x = inp['images']()
            inp['labels']()
        if args.device != 'cpu':
            import torch
            torch.cuda.synchronize()
        el = time.time() - t0
        print('loader: %.0f images/s sustained (%d batches of %d after %d untimed, %dx%d JPEG -> 128x128 -> crop 112x112, workers %s, os.cpu_count=%d, usable CPUs (affinity / cgroup quota) %d, device %s%s), batch %s %s'
              % (args.batches * args.batch / el, args.batches, args.batch, args.warmup, args.src, args.src,
                 'auto' if args.workers is None else args.workers, os.cpu_count(), data.usable_cpus(), args.device,
                 (', augmentation %d, gpu_transform %s' % (args.augmentation, bool(inp['gpu_transform'])) if args.augmentation else '')
                 + (', aligned from landmarks, gpu_transform %s' % bool(inp['gpu_transform']) if args.landmark_list_path else '')
                 + (', image pack: %s' % inp['packed'] if inp['packed'] else ''), tuple(x.shape), x.dtype))
        inp['close']()


if __name__ == '__main__':
    main()
