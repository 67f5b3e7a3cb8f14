"""Step figures of an SE-IResNet (or IResNet) net for profiles/se_iresnet.md, one line of JSON -- scripts/iresnet_profile.py with
the entry points of the SE block tail among the timed ones:

    [FTE_MFMA_DTYPE=bf16] python scripts/se_iresnet_profile.py SE-IResNet-50-arcface 128 [steps]

  ms_per_step / images_per_s   host clock around `steps` training steps that end in a device synchronise (after 3 warm-up steps)
  entry_points                 device-event time around every fte_se_lin_* / fte_se_bn_bwd_* / fte_bn_prelu_* call of ONE step (a run of its own: the events serialise
                               nothing, but the bookkeeping slows the host), per entry point: calls, ms, share of ms_per_step
  mfma                         the launch profiler's records of one step (fte_prof_*: every gathered-GEMM launch of the igemm family):
                               FLOPs executed, their summed kernel time, and executed FLOPs / ms_per_step over the MFMA peak of the
                               operand mode (157.3 TFLOP/s fp32, 2500 TFLOP/s bf16: MI355X data sheet)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                             # noqa: E402
from tf_face_toolbox_amd import net_select, Singular, _lib               # noqa: E402

PEAK = {'f32': 157.3e12, 'bf16': 2500e12}
TIMED = ('fte_se_lin_', 'fte_se_bn_bwd_', 'fte_bn_prelu_')


def main():
    name, B = sys.argv[1], int(sys.argv[2])
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    ncls = 10575
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 112, 112, 3, generator=g) * 2 - 1).cuda()
    y = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32).cuda()
    net = net_select(name, 'NCHW', 5e-4)
    step, losses, names, _ = Singular(net, 1e-3, 'Momentum')({'images': x, 'labels': y, 'num_classes': ncls, 'num_examples': B})
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    # the launch profiler: one step
    _lib.query('fte_prof_enable', 1)
    step()
    torch.cuda.synchronize()
    _lib.query('fte_prof_enable', 0)
    recs = _lib.prof_records()
    flops, mfma_ms = sum(r[1] for r in recs), sum(r[2] for r in recs)
    # device events around the new entry points: one step
    real, ev = _lib.call, []

    def timed_call(fn, *args):
        if not fn.startswith(TIMED):
            return real(fn, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(fn, *args)
        e1.record()
        ev.append((fn, e0, e1))
        return r
    _lib.call = timed_call
    try:
        step()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    per = {}
    for fn, e0, e1 in ev:
        a = per.setdefault(fn, [0, 0.0])
        a[0] += 1
        a[1] += e0.elapsed_time(e1)
    mode = _lib.get_mfma_dtype()
    out = {'net': name, 'batch': B, 'mode': _lib.precision_mode(), 'steps': steps, 'ms_per_step': round(ms, 3), 'images_per_s': round(B / ms * 1e3, 1),
           'losses': [round(float(v), 4) for v in losses],
           'entry_points': {k: {'calls': v[0], 'ms': round(v[1], 3), 'share_of_step': round(v[1] / ms, 4)} for k, v in sorted(per.items())},
           'se_lin_share_of_step': round(sum(v[1] for k, v in per.items() if k.startswith('fte_se_lin_')) / ms, 4),
           'se_tail_share_of_step': round(sum(v[1] for k, v in per.items() if k.startswith('fte_se_')) / ms, 4),
           'mfma': {'launches': len(recs), 'executed_tflop_per_step': round(flops / 1e12, 3), 'kernel_ms': round(mfma_ms, 3),
                    'executed_flops_over_step_time_of_peak': round(flops / (ms * 1e-3) / PEAK[mode], 4), 'peak_tflops': PEAK[mode] / 1e12}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
