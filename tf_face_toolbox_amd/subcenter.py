"""The cleaning pass of sub-center ArcFace (Deng et al., ECCV 2020): after a run with K centres per class, keep the
dominant centre of every class, drop the training samples that lie further than `angle` degrees from it, and write a K = 1 model
and the cleaned list the run continues with.  subcenter_clean.py is the command line.

The cosines come from fte_subcenter_assign (one wave per sample, K dot products against the centres of the sample's OWN class: the
[N, K * C] product is never formed); the counts are torch integer ops on the device.  Rules, all fixed:
  * a sample selects the centre of its class with the largest cosine, the lowest k on a tie;
  * the dominant centre of a class is the one most of its samples select, the lowest k on a tie; a class without samples keeps centre 0;
  * a sample is kept iff cos(feature, dominant centre of its class) >= fp32(cos(angle)), the threshold computed in float64 and rounded
    once; a label outside [0, C) is dropped and counted in no class."""
import math

import numpy as np
import torch

from . import _lib

CLASSIFIER = 'classifier/fc_classifier/weights'


def threshold(angle_deg):
    """cos(angle) in float64, rounded to fp32 once: what the fp32 cosines are compared against"""
    return float(np.float32(math.cos(math.radians(float(angle_deg)))))


def packed_planes(W, K):
    """checkpoint layout [D, K * C] (column k * C + j = centre k of class j) -> [D, K, C] view"""
    d, wide = W.shape
    if K < 1 or wide % K:
        raise ValueError('a classifier of %d columns does not hold sub_centers = %d centres per class' % (wide, K))
    return W.reshape(d, K, wide // K)


def assign(features, Wt, labels, K, num_classes):
    """fte_subcenter_assign on one chunk: features [n, d] float32, Wt [K * C, d] float32 (row k * C + j = centre k of class j), labels [n]
    int32, all CUDA -> (sel [n] int32, cosv [K, n] float32)"""
    n, d = features.shape
    sel = torch.empty(n, dtype=torch.int32, device=features.device)
    cosv = torch.empty(K, n, dtype=torch.float32, device=features.device)
    _lib.call('fte_subcenter_assign', features, Wt, labels, K, sel, cosv, n, d, int(num_classes), torch.cuda.current_stream().cuda_stream)
    return sel, cosv


def clean(features, labels, W, K, angle=75.0, chunk=65536, device='cuda'):
    """features [N, d] (numpy or tensor, float32), labels [N] integers, W [d, K * C] the classifier in checkpoint layout.
    -> dict: keep [N] bool, dominant [C] int64, kept / dropped [C] int64 (per class), invalid (labels outside [0, C)), non_dominant (samples
    whose own choice is not their class's dominant centre), total, threshold, weights [d, C] = the dominant columns of W, bitwise copies
    (all tensors on the CPU)."""
    dev = torch.device(device)
    W = torch.as_tensor(W, dtype=torch.float32)
    planes = packed_planes(W, K)
    d, _, C = planes.shape
    feats = torch.as_tensor(np.ascontiguousarray(features) if isinstance(features, np.ndarray) else features)
    if feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != d:
        raise ValueError('features must be float32 [N, %d] (the classifier has %d rows): got %s %s' % (d, d, feats.dtype, tuple(feats.shape)))
    N = feats.shape[0]
    lab = torch.as_tensor(np.asarray(labels).astype(np.int64))
    if lab.shape != (N,):
        raise ValueError('%d features but %d labels' % (N, lab.numel()))
    lab = lab.clamp(-1, C).to(torch.int32).to(dev)          # anything out of range stays out of range, inside int32
    Wt = planes.permute(1, 2, 0).reshape(K * C, d).contiguous().to(dev)      # transposed once
    sel = torch.empty(N, dtype=torch.int32, device=dev)
    cosv = torch.empty(K, N, dtype=torch.float32, device=dev)
    counts = torch.zeros(C * K, dtype=torch.int64, device=dev)
    for a in range(0, N, chunk):
        b = min(N, a + chunk)
        s, cv = assign(feats[a:b].contiguous().to(dev), Wt, lab[a:b], K, C)
        sel[a:b] = s
        cosv[:, a:b] = cv
        ok = s >= 0
        counts += torch.bincount((lab[a:b].long() * K + s.long())[ok], minlength=C * K)
    dominant = torch.argmax(counts.reshape(C, K), dim=1)     # the first maximal index: the lowest k on a tie, 0 for an empty class
    valid = sel >= 0
    safe = lab.long().clamp(0, C - 1)
    dom_i = dominant[safe]
    cos_dom = cosv.gather(0, dom_i.reshape(1, N)).reshape(N)
    thr = threshold(angle)
    keep = valid & (cos_dom >= thr)
    kept = torch.bincount(safe[keep], minlength=C)
    per_class = torch.bincount(safe[valid], minlength=C)
    non_dominant = int((valid & (sel.long() != dom_i)).sum())
    dom_cpu = dominant.cpu()
    weights = planes[:, dom_cpu, torch.arange(C)].contiguous()
    return dict(keep=keep.cpu(), dominant=dom_cpu, kept=kept.cpu(), dropped=(per_class - kept).cpu(), invalid=int((~valid).sum()),
                non_dominant=non_dominant, total=N, threshold=thr, weights=weights)


def reduce_checkpoint(state, weights):
    """The checkpoint dict `state` (saver.py) with the K-centre classifier replaced by `weights` [D, C].  The classifier's optimizer
    slots are ZEROED at the new shape (the momentum of the dropped centres has no meaning for the kept one's continued run; the other
    variables keep theirs), so the file restores into a K = 1 net with or without its optimizer."""
    out = dict(state)
    out['variables'] = dict(state['variables'])
    out['variables'][CLASSIFIER] = weights.clone()
    out['slots'] = []
    for slot in state.get('slots') or []:
        slot = dict(slot)
        if CLASSIFIER in slot:
            slot[CLASSIFIER] = torch.zeros_like(weights)
        out['slots'].append(slot)
    return out


def report(res, out=print):
    """the per-class kept / dropped totals and the share of samples on non-dominant centres"""
    for j in range(res['kept'].numel()):
        out('class %d: dominant centre %d, kept %d, dropped %d' % (j, int(res['dominant'][j]), int(res['kept'][j]), int(res['dropped'][j])))
    kept, dropped = int(res['kept'].sum()), int(res['dropped'].sum())
    out('total: kept %d, dropped %d of %d samples (threshold cos = %.9g)%s'
        % (kept, dropped + res['invalid'], res['total'], res['threshold'],
           ', %d of the dropped with a label outside the classes' % res['invalid'] if res['invalid'] else ''))
    labelled = res['total'] - res['invalid']
    out('samples on non-dominant centres: %d of %d (%.4f%%)' % (res['non_dominant'], labelled, 100.0 * res['non_dominant'] / max(labelled, 1)))
