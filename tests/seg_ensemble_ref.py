"""float64 reference of the two-student ensemble tail (a helper, not a test), written from the definition of
dupl_seg_ensemble (include/dupl_hip.h) in numpy:

    u_s[c] = bilinear (align_corners False) up-sampling of student s's logits to (H,W); the logits themselves when (h,w) == (H,W)
    p_s    = softmax_c(u_s), channel maximum subtracted;   e = (p_1 + p_2) / 2
    predictions = argmax_c of u_1, u_2 and e, first maximum wins

and the shapes and seeded inputs that tests/test_seg_ensemble_host.py and tests/test_seg_ensemble_gpu.py share."""
import functools

import numpy as np
import torch

import kernel_guard as KG

# (C, h, w, H, W): one source pixel; odd sizes and partial tiles; identity (the VOC form); the COCO channel count across a tile
# edge; the channel cap = the global-atomics histogram; one column past 256; and the two paths of csrc/seg_ens.hip those do not reach:
# down-sampling (a tile's footprint too large to stage) and identity with more channels than a thread keeps in registers
SHAPES = ((2, 1, 1, 5, 3), (21, 7, 9, 37, 53), (21, 37, 53, 37, 53), (81, 28, 28, 97, 131), (255, 3, 2, 9, 70), (21, 28, 28, 64, 257),
          (5, 40, 90, 7, 11), (30, 6, 9, 6, 9))
MARGIN = 1e-5          # fp64 top-2 margin of e under which the ensemble's argmax may differ
TIE_SHARE = 2e-3       # cap on the share of such pixels per shape
# pixels under MARGIN per shape, from this reference alone (tests/test_seg_ensemble_host.py pins them)
REF_TIES = (0, 0, 0, 3, 0, 2, 0, 0)


def inputs(C, h, w, H, W):
    """(a, b) (1,C,h,w) fp32 and gt (H,W) int64 with about 10 % of the labels 255, all on the host."""
    a, b = KG.rnd(1, C, h, w, seed=11, scale=3.0), KG.rnd(1, C, h, w, seed=12, scale=3.0)
    gt = KG.rndint(0, C, H, W, seed=13)
    gt[torch.rand((H, W), generator=torch.Generator().manual_seed(14)) < 0.1] = 255
    return a, b, gt


def src_index(out, inp):
    """upsample_bilinear2d's source taps of every output coordinate: (i0, i1, weight of i1)."""
    r = np.maximum((inp / out) * (np.arange(out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(r.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    return i0, i1, r - i0


def upsample64(x, H, W):
    """x (C,h,w) -> (C,H,W) float64."""
    x = np.asarray(x, dtype=np.float64)
    C, h, w = x.shape
    if (h, w) == (H, W):
        return x.copy()
    y0, y1, ly = src_index(H, h)
    x0, x1, lx = src_index(W, w)
    out = np.empty((C, H, W), dtype=np.float64)
    for y in range(H):
        top = (1.0 - lx) * x[:, y0[y], x0] + lx * x[:, y0[y], x1]
        bot = (1.0 - lx) * x[:, y1[y], x0] + lx * x[:, y1[y], x1]
        out[:, y, :] = (1.0 - ly[y]) * top + ly[y] * bot
    return out


def softmax64(u):
    ex = np.exp(u - u.max(axis=0, keepdims=True))
    return ex / ex.sum(axis=0, keepdims=True)


def ensemble64(a, b, H, W):
    """a, b (C,h,w) -> dict(e (C,H,W) float64, pred1, pred2, pred (H,W) int64, margin (H,W) = top-1 - top-2 of e)."""
    u1, u2 = upsample64(a, H, W), upsample64(b, H, W)
    e = 0.5 * (softmax64(u1) + softmax64(u2))
    if e.shape[0] > 1:
        top = np.sort(e, axis=0)[-2:]
        margin = top[1] - top[0]
    else:
        margin = np.full((H, W), np.inf)
    return {"e": e, "pred1": u1.argmax(0), "pred2": u2.argmax(0), "pred": e.argmax(0), "margin": margin}


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs and the float64 reference of one of SHAPES, computed once per session and shared; treat as read-only."""
    C, h, w, H, W = shape
    a, b, gt = inputs(C, h, w, H, W)
    ref = ensemble64(a[0].numpy(), b[0].numpy(), H, W)
    return a, b, gt, ref
