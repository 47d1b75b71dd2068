"""Plain float64 references for the HBM-bound glue kernels (csrc/tokens.hip, cam.hip, conv.hip, eval.hip), and the bounds a
correct fp32 kernel may differ from them by.  Everything is gathers over whole axes (no pixel loops), torch on the CPU.

tests/test_glue_ref_host.py checks these references against torch and checks that the bounds are neither too tight (torch's own
fp32 interpolate passes) nor too loose (three classic resampling mistakes fail); tests/test_glue_kernels_gpu.py then holds the
kernels to them."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

EPS24 = 2.0 ** -24


def ulp32(v: torch.Tensor) -> torch.Tensor:
    """Spacing of float32 at |v| (v float64), as float64."""
    a = np.abs(v.numpy()).astype(np.float32)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def src_coords(out: int, inn: int, align: bool):
    """Source coordinate r, taps i0 / i1 and weight l of i1 for every output index: the exact definition, in float64."""
    o = torch.arange(out, dtype=torch.float64)
    if align:
        scale = (inn - 1) / (out - 1) if out > 1 else 0.0
        r = scale * o
    else:
        r = ((inn / out) * (o + 0.5) - 0.5).clamp_min(0.0)
    i0 = r.floor().long().clamp_max(inn - 1)
    i1 = (i0 + 1).clamp_max(inn - 1)
    return r, i0, i1, r - i0.double()


def bilinear64(x: torch.Tensor, Ho: int, Wo: int, align_corners: bool, coords=src_coords) -> torch.Tensor:
    """Bilinear resize of (..., Hi, Wi) to (..., Ho, Wo) in float64.  `coords` exists so that the host suite can feed wrong
    coordinate rules through the same blend."""
    x = x.double()
    Hi, Wi = x.shape[-2:]
    _, y0, y1, ly = coords(Ho, Hi, align_corners)
    _, x0, x1, lx = coords(Wo, Wi, align_corners)
    ly = ly.view(-1, 1)
    rows = x.index_select(-2, y0) * (1.0 - ly) + x.index_select(-2, y1) * ly
    return rows.index_select(-1, x0) * (1.0 - lx) + rows.index_select(-1, x1) * lx


def _dyadic(inn: int, out: int, align: bool) -> bool:
    """The fp32 source coordinates are exact: the scale is a power of two (identity included), or there is one sample."""
    if inn == 1:
        return True
    if align:
        if out == 1:
            return True
        inn, out = inn - 1, out - 1
    a, b = max(inn, out), min(inn, out)
    return a % b == 0 and ((a // b) & ((a // b) - 1)) == 0


def _coord_err(out: int, inn: int, align: bool) -> torch.Tensor:
    """What fp32 may be off in the source coordinate: 2 ulp (one multiply and one subtract, or one FMA, of a rounded scale);
    nothing at dyadic scales."""
    if _dyadic(inn, out, align):
        return torch.zeros(out, dtype=torch.float64)
    r = src_coords(out, inn, align)[0]
    return 2.0 * ulp32(r)


def bilinear_bound(x: torch.Tensor, Ho: int, Wo: int, align_corners: bool) -> torch.Tensor:
    """Per output pixel: 2 ulp32(r_y) L_y + 2 ulp32(r_x) L_x + 6 * 2^-24 * M.  L_y / L_x: largest step between vertically /
    horizontally adjacent samples of the plane (bilinear is continuous and piecewise linear with these slopes, so a coordinate
    error d moves the value by at most d * L); M = max |x| of the plane; 6 * 2^-24 M covers the blend (at most 6 nested
    roundings of quantities <= M without FMA)."""
    x = x.double()
    Hi, Wi = x.shape[-2:]
    zero = torch.zeros(x.shape[:-2] + (1, 1), dtype=torch.float64)
    Ly = (x[..., 1:, :] - x[..., :-1, :]).abs().amax((-2, -1), keepdim=True) if Hi > 1 else zero
    Lx = (x[..., :, 1:] - x[..., :, :-1]).abs().amax((-2, -1), keepdim=True) if Wi > 1 else zero
    M = x.abs().amax((-2, -1), keepdim=True)
    ey = _coord_err(Ho, Hi, align_corners).view(-1, 1)
    ex = _coord_err(Wo, Wi, align_corners).view(1, -1)
    return ey * Ly + ex * Lx + 6.0 * EPS24 * M


def _cubic_w(t: torch.Tensor):
    A = -0.75
    def c1(v): return ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0
    def c2(v): return ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A
    return torch.stack((c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)), -1)       # [out, 4]


def _cubic_axis(x: torch.Tensor, out: int, dim: int) -> torch.Tensor:
    inn = x.shape[dim]
    o = torch.arange(out, dtype=torch.float64)
    r = (inn / out) * (o + 0.5) - 0.5            # no clamp at 0 for bicubic
    f = r.floor()
    wts = _cubic_w(r - f)
    shape = [1] * x.dim()
    shape[dim] = out
    acc = 0.0
    for k in range(4):
        idx = (f.long() - 1 + k).clamp(0, inn - 1)
        acc = acc + x.index_select(dim, idx) * wts[:, k].view(shape)
    return acc


def bicubic64(x: torch.Tensor, Ho: int, Wo: int) -> torch.Tensor:
    """torch's bicubic (A = -0.75, align_corners=False, border clamp) of (..., Hi, Wi) in float64."""
    x = x.double()
    return _cubic_axis(_cubic_axis(x, Wo, x.dim() - 1), Ho, x.dim() - 2)


def pos_embed64(pe: torch.Tensor, g: int, h: int, w: int) -> torch.Tensor:
    """pe [1 + g*g, D] -> [1 + h*w, D]: row 0 copied, the g x g grid resized with bicubic64."""
    D = pe.shape[-1]
    grid = pe[1:].double().view(g, g, D).permute(2, 0, 1)
    return torch.cat((pe[:1].double(), bicubic64(grid, h, w).permute(1, 2, 0).reshape(h * w, D)), 0)


def _low_planes(low: torch.Tensor, hs: int, ws: int, B2: int, C: int, row_off: int, ldc: int) -> torch.Tensor:
    rows = row_off + hs * ws
    return low.view(B2, rows, ldc)[:, row_off:, :C].transpose(1, 2).reshape(B2, C, hs, ws)


def cam_fuse64(lows, sizes, B: int, C: int, H: int, W: int, row_off: int, ldc: int):
    """sum_s relu(max(up(low_s[:B]), flip(up(low_s[B:])))) in float64 and its per-pixel fp32 bound: per scale the larger of the two
    images' bilinear_bound (max and relu are 1-Lipschitz), plus (nscale - 1) * 2^-24 * sum_s max for the running sum."""
    cam = torch.zeros(B, C, H, W, dtype=torch.float64)
    bound = torch.zeros(B, C, H, W, dtype=torch.float64)
    tops = torch.zeros(B, C, 1, 1, dtype=torch.float64)
    for low, (hs, ws) in zip(lows, sizes):
        m = _low_planes(low, hs, ws, 2 * B, C, row_off, ldc)
        up, bb = bilinear64(m, H, W, False), bilinear_bound(m, H, W, False)
        v = torch.relu(torch.max(up[:B], up[B:].flip(-1)))
        cam += v
        bound += torch.max(bb[:B], bb[B:].flip(-1))
        tops += v.amax((-2, -1), keepdim=True)
    return cam, bound + (len(lows) - 1) * EPS24 * tops


def msc_seg64(segs: torch.Tensor, acc: torch.Tensor, mode: int):
    """v = up(segs[0]) + flip(up(segs[1])); mode 0: v, 1: max(acc, v), 2: acc + v.  Bound: both bilinear_bounds plus one rounding
    of the sum of the two and one of the accumulation."""
    H, W = acc.shape[-2:]
    up, bb = bilinear64(segs, H, W, False), bilinear_bound(segs, H, W, False)
    v = up[0] + up[1].flip(-1)
    a = acc.double().reshape(v.shape)
    ref = v if mode == 0 else (torch.max(a, v) if mode == 1 else a + v)
    a_abs = torch.zeros_like(v) if mode == 0 else a.abs()
    return ref, bb[0] + bb[1].flip(-1) + 2.0 * EPS24 * (v.abs() + a_abs)


def upsample_argmax64(logits: torch.Tensor, H: int, W: int):
    """(argmax (B,H,W), top-1 - top-2 margin, largest bilinear_bound over the channels) of the float64 up-sampling."""
    up = bilinear64(logits, H, W, False)
    arg = up.argmax(1)
    if up.shape[1] > 1:
        top = up.topk(2, dim=1).values
        margin = top[:, 0] - top[:, 1]
    else:
        margin = torch.full(arg.shape, float("inf"), dtype=torch.float64)
    bound = torch.zeros(arg.shape, dtype=torch.float64)
    for c in range(logits.shape[1]):                       # channel by channel: no (B, C, H, W) temporary
        bound = torch.max(bound, bilinear_bound(logits[:, c], H, W, False))
    return arg, margin, bound


def im2col64(x: torch.Tensor, dil: int) -> torch.Tensor:
    """x (B, Cin, h, w) -> rows [B*h*w, Cin*9], column = c*9 + tap: F.unfold's own order."""
    B, Cin = x.shape[:2]
    return F.unfold(x, 3, dilation=dil, padding=dil).transpose(1, 2).reshape(-1, Cin * 9)


def col2im64(col: torch.Tensor, B: int, h: int, w: int, dil: int) -> torch.Tensor:
    """The adjoint: rows [B*h*w, Cin*9] -> (B, Cin, h, w)."""
    return F.fold(col.view(B, h * w, -1).transpose(1, 2), (h, w), 3, dilation=dil, padding=dil)


# (Hi, Wi, Ho, Wo, align_corners): the bilinear cases of both suites
RESIZE_CASES = [(64, 64, 28, 28, False), (13, 17, 75, 100, False), (375, 500, 224, 224, False), (448, 448, 336, 336, False),
                (500, 375, 250, 187, False), (1, 1, 5, 7, False), (2, 3, 1000, 999, False), (224, 224, 448, 448, False),
                (64, 64, 50, 40, True), (5, 7, 1, 1, True), (3, 4, 1, 9, True)]
