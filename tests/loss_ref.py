"""Plain float64 references for the loss kernels (csrc/loss.hip) and the LayerNorm kernels (csrc/norm.hip), the bounds a correct
fp32 kernel may differ from them by, and the case lists of tests/test_loss_norm_kernels_gpu.py (kept here so that
tests/test_loss_ref_host.py checks the bounds on the very cases the kernels are held to).  CPU only: torch + numpy.

Every bound is a function of the data (per pixel, per cell, per row), never a constant times the largest value: a wrong border
weight changes border cells only and must not hide behind the interior.

Depth convention: a sum of n fp32 terms accumulated in any order is off by at most (n - 1) * 2^-24 * sum |terms| (first order);
where a kernel's order is a tree or a short serial chain the depth of that chain is used and said so."""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

import glue_ref as G

EPS24 = G.EPS24
f32 = np.float32


# =========================================================================================== fused up-sample + CE
def finish32(mode: int, s0, s1, s2, s3) -> np.float32:
    """loss_finish of csrc/loss.hip in numpy float32, one rounding per operation, in the order the kernel writes them."""
    s0, s1, s2, s3 = f32(s0), f32(s1), f32(s2), f32(s3)
    with np.errstate(all="ignore"):
        if mode == 1:
            pos = f32(0.5) * (f32(1) - s0 / (s1 + f32(1)))
            neg = (f32(0.5) * s2) / (s3 + f32(1))
            return f32(pos + neg)
        if mode == 2:
            return f32(f32(0.5) * (s0 / (s1 + f32(1e-6)) + s2 / (s3 + f32(1e-6))))
        return f32((s0 + s2) / np.maximum(f32(s1 + s3), f32(1)))


def seg_grid_blocks(b, h, w, H, W) -> int:
    """blocks of the seg-loss forward: 16 x 16 pixel tiles shifted by half a cell, one extra tile per axis"""
    return ((W + (W // w) // 2 + 15) // 16 + 1) * ((H + (H // h) // 2 + 15) // 16 + 1) * b


def up64(x, H, W, variant="ok"):
    """The up-sampling of the seg loss on (b, C1, h, w) logits: glue_ref.bilinear64, align_corners False.  The other variants are
    the reference-side MISTAKES tests/test_loss_ref_host.py shows to leave the bounds."""
    if variant == "ok":
        return G.bilinear64(x, H, W, False)
    if variant == "align_corners":
        return G.bilinear64(x, H, W, True)
    if variant == "no_half_pixel":                        # r = (in / out) * o, without the +0.5 / -0.5
        def coords(out, inn, align):
            r = (inn / out) * torch.arange(out, dtype=torch.float64)
            i0 = r.floor().long().clamp_max(inn - 1)
            return r, i0, (i0 + 1).clamp_max(inn - 1), r - i0.double()
        return G.bilinear64(x, H, W, False, coords=coords)
    if variant == "border_dropped":                       # the clamped far tap contributes nothing instead of merging into the near one
        xp = F.pad(x.double(), (0, 1, 0, 1))

        def coords(out, inn, align):
            r, i0, _, l = G.src_coords(out, inn - 1, False)
            return r, i0, i0 + 1, l
        return G.bilinear64(xp, H, W, False, coords=coords)
    raise ValueError(variant)


def up64_flipped(x, H, W, variant="ok"):
    """up(flip_w(x)).  Mirroring commutes with the align_corners False resize, so flipping the OUTPUT instead is no mistake; the
    mistake that exists is to mirror the base tap only and take its neighbour on the old side ("flip_base_tap_only"): the weight
    l then sits on column (w - 1 - x0) + 1 instead of (w - 1 - x0) - 1."""
    if variant != "flip_base_tap_only":
        return up64(torch.flip(x, dims=[3]), H, W, variant)
    x = x.double()
    h, w = x.shape[-2:]
    _, y0, y1, ly = G.src_coords(H, h, False)
    _, x0, _, lx = G.src_coords(W, w, False)
    ly = ly.view(-1, 1)
    rows = x.index_select(-2, y0) * (1.0 - ly) + x.index_select(-2, y1) * ly
    f0 = w - 1 - x0
    return rows.index_select(-1, f0) * (1.0 - lx) + rows.index_select(-1, (f0 + 1).clamp_max(w - 1)) * lx


def _spread_adjoint(q, h, w, wide=True):
    """Upper bound of what a per-pixel quantity q (b, C1, H, W) >= 0 can leak into low-res cells through WEIGHT errors: q is
    added, un-weighted, to every cell within one of the pixel's taps on either axis (a coordinate off by an ulp at a cell
    boundary moves a vanishing weight onto the next cell).  wide=False: the pixel's own taps only (a clamped tap counts twice)."""
    H, W = q.shape[-2:]
    _, y0, y1, _ = G.src_coords(H, h, False)
    _, x0, x1, _ = G.src_coords(W, w, False)
    rows = torch.zeros(q.shape[:-2] + (h, W), dtype=torch.float64)
    for iy in ((y0 - 1).clamp_min(0), y0, y1, (y1 + 1).clamp_max(h - 1)) if wide else (y0, y1):
        rows.index_add_(-2, iy, q)
    out = torch.zeros(q.shape[:-2] + (h, w), dtype=torch.float64)
    for ix in ((x0 - 1).clamp_min(0), x0, x1, (x1 + 1).clamp_max(w - 1)) if wide else (x0, x1):
        out.index_add_(-1, ix, rows)
    return out


def seg_ref(logits, label, H, W, ignore=255, flip=0, balanced=1, g=1.0, variant="ok", want_grad=True):
    """Fused bilinear up-sample (align_corners False; flip: of the w-flipped low-res logits) + cross entropy in float64.
    logits (b, C1, h, w) fp32 values, label (b, H, W) with values in [0, C1) or `ignore`.

    ce, ce_bound  per pixel (0 where ignored).  ce_bound = 2 Bz + (C1 + 8) 2^-24 max(1, |lse|, max_c |z_c|): Bz, the largest
                  glue_ref.bilinear_bound over the channels, enters twice (z_label and, 1-Lipschitz in the max norm, lse); the
                  running log-sum-exp costs at most one rounding per channel of a quantity <= max(1, |lse|, max |z|), plus
                  expf / logf / the final subtraction.
    sums, sums_bound   {ce_bg, n_bg, ce_fg, n_fg}; the ce sums carry their pixels' bounds summed, the block tree (8 levels of a
                  256-thread block sum and one more: 9 2^-24 sum |ce|), nblocks 2^-29 for the rounding of every block's partial to
                  Q28 fixed point and one final rounding; the counts are integers: bound 0.
    loss          float64 value of finish 2 (balanced) or the plain mean (sum / count, 0 when nothing is valid).
    dlogits, dlogits_bound (b, C1, h, w): g * d loss / d logits by float64 autograd through this very function, and

        dlogits[cell, c] = sum_p coef_p w_p(cell) r_pc,   r_pc = softmax_c(z_p) - [c == label_p],
        coef_p = 0.5 g / (n_bg + 1e-6) | 0.5 g / (n_fg + 1e-6) | g / (n_bg + n_fg),  w_p(cell) the merged bilinear tap weight.

      A correct fp32 kernel is off per term by
        |coef_p| w_p ( softmax_c (e_p + (|z_c - lse| + 4) 2^-24) + 6 2^-24 |r_pc| )        e_p = ce_bound of the pixel: it bounds the
                      error of z_c - lse, and exp turns an absolute error of its argument into a relative one of its value; 4 + 6
                      roundings cover the subtraction, expf, the indicator, coef (three operations) and the two weight products,
      + |coef_p| |r_pc| (dy_p + dx_p)   a coordinate off by d (glue_ref's 2 ulp, 0 at dyadic scales) moves a tap weight by d; charged
                      un-weighted to every cell next to the pixel's taps (_spread_adjoint),
      and the cell's sum of n (its pixels with a non-zero weight) terms, added in ANY order (atomics), by n 2^-24 sum |terms|.
      All three are summed over the cell's own footprint: border cells are held to their own values."""
    x = logits.detach().double().clone().requires_grad_(want_grad)
    b, C1, h, w = x.shape
    lab = label.long()
    valid = lab != ignore
    lab0 = torch.where(valid, lab, torch.zeros_like(lab))
    up = up64_flipped(x, H, W, variant) if flip else up64(x, H, W, variant)
    lse = torch.logsumexp(up, 1)
    zl = up.gather(1, lab0.unsqueeze(1)).squeeze(1)
    ce = torch.where(valid, lse - zl, torch.zeros_like(lse))
    bg, fg = valid & (lab == 0), valid & (lab != 0)
    s = [ce[bg].sum(), bg.sum().double(), ce[fg].sum(), fg.sum().double()]
    if balanced:
        loss = 0.5 * (s[0] / (s[1] + 1e-6) + s[2] / (s[3] + 1e-6))
    else:
        loss = (s[0] + s[2]) / (s[1] + s[3]).clamp_min(1.0)
    out = NS(up=up.detach(), lse=lse.detach(), ce=ce.detach(), sums=torch.stack([v.detach() for v in s]), loss=float(loss.detach()))
    xin = (torch.flip(logits, dims=[3]) if flip else logits).double()
    Bz = G.bilinear_bound(xin, H, W, False).amax(1)
    zmax = out.up.abs().amax(1)
    e = 2.0 * Bz + (C1 + 8) * EPS24 * torch.maximum(torch.ones_like(zmax), torch.maximum(out.lse.abs(), zmax))
    out.ce_bound = torch.where(valid, e, torch.zeros_like(e))
    nblk = seg_grid_blocks(b, h, w, H, W)
    sb = []
    for m, tot in ((bg, out.sums[0]), (fg, out.sums[2])):
        sb += [float(out.ce_bound[m].sum() + 9 * EPS24 * out.ce[m].abs().sum() + nblk * 2.0 ** -29 + EPS24 * tot.abs()), 0.0]
    out.sums_bound = torch.tensor(sb, dtype=torch.float64)
    if not want_grad:
        return out
    (loss * g).backward()
    out.dlogits = x.grad.clone() if x.grad is not None else torch.zeros_like(x)
    # ---- the gradient bound, cell by cell
    if balanced:
        coef = torch.where(lab == 0, 0.5 * g / (s[1].detach() + 1e-6), 0.5 * g / (s[3].detach() + 1e-6))
    else:
        coef = torch.full(lab.shape, 1.0, dtype=torch.float64) * g / (s[1] + s[3]).detach().clamp_min(1.0)
    coef = torch.where(valid, coef, torch.zeros_like(coef)).abs().unsqueeze(1)               # (b, 1, H, W)
    zrel = out.up - out.lse.unsqueeze(1)
    sm = zrel.exp()
    r = (sm - F.one_hot(lab0, C1).permute(0, 3, 1, 2).double()).abs()
    per_term = coef * (sm * (e.unsqueeze(1) + (zrel.abs() + 4.0) * EPS24) + 6.0 * EPS24 * r)
    mag = coef * r

    def adjoint(q):                                         # sum_p w_p(cell) q_p: the transpose of the up-sampling, by autograd
        t = torch.zeros(b, C1, h, w, dtype=torch.float64, requires_grad=True)
        u = up64_flipped(t, H, W) if flip else up64(t, H, W)
        (u * q).sum().backward()
        return t.grad
    hd, wd = G.src_coords(H, h, False), G.src_coords(W, w, False)
    dy = (2.0 * G.ulp32(hd[0]) if not G._dyadic(h, H, False) else torch.zeros(H, dtype=torch.float64)).view(-1, 1)
    dx = (2.0 * G.ulp32(wd[0]) if not G._dyadic(w, W, False) else torch.zeros(W, dtype=torch.float64)).view(1, -1)
    leak = _spread_adjoint(mag * (dy + dx), h, w)
    if flip:
        leak = torch.flip(leak, dims=[3])
    n_cell = _spread_adjoint(valid.double().unsqueeze(1), h, w, wide=False)                  # valid pixels with a tap on the cell
    if flip:
        n_cell = torch.flip(n_cell, dims=[3])
    out.dlogits_bound = adjoint(per_term) + leak + n_cell * EPS24 * adjoint(mag)
    return out


def seg_fp32(logits, label, H, W, ignore=255, flip=0, balanced=1, g=1.0):
    """The same in torch fp32 (F.interpolate + F.cross_entropy + autograd): what the bounds must admit."""
    x = logits.detach().float().clone().requires_grad_(True)
    lab = label.long()
    up = F.interpolate(torch.flip(x, dims=[3]) if flip else x, size=(H, W), mode="bilinear", align_corners=False)
    ce = F.cross_entropy(up, lab, ignore_index=ignore, reduction="none")
    bg, fg = lab == 0, (lab != 0) & (lab != ignore)
    s = [(ce * bg).sum(), bg.sum().float(), (ce * fg).sum(), fg.sum().float()]
    if balanced:
        loss = 0.5 * (s[0] / (s[1] + 1e-6) + s[2] / (s[3] + 1e-6))
    else:
        loss = (s[0] + s[2]) / (s[1] + s[3]).clamp_min(1.0)
    (loss * g).backward()
    return NS(ce=ce.detach(), sums=torch.stack([v.detach() for v in s]), dlogits=x.grad)


def pseudo_ref(logits, other, H, W, ignore, thr):
    """Consistency targets: (label where kept else ignore, kept mask, arg-max, top-1 - top-2 margin of the up-sampled logits, the
    largest bilinear_bound over the channels, conf = max softmax, its fp32 bound).  A pixel's decision is PROVEN only when the
    margin exceeds twice the bound (arg-max) and |conf - thr| exceeds the conf bound (threshold)."""
    C1 = logits.shape[1]
    up = up64(logits, H, W)
    arg, margin, bound = G.upsample_argmax64(logits, H, W)
    lse = torch.logsumexp(up, 1)
    conf = (up.amax(1) - lse).exp()
    zmax = up.abs().amax(1)
    cb = conf * (2.0 * bound + (C1 + 8) * EPS24 * torch.maximum(torch.ones_like(zmax), torch.maximum(lse.abs(), zmax))) + 4 * EPS24 * conf
    keep = (other.long() == ignore) & (conf > thr)
    lab = torch.where(keep, arg, torch.full_like(arg, ignore))
    return NS(label=lab, keep=keep, arg=arg, margin=margin, bound=bound, conf=conf, conf_bound=cb)


# (h, w, H, W): what each shape reaches is said next to it
SEG_SHAPES = [(1, 1, 16, 16),          # one cell, every tap clamped
              (2, 3, 32, 48),          # factor 16 both ways: the wave-reduced backward
              (2, 1, 64, 32),          # factor 32
              (1, 2, 48, 32),          # factors 48 and 16
              (2, 2, 32, 40),          # 16 (fast) x 20 (generic): the generic path decides
              (4, 4, 60, 60),          # integer 15: generic
              (3, 5, 17, 23),          # non-integer
              (5, 3, 5, 3)]            # identity
SEG_BIG = (28, 28, 448, 448)
SEG_PATTERNS = ("random", "all_ignored", "bg_only", "fg_only", "corners")
SEG_C1_DET = (63, 64, 127, 128, 255)   # the gather backward's block size: 256 up to 63, 128 from 64, 64 from 128


def seg_cases():
    """dicts (h, w, H, W, b, C1, flip, balanced, f32lab, pattern, det_only, scale): every shape with both flips, both balanced
    values, both label types and b in {1, 3}; every label pattern on a fast and on a generic shape; every C1.
    The knobs are not tied to one another: over the eight shapes (index bits i0 i1 i2) the first case of a shape takes flip = i0,
    float labels = i1, balanced = i2, b = 3 iff i0 = i1, C1 = 21 iff i1 = i2 (else 2), scale 3 iff i0 = i2 (else 30) -- six distinct
    parities, so every pair of knobs meets in all four combinations -- and the second case is its complement in every knob."""
    cases = []
    for i, s in enumerate(SEG_SHAPES):
        i0, i1, i2 = i & 1, (i >> 1) & 1, (i >> 2) & 1
        for inv in (0, 1):
            cases.append(dict(shape=s, b=3 if (i0 ^ i1) == inv else 1, C1=21 if (i1 ^ i2) == inv else 2, flip=i0 ^ inv, balanced=i2 ^ inv,
                              f32lab=i1 ^ inv, pattern="random", det_only=False, scale=3.0 if (i0 ^ i2) == inv else 30.0))
    for si, s in enumerate((SEG_SHAPES[1], SEG_SHAPES[6])):
        for j, p in enumerate(SEG_PATTERNS[1:]):
            for bal in (0, 1):
                cases.append(dict(shape=s, b=3 if (j + bal + si) % 2 == 0 else 1, C1=21, flip=(j + bal) % 2, balanced=bal, f32lab=j % 2,
                                  pattern=p, det_only=False, scale=3.0))
    for si, s in enumerate((SEG_SHAPES[1], SEG_SHAPES[6])):
        cases.append(dict(shape=s, b=1, C1=1, flip=1 - si, balanced=1 - si, f32lab=si, pattern="random", det_only=False, scale=3.0))
        for j, C1 in enumerate(SEG_C1_DET):
            cases.append(dict(shape=s, b=1, C1=C1, flip=j % 2, balanced=(j + si) % 2, f32lab=(j // 2 + si) % 2, pattern="random",
                              det_only=True, scale=3.0))
    cases.append(dict(shape=SEG_BIG, b=1, C1=21, flip=1, balanced=1, f32lab=0, pattern="random", det_only=False, scale=3.0))
    return cases


def seg_case_id(c):
    return "{}x{}to{}x{}-b{}-C{}-f{}-bal{}-{}-{}".format(*c["shape"], c["b"], c["C1"], c["flip"], c["balanced"],
                                                         "f32" if c["f32lab"] else "i64", c["pattern"])


def seg_inputs(c, ignore=255):
    """(logits (b, C1, h, w) fp32, label (b, H, W) int64) of a case"""
    h, w, H, W = c["shape"]
    gen = torch.Generator().manual_seed(h * 1000003 + w * 10007 + H * 101 + W + c["C1"] * 7 + c["b"])
    logits = torch.randn(c["b"], c["C1"], h, w, generator=gen) * c["scale"]
    lab = torch.randint(0, c["C1"], (c["b"], H, W), generator=gen)
    p = c["pattern"]
    if p == "random":
        lab[torch.rand(c["b"], H, W, generator=gen) < 0.6] = ignore
    elif p == "all_ignored":
        lab[:] = ignore
    elif p == "bg_only":
        lab[lab != 0] = ignore
        lab[:, 0, 0] = 0
    elif p == "fg_only":
        lab[lab == 0] = 1
    elif p == "corners":
        keep = torch.zeros_like(lab, dtype=torch.bool)
        for yy in (0, H - 1):
            for xx in (0, W - 1):
                keep[:, yy, xx] = True
        lab[~keep] = ignore
        lab[:, 0, 0] = 0
    return logits, lab


# =========================================================================================== PTC
PTC_HW = (1, 2, 95, 96, 97, 257, 363)
PTC_CASES = [(hw, b, form, ign) for hw in PTC_HW for b in (1, 3) for form, ign in (("label", 255), ("label", 7), ("mask", 255))]


def ptc_case_inputs(hw, b, form, ign):
    return ptc_inputs(b, hw, form, ign, seed=hw * 10 + b)


def ptc_kind(hw, label=None, mask=None, ignore=255, count_diagonal=False):
    """(b, hw, hw) int: 1 positive, 0 negative, -1 ignored.  label (b, hw): same label / different, ignored where either is
    `ignore` or on the diagonal.  mask (b, hw, hw): 1 / 0, every other value is ignored."""
    if mask is not None:
        return torch.where(mask == 1, 1, torch.where(mask == 0, 0, -1))
    lr, lc = label.unsqueeze(2), label.unsqueeze(1)
    kind = (lr == lc).long()
    dead = (lr == ignore) | (lc == ignore)
    if not count_diagonal:
        dead = dead | torch.eye(hw, dtype=torch.bool).unsqueeze(0)
    return torch.where(dead, torch.full_like(kind, -1), kind)


def ptc_ref(cos, kind):
    """sums {sum_pos |cos|, n_pos, sum_neg |cos|, n_neg} and the loss 0.5 (1 - s0 / (s1 + 1)) + 0.5 s2 / (s3 + 1) in float64 of a
    given cosine matrix (entries of ignored pairs are never read: they may be NaN).  Bound of the |cos| sums: a thread adds at
    most ceil(hw / 256) ceil(hw / min(hw, 96)) values in a chain, the block tree adds 9 levels, every block's partial is rounded
    to Q28 (2^-29 each) and the result once more."""
    b, hw, _ = cos.shape
    a = torch.where(kind >= 0, cos.double().abs(), torch.zeros((), dtype=torch.float64))
    pos, neg = kind == 1, kind == 0
    s = torch.stack([a[pos].sum(), pos.sum().double(), a[neg].sum(), neg.sum().double()])
    gx = min(hw, 96)
    depth = math.ceil(hw / 256) * math.ceil(hw / gx) + 9
    bound = torch.tensor([float(depth * EPS24 * s[0] + gx * b * 2.0 ** -29 + EPS24 * s[0]), 0.0,
                          float(depth * EPS24 * s[2] + gx * b * 2.0 ** -29 + EPS24 * s[2]), 0.0], dtype=torch.float64)
    loss = 0.5 * (1 - s[0] / (s[1] + 1)) + 0.5 * s[2] / (s[3] + 1)
    return NS(sums=s, sums_bound=bound, loss=float(loss.detach()))


def ptc_bwd_ref(cos, kind, n_pos, n_neg, g):
    """d loss / d cos_signed = sign(cos) (-0.5 g / (n_pos + 1) | 0.5 g / (n_neg + 1) | 0), sign(0) = 0, and 0 on ignored pairs whatever
    they hold.  Three fp32 operations: bound 4 2^-24 |value|."""
    sg = torch.where(kind >= 0, torch.sign(torch.nan_to_num(cos.double())), torch.zeros((), dtype=torch.float64))
    cp = torch.tensor(-0.5 * g / (n_pos + 1.0), dtype=torch.float64)
    v = sg * torch.where(kind == 1, cp, torch.tensor(0.5 * g / (n_neg + 1.0), dtype=torch.float64))
    v = torch.where(kind >= 0, v, torch.zeros_like(v))
    return v, 4 * EPS24 * v.abs()


def ptc_inputs(b, hw, form, ignore, seed):
    """(cos (b, hw, hw) fp32 with exact zeros sprinkled in, label or None, mask or None).  The explicit mask is NOT symmetric and
    holds {0, 1, 2, -1, 255}; labels hold 4 classes and ~30 % `ignore`."""
    gen = torch.Generator().manual_seed(seed)
    cos = torch.rand(b, hw, hw, generator=gen) * 2 - 1
    cos[torch.rand(b, hw, hw, generator=gen) < 0.05] = 0.0
    if form == "mask":
        vals = torch.tensor([0, 1, 2, -1, 255])
        return cos, None, vals[torch.randint(0, 5, (b, hw, hw), generator=gen)]
    lab = torch.randint(0, 4, (b, hw), generator=gen)
    lab[torch.rand(b, hw, generator=gen) < 0.3] = ignore
    return cos, lab, None


# =========================================================================================== F.normalize rows
L2_ROWS, L2_C = (1, 5, 9), (1, 63, 64, 65, 130)


def _chain(c):
    """a wave's sum over c channels: ceil(c / 64) terms per lane in a chain, 6 shuffle levels, and slack for the products"""
    return math.ceil(c / 64) + 8


def l2norm_ref(x, eps):
    """F.normalize(x, p=2, dim=-1, eps) of rows x (rows, c): (xhat, norm, xhat bound, norm bound)"""
    x = x.double()
    c = x.shape[-1]
    nrm = x.norm(dim=-1)
    xh = x / nrm.clamp_min(eps).unsqueeze(-1)
    rel = (_chain(c) + 2) * EPS24
    return xh, nrm, rel * xh.abs(), rel * nrm


def l2norm_bwd_ref(dxh, xh, nrm, eps, guard=True):
    """dx = (dxh - xh <xh, dxh>) / max(norm, eps); where norm <= eps the clamp has zero slope and dx = dxh / eps (guard=False: the
    projection kept there, the mistake).  xh / norm are the values handed to the kernel."""
    dxh, xh, nrm = dxh.double(), xh.double(), nrm.double()
    c = xh.shape[-1]
    s = (xh * dxh).sum(-1, keepdim=True)
    proj = torch.where(nrm.unsqueeze(-1) > eps, s, torch.zeros_like(s)) if guard else s
    inv = 1.0 / nrm.clamp_min(eps).unsqueeze(-1)
    dx = (dxh - xh * proj) * inv
    es = _chain(c) * EPS24 * (xh * dxh).abs().sum(-1, keepdim=True)
    bound = inv * (xh.abs() * es + 4 * EPS24 * (dxh.abs() + (xh * proj).abs()))
    return dx, bound


# =========================================================================================== cosine over tokens
COS_N, COS_C = (1, 15, 16, 17, 50), (1, 63, 64, 65, 130)


def cos_ref(a, b, eps):
    """cosine over the tokens (dim 1) of a, b (B, n, c): out (B, c), stats (B, c, 3) = {dot, |a|^2, |b|^2} and their bounds.  16
    row groups: ceil(n / 16) terms in a chain per thread and 16 more across the groups."""
    a, b = a.double(), b.double()
    n = a.shape[1]
    depth = (math.ceil(n / 16) + 17) * EPS24
    st = torch.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], -1)
    sb = depth * torch.stack([(a * b).abs().sum(1), (a * a).sum(1), (b * b).sum(1)], -1)
    na, nb = st[..., 1].sqrt().clamp_min(eps), st[..., 2].sqrt().clamp_min(eps)
    out = st[..., 0] / (na * nb)
    ob = (sb[..., 0] + st[..., 0].abs() * (depth + 4 * EPS24)) / (na * nb)
    return out, st, ob, sb


def cos_bwd_ref(a, b, st, gv, eps, variant="ok"):
    """gv * d cos / d b from GIVEN stats (B, c, 3): a / (na nb) - [|b| > eps] cos b / nb^2 with the clamped norms -- below eps the
    clamp has zero slope: the derivative of dot / (max(|a|, eps) max(|b|, eps)), the function computed.  (torch's autograd of
    F.cosine_similarity agrees above eps only: it clamps its norms in place outside the graph and back-propagates as if it had
    not, see tests/test_loss_ref_host.py.)  variant "second_term_kept": without that guard;
    "clamp_product": one clamp on the product na * nb.
    Bound, counting every fp32 rounding (u = 2^-24 each, division and square root correctly rounded) from the given stats on:
    na, nb one each, P = na nb three in all; term 1 = a / P: 4; cos = dot / P: 4, cos b: 5, nb nb: 3, term 2 = cos b / (nb nb): 9;
    the subtraction one on either term, gv = g gmul one, the product with gv one: 7 u |term 1| + 12 u |term 2|, to first order."""
    a, b, st = a.double(), b.double(), st.double().unsqueeze(1)                               # stats (B, 1, c, 3)
    ra, rb = st[..., 1].sqrt(), st[..., 2].sqrt()
    if variant == "clamp_product":
        den = (ra * rb).clamp_min(eps)
        t1, t2 = a / den, torch.where(ra * rb > eps, st[..., 0] / den * b / (rb * rb).clamp_min(1e-300), torch.zeros_like(b))
    else:
        na, nb = ra.clamp_min(eps), rb.clamp_min(eps)
        t1 = a / (na * nb)
        t2 = st[..., 0] / (na * nb) * b / (nb * nb)
        if variant == "ok":
            t2 = torch.where(rb > eps, t2, torch.zeros_like(t2))
    return gv * (t1 - t2), EPS24 * abs(gv) * (7 * t1.abs() + 12 * t2.abs())


def cos_inputs(B, n, c, seed, eps):
    """a, b (B, n, c): column 0 of b is zero and column c - 1 has |b| = 0.3 eps; the same for a in columns 1 and c - 2 (where c allows)"""
    gen = torch.Generator().manual_seed(seed)
    a, b = torch.randn(B, n, c, generator=gen), torch.randn(B, n, c, generator=gen)
    b[:, :, 0] = 0.0
    if c > 1:
        b[:, :, c - 1] *= 0.3 * eps / b[:, :, c - 1].norm(dim=1, keepdim=True)
    if c > 3:
        a[:, :, 1] = 0.0
        a[:, :, c - 2] *= 0.3 * eps / a[:, :, c - 2].norm(dim=1, keepdim=True)
    return a, b


def cos_cases():
    """(B, n, c, strided) of every cosine case of the GPU suite: dense for B = 1, gapped (ld > c, an image stride) for B = 3, and the
    one case whose B n c exceeds the backward's 4096 x 256 threads (a second trip of its grid-stride loop)"""
    return [(B, n, c, B == 3) for n in COS_N for c in COS_C for B in (1, 3)] + [COS_GRID_STRIDE + (False,)]


COS_GRID_STRIDE = (2, 65, 8192)


def cos_case_inputs(B, n, c, eps):
    return cos_inputs(B, n, c, n * 131 + c + B, eps)


# ---- the recorded gradient of the parent kernel (tests/golden/cos_bwd_workload.npz)
COS_WORKLOAD = (2, 784, 768)                 # (B, tokens, channels) of the discrepancy loss at 448^2, ViT-B


def hashed_i24(count, seed):
    """`count` signed 24-bit integers (int64 array) from a 64-bit integer mix of the index: the same on every machine and library
    version (no generator involved); scaled by 2^-22 they are float32 in [-2, 2) and sums of their products are exact in int64"""
    h = (np.arange(count, dtype=np.uint64) + np.uint64(seed)) * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xff51afd7ed558ccd)
    h ^= h >> np.uint64(33)
    return (h >> np.uint64(40)).astype(np.int64) - (1 << 23)


def cos_workload_inputs():
    """a, b (B, n, c) float32 of the workload's shape, every column far above eps, and the stats {dot, |a|^2, |b|^2} (B, c, 3) the
    backward is handed: computed here in exact integer arithmetic and rounded once, so that the recorded gradient depends on
    dupl_cos_sim_bwd alone"""
    B, n, c = COS_WORKLOAD
    ka, kb = hashed_i24(B * n * c, 1).reshape(B, n, c), hashed_i24(B * n * c, 1 << 40).reshape(B, n, c)
    st = np.stack([(ka * kb).sum(1), (ka * ka).sum(1), (kb * kb).sum(1)], -1)                # |k| < 2^23, n < 2^10: below 2^56
    stats = (st.astype(np.float64) * 2.0 ** -44).astype(f32)
    a, b = (ka.astype(np.float64) * 2.0 ** -22).astype(f32), (kb.astype(np.float64) * 2.0 ** -22).astype(f32)
    return torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(stats)


def digest(t):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t).tobytes()).hexdigest()


# =========================================================================================== small reductions
SMALL_N = (1, 255, 256, 257, 1000)


def mean_accum_ref(x, loss0, mul):
    """loss0 + mul * sum(x): ceil(n / 256) terms in a chain per thread + the block tree"""
    x = x.double()
    v = float(loss0) + mul * float(x.sum())
    bound = (math.ceil(x.numel() / 256) + 9) * EPS24 * abs(mul) * float(x.abs().sum()) + 2 * EPS24 * (abs(v) + abs(float(loss0)))
    return v, bound


def msm_ref(x, y, g=1.0, divide_by=None):
    """F.multilabel_soft_margin_loss (b, C): mean over ALL elements of -(y logsig(x) + (1 - y) logsig(-x)); dx = g (sigmoid(x) - y) / n.
    Per element the fp32 value is off by at most 8 2^-24 (|x| + 1)(|y| + |1 - y|); the sum as mean_accum_ref.  dx: 5 operations,
    plus what is below fp32's normal range (1e-37) at x = -100."""
    x, y = x.double(), y.double()
    n = x.numel()
    el = -(y * F.logsigmoid(x) + (1 - y) * F.logsigmoid(-x))
    loss = float(el.sum()) / (divide_by or n)
    bound = float((8 * EPS24 * (x.abs() + 1) * (y.abs() + (1 - y).abs())).sum() + (math.ceil(n / 256) + 9) * EPS24 * el.abs().sum()) / n \
        + 2 * EPS24 * abs(loss)
    sig = torch.sigmoid(x)
    dx = g * (sig - y) / n
    return loss, bound, dx, 5 * EPS24 * abs(g) * (sig + y.abs()) / n + 1e-37


def loss_total_ref(terms, add, group, weight, n_groups):
    """dupl_loss_total in numpy float32: G_g = the v_i of group g summed left to right in list order, v_i = add_i + term_i only where
    add_i != 0; total = ((w_0 G_0 + w_1 G_1) + w_2 G_2) + ...; an empty group has G = 0.  Returns (total, G[n_groups])."""
    Gs = np.zeros(n_groups, dtype=f32)
    total = f32(0)
    for g in range(n_groups):
        G, first = f32(0), True
        for t, a, gi in zip(terms, add, group):
            if gi != g:
                continue
            v = f32(t)
            if f32(a) != 0:
                v = f32(f32(a) + v)
            G = v if first else f32(G + v)
            first = False
        Gs[g] = G
        wg = f32(f32(weight[g]) * G)
        total = wg if g == 0 else f32(total + wg)
    return total, Gs


def loss_total_bwd_ref(gout, group, weight):
    return np.array([f32(f32(gout) * f32(weight[gi])) for gi in group], dtype=f32)


# =========================================================================================== LayerNorm
LN_D = (4, 252, 256, 260, 768, 772, 1024, 1028, 2048)
LN_FWD_ROWS = (1, 3, 4, 5, 9)
LN_BWD_ROWS = (1, 15, 16, 17, 33)
LN_RPW = (0, 1, 2, 8, 64)


def _ln_depth(D):
    """a row sum: per lane ceil(D / 256) float4 chunks of 3 additions each in a chain, 6 shuffle levels, the division"""
    return 3 * math.ceil(D / 256) + 8


def ln_inputs(rows, D, seed, special=True):
    """x (rows, D), gamma, beta; with `special` row 0 is constant and the last row sits at offset 1e4 (where rows allow)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=gen) * 2 + 0.5
    if special and rows >= 3:
        x[0] = 1.25
        x[rows - 1] += 1e4
    return x, torch.randn(D, generator=gen), torch.randn(D, generator=gen)


def ln_fwd_ref(x, gamma, beta, eps, one_pass=False):
    """(y, mean, rstd) in float64 and their bounds, row by row.  The fp32 mean is off by dm = depth 2^-24 mean |x| -- for a row at
    offset 1e4 that is 1e4 * rstd units of 2^-24 in y, not a constant; a constant shift of the centred row changes the variance
    only in second order (dm^2), its own roundings by (depth + 4) 2^-24 var.  one_pass: var = E x^2 - mean^2 evaluated in fp32
    (the mistake: it cancels)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    D = x.shape[-1]
    depth = _ln_depth(D)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    var = (xc * xc).mean(-1, keepdim=True)
    if one_pass:
        x32 = x.float()
        var = ((x32 * x32).mean(-1, keepdim=True) - x32.mean(-1, keepdim=True) ** 2).double()
    rstd = 1.0 / torch.sqrt(var + eps)
    y = xc * rstd * gamma + beta
    dm = depth * EPS24 * x.abs().mean(-1, keepdim=True)
    rel_r = 0.5 * ((depth + 4) * EPS24 * var + dm * dm) / (var + eps) + 3 * EPS24
    yb = gamma.abs() * rstd * (dm + EPS24 * xc.abs()) + (xc * rstd * gamma).abs() * (rel_r + 3 * EPS24) + EPS24 * y.abs()
    return NS(y=y, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), y_bound=yb, mean_bound=(dm + EPS24 * mean.abs()).squeeze(-1),
              rstd_bound=(rstd * rel_r).squeeze(-1))


def ln_fwd_np32(x, gamma, beta, eps):
    """two-pass LayerNorm in numpy float32, what the bounds must admit"""
    x, gamma, beta = (t.numpy().astype(f32) for t in (x, gamma, beta))
    D = f32(x.shape[-1])
    mean = (x.sum(-1, keepdims=True, dtype=f32) / D).astype(f32)
    xc = (x - mean).astype(f32)
    var = ((xc * xc).sum(-1, keepdims=True, dtype=f32) / D).astype(f32)
    rstd = (f32(1) / np.sqrt(var + f32(eps))).astype(f32)
    return (xc * rstd * gamma + beta).astype(f32), mean[:, 0], rstd[:, 0]


def ln_bwd_ref(dy, x, gamma, mean, rstd, dres=None, dg0=None, db0=None, amax_before_dres=False):
    """dx = [dres +] rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, xhat = (x - mean) rstd with the GIVEN mean / rstd;
    dgamma = dg0 + sum_rows dy xhat, dbeta = db0 + sum_rows dy; amax = max |dx| (amax_before_dres: of dx without dres, the mistake).
    Bounds per element of the row: xhat is off by 2 2^-24 |xhat|, the two row means by their chains, and the column sums by
    (rows + 3) 2^-24 sum |terms| (any order) plus what xhat's error carries in."""
    dy, x, gamma, mean, rstd = (t.double() for t in (dy, x, gamma, mean, rstd))
    rows, D = x.shape
    depth = _ln_depth(D)
    mu, rs = mean.unsqueeze(-1), rstd.unsqueeze(-1)
    xh = (x - mu) * rs
    g = dy * gamma
    m1, m2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    core = rs * (g - m1 - xh * m2)
    dx = core + (dres.double() if dres is not None else 0.0)
    exh = 2 * EPS24 * xh.abs()
    em1 = (depth + 1) * EPS24 * g.abs().mean(-1, keepdim=True)
    em2 = (depth + 2) * EPS24 * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * exh).mean(-1, keepdim=True)
    dxb = rs * (EPS24 * g.abs() + em1 + xh.abs() * em2 + m2.abs() * exh + 3 * EPS24 * (g.abs() + m1.abs() + (xh * m2).abs())) \
        + 2 * EPS24 * (dx.abs() + core.abs())
    dg = (dy * xh).sum(0) + (dg0.double() if dg0 is not None else 0.0)
    db = dy.sum(0) + (db0.double() if db0 is not None else 0.0)
    dgb = (rows + 3) * EPS24 * (dy * xh).abs().sum(0) + (dy.abs() * exh).sum(0) + 2 * EPS24 * dg.abs() \
        + (EPS24 * dg0.double().abs() if dg0 is not None else 0.0)
    dbb = (rows + 3) * EPS24 * dy.abs().sum(0) + 2 * EPS24 * db.abs() + (EPS24 * db0.double().abs() if db0 is not None else 0.0)
    amax = float((core if amax_before_dres else dx).abs().max())
    return NS(dx=dx, dgamma=dg, dbeta=db, amax=amax, dx_bound=dxb, dgamma_bound=dgb, dbeta_bound=dbb)


# =========================================================================================== inputs of the remaining case lists
def l2_inputs(rows, c, seed, eps):
    """x (rows, c) and an up-stream gradient; row 0 is all zero and the last row has 0 < |x| < eps (where rows allow)"""
    gen = torch.Generator().manual_seed(seed)
    x, dxh = torch.randn(rows, c, generator=gen), torch.randn(rows, c, generator=gen)
    if rows >= 2:
        x[0] = 0.0
    x[rows - 1] *= 0.3 * eps / x[rows - 1].norm()
    return x, dxh


def msm_shape(n):
    """(b, C) with b * C == n"""
    return {1: (1, 1), 255: (3, 85), 256: (4, 64), 257: (1, 257), 1000: (8, 125)}[n]


def msm_inputs(n, seed):
    """logits with +-100 among them, soft targets in [0, 1] with exact 0 / 1 among them"""
    b, C = msm_shape(n)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(b, C, generator=gen) * 3
    y = torch.rand(b, C, generator=gen)
    flat_x, flat_y = x.view(-1), y.view(-1)
    flat_x[0] = -100.0
    flat_y[0] = 1.0
    if n > 4:
        flat_x[1], flat_x[2], flat_x[3] = 100.0, 100.0, -100.0
        flat_y[1], flat_y[2], flat_y[3] = 0.0, 1.0, 0.0
    return x, y


def ln_bwd_inputs(rows, D, seed, with_dres=True):
    """x (one row at offset 30), gamma, dy, dres of a backward case"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=gen) * 2 + 0.5
    x[rows // 2] += 30.0
    gamma = torch.randn(D, generator=gen)
    dy = torch.randn(rows, D, generator=gen) * 0.1
    dres = torch.randn(rows, D, generator=gen) * 0.1 if with_dres else None
    return x, gamma, dy, dres
