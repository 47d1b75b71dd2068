"""The references of tests/glue_ref.py and their bounds, checked on the CPU before the GPU suite trusts them."""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as G


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


CASE_IDS = [f"{a}x{b}-{c}x{d}-{'ac' if e else 'hp'}" for a, b, c, d, e in G.RESIZE_CASES]


@pytest.mark.parametrize("case", G.RESIZE_CASES, ids=CASE_IDS)
def test_bilinear64_is_torch_float64(case):
    Hi, Wi, Ho, Wo, al = case
    x = rnd(2, 3, Hi, Wi, seed=1)
    ref = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=al)
    assert float((G.bilinear64(x, Ho, Wo, al) - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", G.RESIZE_CASES, ids=CASE_IDS)
def test_bound_admits_torch_fp32(case):
    """Not too tight: torch's fp32 CPU interpolate lies within bilinear_bound of bilinear64 at every pixel."""
    Hi, Wi, Ho, Wo, al = case
    worst = 0.0
    for seed in (1, 2, 3):
        x = rnd(2, 3, Hi, Wi, seed=seed)
        got = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=al).double()
        ratio = float(((got - G.bilinear64(x, Ho, Wo, al)).abs() / G.bilinear_bound(x, Ho, Wo, al)).max())
        worst = max(worst, ratio)
    print(f"torch fp32 {CASE_IDS[G.RESIZE_CASES.index(case)]}: worst err / bound {worst:.3f}")
    assert worst <= 1.0, f"worst err / bound {worst:.3f}"


def _swapped(out, inn, align):
    return G.src_coords(out, inn, not align)


def _no_clamp(out, inn, align):
    if align:
        return G.src_coords(out, inn, align)
    o = torch.arange(out, dtype=torch.float64)
    r = (inn / out) * (o + 0.5) - 0.5
    i0 = r.floor().long().clamp(0, inn - 1)          # stays in bounds; the weight goes negative instead
    return r, i0, (i0 + 1).clamp_max(inn - 1), r - i0.double()


def _x1_unclamped(out, inn, align):
    r, i0, _, l = G.src_coords(out, inn, align)
    # the tap after the last one wraps to a wrong in-bounds sample instead of repeating the edge
    i1 = torch.where(i0 + 1 > inn - 1, torch.zeros_like(i0), torch.min(i0 + 1, torch.full_like(i0, inn - 1)))
    return r, i0, i1, l


def _affected(variant, out, inn, align):
    """Whether the variant changes any tap or weight along an axis with more than one input sample."""
    if inn <= 1:
        return False
    a, b = variant(out, inn, align), G.src_coords(out, inn, align)
    # compare the resampling matrices: a tap with zero weight does not count
    eff_a = torch.stack(((1 - a[3]), a[3])), torch.stack((a[1], a[2]))
    eff_b = torch.stack(((1 - b[3]), b[3])), torch.stack((b[1], b[2]))
    wa = torch.zeros(out, inn, dtype=torch.float64)
    wb = torch.zeros(out, inn, dtype=torch.float64)
    for k in range(2):
        wa.scatter_add_(1, eff_a[1][k].view(-1, 1), eff_a[0][k].view(-1, 1))
        wb.scatter_add_(1, eff_b[1][k].view(-1, 1), eff_b[0][k].view(-1, 1))
    return float((wa - wb).abs().max()) > 1e-9


@pytest.mark.parametrize("variant", [_swapped, _no_clamp, _x1_unclamped], ids=["half-pixel-shift", "no-clamp-at-0", "x1-unclamped"])
@pytest.mark.parametrize("case", G.RESIZE_CASES, ids=CASE_IDS)
def test_bound_rejects_wrong_resampling(case, variant):
    """Not too loose: each classic mistake leaves the bound on every case where it changes the resampling matrix at all (an
    axis with more than one input sample whose taps or weights the mistake touches)."""
    Hi, Wi, Ho, Wo, al = case
    hit = _affected(variant, Ho, Hi, al) or _affected(variant, Wo, Wi, al)
    x = rnd(2, 3, Hi, Wi, seed=4)
    bad = G.bilinear64(x, Ho, Wo, al, coords=variant)
    ratio = float(((bad - G.bilinear64(x, Ho, Wo, al)).abs() / G.bilinear_bound(x, Ho, Wo, al)).max())
    if hit:
        assert ratio > 1.0, f"the wrong variant stays inside the bound (err / bound {ratio:.3f})"
    else:
        assert ratio <= 1e-6          # the same samples with the same total weight: float64 rounding only


@pytest.mark.parametrize("g,h,w", [(14, 28, 28), (14, 4, 6), (14, 6, 4), (14, 1, 1), (14, 7, 9), (14, 30, 39), (14, 14, 14), (1, 3, 5)])
def test_bicubic64_is_torch_float64(g, h, w):
    x = rnd(5, g, g, seed=5)
    ref = F.interpolate(x.double()[None], size=(h, w), mode="bicubic", align_corners=False)[0]
    assert float((G.bicubic64(x, h, w) - ref).abs().max()) <= 1e-12
    pe = rnd(1 + g * g, 8, seed=6)
    out = G.pos_embed64(pe, g, h, w)
    grid = pe[1:].double().view(1, g, g, 8).permute(0, 3, 1, 2)
    refp = F.interpolate(grid, size=(h, w), mode="bicubic", align_corners=False).reshape(8, h * w).t()
    assert torch.equal(out[0], pe[0].double()) and float((out[1:] - refp).abs().max()) <= 1e-12


@pytest.mark.parametrize("row_off,pad", [(0, 0), (1, 3)])
def test_cam_fuse64_is_the_torch_composition(row_off, pad):
    B, C, H, W = 2, 5, 37, 52
    sizes = [(4, 4), (2, 3), (60, 70)]
    ldc = C + pad
    lows = []
    for i, (hs, ws) in enumerate(sizes):
        t = rnd(2 * B, row_off + hs * ws, ldc, seed=10 + i)
        t[:, :row_off] = float("nan")
        t[:, :, C:] = float("nan")
        lows.append(t.view(-1, ldc))
    acc = 0
    for lw, (hs, ws) in zip(lows, sizes):
        m = lw.view(2 * B, -1, ldc)[:, row_off:, :C].transpose(1, 2).reshape(2 * B, C, hs, ws).double()
        m = F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)
        acc = acc + F.relu(torch.max(m[:B], m[B:].flip(-1)))
    cam, bound = G.cam_fuse64(lows, sizes, B, C, H, W, row_off, ldc)
    assert float((cam - acc).abs().max()) <= 1e-12
    assert torch.isfinite(bound).all() and float(bound.min()) > 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_msc_seg64_is_the_torch_composition(mode):
    C, h, w, H, W = 4, 6, 9, 31, 45
    segs, acc = rnd(2, C, h, w, seed=7), rnd(1, C, H, W, seed=8)
    up = F.interpolate(segs.double(), size=(H, W), mode="bilinear", align_corners=False)
    v = up[0] + up[1].flip(-1)
    want = v if mode == 0 else (torch.max(acc[0].double(), v) if mode == 1 else acc[0].double() + v)
    ref, bound = G.msc_seg64(segs, torch.full_like(acc, float("nan")) if mode == 0 else acc, mode)
    assert float((ref - want).abs().max()) <= 1e-12 and torch.isfinite(bound).all()


def test_upsample_argmax64_margin():
    x = rnd(2, 6, 5, 7, seed=9)
    arg, margin, bound = G.upsample_argmax64(x, 23, 31)
    up = F.interpolate(x.double(), size=(23, 31), mode="bilinear", align_corners=False)
    assert torch.equal(arg, up.argmax(1))
    s = up.sort(1, descending=True).values
    assert float((margin - (s[:, 0] - s[:, 1])).abs().max()) <= 1e-12 and float(margin.min()) >= 0
    assert bound.shape == arg.shape
    one = G.upsample_argmax64(x[:, :1], 4, 4)
    assert int(one[0].abs().max()) == 0 and bool(torch.isinf(one[1]).all())


@pytest.mark.parametrize("B,h,w,Cin,dil", [(2, 12, 12, 24, 5), (1, 6, 10, 7, 12), (3, 5, 9, 33, 1), (1, 1, 1, 4, 3)])
def test_unfold_is_the_im2col_order_and_fold_its_adjoint(B, h, w, Cin, dil):
    x = rnd(B, Cin, h, w, seed=11).double()
    col = G.im2col64(x, dil)
    # column c*9 + tap of pixel (py, px) is x[c, py + (tap / 3 - 1) dil, px + (tap % 3 - 1) dil] or 0
    xp = F.pad(x, (dil, dil, dil, dil))
    want = torch.stack([xp[:, :, (t // 3) * dil:(t // 3) * dil + h, (t % 3) * dil:(t % 3) * dil + w] for t in range(9)], 2)
    want = want.permute(0, 3, 4, 1, 2).reshape(B * h * w, Cin * 9)
    assert torch.equal(col, want)
    c = rnd(B * h * w, Cin * 9, seed=12).double()
    lhs, rhs = float((col * c).sum()), float((x * G.col2im64(c, B, h, w, dil)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((col.abs() * c.abs()).sum())
