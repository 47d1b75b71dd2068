"""The references of tests/loss_ref.py and their bounds, checked on the CPU before tests/test_loss_norm_kernels_gpu.py trusts them:
they agree with torch's float64, a straightforward fp32 evaluation stays inside every bound on every case list of the GPU suite
(not too tight), and the classic mistakes leave them (not too loose).  Each test prints its worst ratio."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as G
import loss_ref as R
from kernel_guard import ratio_report

SEG_CASES = R.seg_cases()
SEG_IDS = [R.seg_case_id(c) for c in SEG_CASES]
EPS_PTC, EPS_COS, EPS_LN = 1e-8, 1e-6, 1e-6


def exceed(tag, err, bound):
    """largest err / bound of a MISTAKE: must be above 1 somewhere"""
    worst = ratio_report(tag, err, bound)
    assert worst > 1.0, f"{tag}: the mistake stays inside the bound (worst ratio {worst:.3g})"
    return worst


# =========================================================================================== agreement with torch float64
@pytest.mark.parametrize("c", SEG_CASES, ids=SEG_IDS)
def test_seg_ref_is_torch_float64(c):
    from oracle import dupl_oracle as O
    h, w, H, W = c["shape"]
    lg, lab = R.seg_inputs(c)
    r = R.seg_ref(lg, lab, H, W, 255, c["flip"], c["balanced"], g=0.7)
    x = lg.double().requires_grad_(True)
    up = F.interpolate(torch.flip(x, dims=[3]) if c["flip"] else x, size=(H, W), mode="bilinear", align_corners=False)
    ce = F.cross_entropy(up, lab, ignore_index=255, reduction="none")
    assert float((r.ce - ce.detach()).abs().max()) <= 1e-11
    n = int((lab != 255).sum())
    bg, fg = lab == 0, (lab != 0) & (lab != 255)
    if c["balanced"]:
        loss = 0.5 * ((ce * bg).sum() / (bg.sum().double() + 1e-6) + (ce * fg).sum() / (fg.sum().double() + 1e-6))
        # the oracle adds its 1e-6 to an integer tensor, i.e. in fp32 as the model does: the same up to 1e-6 / count
        assert abs(r.loss - float(O.seg_loss(up.detach(), lab))) <= 2e-6 * max(1.0, abs(r.loss))
    else:
        loss = ce.sum() / max(n, 1)
    assert abs(r.loss - float(loss.detach())) <= 1e-11 * max(1.0, abs(r.loss))
    (0.7 * loss).backward()
    gref = x.grad if x.grad is not None else torch.zeros_like(x)
    assert float((r.dlogits - gref).abs().max()) <= 1e-12
    assert r.sums[1] == int(bg.sum()) and r.sums[3] == int(fg.sum())
    if c["pattern"] == "all_ignored":
        assert r.loss == 0.0 and not bool(r.dlogits.any()) and not bool(r.dlogits_bound.any())


def test_flip_commutes_with_the_resize():
    """why "flip after the up-sampling" is no mistake to test for: it is the same function"""
    x = torch.randn(2, 3, 3, 5, generator=torch.Generator().manual_seed(1))
    assert float((R.up64(torch.flip(x, dims=[3]), 17, 23) - torch.flip(R.up64(x, 17, 23), dims=[3])).abs().max()) <= 1e-14


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_finish32_is_the_torch_fp32_expression(mode):
    gen = torch.Generator().manual_seed(mode)
    for s in (torch.rand(4, generator=gen) * 1000).tolist(), [0.0, 0.0, 0.0, 0.0], [3.5, 0.0, 7.25, 2.0]:
        s0, s1, s2, s3 = (torch.tensor(v, dtype=torch.float32) for v in s)
        if mode == 1:
            want = 0.5 * (1 - s0 / (s1 + 1)) + 0.5 * s2 / (s3 + 1)
        elif mode == 2:
            want = (s0 / (s1 + 1e-6) + s2 / (s3 + 1e-6)) * 0.5
        else:
            want = (s0 + s2) / (s1 + s3).clamp_min(1.0)
        assert np.float32(want.item()) == R.finish32(mode, *s)
    assert R.finish32(1, 0, 0, 0, 0) == np.float32(0.5) and R.finish32(2, 0, 0, 0, 0) == 0 and R.finish32(3, 0, 0, 0, 0) == 0


@pytest.mark.parametrize("form", ["label", "mask"])
def test_ptc_ref_is_the_oracle(form):
    from oracle import dupl_oracle as O
    gen = torch.Generator().manual_seed(5)
    fmap = torch.randn(2, 16, 5, 7, generator=gen).double()
    hw = 35
    _, lab, mask = R.ptc_inputs(2, hw, form, 255, seed=9)
    if form == "label":
        mask = O.label_to_aff_mask(lab.view(2, 5, 7))
    kind = R.ptc_kind(hw, lab, mask if form == "mask" else None, 255)
    assert torch.equal(kind == 1, mask == 1) and torch.equal(kind == 0, mask == 0)
    xh = F.normalize(fmap.reshape(2, 16, hw), p=2, dim=1, eps=EPS_PTC)
    cos = torch.matmul(xh.transpose(1, 2), xh).requires_grad_(True)
    want = 0.5 * (1 - torch.sum((mask == 1) * cos.abs()) / ((mask == 1).sum() + 1)) + 0.5 * torch.sum((mask == 0) * cos.abs()) / ((mask == 0).sum() + 1)
    assert abs(float(want.detach()) - float(O.masked_ptc_loss(fmap, mask))) <= 1e-13
    r = R.ptc_ref(cos.detach(), kind)
    assert abs(r.loss - float(want.detach())) <= 1e-13
    (1.7 * want).backward()
    v, _ = R.ptc_bwd_ref(cos.detach(), kind, float(r.sums[1]), float(r.sums[3]), 1.7)
    assert float((v - cos.grad).abs().max()) <= 1e-15
    allign = R.ptc_ref(cos.detach(), torch.full_like(kind, -1))
    assert allign.loss == 0.5


def test_l2norm_ref_is_f_normalize():
    x, dxh = R.l2_inputs(9, 65, 3, EPS_PTC)
    xd = x.double().requires_grad_(True)
    want = F.normalize(xd, p=2, dim=-1, eps=EPS_PTC)
    xh, nrm, _, _ = R.l2norm_ref(x, EPS_PTC)
    assert float((xh - want.detach()).abs().max()) <= 1e-15 and nrm[0] == 0 and 0 < nrm[-1] < EPS_PTC
    (want * dxh.double()).sum().backward()
    dx, _ = R.l2norm_bwd_ref(dxh, xh, nrm, EPS_PTC)
    scale = xd.grad.abs().amax(-1, keepdim=True)
    assert float(((dx - xd.grad).abs() / scale).max()) <= 1e-14


@pytest.mark.parametrize("n,c", [(7, 5), (50, 65), (1, 4)])
def test_cos_ref_is_f_cosine_similarity(n, c):
    from oracle import dupl_oracle as O
    a, b = R.cos_inputs(2, n, c, 11, EPS_COS)
    ad, bd = a.double(), b.double().requires_grad_(True)
    want = F.cosine_similarity(ad.transpose(1, 2), bd.transpose(1, 2), dim=-1, eps=EPS_COS)
    out, st, _, _ = R.cos_ref(a, b, EPS_COS)
    assert float((out - want).abs().max()) <= 1e-14
    (want * 0.37).sum().backward()
    got, _ = R.cos_bwd_ref(a, b, st, 0.37, EPS_COS)
    # the function itself, written with clamps that autograd differentiates (zero slope below eps)
    b2 = b.double().requires_grad_(True)
    f = (ad * b2).sum(1) / (ad.norm(dim=1).clamp_min(EPS_COS) * b2.norm(dim=1).clamp_min(EPS_COS))
    assert float((f - want).abs().max()) <= 1e-14
    (f * 0.37).sum().backward()
    scale = b2.grad.abs().amax(1, keepdim=True).clamp_min(1e-3)       # (with one token the gradient above eps is rounding noise around 0)
    assert float(((got - b2.grad).abs() / scale).max()) <= 1e-12
    # F.cosine_similarity's autograd: the same wherever |b| > eps.  Below eps it is NOT the derivative of its own forward (the
    # norms are clamped in place under no_grad, so the backward uses d|b| / db as if unclamped); reported, not asserted
    above = (st[..., 2].sqrt() > EPS_COS).unsqueeze(1).expand_as(got)
    rel = (got - bd.grad).abs() / scale
    assert float(rel[above].max() if above.any() else 0.0) <= 1e-12
    if (~above).any():
        print(f"n{n} c{c}: torch's autograd differs from the true derivative below eps by {100 * float(rel[~above].max()):.2f} % of the column's largest gradient")
    f1, f2 = a.transpose(1, 2).reshape(2, c, n, 1).double(), b.transpose(1, 2).reshape(2, c, n, 1).double()
    o2 = R.cos_ref(b, a, EPS_COS)[0]
    assert abs(float(O.sim_loss(f1, f2)) - float((1 + out.mean()) + (1 + o2.mean()))) <= 1e-13


@pytest.mark.parametrize("n", R.SMALL_N)
def test_msm_and_mean_accum_refs_are_torch(n):
    x, y = R.msm_inputs(n, n)
    xd = x.double().requires_grad_(True)
    want = F.multilabel_soft_margin_loss(xd, y.double())
    loss, _, dx, _ = R.msm_ref(x, y, g=0.8)
    assert abs(loss - float(want)) <= 1e-13 * max(1.0, abs(loss))
    (0.8 * want).backward()
    assert float((dx - xd.grad).abs().max()) <= 1e-16
    v, _ = R.mean_accum_ref(x, 0.25, 1.0 / n)
    assert abs(v - (0.25 + float(x.double().mean()))) <= 1e-13


@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_refs_are_f_layer_norm(D):
    rows = 5
    x, gamma, beta = R.ln_inputs(rows, D, D, special=False)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    want = F.layer_norm(xd, (D,), gd, bd, EPS_LN)
    f = R.ln_fwd_ref(x, gamma, beta, EPS_LN)
    assert float((f.y - want).abs().max()) <= 1e-12
    _, _, dy, dres = R.ln_bwd_inputs(rows, D, D + 1)
    want.backward(dy.double())
    b = R.ln_bwd_ref(dy, x, gamma, f.mean, f.rstd, dres)
    assert float((b.dx - dres.double() - xd.grad).abs().max()) <= 1e-12
    assert float((b.dgamma - gd.grad).abs().max()) <= 1e-12 and float((b.dbeta - bd.grad).abs().max()) <= 1e-12
    assert b.amax == float(b.dx.abs().max())


def test_loss_total_ref_follows_the_documented_order():
    """against the same expression written out in torch fp32, and an empty middle group contributes w * 0"""
    t = [0.1, 0.7, 1.3, 2.9, 0.33]
    add = [0.0, 1.0, 0.0, 1.0, 0.0]
    group = [0, 2, 0, 2, 3]
    w = [1.0, 5.0, 0.1, 0.05]
    total, Gs = R.loss_total_ref(t, add, group, w, 4)
    T = [torch.tensor(v, dtype=torch.float32) for v in t]
    G0, G2, G3 = T[0] + T[2], (1.0 + T[1]) + (1.0 + T[3]), T[4]
    want = ((1.0 * G0 + 5.0 * torch.zeros(())) + 0.1 * G2) + 0.05 * G3
    assert np.float32(want.item()) == total and Gs[1] == 0 and Gs[0] == np.float32(G0.item()) and Gs[2] == np.float32(G2.item())
    assert np.array_equal(R.loss_total_bwd_ref(0.3, group, w), np.array([np.float32(0.3) * np.float32(w[g]) for g in group], dtype=np.float32))


# =========================================================================================== bounds not too tight
@pytest.mark.parametrize("c", SEG_CASES, ids=SEG_IDS)
def test_seg_bounds_admit_torch_fp32(c):
    h, w, H, W = c["shape"]
    lg, lab = R.seg_inputs(c)
    r = R.seg_ref(lg, lab, H, W, 255, c["flip"], c["balanced"], g=0.7)
    f = R.seg_fp32(lg, lab, H, W, 255, c["flip"], c["balanced"], g=0.7)
    tag = "seg fp32 " + R.seg_case_id(c)
    worst = max(ratio_report(tag + " ce", (f.ce.double() - r.ce).abs(), r.ce_bound),
                ratio_report(tag + " sums", (f.sums.double() - r.sums).abs(), r.sums_bound),
                ratio_report(tag + " dlogits", (f.dlogits.double() - r.dlogits).abs(), r.dlogits_bound))
    assert worst < 1.0


@pytest.mark.parametrize("hw,b,form,ign", R.PTC_CASES)
def test_ptc_bounds_admit_torch_fp32(hw, b, form, ign):
    cos, lab, mask = R.ptc_case_inputs(hw, b, form, ign)
    kind = R.ptc_kind(hw, lab, mask, ign)
    r = R.ptc_ref(cos, kind)
    a = cos.abs()
    got = torch.stack([a[kind == 1].sum(), (kind == 1).sum().float(), a[kind == 0].sum(), (kind == 0).sum().float()]).double()
    assert ratio_report(f"ptc fp32 hw{hw} b{b} {form} ign{ign}", (got - r.sums).abs(), r.sums_bound) < 1.0
    v, vb = R.ptc_bwd_ref(cos, kind, float(r.sums[1]), float(r.sums[3]), 1.7)
    g32 = torch.sign(cos) * torch.where(kind == 1, -0.5 * torch.tensor(1.7) / (got[1].float() + 1), 0.5 * torch.tensor(1.7) / (got[3].float() + 1))
    g32 = torch.where(kind >= 0, g32, torch.zeros_like(g32))
    assert ratio_report(f"ptc bwd fp32 hw{hw} b{b} {form} ign{ign}", (g32.double() - v).abs(), vb) < 1.0


@pytest.mark.parametrize("rows", R.L2_ROWS)
@pytest.mark.parametrize("c", R.L2_C)
def test_l2norm_bounds_admit_torch_fp32(rows, c):
    x, dxh = R.l2_inputs(rows, c, rows * 131 + c, EPS_PTC)
    x32 = x.clone().requires_grad_(True)
    y32 = F.normalize(x32, p=2, dim=-1, eps=EPS_PTC)
    xh, nrm, xb, nb = R.l2norm_ref(x, EPS_PTC)
    worst = ratio_report(f"l2norm fp32 {rows}x{c}", (y32.detach().double() - xh).abs(), xb)
    n32 = x.norm(dim=-1)
    worst = max(worst, ratio_report(f"l2norm fp32 norm {rows}x{c}", (n32.double() - nrm).abs(), nb))
    # backward from the fp32 forward's own xhat / norm, as the kernel gets them
    dx, db = R.l2norm_bwd_ref(dxh, y32.detach(), n32, EPS_PTC)
    s = (y32.detach() * dxh).sum(-1, keepdim=True)
    proj = torch.where(n32.unsqueeze(-1) > EPS_PTC, s, torch.zeros_like(s))
    got = (dxh - y32.detach() * proj) * (1.0 / n32.clamp_min(EPS_PTC).unsqueeze(-1))
    worst = max(worst, ratio_report(f"l2norm bwd fp32 {rows}x{c}", (got.double() - dx).abs(), db))
    assert worst < 1.0


@pytest.mark.parametrize("B,n,c,strided", R.cos_cases())
def test_cos_bounds_admit_torch_fp32(B, n, c, strided):
    """every case of the GPU suite, the grid-stride one included (the layout does not enter the arithmetic)"""
    a, b = R.cos_case_inputs(B, n, c, EPS_COS)
    out, st, ob, sb = R.cos_ref(a, b, EPS_COS)
    st32 = torch.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], -1)
    na, nb = st32[..., 1].sqrt().clamp_min(EPS_COS), st32[..., 2].sqrt().clamp_min(EPS_COS)
    o32 = st32[..., 0] / (na * nb)
    worst = max(ratio_report(f"cos fp32 stats n{n} c{c} B{B}", (st32.double() - st).abs(), sb),
                ratio_report(f"cos fp32 out n{n} c{c} B{B}", (o32.double() - out).abs(), ob))
    want, wb = R.cos_bwd_ref(a, b, st32, 0.37, EPS_COS)
    s = st32.unsqueeze(1)
    rb = s[..., 2].sqrt()
    na, nb = s[..., 1].sqrt().clamp_min(EPS_COS), rb.clamp_min(EPS_COS)
    gv = torch.tensor(0.37)
    got = torch.where(rb > EPS_COS, gv * (a / (na * nb) - s[..., 0] / (na * nb) * b / (nb * nb)), gv * (a / (na * nb)))
    worst = max(worst, ratio_report(f"cos bwd fp32 n{n} c{c} B{B}", (got.double() - want).abs(), wb))
    assert worst < 1.0


@pytest.mark.parametrize("n", R.SMALL_N)
def test_msm_and_mean_accum_bounds_admit_torch_fp32(n):
    x, y = R.msm_inputs(n, n)
    loss, lb, dx, dxb = R.msm_ref(x, y, g=0.8)
    x32 = x.clone().requires_grad_(True)
    l32 = F.multilabel_soft_margin_loss(x32, y)
    (0.8 * l32).backward()
    worst = max(ratio_report(f"msm fp32 n{n}", torch.tensor(abs(float(l32) - loss)), torch.tensor(lb)),
                ratio_report(f"msm dx fp32 n{n}", (x32.grad.double() - dx).abs(), dxb))
    v, vb = R.mean_accum_ref(x, 0.25, 1.0 / n)
    got = torch.tensor(0.25) + x.sum() * torch.tensor(1.0 / n)
    worst = max(worst, ratio_report(f"mean_accum fp32 n{n}", torch.tensor(abs(float(got) - v)), torch.tensor(vb)))
    assert worst < 1.0


@pytest.mark.parametrize("D", R.LN_D)
@pytest.mark.parametrize("rows", R.LN_FWD_ROWS)
def test_layernorm_fwd_bounds_admit_numpy_fp32(rows, D):
    x, gamma, beta = R.ln_inputs(rows, D, rows * 7919 + D)
    f = R.ln_fwd_ref(x, gamma, beta, EPS_LN)
    y, mean, rstd = R.ln_fwd_np32(x, gamma, beta, EPS_LN)
    worst = max(ratio_report(f"ln fwd np32 {rows}x{D} y", (torch.from_numpy(y).double() - f.y).abs(), f.y_bound),
                ratio_report(f"ln fwd np32 {rows}x{D} mean", (torch.from_numpy(mean).double() - f.mean).abs(), f.mean_bound),
                ratio_report(f"ln fwd np32 {rows}x{D} rstd", (torch.from_numpy(rstd).double() - f.rstd).abs(), f.rstd_bound))
    assert worst < 1.0


@pytest.mark.parametrize("D", R.LN_D)
@pytest.mark.parametrize("rows", R.LN_BWD_ROWS)
def test_layernorm_bwd_bounds_admit_torch_fp32(rows, D):
    x, gamma, dy, dres = R.ln_bwd_inputs(rows, D, rows * 7919 + D)
    _, mean, rstd = R.ln_fwd_np32(x, gamma, torch.zeros(D), EPS_LN)
    mean, rstd = torch.from_numpy(mean), torch.from_numpy(rstd)
    dg0, db0 = torch.full((D,), 0.5), torch.full((D,), -0.25)
    r = R.ln_bwd_ref(dy, x, gamma, mean, rstd, dres, dg0, db0)
    xh = (x - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    g = dy * gamma
    dx = rstd.unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True)) + dres
    dg, db = dg0 + (dy * xh).sum(0), db0 + dy.sum(0)
    worst = max(ratio_report(f"ln bwd fp32 {rows}x{D} dx", (dx.double() - r.dx).abs(), r.dx_bound),
                ratio_report(f"ln bwd fp32 {rows}x{D} dgamma", (dg.double() - r.dgamma).abs(), r.dgamma_bound),
                ratio_report(f"ln bwd fp32 {rows}x{D} dbeta", (db.double() - r.dbeta).abs(), r.dbeta_bound))
    assert worst < 1.0


# =========================================================================================== bounds not too loose
MISTAKE_SHAPES = [c for c in SEG_CASES if c["shape"] in ((2, 3, 32, 48), (3, 5, 17, 23), (4, 4, 60, 60)) and c["C1"] == 21
                  and c["pattern"] == "random"]


@pytest.mark.parametrize("variant", ["align_corners", "no_half_pixel", "flip_base_tap_only", "border_dropped"])
def test_resampling_mistakes_leave_the_seg_bounds(variant):
    """in the CE map AND in the gradient, on a fast-path, a generic integer and a non-integer shape"""
    for c in MISTAKE_SHAPES:
        h, w, H, W = c["shape"]
        lg, lab = R.seg_inputs(c)
        r = R.seg_ref(lg, lab, H, W, 255, 1, c["balanced"], g=0.7)
        m = R.seg_ref(lg, lab, H, W, 255, 1, c["balanced"], g=0.7, variant=variant)
        tag = f"mistake {variant} {R.seg_case_id(c)}"
        exceed(tag + " ce", (m.ce - r.ce).abs(), r.ce_bound)
        exceed(tag + " sums", (m.sums - r.sums).abs(), r.sums_bound)
        exceed(tag + " dlogits", (m.dlogits - r.dlogits).abs(), r.dlogits_bound)


def test_border_mistake_is_seen_in_border_cells_only():
    """the gradient bound is per cell: dropping the clamped tap changes the last row / column of cells and nothing else, and the
    bound of exactly those cells is exceeded"""
    c = dict(shape=(4, 4, 64, 64), b=1, C1=21, flip=0, balanced=1, f32lab=0, pattern="random", det_only=False, scale=3.0)
    lg, lab = R.seg_inputs(c)
    r = R.seg_ref(lg, lab, 64, 64, 255, 0, 1)
    m = R.seg_ref(lg, lab, 64, 64, 255, 0, 1, variant="border_dropped")
    over = (m.dlogits - r.dlogits).abs() > r.dlogits_bound
    assert bool(over[:, :, -1, :].any()) and bool(over[:, :, :, -1].any()) and not bool(over[:, :, :-1, :-1].any())


def test_ptc_diagonal_mistake_leaves_the_bound():
    cos, lab, _ = R.ptc_inputs(3, 97, "label", 255, seed=97)
    cos = cos + 3.0 * torch.eye(97)                      # a cosine matrix has a unit diagonal: the mistake is not small
    r = R.ptc_ref(cos, R.ptc_kind(97, lab, None, 255))
    m = R.ptc_ref(cos, R.ptc_kind(97, lab, None, 255, count_diagonal=True))
    assert m.sums[1] != r.sums[1], "the counts are exact: any difference fails"
    exceed("mistake ptc diagonal: sum_pos", (m.sums[0] - r.sums[0]).abs(), r.sums_bound[0])


@pytest.mark.parametrize("variant", ["clamp_product", "second_term_kept"])
def test_cosine_clamp_mistakes_leave_the_bound(variant):
    a, b = R.cos_inputs(2, 7, 5, 11, EPS_COS)
    _, st, _, _ = R.cos_ref(a, b, EPS_COS)
    want, wb = R.cos_bwd_ref(a, b, st, 1.0, EPS_COS)
    got, _ = R.cos_bwd_ref(a, b, st, 1.0, EPS_COS, variant=variant)
    err = (got - want).abs()
    exceed(f"mistake cosine {variant}", err, wb)
    healthy = [2] if variant == "second_term_kept" else []
    for col in healthy:                                   # both norms above eps: the same arithmetic
        assert float(err[:, :, col].max()) == 0.0
    if variant == "second_term_kept":
        rel = float((err[:, :, 4] / want[:, :, 4].abs().amax(1, keepdim=True)).max())
        print(f"second term kept below eps: {100 * rel:.2f} % of the column's largest gradient")


def test_l2norm_guard_mistake_leaves_the_bound():
    x, dxh = R.l2_inputs(5, 65, 3, EPS_PTC)
    xh, nrm, _, _ = R.l2norm_ref(x, EPS_PTC)
    want, wb = R.l2norm_bwd_ref(dxh, xh, nrm, EPS_PTC)
    got, _ = R.l2norm_bwd_ref(dxh, xh, nrm, EPS_PTC, guard=False)
    exceed("mistake l2norm projection kept below eps", (got - want).abs()[-1], wb[-1])
    assert float((got - want).abs()[:-1].max()) == 0.0


def test_one_pass_variance_leaves_the_bound():
    x, gamma, beta = R.ln_inputs(5, 768, 1)
    f = R.ln_fwd_ref(x, gamma, beta, EPS_LN)
    m = R.ln_fwd_ref(x, gamma, beta, EPS_LN, one_pass=True)
    exceed("mistake one-pass variance: y of the row at offset 1e4", (m.y - f.y).abs()[-1], f.y_bound[-1])
    exceed("mistake one-pass variance: rstd", (m.rstd - f.rstd).abs()[-1], f.rstd_bound[-1])


def test_amax_without_dres_leaves_the_bound():
    x, gamma, dy, dres = R.ln_bwd_inputs(17, 260, 5)
    f = R.ln_fwd_ref(x, gamma, torch.zeros(260), EPS_LN)
    r = R.ln_bwd_ref(dy, x, gamma, f.mean, f.rstd, dres)
    m = R.ln_bwd_ref(dy, x, gamma, f.mean, f.rstd, dres, amax_before_dres=True)
    exceed("mistake amax before dres", torch.tensor(abs(m.amax - r.amax)), r.dx_bound.max())
