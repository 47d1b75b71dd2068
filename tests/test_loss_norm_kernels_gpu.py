"""The loss kernels (csrc/loss.hip) and the LayerNorm kernels (csrc/norm.hip) at their edges: non-square and mixed up-sampling
factors, every backward path of the fused up-sample + CE (wave-reduced, per-lane, deterministic gather at each of its block sizes),
label types and degenerate label maps, strided / gapped operands, accumulation onto non-zero starts, values below eps, every
LN_MAXC boundary, rows_per_wave, every dgamma / dbeta reduction form and the dy_clear paths -- each against the float64 (or
bit-exact fp32) references of tests/loss_ref.py, whose bounds tests/test_loss_ref_host.py checks first.

Technique (tests/kernel_guard.py): outputs live inside sentinel slack that must be bit-unchanged, inputs inside NaN slack; every
element a kernel is told to skip (ignored / diagonal PTC pairs, the gap of ld > c, the gap between images, rows past `rows`) holds
NaN on the input side and a sentinel on the output side.  Kernels are called through ops.L() on the current stream.  Refusal
tests only exercise host-side DUPL_ERR_ARG returns: nothing is launched by them.  Every tolerance test prints its worst err / bound."""
import ctypes
import math

import numpy as np
import pytest
import torch

import loss_ref as R
from kernel_guard import (NAN, EPS24, PAD, SENT, _ALIVE, Guard, Tally, bits, nan_in, rnd, rndint, same_bits, stream)  # noqa: F401
from parity_util import assert_labels_equal_up_to_ties

pytestmark = pytest.mark.gpu

ERR_ARG = -1
IGN = 255
G_UP = 0.7                   # the up-stream gradient of every backward here: never 1
EPS_PTC, EPS_COS, EPS_LN = 1e-8, 1e-6, 1e-6
INF = float("inf")


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _ALIVE.clear()


def L():
    from dupl_amd import ops
    return ops.L()


def f32bits(v):
    return np.asarray(v, dtype=np.float32).view(np.int32)


def gapped(rows_t, idx, total, dev):
    """rows_t scattered to flat positions idx of a NaN-filled device buffer of `total` floats (the gaps stay NaN)"""
    flat = torch.full((total,), NAN)
    flat[idx.reshape(-1)] = rows_t.reshape(-1)
    return nan_in(flat, dev)


def gapped_out(idx, total, dev, start=None):
    """a sentinel-filled output buffer of `total` floats; `start` (if given) is written at positions idx"""
    g = Guard((total,), dev)
    if start is not None:
        g.view.index_put_((idx.reshape(-1).to(dev),), start.reshape(-1).to(dev))
    return g


def gaps_untouched(g, idx):
    flat = bits(g.cpu())
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    keep[idx.reshape(-1)] = False
    return bool((flat[keep] == SENT[torch.float32][1]).all())


# =========================================================================================== fused up-sample + CE
SEG_CASES = R.seg_cases()
SEG_IDS = [R.seg_case_id(c) for c in SEG_CASES]
_SEG_REF = {}


def _seg_ref(c):
    key = R.seg_case_id(c)
    if key not in _SEG_REF:
        lg, lab = R.seg_inputs(c)
        h, w, H, W = c["shape"]
        _SEG_REF[key] = R.seg_ref(lg, lab, H, W, IGN, c["flip"], c["balanced"], g=G_UP)
    return _SEG_REF[key]


def _tok(t):
    """(b, C1, h, w) -> token-major (b, h * w, C1)"""
    b, C1, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b, h * w, C1).contiguous()


@pytest.mark.parametrize("c", SEG_CASES, ids=SEG_IDS)
def test_seg_loss_edges(dev, c):
    """forward sums + finish, CE map, the atomics backward (wave-reduced or per-lane, as the shape decides), the deterministic gather
    backward (twice: bit-identical; onto a non-zero start) and the pseudo labels of one case"""
    h, w, H, W = c["shape"]
    b, C1, flip, bal = c["b"], c["C1"], c["flip"], c["balanced"]
    lg, lab = R.seg_inputs(c)
    ref = _seg_ref(c)
    T = Tally("seg " + R.seg_case_id(c))
    tl = nan_in(_tok(lg), dev)
    if c["f32lab"]:
        lp, i64 = nan_in(lab.float(), dev).data_ptr(), 0
    else:
        labg = Guard(tuple(lab.shape), dev, torch.int64, init=lab)
        lp, i64 = labg.ptr, 1
    finish = 2 if bal else 3
    sums = Guard((136,), dev, init=torch.zeros(136))
    L().dupl_seg_loss_fwd(tl.data_ptr(), lp, i64, IGN, sums.ptr, b, C1, h, w, H, W, flip, finish, stream())
    s = sums.cpu()
    assert float(s[1]) == float(ref.sums[1]) and float(s[3]) == float(ref.sums[3]), "the counts are exact"
    T.add("sums", (s[:4].double() - ref.sums).abs(), ref.sums_bound)
    assert f32bits(s[6].item()) == f32bits(R.finish32(finish, *s[:4].tolist())), "sums[6] is the fp32 finish formula of sums[0..3]"
    if c["pattern"] == "all_ignored":
        assert not bool(s[:4].any()) and float(s[6]) == 0.0
    # ---- the per-pixel CE map
    cm = Guard((b, H, W), dev)
    L().dupl_seg_ce_map(tl.data_ptr(), lp, i64, IGN, cm.ptr, b, C1, h, w, H, W, flip, stream())
    got = cm.cpu()
    assert bool((got[lab == IGN] == 0).all())
    T.add("ce map", (got.double() - ref.ce).abs(), ref.ce_bound)
    # ---- both backwards
    gs = nan_in(torch.tensor([G_UP]), dev)
    want, wb = _tok(ref.dlogits), _tok(ref.dlogits_bound)
    for det in ((1,) if c["det_only"] else (0, 1)):
        start = rnd(b, h * w, C1, seed=5, scale=0.01) if det else torch.zeros(b, h * w, C1)

        def run():
            D = Guard((b, h * w, C1), dev, init=start)
            L().dupl_seg_loss_bwd(tl.data_ptr(), lp, i64, IGN, sums.ptr, gs.data_ptr(), D.ptr, b, C1, h, w, H, W, flip, bal, det,
                                  stream())
            return D.cpu()
        got = run()
        assert bool(torch.isfinite(got).all())
        # the last addition onto the start rounds once more
        T.add(f"dlogits det={det}", (got.double() - start.double() - want).abs(), wb + 2 * EPS24 * (start.abs() + got.abs()).double())
        if c["pattern"] == "all_ignored":
            assert same_bits(got, start), "no valid pixel: the gradient is exactly zero"
        if det:
            assert same_bits(run(), got), "the gather backward is bit-reproducible"
    # ---- consistency targets (no flip in this kernel)
    if not c["det_only"] and c["pattern"] == "random":
        thr = 0.6
        p = R.pseudo_ref(lg, lab, H, W, IGN, thr)
        out, cnt = Guard((b, H, W), dev, torch.int64), Guard((1,), dev, init=torch.tensor([5.0]))
        L().dupl_seg_pseudo_label(tl.data_ptr(), nan_in(lab.float(), dev).data_ptr(), IGN, thr, out.ptr, cnt.ptr, b, C1, h, w, H, W,
                                  stream())
        got = out.cpu()
        # a decision is proven where the arg-max margin exceeds twice the up-sampling bound AND conf is off the threshold by more
        # than its bound; where the other label is not `ignore` there is no decision at all
        proof = torch.minimum(p.margin / (2 * p.bound).clamp_min(1e-300), (p.conf - thr).abs() / p.conf_bound.clamp_min(1e-300))
        proof = torch.where(lab == IGN, proof, torch.full_like(proof, INF))
        assert_labels_equal_up_to_ties(got, p.label, proof, "pseudo " + R.seg_case_id(c), tol=1.0)
        kept = got != IGN
        assert float(cnt.cpu()[0]) == 5.0 + int(kept.sum()), "count += exactly the pixels kept"
        assert bool((kept == p.keep)[proof > 1.0].all())
    T.done()


def test_seg_refusals(dev):
    """host-side argument checks only: DUPL_ERR_ARG, nothing launched, no buffer touched"""
    b, C1, h, w, H, W = 1, 2, 2, 2, 32, 32
    tl, lab = nan_in(rnd(b, h * w, 256), dev), nan_in(torch.zeros(b, H, W), dev)
    sums, D = Guard((136,), dev), Guard((b, h * w, 256), dev)
    gs = nan_in(torch.tensor([1.0]), dev)
    out, cnt, cm = Guard((b, H, W), dev, torch.int64), Guard((1,), dev), Guard((b, H, W), dev)
    bwd, st = L().dupl_seg_loss_bwd.raw, stream()
    a = (tl.data_ptr(), lab.data_ptr(), 0, IGN, sums.ptr, gs.data_ptr(), D.ptr)
    assert bwd(*a, b, 256, h, w, H, W, 0, 1, 1, st) == ERR_ARG, "C1 = 256 does not fit the gather backward's LDS"
    for det in (0, 1):
        for hh, ww in ((0, w), (h, 0), (-1, w), (h, -3)):
            assert bwd(*a, b, C1, hh, ww, H, W, 0, 1, det, st) == ERR_ARG
        assert bwd(*a, b, C1, h, w, h - 1, W, 0, 1, det, st) == ERR_ARG and bwd(*a, b, C1, h, w, H, w - 1, 0, 1, det, st) == ERR_ARG
    for HH, WW in ((h - 1, W), (H, w - 1), (0, 0)):
        assert L().dupl_seg_pseudo_label.raw(tl.data_ptr(), lab.data_ptr(), IGN, 0.5, out.ptr, cnt.ptr, b, C1, h, w, HH, WW, st) == ERR_ARG
        assert L().dupl_seg_ce_map.raw(tl.data_ptr(), lab.data_ptr(), 0, IGN, cm.ptr, b, C1, h, w, HH, WW, 0, st) == ERR_ARG
        assert L().dupl_seg_loss_fwd.raw(tl.data_ptr(), lab.data_ptr(), 0, IGN, sums.ptr, b, C1, h, w, HH, WW, 0, 2, st) == ERR_ARG
    assert L().dupl_seg_loss_fwd.raw(tl.data_ptr(), lab.data_ptr(), 0, IGN, sums.ptr, b, C1, h, w, H, W, 0, 1, st) == ERR_ARG   # finish 1 is PTC's
    torch.cuda.synchronize()
    assert sums.untouched() and D.untouched() and out.untouched() and cnt.untouched() and cm.untouched()


# =========================================================================================== PTC
@pytest.mark.parametrize("hw,b,form,ign", R.PTC_CASES)
def test_ptc_reduce_and_backward_mask(dev, hw, b, form, ign):
    """sums / counts / loss of a GIVEN cosine matrix whose ignored pairs (the diagonal included) hold NaN; the in-place backward
    writes 0 there, sign(0) = 0; all pairs ignored: the loss is exactly 0.5"""
    cos, lab, mask = R.ptc_case_inputs(hw, b, form, ign)
    kind = R.ptc_kind(hw, lab, mask, ign)
    ref = R.ptc_ref(cos, kind)
    T = Tally(f"ptc hw{hw} b{b} {form} ign{ign}")
    cn = cos.clone()
    cn[kind < 0] = NAN
    labg = Guard(tuple(lab.shape), dev, torch.int64, init=lab) if lab is not None else None
    mskg = Guard(tuple(mask.shape), dev, torch.int64, init=mask) if mask is not None else None
    lp, mp = labg.ptr if labg else None, mskg.ptr if mskg else None
    sums = Guard((136,), dev, init=torch.zeros(136))
    L().dupl_ptc_reduce(nan_in(cn, dev).data_ptr(), lp, mp, ign, sums.ptr, b, hw, 1, stream())
    s = sums.cpu()
    assert float(s[1]) == float(ref.sums[1]) and float(s[3]) == float(ref.sums[3]), "the counts are exact"
    T.add("sums", (s[:4].double() - ref.sums).abs(), ref.sums_bound)
    assert f32bits(s[6].item()) == f32bits(R.finish32(1, *s[:4].tolist()))
    # ---- backward, in place
    cg = Guard((b, hw, hw), dev, init=cn)
    L().dupl_ptc_bwd_mask(cg.ptr, lp, mp, ign, sums.ptr, nan_in(torch.tensor([1.7]), dev).data_ptr(), b, hw, stream())
    got = cg.cpu()
    want, wb = R.ptc_bwd_ref(cn, kind, float(s[1]), float(s[3]), 1.7)
    assert bool((got[kind < 0] == 0).all()), "ignored pairs get 0, whatever they held"
    assert bool((got[(kind >= 0) & (cos == 0)] == 0).all()), "sign(0) = 0"
    T.add("backward", (got.double() - want).abs(), wb)
    # ---- nothing valid: 0.5 exactly, from a matrix that is NaN everywhere
    if form == "label":
        alli = Guard((b, hw), dev, torch.int64, init=torch.full((b, hw), ign, dtype=torch.int64))
        lp2, mp2 = alli.ptr, None
    else:
        alli = Guard((b, hw, hw), dev, torch.int64, init=torch.full((b, hw, hw), 2, dtype=torch.int64))
        lp2, mp2 = None, alli.ptr
    sums2 = Guard((136,), dev, init=torch.zeros(136))
    L().dupl_ptc_reduce(nan_in(torch.full((b, hw, hw), NAN), dev).data_ptr(), lp2, mp2, ign, sums2.ptr, b, hw, 1, stream())
    s2 = sums2.cpu()
    assert not bool(s2[:4].any()) and float(s2[6]) == 0.5
    T.done()


# =========================================================================================== F.normalize rows
def _row_layout(rows, c, strided):
    """(ldx, rows_per_img, img_stride, total floats, flat index (rows, c))"""
    if strided:
        ldx, rpi = c + 3, 2
        ims = rpi * ldx + 5
    else:
        ldx, rpi = c, rows
        ims = rows * c
    r = torch.arange(rows)
    base = (r // rpi) * ims + (r % rpi) * ldx
    total = int(base[-1]) + c + (3 if strided else 0)
    return ldx, rpi, ims, total, base.unsqueeze(1) + torch.arange(c).unsqueeze(0)


@pytest.mark.parametrize("strided", [0, 1])
@pytest.mark.parametrize("c", R.L2_C)
@pytest.mark.parametrize("rows", R.L2_ROWS)
def test_l2norm_rows(dev, rows, c, strided):
    """forward and adjoint on dense and gapped rows (ldx > c, an image stride; the gaps hold NaN / a sentinel), accumulate 0 / 1,
    an all-zero row and a row with 0 < |x| < eps (zero slope of the clamp: dx = dxh / eps)"""
    x, dxh = R.l2_inputs(rows, c, rows * 131 + c, EPS_PTC)
    ldx, rpi, ims, total, idx = _row_layout(rows, c, strided)
    T = Tally(f"l2norm {rows}x{c} strided={strided}")
    xd = gapped(x, idx, total, dev)
    xh, nrm = Guard((rows, c), dev), Guard((rows,), dev)
    L().dupl_l2norm_rows_fwd(xd.data_ptr(), xh.ptr, nrm.ptr, rows, c, ldx, rpi, ims, EPS_PTC, stream())
    gx, gn = xh.cpu(), nrm.cpu()
    rx, rn, xb, nb = R.l2norm_ref(x, EPS_PTC)
    T.add("xhat", (gx.double() - rx).abs(), xb)
    T.add("norm", (gn.double() - rn).abs(), nb)
    if rows >= 2:
        assert float(gn[0]) == 0.0 and not bool(gx[0].any())
    assert 0 < float(gn[-1]) < EPS_PTC
    want, wb = R.l2norm_bwd_ref(dxh, gx, gn, EPS_PTC)               # from the xhat / norm the kernel is handed
    dxh_d = nan_in(dxh, dev)
    for acc in (0, 1):
        start = rnd(rows, c, seed=9) if acc else None
        dx = gapped_out(idx, total, dev, start)
        L().dupl_l2norm_rows_bwd(dxh_d.data_ptr(), xh.ptr, nrm.ptr, dx.ptr, rows, c, ldx, rpi, ims, EPS_PTC, acc, stream())
        assert gaps_untouched(dx, idx), "the gaps between rows / images are not written"
        got = dx.cpu()[idx.reshape(-1)].view(rows, c)
        base = start.double() if acc else torch.zeros(rows, c, dtype=torch.float64)
        T.add(f"dx accumulate={acc}", (got.double() - base - want).abs(), wb + 2 * EPS24 * (base.abs() + got.abs().double()))
    T.done()


# =========================================================================================== cosine over tokens
def _cos_layout(B, n, c, strided):
    ld = c + 5 if strided else c
    ims = n * ld + (7 if strided else 0)
    i, t, k = torch.arange(B).view(B, 1, 1), torch.arange(n).view(1, n, 1), torch.arange(c).view(1, 1, c)
    return ld, ims, B * ims, i * ims + t * ld + k


def _cos_case(dev, B, n, c, strided, T):
    a, b = R.cos_case_inputs(B, n, c, EPS_COS)
    ld, ims, total, idx = _cos_layout(B, n, c, strided)
    ad, bd = gapped(a, idx, total, dev), gapped(b, idx, total, dev)
    out, st = Guard((B, c), dev), Guard((B, c, 3), dev)
    L().dupl_cos_sim_fwd(ad.data_ptr(), bd.data_ptr(), out.ptr, st.ptr, B, n, c, ld, ims, EPS_COS, stream())
    go, gst = out.cpu(), st.cpu()
    ro, rst, ob, sb = R.cos_ref(a, b, EPS_COS)
    T.add("stats", (gst.double() - rst).abs(), sb)
    T.add("out", (go.double() - ro).abs(), ob)
    assert float(gst[:, 0, 2].abs().max()) == 0.0                   # the zero column of b
    if c > 1:
        assert 0 < float(gst[:, c - 1, 2].sqrt().max()) < EPS_COS   # the column of b below eps
    g, gmul = 1.5, 0.25
    want, wb = R.cos_bwd_ref(a, b, gst, g * gmul, EPS_COS)          # from the stats the kernel is handed
    gd = nan_in(torch.tensor([g]), dev)
    for acc in (0, 1):
        start = rnd(B, n, c, seed=3) if acc else None
        db = gapped_out(idx, total, dev, start)
        L().dupl_cos_sim_bwd(ad.data_ptr(), bd.data_ptr(), st.ptr, gd.data_ptr(), gmul, db.ptr, B, n, c, ld, ims, EPS_COS, acc, stream())
        assert gaps_untouched(db, idx)
        got = db.cpu()[idx.reshape(-1)].view(B, n, c)
        base = start.double() if acc else torch.zeros(B, n, c, dtype=torch.float64)
        T.add(f"db accumulate={acc}", (got.double() - base - want).abs(), wb + 2 * EPS24 * (base.abs() + got.abs().double()))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c", R.COS_C)
@pytest.mark.parametrize("n", R.COS_N)
def test_cos_sim(dev, n, c, B):
    """forward (out and stats) and the gradient wrt b, dense (B = 1) and gapped (B = 3: ld > c, an image stride), accumulate 0 / 1,
    gmul != 1; zero columns and columns below eps of either operand (below eps the clamp has zero slope: a / (na eps) alone)"""
    T = Tally(f"cos n{n} c{c} B{B}")
    _cos_case(dev, B, n, c, B == 3, T)
    T.done()


def test_cos_sim_grid_stride(dev):
    """B n c > 4096 x 256: the backward's grid-stride loop takes a second trip"""
    B, n, c = R.COS_GRID_STRIDE
    assert B * n * c > 4096 * 256
    T = Tally(f"cos n{n} c{c} B{B}")
    _cos_case(dev, B, n, c, False, T)
    T.done()


def test_cos_sim_bwd_above_eps_keeps_the_recorded_bits(dev):
    """dropping the second term below eps changed nothing above it: at the workload's shape, every column far above eps, db is bit
    for bit what the kernel gave BEFORE that change (tests/golden/cos_bwd_workload.npz: its sha256 and every 61st element,
    recorded on an MI355X from the library built at the commit before).  The inputs come from integer arithmetic and the stats
    from exact sums, so the record depends on dupl_cos_sim_bwd alone."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cos_bwd_workload.npz"))
    B, n, c = R.COS_WORKLOAD
    a, b, st = R.cos_workload_inputs()
    assert R.digest(a) == str(gold["a_sha256"]) and R.digest(b) == str(gold["b_sha256"]) and R.digest(st) == str(gold["stats_sha256"]), \
        "the inputs are not the recorded ones"
    assert float(st[..., 1:].sqrt().min()) > 1e3 * EPS_COS
    g, gmul = float(gold["g"]), float(gold["gmul"])
    db = Guard((B, n, c), dev)
    L().dupl_cos_sim_bwd(nan_in(a, dev).data_ptr(), nan_in(b, dev).data_ptr(), nan_in(st, dev).data_ptr(),
                         nan_in(torch.tensor([g]), dev).data_ptr(), gmul, db.ptr, B, n, c, c, n * c, EPS_COS, 0, stream())
    got = db.cpu()
    want = torch.from_numpy(gold["db_every_61st"])
    assert same_bits(got.view(-1)[::61], want), "db differs from the record"
    assert R.digest(got) == str(gold["db_sha256"]), "db differs from the record outside the sampled elements"
    T = Tally("cos bwd workload " + "x".join(map(str, R.COS_WORKLOAD)))
    ref, rb = R.cos_bwd_ref(a, b, st, float(np.float32(g)) * float(np.float32(gmul)), EPS_COS)
    T.add("db", (got.double() - ref).abs(), rb)
    T.done()
    print("cos bwd workload: bit-equal to the record of the kernel before the change below eps")


# =========================================================================================== mean_accum, msm, mask_fill
@pytest.mark.parametrize("n", R.SMALL_N)
def test_mean_accum_and_msm(dev, n):
    """both accumulate onto a non-zero loss[0]; msm with logits of +-100 and soft targets: loss only, dx only (no gscale: g = 1),
    dx with gscale, both"""
    T = Tally(f"mean_accum / msm n{n}")
    x, y = R.msm_inputs(n, n)
    b, C = R.msm_shape(n)
    xd, yd = nan_in(x, dev), nan_in(y, dev)
    loss = Guard((1,), dev, init=torch.tensor([0.25]))
    L().dupl_mean_accum(xd.data_ptr(), loss.ptr, n, 1.0 / n, stream())
    v, vb = R.mean_accum_ref(x, 0.25, float(np.float32(1.0 / n)))
    T.add("mean_accum", abs(float(loss.cpu()[0]) - v), vb)
    gs = nan_in(torch.tensor([0.8]), dev)
    for want_loss, want_dx, with_g in ((1, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 0, 1)):
        g = 0.8 if (with_g and want_dx) else 1.0
        rl, lb, rdx, dxb = R.msm_ref(x, y, g=float(np.float32(g)))
        loss, dx = Guard((1,), dev, init=torch.tensor([0.25])), Guard((b, C), dev)
        L().dupl_multilabel_soft_margin(xd.data_ptr(), yd.data_ptr(), loss.ptr if want_loss else None, dx.ptr if want_dx else None,
                                        gs.data_ptr() if with_g else None, b, C, stream())
        torch.cuda.synchronize()
        if want_loss:
            T.add(f"msm loss {want_loss}{want_dx}{with_g}", abs(float(loss.cpu()[0]) - 0.25 - rl), lb + 2 * EPS24 * (0.25 + abs(rl)))
        else:
            assert float(loss.cpu()[0]) == 0.25, "loss NULL: nothing is accumulated"
        if want_dx:
            T.add(f"msm dx {want_loss}{want_dx}{with_g}", (dx.cpu().double() - rdx).abs(), dxb)
        else:
            assert dx.untouched()
    T.done()


def test_mask_fill_grid_stride(dev):
    """n = 4096 x 256 + 3 (a second trip of the loop and a ragged tail); any non-zero mask byte counts"""
    n = 4096 * 256 + 3
    lab = rnd(n, seed=1)
    m = torch.tensor([0, 1, 255], dtype=torch.uint8)[rndint(0, 3, n, seed=2)]
    mbuf = torch.full((n + 2 * PAD,), 255, dtype=torch.uint8, device=dev)
    mbuf[PAD:PAD + n].copy_(m)
    out = Guard((n,), dev, init=lab)
    L().dupl_mask_fill(out.ptr, mbuf[PAD:].data_ptr(), -3.5, n, stream())
    assert same_bits(out.cpu(), torch.where(m != 0, torch.tensor(-3.5), lab))


# =========================================================================================== loss_total
def _lt_call(dev, vals, add, group, weight, ng, backward_g=None, gsums=True):
    n = len(vals)
    vd = nan_in(torch.tensor(vals, dtype=torch.float32), dev)
    ptrs = (ctypes.c_void_p * n)(*[vd.data_ptr() + 4 * i for i in range(n)])
    ca, cg, cw = (ctypes.c_float * n)(*add), (ctypes.c_int32 * n)(*group), (ctypes.c_float * ng)(*weight)
    if backward_g is None:
        tot, gs = Guard((1,), dev), Guard((ng,), dev)
        L().dupl_loss_total(ptrs, ca, cg, n, cw, ng, tot.ptr, gs.ptr if gsums else None, None, None, stream())
        torch.cuda.synchronize()
        assert gsums or gs.untouched()
        return tot.cpu().numpy()[0], gs.cpu().numpy()
    gt = Guard((n,), dev)
    L().dupl_loss_total(ptrs, ca, cg, n, cw, ng, None, None, nan_in(torch.tensor([backward_g]), dev).data_ptr(), gt.ptr, stream())
    return gt.cpu().numpy()


def _lt_cases():
    gen = np.random.RandomState(7)
    cases = [("1 term", [0], 1), ("16 terms 1 group", [0] * 16, 1), ("16 groups", list(range(16)), 16),
             ("reversed groups", list(range(15, -1, -1)), 16), ("interleaved", [i % 3 for i in range(16)], 3),
             ("empty middle group", [0, 2, 0, 2, 3], 4)]
    cases += [(f"{ng} groups", [(i * 7) % ng for i in range(16)], ng) for ng in range(1, 17)]
    out = []
    for name, group, ng in cases:
        n = len(group)
        vals = (gen.randn(n) * 3).astype(np.float32).tolist()
        add = [float(a) for a in gen.choice([0.0, 1.0, -0.37], size=n)]
        weight = gen.choice([1.0, 0.1, 0.05, 0.2, 12.0, 1.0 / 3.0], size=ng).astype(np.float32).tolist()
        out.append((name, vals, add, group, weight, ng))
    return out


def test_loss_total_is_the_fp32_expression(dev):
    """total, the group sums and the backward are BIT-equal to the numpy float32 emulation: group sums in list order, add + term only
    where add != 0, ((w0 G0 + w1 G1) + ...), backward g * w_group"""
    for name, vals, add, group, weight, ng in _lt_cases():
        total, Gs = R.loss_total_ref(vals, add, group, weight, ng)
        got_t, got_g = _lt_call(dev, vals, add, group, weight, ng)
        assert f32bits(got_t) == f32bits(total), name
        assert np.array_equal(f32bits(got_g), f32bits(Gs)), name
        got_t2, _ = _lt_call(dev, vals, add, group, weight, ng, gsums=False)
        assert f32bits(got_t2) == f32bits(total), name
        gt = _lt_call(dev, vals, add, group, weight, ng, backward_g=0.3)
        assert np.array_equal(f32bits(gt), f32bits(R.loss_total_bwd_ref(np.float32(0.3), group, weight))), name
    print(f"loss_total: {len(_lt_cases())} cases bit-equal")


def test_loss_total_refusals(dev):
    vd = nan_in(torch.ones(17), dev)
    tot, gs, gt, g = Guard((1,), dev), Guard((16,), dev), Guard((17,), dev), nan_in(torch.ones(1), dev)

    def call(n=2, ng=2, terms="ok", add=True, group=(0, 1), weight=True, total=True, gterm=False, gg=False):
        m = max(n, 1)
        ptr_list = [vd.data_ptr() + 4 * i for i in range(m)]
        if terms == "null_entry":
            ptr_list[-1] = None
        ptrs = None if terms is None else (ctypes.c_void_p * m)(*ptr_list)
        grp = list(group or ()) + [0] * m
        return L().dupl_loss_total.raw(ptrs, (ctypes.c_float * m)(*([0.0] * m)) if add else None,
                                       (ctypes.c_int32 * m)(*grp[:m]) if group is not None else None, n,
                                       (ctypes.c_float * max(ng, 1))(*([1.0] * max(ng, 1))) if weight else None, ng,
                                       tot.ptr if total else None, gs.ptr, g.data_ptr() if gg else None, gt.ptr if gterm else None, stream())
    assert call(terms=None) == ERR_ARG and call(group=None) == ERR_ARG and call(weight=False) == ERR_ARG
    assert call(n=0) == ERR_ARG and call(n=17, ng=1, group=(0,)) == ERR_ARG
    assert call(ng=0) == ERR_ARG and call(ng=17) == ERR_ARG
    assert call(total=True, gterm=True, gg=True) == ERR_ARG, "forward XOR backward"
    assert call(total=False, gterm=False) == ERR_ARG
    assert call(total=False, gterm=True, gg=False) == ERR_ARG, "a backward needs g"
    assert call(terms="null_entry") == ERR_ARG
    assert call(group=(0, 2)) == ERR_ARG and call(group=(-1, 0)) == ERR_ARG
    torch.cuda.synchronize()
    assert tot.untouched() and gs.untouched() and gt.untouched()


# =========================================================================================== LayerNorm forward
HALF_SENT = -1234.0


def _planes(rows, D, dev):
    """hi / lo fp16 planes [rows, D], each between two sentinel rows"""
    buf = torch.full((2, rows + 2, D), HALF_SENT, dtype=torch.float16, device=dev)
    return buf, buf[0, 1].data_ptr(), buf[1, 1].data_ptr()


def _planes_ok(buf, want):
    torch.cuda.synchronize()
    b = buf.cpu()
    assert bool((b[:, 0] == HALF_SENT).all()) and bool((b[:, -1] == HALF_SENT).all()), "the kernel wrote outside its planes"
    return torch.equal(b[:, 1:-1].contiguous().view(torch.int16), want.cpu().contiguous().view(torch.int16))


@pytest.mark.parametrize("rows", R.LN_FWD_ROWS)
@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_fwd_edges(dev, D, rows):
    """y / mean / rstd against float64 with row-wise bounds (a constant row, a row at offset 1e4); y only, planes only, both; plane_exp
    0 / 3 bit-equal to dupl_split_f16x2 / dupl_split_f16x2b of the kernel's own fp32 output; f32_rows in {0, 1, rows - 1, rows}: rows
    of y / mean / rstd beyond it untouched; mean / rstd NULL"""
    from dupl_amd import ops
    x, gamma, beta = R.ln_inputs(rows, D, rows * 7919 + D)
    ref = R.ln_fwd_ref(x, gamma, beta, EPS_LN)
    T = Tally(f"ln fwd {rows}x{D}")
    xd, gd, bd = nan_in(x, dev), nan_in(gamma, dev), nan_in(beta, dev)
    y, m, r = Guard((rows, D), dev), Guard((rows,), dev), Guard((rows,), dev)
    L().dupl_layernorm_fwd16(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.ptr, None, None, m.ptr, r.ptr, rows, D, EPS_LN, 0, 0, stream())
    y0, m0, r0 = y.cpu(), m.cpu(), r.cpu()
    T.add("y", (y0.double() - ref.y).abs(), ref.y_bound)
    T.add("mean", (m0.double() - ref.mean).abs(), ref.mean_bound)
    T.add("rstd", (r0.double() - ref.rstd).abs(), ref.rstd_bound)
    y1 = Guard((rows, D), dev)
    L().dupl_layernorm_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y1.ptr, None, None, rows, D, EPS_LN, stream())
    assert same_bits(y1.cpu(), y0), "mean / rstd NULL: the same y"
    want = {e: ops.split16(y.view, exp=e).planes for e in (0, 3)}
    sent = SENT[torch.float32][1]
    for e in (0, 3):
        # planes only
        buf, hi, lo = _planes(rows, D, dev)
        m2 = Guard((rows,), dev)
        L().dupl_layernorm_fwd16(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), None, hi, lo, m2.ptr, None, rows, D, EPS_LN, 0, e, stream())
        assert _planes_ok(buf, want[e]), f"planes only, plane_exp {e}"
        assert same_bits(m2.cpu(), m0)
        # both, for every f32_rows
        for fr in sorted({0, 1, rows - 1, rows}):
            keep = fr or rows
            buf, hi, lo = _planes(rows, D, dev)
            y2, m2, r2 = Guard((rows, D), dev), Guard((rows,), dev), Guard((rows,), dev)
            L().dupl_layernorm_fwd16(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y2.ptr, hi, lo, m2.ptr, r2.ptr, rows, D, EPS_LN, fr, e,
                                     stream())
            assert _planes_ok(buf, want[e]), f"planes of all rows, f32_rows {fr}, plane_exp {e}"
            for got, full in ((y2.cpu(), y0), (m2.cpu(), m0), (r2.cpu(), r0)):
                assert same_bits(got[:keep], full[:keep]), f"f32_rows {fr}"
                assert bool((bits(got[keep:]) == sent).all()), f"f32_rows {fr}: rows beyond it are untouched"
    T.done()


def test_layernorm_fwd_refusals(dev):
    xd, gd = nan_in(rnd(2, 2052), dev), nan_in(rnd(2052), dev)
    y, m = Guard((2, 2052), dev), Guard((2,), dev)
    buf, hi, lo = _planes(2, 2052, dev)
    f = L().dupl_layernorm_fwd16.raw
    a = (xd.data_ptr(), gd.data_ptr(), gd.data_ptr())
    for D in (0, 2, 2052, 6, -4):
        assert f(*a, y.ptr, hi, lo, m.ptr, m.ptr, 2, D, EPS_LN, 0, 0, stream()) == ERR_ARG, D
    assert f(*a, y.ptr, hi, lo, m.ptr, m.ptr, 2, 8, EPS_LN, 0, 16, stream()) == ERR_ARG, "plane_exp 16"
    assert f(*a, y.ptr, hi, lo, m.ptr, m.ptr, 2, 8, EPS_LN, 0, -1, stream()) == ERR_ARG
    assert f(*a, y.ptr, None, None, m.ptr, m.ptr, 2, 8, EPS_LN, 1, 0, stream()) == ERR_ARG, "f32_rows without planes"
    assert f(*a, y.ptr, hi, lo, m.ptr, m.ptr, 2, 8, EPS_LN, 3, 0, stream()) == ERR_ARG, "f32_rows > rows"
    assert f(*a, y.ptr, hi, None, m.ptr, m.ptr, 2, 8, EPS_LN, 0, 0, stream()) == ERR_ARG, "one plane only"
    assert f(*a, None, None, None, m.ptr, m.ptr, 2, 8, EPS_LN, 0, 0, stream()) == ERR_ARG, "no output"
    assert f(*a, y.ptr, hi, lo, m.ptr, m.ptr, 0, 8, EPS_LN, 0, 0, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert y.untouched() and m.untouched() and bool((buf == HALF_SENT).all())


# =========================================================================================== LayerNorm backward
LN_FORMS = ("atomics", "two_stage", "det_partials", "det_walk")


class _LnBwd:
    """the operands of one backward case on the device, and a launcher"""

    def __init__(self, dev, rows, D):
        self.dev, self.rows, self.D = dev, rows, D
        self.x, self.gamma, self.dy, self.dres = R.ln_bwd_inputs(rows, D, rows * 7919 + D)
        self.xd, self.gd, self.dresd = nan_in(self.x, dev), nan_in(self.gamma, dev), nan_in(self.dres, dev)
        self.m, self.r = Guard((rows,), dev), Guard((rows,), dev)
        y = Guard((rows, D), dev)
        L().dupl_layernorm_fwd(self.xd.data_ptr(), self.gd.data_ptr(), nan_in(torch.zeros(D), dev).data_ptr(), y.ptr, self.m.ptr, self.r.ptr,
                               rows, D, EPS_LN, stream())
        self.mean, self.rstd = self.m.cpu(), self.r.cpu()
        self.dg0, self.db0 = rnd(D, seed=21, scale=0.5), rnd(D, seed=22, scale=0.5)

    def ref(self, dres=True, dy=None):
        return R.ln_bwd_ref(self.dy if dy is None else dy, self.x, self.gamma, self.mean, self.rstd, self.dres if dres else None,
                            self.dg0, self.db0)

    def run(self, rpw=0, form="atomics", dres=True, dgamma=True, dbeta=True, clear=False, dy=None, amax0=0):
        dev, rows, D = self.dev, self.rows, self.D
        dyv = self.dy if dy is None else dy
        dyg, dx = Guard((rows, D), dev, init=dyv), Guard((rows, D), dev)
        dg, db = Guard((D,), dev, init=self.dg0), Guard((D,), dev, init=self.db0)
        am = Guard((1,), dev, torch.int32, init=torch.tensor([amax0], dtype=torch.int32))
        part, nb = None, 0
        if form in ("two_stage", "det_partials"):
            nb = L().dupl_layernorm_bwd_blocks(rows, rpw)
            part = Guard((nb, 2 * D), dev)
        det = int(form in ("det_partials", "det_walk"))
        L().dupl_layernorm_bwd(dyg.ptr, self.xd.data_ptr(), self.gd.data_ptr(), self.m.ptr, self.r.ptr,
                               self.dresd.data_ptr() if dres else None, dx.ptr, dg.ptr if dgamma else None, db.ptr if dbeta else None,
                               rows, D, am.ptr, part.ptr if part else None, nb, rpw, dyg.ptr if clear else None, det, stream())
        torch.cuda.synchronize()
        if part is not None:
            assert part.intact(), "the partial sums stay inside [blocks][2 D]"
        assert dgamma or same_bits(dg.cpu(), self.dg0), "dgamma NULL: nothing is accumulated"
        assert dbeta or same_bits(db.cpu(), self.db0)
        got_dy = dyg.cpu()
        if clear:
            assert not bool(bits(got_dy).any()), "dy comes back zero-filled"
        else:
            assert same_bits(got_dy, dyv), "dy is an input"
        return dict(dx=dx.cpu(), dg=dg.cpu(), db=db.cpu(), amax=int(am.cpu()[0]))

    def check(self, T, tag, got, ref, dgamma=True, dbeta=True):
        T.add(tag + " dx", (got["dx"].double() - ref.dx).abs(), ref.dx_bound)
        if dgamma:
            T.add(tag + " dgamma", (got["dg"].double() - ref.dgamma).abs(), ref.dgamma_bound)
        if dbeta:
            T.add(tag + " dbeta", (got["db"].double() - ref.dbeta).abs(), ref.dbeta_bound)
        assert got["amax"] == int(f32bits(float(got["dx"].abs().max()))), tag + ": amax is max |dx| of the dx returned, bit for bit"


@pytest.mark.parametrize("rows", R.LN_BWD_ROWS)
@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_bwd_edges(dev, D, rows):
    """every rows_per_wave x every reduction form (accumulating onto non-zero dgamma / dbeta, with dres, with amax_out); the
    deterministic forms twice; dres NULL; dgamma / dbeta each NULL and both; amax untouched by an all-zero dx; dy_clear on the
    in-kernel path (D <= 1024) or the fill path (D > 1024), deterministic with partials, with the column walk, in the plain two-stage form and with atomics"""
    K = _LnBwd(dev, rows, D)
    T = Tally(f"ln bwd {rows}x{D}")
    ref = K.ref()
    base, dx_by_rpw = {}, {}
    for rpw in R.LN_RPW:
        for form in LN_FORMS:
            got = K.run(rpw, form)
            K.check(T, f"rpw{rpw} {form}", got, ref)
            if form.startswith("det"):
                again = K.run(rpw, form)
                assert all(same_bits(got[k], again[k]) for k in ("dx", "dg", "db")), f"rpw{rpw} {form}: bit-reproducible"
            if rpw == 0:
                base[form] = got
        dx_by_rpw[rpw] = got["dx"]
    same = all(same_bits(dx_by_rpw[0], v) for v in dx_by_rpw.values())
    print(f"ln bwd {rows}x{D}: dx bit-equal across rows_per_wave {list(R.LN_RPW)}: {same}")
    # ---- dres NULL
    K.check(T, "no dres", K.run(0, "atomics", dres=False), K.ref(dres=False))
    # ---- dgamma / dbeta NULL
    for form in ("atomics", "det_partials", "det_walk"):
        for dgamma, dbeta in ((1, 0), (0, 1), (0, 0)):
            got = K.run(0, form, dgamma=bool(dgamma), dbeta=bool(dbeta))
            K.check(T, f"{form} dgamma={dgamma} dbeta={dbeta}", got, ref, dgamma, dbeta)
            assert same_bits(got["dx"], base[form]["dx"])
    # ---- an all-zero dx leaves the amax word alone
    got = K.run(0, "atomics", dres=False, dy=torch.zeros(rows, D), amax0=7)
    assert not bool(got["dx"].any()) and got["amax"] == 7
    # ---- dy_clear == dy
    # dgamma / dbeta of the run with clearing are bit-equal to the run without wherever the reduction has ONE order: the two
    # deterministic forms, and the plain two-stage form while its second stage is a single block row (grid <= 64 first-stage
    # blocks, i.e. every case here: one partial row per wave, then a fixed-order sum and a plain +=).  The atomics form adds the
    # blocks' LDS sums with atomicAdd in whatever order the blocks retire, so two runs of it need not agree in the last bits whether
    # dy is cleared or not: there dgamma / dbeta are held to the float64 bound instead, and dx / amax (no atomics) to bit-equality.
    assert L().dupl_layernorm_bwd_blocks(rows, 0) <= 4 * 64
    for form in ("det_partials", "det_walk", "two_stage", "atomics"):
        got = K.run(0, form, clear=True)
        assert same_bits(got["dx"], base[form]["dx"]) and got["amax"] == base[form]["amax"], f"dy_clear {form}"
        if form == "atomics":
            K.check(T, "dy_clear atomics", got, ref)
        else:
            assert same_bits(got["dg"], base[form]["dg"]) and same_bits(got["db"], base[form]["db"]), f"dy_clear {form}"
    T.done()


def test_layernorm_bwd_refusals(dev):
    rows, D = 17, 8
    K = _LnBwd(dev, rows, D)
    dyg, dx, dg = Guard((rows, D), dev, init=K.dy), Guard((rows, D), dev), Guard((D,), dev)
    other = Guard((rows, D), dev)
    f = L().dupl_layernorm_bwd.raw
    a = (dyg.ptr, K.xd.data_ptr(), K.gd.data_ptr(), K.m.ptr, K.r.ptr, None, dx.ptr, dg.ptr, dg.ptr)
    for rpw in (0, 1, 8):
        nb = L().dupl_layernorm_bwd_blocks(rows, rpw)
        assert nb == 4 * math.ceil(rows / (4 * (rpw or 4)))
        part = Guard((nb, 2 * D), dev)
        for det in (0, 1):
            assert f(*a, rows, D, None, part.ptr, nb - 1, rpw, None, det, stream()) == ERR_ARG, "partial_rows one too small"
        torch.cuda.synchronize()
        assert part.untouched()
    assert f(*a, rows, D, None, None, 0, 0, other.ptr, 0, stream()) == ERR_ARG, "dy_clear must be dy itself"
    assert f(*a, rows, D, None, None, 0, 65, None, 0, stream()) == ERR_ARG and f(*a, rows, D, None, None, 0, -1, None, 0, stream()) == ERR_ARG
    for badD in (0, 2, 2052):
        assert f(*a, rows, badD, None, None, 0, 0, None, 0, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert dx.untouched() and dg.untouched() and other.untouched() and same_bits(dyg.cpu(), K.dy)
