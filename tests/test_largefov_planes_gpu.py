"""The LargeFOV decoder on operand planes (csrc/conv.hip: im2col_dil3_planes, split_wT_tc, col2im_dil3_tc; engine.DECODER_PLANES):
every new kernel is BIT-equal to the fp32-col route it replaces -- im2col + split16 / split_prepare, the transposing split of the
conv weight, col2im_dil3 -- and so is the step's decoder (forward values, the three weight gradients, the gradient into the tokens).

Technique of tests/test_glue_kernels_gpu.py: NaN in every element a kernel must skip (cls rows, padding columns, buffer slack),
sentinels around every output."""
import pytest
import torch

import glue_ref as G
from kernel_guard import NAN, EPS24, _ALIVE, Guard, bits, nan_in, ratio_report, rnd, rndint, same_bits, stream  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _ALIVE.clear()


# (B, h, w, Cin): every non-centre tap outside the image at dil 5; not square; 363 rows (no multiple of 32: Mp > M); the phase C grid
SHAPES = [(1, 3, 4, 32), (2, 7, 12, 32), (3, 11, 11, 96), (2, 21, 21, 64)]


def _token_major(x, ld, lead, fill=NAN):
    """(B, Cin, h, w) -> the engine's layout [B][lead + h*w][ld] (lead cls rows, ld - Cin padding columns, both `fill`)."""
    B, Cin, h, w = x.shape
    t = torch.full((B, lead + h * w, ld), fill, dtype=torch.float32)
    t[:, lead:, :Cin] = x.permute(0, 2, 3, 1).reshape(B, h * w, Cin)
    return t


class Planes:
    """fp16 hi / lo planes [rows][cols], each inside its own sentinel-guarded allocation."""

    def __init__(self, rows, cols, dev):
        assert rows * cols % 2 == 0
        self.g = [Guard((rows * cols // 2,), dev) for _ in range(2)]
        self.rows, self.cols = rows, cols

    @property
    def hi(self):
        return self.g[0].ptr

    @property
    def lo(self):
        return self.g[1].ptr

    def cpu(self):
        """[2, rows, cols] as int16 bit patterns (asserts the sentinels)"""
        return torch.stack([g.cpu().view(torch.int16).view(self.rows, self.cols) for g in self.g])


def _bits16(split):
    torch.cuda.synchronize()
    return split.planes.cpu().view(torch.int16)


@pytest.mark.parametrize("dil", [1, 5])
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("B,h,w,Cin", SHAPES)
def test_im2col_planes_are_the_split_of_the_fp32_col(dev, B, h, w, Cin, lead, pad, dil):
    """Row-major planes == split16(dupl_im2col_dil3(x)); transposed planes == split_prepare(col, scaled=False, want_T=True,
    rows_pad=Mp) including the zero rows M .. Mp-1; each pair also when asked for alone; nothing written outside either image."""
    from dupl_amd import ops
    ld, hw = Cin + pad, h * w
    M, K9 = B * hw, 9 * Cin
    Mp = (M + 31) // 32 * 32
    x = rnd(B, Cin, h, w, seed=h + Cin)
    x.view(-1)[::7] = 0.0
    x.view(-1)[3::11] *= -1e-6            # small values: a subnormal / zero hi with a live lo
    x.view(-1)[5::13] *= 3e4
    xt = nan_in(_token_major(x, ld, lead), dev)
    src, img = xt.data_ptr() + 4 * lead * ld, (lead + hw) * ld
    col = torch.empty((M, K9), device=dev, dtype=torch.float32)
    ops.L().dupl_im2col_dil3(src, col.data_ptr(), B, h, w, Cin, dil, ld, img, stream())
    want_rm = _bits16(ops.split16(col))
    want_T = _bits16(ops.split_prepare(col, scaled=False, want_rm=False, want_T=True, rows_pad=Mp)[1])
    assert Mp == M or bool((want_T[:, :, M:] == 0).all())
    for rm, T in ((True, True), (True, False), (False, True)):
        p, pT = Planes(M, K9, dev), Planes(K9, Mp, dev)
        ops.L().dupl_im2col_dil3_planes(src, p.hi if rm else None, p.lo if rm else None, pT.hi if T else None, pT.lo if T else None,
                                        B, h, w, Cin, dil, ld, img, Mp, stream())
        torch.cuda.synchronize()
        if rm:
            assert torch.equal(p.cpu(), want_rm), "row-major planes"
        else:
            assert all(g.untouched() for g in p.g)
        if T:
            assert torch.equal(pT.cpu(), want_T), "transposed planes"
        else:
            assert all(g.untouched() for g in pT.g)
    # the wrapper the engine calls
    rm16, T16 = ops.im2col_dil3_planes(src, dev, B, h, w, Cin, dil, ld, img, want_T=True, rows_pad=Mp)
    assert torch.equal(_bits16(rm16), want_rm) and torch.equal(_bits16(T16), want_T)


def test_im2col_planes_refuses_what_it_cannot_run(dev):
    from dupl_amd import ops
    x = nan_in(rnd(2 * 12 * 40), dev)
    p, pT = Planes(12, 9 * 40, dev), Planes(9 * 40, 32, dev)
    raw = ops.L().dupl_im2col_dil3_planes.raw
    ok = dict(x=x.data_ptr(), hi=p.hi, lo=p.lo, hiT=pT.hi, loT=pT.lo, B=1, h=3, w=4, Cin=40, dil=5, ld=40, img=480, Mp=32)
    for bad in (dict(Cin=36, ld=36), dict(ld=42), dict(ld=32), dict(img=482), dict(Mp=8), dict(Mp=20), dict(lo=None), dict(loT=None),
                dict(hi=None, lo=None, hiT=None, loT=None), dict(x=x.data_ptr() + 4), dict(hi=p.hi + 2), dict(dil=0), dict(x=None)):
        a = dict(ok, **bad)
        assert raw(a["x"], a["hi"], a["lo"], a["hiT"], a["loT"], a["B"], a["h"], a["w"], a["Cin"], a["dil"], a["ld"], a["img"],
                   a["Mp"], stream()) == -1, bad
    torch.cuda.synchronize()
    assert all(g.untouched() for g in p.g + pT.g)


@pytest.mark.parametrize("Cout,Cin", [(32, 32), (96, 96)])
def test_wT_planes_in_tap_major_row_order(dev, Cout, Cin):
    """[Cout][9 Cin] = [32][288] and [96][864]: row tap*Cin + c of the new planes == row c*9 + tap of the present transposing split."""
    from dupl_amd import ops
    w = rnd(Cout, 9 * Cin, seed=Cout, scale=0.05)
    w.view(-1)[::5] *= 1e-4
    wd = nan_in(w, dev)
    old = _bits16(ops.split_prepare(wd, scaled=False, want_rm=False, want_T=True, rows_pad=Cout)[1])       # [2, 9 Cin, Cout]
    want = old.view(2, Cin, 9, Cout).permute(0, 2, 1, 3).reshape(2, 9 * Cin, Cout)
    pT = Planes(9 * Cin, Cout, dev)
    ops.L().dupl_split_wT_tc(wd.data_ptr(), 9 * Cin, Cout, Cin, pT.hi, pT.lo, Cout, stream())
    assert torch.equal(pT.cpu(), want)
    assert torch.equal(_bits16(ops.split_wT_tc(wd, Cin)), want)
    # rows Cout .. Rp-1 of the transposed image are zeros, as in split_prepare
    Rp = Cout + 8
    old = _bits16(ops.split_prepare(wd, scaled=False, want_rm=False, want_T=True, rows_pad=Rp)[1])
    pT = Planes(9 * Cin, Rp, dev)
    ops.L().dupl_split_wT_tc(wd.data_ptr(), 9 * Cin, Cout, Cin, pT.hi, pT.lo, Rp, stream())
    assert torch.equal(pT.cpu(), old.view(2, Cin, 9, Rp).permute(0, 2, 1, 3).reshape(2, 9 * Cin, Rp))
    raw = ops.L().dupl_split_wT_tc.raw
    for a in ((wd.data_ptr(), 9 * Cin, Cout, Cin, pT.hi, pT.lo, Cout + 4), (wd.data_ptr(), 9 * Cin - 4, Cout, Cin, pT.hi, pT.lo, Rp),
              (wd.data_ptr(), 9 * Cin, Cout, Cin, pT.hi, None, Rp), (wd.data_ptr() + 4, 9 * Cin, Cout, Cin, pT.hi, pT.lo, Rp),
              (wd.data_ptr(), 9 * Cin, Cout, Cin, pT.hi, pT.lo, Cout - 8)):
        assert raw(*a, stream()) == -1


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dil", [1, 5])
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("B,h,w,Cin", SHAPES)
def test_col2im_tc_is_col2im_on_permuted_columns(dev, B, h, w, Cin, lead, pad, dil, acc, relu):
    """dupl_col2im_dil3_tc on dcol with column tap*Cin + c is bit-equal to dupl_col2im_dil3 on the (c*9 + tap) original, bytes
    outside the operand unchanged; and within 9 * 2^-24 * col2im64(|dcol|) of the float64 fold (the existing test's bound)."""
    from dupl_amd import ops
    ld, hw = Cin + pad, h * w
    dcol = rnd(B * hw, Cin * 9, seed=dil + Cin)
    dcol_tc = dcol.view(B * hw, Cin, 9).transpose(1, 2).reshape(B * hw, 9 * Cin)
    start = rnd(B, lead + hw, ld, seed=3)
    mask_d, keep = None, torch.ones(B, Cin, h, w, dtype=torch.bool)
    if relu:
        m = rnd(B, Cin, h, w, seed=4)
        sel = rndint(0, 8, B, Cin, h, w, seed=5)
        m[sel == 0], m[sel == 1], m[sel == 2] = 0.0, -0.0, NAN
        keep = m > 0
        mask_d = nan_in(_token_major(m, ld, lead), dev)
    got = []
    for fn, d in ((ops.L().dupl_col2im_dil3, dcol), (ops.L().dupl_col2im_dil3_tc, dcol_tc)):
        dx = Guard((B, lead + hw, ld), dev, init=start)
        fn(nan_in(d, dev).data_ptr(), dx.ptr + 4 * lead * ld, B, h, w, Cin, dil, ld, (lead + hw) * ld, acc,
           mask_d.data_ptr() + 4 * lead * ld if relu else None, stream())
        got.append(dx.cpu())
    assert same_bits(got[1], got[0])
    outside = torch.ones(B, lead + hw, ld, dtype=torch.bool)
    outside[:, lead:, :Cin] = False
    assert bool((bits(got[1])[outside] == bits(start)[outside]).all()), "col2im_tc wrote outside its operand"
    got_x = got[1][:, lead:, :Cin].reshape(B, h, w, Cin).permute(0, 3, 1, 2).double()
    st_x = start[:, lead:, :Cin].reshape(B, h, w, Cin).permute(0, 3, 1, 2).double()
    s64 = G.col2im64(dcol.double(), B, h, w, dil) * keep
    bound = 9 * EPS24 * G.col2im64(dcol.double().abs(), B, h, w, dil)
    ref = s64 + st_x if acc else s64
    if acc:
        bound = bound + EPS24 * st_x.abs()
    assert bool(torch.isfinite(got_x).all())
    assert ratio_report(f"col2im_dil3_tc B={B} {h}x{w} Cin={Cin} dil={dil} ld+{pad} lead={lead} acc={acc} relu={relu}",
                        (got_x - ref).abs(), bound, quiet=True) <= 1.0


def test_col2im_tc_refuses_what_it_cannot_run(dev):
    from dupl_amd import ops
    dcol = nan_in(rnd(12, 9 * 8), dev)
    dx = Guard((12, 8), dev)
    raw = ops.L().dupl_col2im_dil3_tc.raw
    for a in ((dcol.data_ptr(), dx.ptr, 1, 3, 4, 6, 5, 8, 96, 0, None), (dcol.data_ptr(), dx.ptr, 1, 3, 4, 8, 5, 10, 96, 0, None),
              (dcol.data_ptr(), dx.ptr, 1, 3, 4, 8, 5, 8, 98, 0, None), (dcol.data_ptr() + 4, dx.ptr, 1, 3, 4, 8, 5, 8, 96, 0, None),
              (dcol.data_ptr(), dx.ptr + 8, 1, 3, 4, 8, 5, 8, 96, 0, None), (dcol.data_ptr(), dx.ptr, 1, 3, 4, 8, 5, 8, 96, 0, dx.ptr + 4),
              (dcol.data_ptr(), dx.ptr, 1, 3, 4, 8, 5, 4, 96, 0, None), (None, dx.ptr, 1, 3, 4, 8, 5, 8, 96, 0, None)):
        assert raw(*a, stream()) == -1, a
    torch.cuda.synchronize()
    assert dx.untouched()


# =========================================================================================== the step's decoder, both routes
def _decoder_run(dev, net, x, dseg, planes, monkeypatch):
    """seg, h6, h7, the three decoder weight gradients and the gradient that reaches the tokens, with engine.DECODER_PLANES = planes"""
    from dupl_amd import engine
    grabbed = []
    monkeypatch.setattr(engine, "DECODER_PLANES", planes)
    monkeypatch.setattr(engine, "encoder_backward", lambda P, enc, dtf, dta, on_ready=None: grabbed.append(dtf.clone()))
    net._store.grad.zero_()
    with torch.no_grad():
        (_, seg, _, _), sv = engine.network_forward(net._P, x, save=True)
        on_planes = sv.col6 is None, sv.col7 is None
        engine.network_backward(net._P, sv, None, dseg, None, None)
    torch.cuda.synchronize()
    out = {"seg": seg, "h6": sv.h6, "h7": sv.h7, "dtf": grabbed[0]}
    for k in ("conv6", "conv7", "conv8"):
        out["d" + k] = net._store.view(0, f"decoder.{k}.weight", grad=True).clone()
    return {k: v.cpu() for k, v in out.items()}, on_planes


@pytest.mark.parametrize("S", [96, 112])          # 2 x 36 = 72 token rows; 2 x 49 = 98 (no multiple of 32)
def test_step_decoder_is_bit_equal_on_both_routes(dev, S, monkeypatch):
    """tiny_test backbone, B = 2, deterministic mode: seg, h6, h7, the three decoder weight gradients and the gradient into the
    token map are bit-equal between the planes route (each part alone and both) and the fp32-col route (DUPL_DECODER_PLANES=0)."""
    from dupl_amd import engine, ops
    from dupl_amd.model.model_dupl import network
    from oracle import dupl_oracle as O
    assert engine.GEMM_MODE == "f16x3"
    net = network("tiny_test", num_classes=21, pretrained=False, aux_layer=-3)
    net.load_state_dict(O.make_student_params(O.VIT_TINY, 21, seed=1), strict=True)
    net.to(dev)
    x = O.hash_normal(f"xlf{S}", (2, 3, S, S), seed=1).to(dev)
    dseg = (O.hash_normal(f"dseg{S}", (2, 21, S // 16, S // 16), seed=2) * 1e-3).to(dev)
    prev = ops.deterministic()
    ops.set_deterministic(True)
    try:
        old, on = _decoder_run(dev, net, x, dseg, 0, monkeypatch)
        assert on == (False, False)
        assert float(old["dtf"].abs().max()) > 0 and float(old["dconv6"].abs().max()) > 0
        for planes in (1, 2, 3):
            new, on = _decoder_run(dev, net, x, dseg, planes, monkeypatch)
            assert on == (bool(planes & 1),) * 2, "the guard routed a decoder conv off the planes: the comparison would be empty"
            for k in old:
                assert same_bits(new[k], old[k]), (planes, k)
    finally:
        ops.set_deterministic(prev)
