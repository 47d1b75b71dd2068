"""-m gpu: the exact-f32 attention kernels (csrc/attn.hip: dupl_attention_fwd / dupl_attention_bwd) at their edges.  They are the
yardstick of every bar of the split attention kernels (tests/test_attention_gpu.py: "2 x the exact-f32 kernel's error + ..."), the
fallback of engine.RangeGuard and the backward beyond 2 048 tokens; tests/test_attention_gpu.py sections 1 - 6 cover the split
kernels only and section 7 the lengths 1, 128 and >= 1 765.

  1  shape sweep against float64 (ref64): N around the 32-row wave, the 64-key stage and the 128-row block, both head sizes
  2  analytic cases: q = 0 gives the column mean of v; all the mass on the last key of a partial tile; N = 1 gives out = v
  3  containment: out, lse, delta and dqkv inside guard rows, through the C entry points
  4  isolation: the other image of a B = 2 call (NaN, then 1e30 decoys) never reaches an image's results; an image's rows do not
     depend on where in a (B, H) grid its head sits (xcd_remap3 with block totals that are not multiples of 8)
  5  refusals of both entry points: status -1, nothing written

Bars: the standing ones of test_attention_fwd_bwd (out 5e-6, lse 5e-6, dqkv 2e-5, each relative to the reference's maximum).

Measured on one MI355X (error next to its bar; the worst over B = 2, H = 3 and both head sizes):

    N            out (bar 5e-6)   lse (bar 5e-6)   dqkv (bar 2e-5)
    1, 2         1.6e-7           2.3e-7           6.7e-7
    31, 32, 33   5.1e-7           1.9e-7           1.0e-6
    63, 64, 65   7.1e-7           3.3e-7           9.4e-7
    127 .. 129   1.1e-6           2.4e-7           1.3e-6
    193          6.8e-7           2.0e-7           9.4e-7
    q = 0        5.0e-7           4.4e-8
    spike        5.8e-7           1.3e-7           1.1e-6
    N = 1        out = v exactly (0 ulp, bar 4)

Every containment, isolation and refusal case holds as written: the pass found no defect in csrc/attn.hip.  This module alone
runs in 3.9 s (92 tests; the slowest single test 1.4 s -- the first float64 reference of the process -- all others below 0.05 s).
The whole -m gpu suite with this module and tests/test_gemm_f32_gpu.py: 774 s (2 394 tests); the two are 7.2 s of it."""
import math

import numpy as np
import pytest
import torch

import test_attention_gpu as T
from test_attention_gpu import ref64

pytestmark = pytest.mark.gpu

B2, H3 = 2, 3
SWEEP_N = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193]
HDS = [32, 64]
BAR_OUT, BAR_LSE, BAR_DQKV = 5e-6, 5e-6, 2e-5


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def _f32_bars(tag, out, lse, ref, ref_lse, dqkv=None, ref_grad=None):
    eo, el = _rel(out, ref), _rel(lse, ref_lse)
    eg = _rel(dqkv, ref_grad) if dqkv is not None else 0.0
    print(f"{tag}: out {eo:.2e} (bar {BAR_OUT:.0e}), lse {el:.2e} (bar {BAR_LSE:.0e})" +
          (f", dqkv {eg:.2e} (bar {BAR_DQKV:.0e})" if dqkv is not None else ""))
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and (dqkv is None or torch.isfinite(dqkv).all())
    assert eo < BAR_OUT and el < BAR_LSE and eg < BAR_DQKV, tag


def _run(ops, qkv, dout, B, N, H, hd):
    scale = hd ** -0.5
    out, lse = ops.attention_fwd(qkv, B, N, H, hd, scale, need_lse=True)
    dqkv = ops.attention_bwd(qkv, out, dout, lse, B, N, H, hd, scale) if dout is not None else None
    return out, lse, dqkv


# ------------------------------------------------------------------------------------------ 1. shape sweep
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("N", SWEEP_N)
def test_f32_shape_sweep(dev, N, hd):
    from dupl_amd import ops
    B, H = B2, H3
    qkv = T._randn(B * N, 3 * H * hd, 1000 + N + hd, 1.5).to(dev)
    dout = T._randn(B * N, H * hd, 2000 + N + hd, 1.0).to(dev)
    ref, ref_lse, ref_grad = ref64(qkv, B, N, H, hd, hd ** -0.5, dout)
    out, lse, dqkv = _run(ops, qkv, dout, B, N, H, hd)
    _f32_bars(f"f32 sweep N{N} hd{hd}", out, lse, ref, ref_lse, dqkv, ref_grad)


# ------------------------------------------------------------------------------------------ 2. analytic cases
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("N", [33, 193])
def test_f32_zero_queries_give_the_column_mean(dev, N, hd):
    """q = 0: every probability is 1 / N, out is the column mean of v per head (float64, no softmax involved), lse = log N."""
    from dupl_amd import ops
    B, H = B2, H3
    D = H * hd
    qkv = T._randn(B * N, 3 * D, 40 + N, 1.5)
    qkv[:, :D] = 0.0
    qkv = qkv.to(dev)
    ref = qkv[:, 2 * D:].double().view(B, N, D).mean(1, keepdim=True).expand(B, N, D).reshape(B * N, D)
    ref_lse = torch.full((B, H, N), math.log(N), dtype=torch.float64, device=dev)
    out, lse, _ = _run(ops, qkv, None, B, N, H, hd)
    _f32_bars(f"f32 q=0 N{N} hd{hd}", out, lse, ref, ref_lse)


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("N", [33, 65, 129])
def test_f32_spike_on_the_last_key_of_a_partial_tile(dev, N, hd):
    """The last key (the only row of its 32-key half / 64-key stage / 128-row block) is 6 x query 3 in every head: query 3 puts
    > 0.99 of its probability there.  A mask or a staging guard that is off by one loses exactly this key."""
    from dupl_amd import ops
    B, H = 1, H3
    D = H * hd
    scale = hd ** -0.5
    qkv = T._randn(B * N, 3 * D, 21 + hd, 1.0)
    qkv[N - 1, D:2 * D] = 6.0 * qkv[3, 0:D]
    qkv = qkv.to(dev)
    dout = T._randn(B * N, D, 22 + hd, 1.0).to(dev)
    ref, ref_lse, ref_grad = ref64(qkv, B, N, H, hd, scale, dout)
    t = qkv.double().view(N, 3, H, hd)
    p_last = ((t[3, 0] * t[:, 1]).sum(-1) * scale).softmax(0)[N - 1]
    assert float(p_last.min()) > 0.99
    out, lse, dqkv = _run(ops, qkv, dout, B, N, H, hd)
    _f32_bars(f"f32 spike N{N} hd{hd}", out, lse, ref, ref_lse, dqkv, ref_grad)
    v_last = qkv[N - 1, 2 * D:].double()
    assert float((out[3].double() - v_last).abs().max()) <= 0.02 * float(qkv[:, 2 * D:].abs().max())


@pytest.mark.parametrize("hd", HDS)
def test_f32_one_token_returns_its_value_row(dev, hd):
    """N = 1: the only probability is exp(0) / 1, out = v within 4 ulp per element and lse = the one score."""
    from dupl_amd import ops
    B, H, N = 3, 5, 1
    D = H * hd
    qkv = T._randn(B, 3 * D, 77 + hd, 1.5).to(dev)
    out, lse, _ = _run(ops, qkv, None, B, N, H, hd)
    v = qkv[:, 2 * D:].cpu()
    ulp = torch.from_numpy(np.spacing(v.abs().numpy()))
    err = (out.cpu().double() - v.double()).abs()
    print(f"f32 N1 hd{hd}: out vs v, worst {float((err / ulp.double()).max()):.2f} ulp (bar 4)")
    assert bool((err <= 4 * ulp.double()).all())
    _, ref_lse, _ = ref64(qkv, B, N, H, hd, hd ** -0.5)
    assert _rel(lse, ref_lse) < BAR_LSE


# ------------------------------------------------------------------------------------------ 3. containment
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,N", T.RAGGED[:3] + [(2, 128)], ids=[f"B{b}-N{n}" for b, n in T.RAGGED[:3] + [(2, 128)]])
def test_f32_writes_nothing_outside_its_destinations(dev, B, N, hd):
    """dupl_attention_fwd / dupl_attention_bwd with out, lse, delta and dqkv inside NaN-filled tensors (128 guard rows, N guard
    entries on either side): guards bit-unchanged, destinations fully written and equal to the unguarded call's."""
    from dupl_amd import ops
    H = H3
    D = H * hd
    scale = hd ** -0.5
    qkv = T._randn(B * N, 3 * D, 300 + N, 1.5).to(dev)
    dout = T._randn(B * N, D, 301 + N, 1.0).to(dev)
    out0, lse0, dqkv0 = _run(ops, qkv, dout, B, N, H, hd)
    out = T._guarded_rows(B * N, D, dev, "out")
    lse = T._guarded_flat(B * H * N, N, dev, "lse")
    ops.L().dupl_attention_fwd(qkv.data_ptr(), out.ptr(), lse.ptr(), B, N, H, hd, float(scale), ops._stream())
    out.check()
    lse.check()
    assert T._same_bits(out.view, out0) and T._same_bits(lse.view, lse0.reshape(-1))
    dqkv = T._guarded_rows(B * N, 3 * D, dev, "dqkv")
    delta = T._guarded_flat(B * H * N, N, dev, "delta")
    ops.L().dupl_attention_bwd(qkv.data_ptr(), out0.data_ptr(), dout.data_ptr(), lse0.data_ptr(), delta.ptr(), dqkv.ptr(), B, N, H,
                               hd, float(scale), ops._stream())
    dqkv.check()
    delta.check()
    assert T._same_bits(dqkv.view, dqkv0)
    # delta = sum_d dO O, hd terms in fp32: within gamma(hd) * sum |dO| |O| of float64 in any order
    want_delta = (out0.double() * dout.double()).view(B, N, H, hd).sum(-1).permute(0, 2, 1).reshape(-1)
    mag = (out0.double() * dout.double()).abs().view(B, N, H, hd).sum(-1).permute(0, 2, 1).reshape(-1)
    assert bool(((delta.view.double() - want_delta).abs() <= hd * 2.0 ** -24 / (1 - hd * 2.0 ** -24) * mag).all())
    # and without lse (optional): out alone, the same bits
    out = T._guarded_rows(B * N, D, dev, "out (no lse)")
    ops.L().dupl_attention_fwd(qkv.data_ptr(), out.ptr(), None, B, N, H, hd, float(scale), ops._stream())
    out.check()
    assert T._same_bits(out.view, out0)


# ------------------------------------------------------------------------------------------ 4. isolation
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("poison", ["nan", "decoy"])
@pytest.mark.parametrize("N", [33, 65, 129, 197])
def test_f32_reads_nothing_outside_its_own_image(dev, N, poison, hd):
    """B = 2 with the other image's qkv, dout, out and lse all NaN (then all 1e30): an image's out, lse and dqkv are bit-equal
    to its B = 1 run."""
    from dupl_amd import ops
    H = H3
    D = H * hd
    scale = hd ** -0.5
    bad = float("nan") if poison == "nan" else 1e30
    for img in (0, 1):
        qkv1 = T._randn(N, 3 * D, 500 + N + img, 1.5).to(dev)
        dout1 = T._randn(N, D, 501 + N + img, 1.0).to(dev)
        out1, lse1, dqkv1 = _run(ops, qkv1, dout1, 1, N, H, hd)
        assert torch.isfinite(out1).all() and torch.isfinite(lse1).all() and torch.isfinite(dqkv1).all()
        rs = slice(img * N, (img + 1) * N)
        qkv, dout = torch.full((2 * N, 3 * D), bad, device=dev), torch.full((2 * N, D), bad, device=dev)
        qkv[rs], dout[rs] = qkv1, dout1
        out, lse = ops.attention_fwd(qkv, 2, N, H, hd, scale, need_lse=True)
        assert T._same_bits(out[rs], out1), f"image {img}: out"
        assert T._same_bits(lse[img], lse1[0]), f"image {img}: lse"
        src_out, src_lse = torch.full((2 * N, D), bad, device=dev), torch.full((2, H, N), bad, device=dev)
        src_out[rs], src_lse[img] = out1, lse1[0]
        dqkv = ops.attention_bwd(qkv, src_out, dout, src_lse, 2, N, H, hd, scale)
        assert T._same_bits(dqkv[rs], dqkv1), f"image {img}: dqkv"


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("N", [129, 197])
def test_f32_rows_do_not_depend_on_the_grid_around_them(dev, N, hd):
    """Every (image, head) of a (B, H) = (3, 5) call -- 30 blocks, not a multiple of 8 -- against the same head alone as
    (B, H) = (1, 1): out, lse and dqkv bit-equal."""
    from dupl_amd import ops
    B, H = 3, 5
    D = H * hd
    qkv = T._randn(B * N, 3 * D, 600 + N, 1.5).to(dev)
    dout = T._randn(B * N, D, 601 + N, 1.0).to(dev)
    out, lse, dqkv = _run(ops, qkv, dout, B, N, H, hd)
    q4, g4 = qkv.view(B, N, 3, H, hd), dqkv.view(B, N, 3, H, hd)
    for b in range(B):
        for h in range(H):
            qkv1 = q4[b, :, :, h].reshape(N, 3 * hd).contiguous()
            dout1 = dout.view(B, N, H, hd)[b, :, h].contiguous()
            out1, lse1, dqkv1 = _run(ops, qkv1, dout1, 1, N, 1, hd)
            assert T._same_bits(out.view(B, N, H, hd)[b, :, h], out1), (b, h, "out")
            assert T._same_bits(lse[b, h], lse1[0, 0]), (b, h, "lse")
            assert T._same_bits(g4[b, :, :, h].reshape(N, 3 * hd), dqkv1), (b, h, "dqkv")


# ------------------------------------------------------------------------------------------ 5. refusals
_FWD_BAD = {"fwd-qkv-null": dict(qkv=None), "fwd-out-null": dict(out=None)}
_BWD_BAD = {f"bwd-{k}-null": {k: None} for k in ("qkv", "out", "dout", "lse", "delta", "dqkv")}
_DIM_BAD = {f"{k}{v}": {k: v} for k in ("B", "N", "H") for v in (0, -1)}
_DIM_BAD.update({f"hd{v}": {"hd": v} for v in (0, 16, 48, 128)})
REFUSALS = list(_FWD_BAD) + list(_BWD_BAD) + [f"{e}-{k}" for e in ("fwd", "bwd") for k in _DIM_BAD]


@pytest.mark.parametrize("case", REFUSALS)
def test_f32_entry_points_refuse_bad_arguments_before_launching(dev, case):
    from dupl_amd import ops
    B, N, H, hd = 1, 33, 2, 64
    D = H * hd
    qkv = T._randn(B * N, 3 * D, 700, 1.0).to(dev)
    src_out, dout, src_lse = torch.zeros(B * N, D, device=dev), T._randn(B * N, D, 701, 1.0).to(dev), torch.zeros(B, H, N, device=dev)
    out, lse = T._nan32(B * N, D, dev=dev), T._nan32(B, H, N, dev=dev)
    dqkv, delta = T._nan32(B * N, 3 * D, dev=dev), T._nan32(B, H, N, dev=dev)
    entry, _, what = case.partition("-")
    kw = dict(_FWD_BAD.get(case) or _BWD_BAD.get(case) or _DIM_BAD[what])
    dims = [kw.pop(k, v) for k, v in (("B", B), ("N", N), ("H", H), ("hd", hd))]
    if entry == "fwd":
        p = dict(qkv=qkv.data_ptr(), out=out.data_ptr())
        p.update(kw)
        call = lambda: ops.L().dupl_attention_fwd(p["qkv"], p["out"], lse.data_ptr(), *dims, float(hd ** -0.5), ops._stream())  # noqa: E731
    else:
        p = dict(qkv=qkv.data_ptr(), out=src_out.data_ptr(), dout=dout.data_ptr(), lse=src_lse.data_ptr(), delta=delta.data_ptr(),
                 dqkv=dqkv.data_ptr())
        p.update(kw)
        call = lambda: ops.L().dupl_attention_bwd(p["qkv"], p["out"], p["dout"], p["lse"], p["delta"], p["dqkv"], *dims,  # noqa: E731
                                                  float(hd ** -0.5), ops._stream())
    with pytest.raises(RuntimeError, match="status -1"):
        call()
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv), ("delta", delta)):
        assert T._is_pattern(t), f"{case}: {name} was written"
