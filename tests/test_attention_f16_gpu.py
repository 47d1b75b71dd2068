"""-m gpu: the single-product attention forward (csrc/attn_split.hip attn_fwd16_m16_kernel<1>; `products` = 1 of
dupl_attention_fwd16_prod / dupl_attention_fwd16_segs_prod, ops.attention_fwd16(.., products=1)): S = q_hi k_hi^T, softmax in fp32
with the lazy running maximum of attn_fwd16_m16_kernel, the probabilities rounded to ONE fp16 plane, O = P_hi v_hi.

  1  against float64 attention of the decoded hi planes of q, k, v.  The bound is derived, not measured: rounding a probability to
     fp16 is a relative 2^-11, so |O - ref| <= 2^-10 * max |v_hi| per (image, head) -- the factor 2 so that the bound holds whether the
     row sum is taken before or after the rounding -- plus the existing fp32 forward bar (2 x the exact-f32 kernel's error + 2e-7 of
     max |ref|).  A CPU model of the kernel gives 1e-5 .. 5e-5 of max |v|: the bound does not bind on a correct kernel, and a dropped
     key tile or a wrong row order exceeds it by orders of magnitude.  Shapes: FWD_CASES of test_attention_mfma16_gpu.py up to N = 785.
  2  the planes bar in both formats
  3  one segment = the single launch bit for bit; an image's rows do not depend on B or on the segment layout
  4  containment and isolation at EDGE_N
  5  refusals: lse != NULL, products outside {1, 3}, hd != 64
  6  the single-lane-group spike of the m16 test: the shared lazy maximum must not overflow the single P plane

Helpers, shapes and bars are imported from the existing attention tests.  Every output is pre-filled with its NaN patterns."""
import ctypes

import pytest
import torch

import test_attention_gpu as T
import test_attention_mfma16_gpu as M16
from test_attention_gpu import HD, SCALE

pytestmark = pytest.mark.gpu

FWD_CASES = [c for c in M16.FWD_CASES if c[1] != 1765]


def _hi(qkv16):
    """The values the kernel reads: the hi plane of format 0 planes, as fp32."""
    return qkv16.planes[0].float()


def _check(dev, tag, qkv, B, N, H, planes=True):
    """products = 1 on the planes of qkv against float64 attention of their hi plane; returns (out, qkv16)."""
    from dupl_amd import ops
    D = H * HD
    qkv16 = ops.split16(qkv)
    qh = _hi(qkv16)
    ref, _, _ = T.ref64(qh, B, N, H, HD, SCALE)
    o32, _ = ops.attention_fwd(qh, B, N, H, HD, SCALE)
    out = T._nan32(B * N, D, dev=dev)
    o0 = T._nan_split16(B * N, D, dev) if planes else None
    assert ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out=out, out16=o0, products=1) is None
    assert torch.isfinite(out).all(), tag
    sc = float(ref.abs().max())
    e32 = float((o32.double() - ref).abs().max()) / sc
    fwd_bar = (2.0 * e32 + 2e-7) * sc
    vmax = qh.view(B, N, 3, H, HD)[:, :, 2].abs().amax(dim=(1, 3))                       # [B][H]
    err = (out.double() - ref).abs().view(B, N, H, HD).amax(dim=(1, 3))                  # [B][H]
    bound = 2.0 ** -10 * vmax.double() + fwd_bar
    print(f"{tag}: max err / max |v_hi| {float((err / vmax.double()).max()):.2e} (bound 2^-10 = {2.0 ** -10:.2e} + fp32 bar {fwd_bar:.2e})")
    assert bool((err <= bound).all()), tag
    if planes:
        T._planes_bar(tag, out, o0)
        o1 = T._nan_split16(B * N, D, dev, ops.EXP_ACT)
        ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out16=o1, products=1)
        T._planes_bar(tag, out, o1)
    return out, qkv16


# ------------------------------------------------------------------------------------------ 1, 2. shape sweep
@pytest.mark.parametrize("B,N,H", FWD_CASES, ids=[f"B{b}-N{n}-H{h}" for b, n, h in FWD_CASES])
def test_h1_shape_sweep(dev, B, N, H):
    _check(dev, f"h1 fwd B{B} N{N} H{H}", T._randn(B * N, 3 * H * HD, B * 1000 + N + 7 * H, 1.5).to(dev), B, N, H)


def test_h1_differs_from_the_three_product_kernel(dev):
    """The mode is active: on the same planes the single-product output is not the f16x3 output (whose error against the
    full-precision reference is ~1e-7; the hi-plane rounding alone moves the result by ~1e-4)."""
    from dupl_amd import ops
    B, N, H = 2, 197, 12
    qkv16 = ops.split16(T._randn(B * N, 3 * H * HD, 11, 1.5).to(dev))
    o3, o1 = T._nan32(B * N, H * HD, dev=dev), T._nan32(B * N, H * HD, dev=dev)
    ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out=o3)
    ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out=o1, products=1)
    assert float((o3 - o1).abs().max()) > 1e-5 * float(o3.abs().max())


# ------------------------------------------------------------------------------------------ 6. the lazy maximum
@pytest.mark.parametrize("which", list(M16.SPIKES))
def test_h1_spike_seen_by_one_lane_group(dev, which):
    """test_m16_spike_seen_by_one_lane_group, run single-product: one query's largest score sits in ONE key of the second key tile,
    ~69 (base 2) above its running maximum.  A missed move would leave P = 2^66 in the single fp16 plane (inf, the output NaN)."""
    B, H, N = 1, 12, 130
    D = H * HD
    q, k = M16.SPIKES[which]
    qkv = T._randn(B * N, 3 * D, 31, 1.0)
    keep = qkv[q, 0:D].clone()
    qkv[:, 0:D] *= 0.1
    qkv[q, 0:D] = keep
    qkv[k, D:2 * D] = 6.0 * keep
    qkv = qkv.to(dev)
    out, qkv16 = _check(dev, f"h1 spike {which}", qkv, B, N, H, planes=False)
    t = _hi(qkv16).double().view(N, 3, H, HD)
    s2 = (t[:, 0].unsqueeze(1) * t[:, 1].unsqueeze(0)).sum(-1) * SCALE * 1.4426950408889634          # [query][key][H], base 2
    excess = s2[:, 64:128].amax(1) - s2[:, :64].amax(1)
    assert float(excess[q].min()) > 8.0 + 32.0 and int(s2[q, :, 0].argmax()) == k
    v_spike = _hi(qkv16)[k, 2 * D:].double()
    assert float((out[q].double() - v_spike).abs().max()) <= 0.02 * float(qkv[:, 2 * D:].abs().max())


# ------------------------------------------------------------------------------------------ 3. bit identities
def _segs_run(dev, qkv16, segs, rows, H):
    """One segmented products = 1 launch: ([fp32 out per segment], planes)."""
    from dupl_amd import ops
    D = H * HD
    s16 = T._nan_split16(rows, D, dev)
    outs = [T._nan32(B * N, D, dev=dev) for (_, B, N) in segs]
    lses = ops.attention_fwd16_segs(qkv16, [(r0, B, N, outs[i], False, 0) for i, (r0, B, N) in enumerate(segs)], H, HD, SCALE,
                                    out16=s16, products=1)
    assert all(l is None for l in lses)
    return outs, s16


def test_h1_one_segment_equals_the_single_launch(dev):
    from dupl_amd import ops
    H, B, N = 12, 2, 197
    D = H * HD
    qkv16 = ops.split16(T._randn(B * N, 3 * D, 5, 1.5).to(dev))
    outs, s16 = _segs_run(dev, qkv16, [(0, B, N)], B * N, H)
    o, o16 = T._nan32(B * N, D, dev=dev), T._nan_split16(B * N, D, dev)
    ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out=o, out16=o16, products=1)
    assert torch.isfinite(o).all() and T._same_bits(outs[0], o) and T._same_bits(s16.planes, o16.planes)


def test_h1_rows_of_an_image_do_not_depend_on_B_or_the_layout(dev):
    """3 x 197 | 2 x 50 | 2 x 401 tokens (the longest last) as one segmented launch against ONE CALL PER IMAGE on rows_slices of the
    same planes: fp32 out and planes bit-identical."""
    from dupl_amd import ops
    H = 12
    D = H * HD
    segs = [(0, 3, 197), (591, 2, 50), (691, 2, 401)]
    rows = 1493
    qkv16 = ops.split16(T._randn(rows, 3 * D, 77, 1.5).to(dev))
    outs, s16 = _segs_run(dev, qkv16, segs, rows, H)
    r16 = T._nan_split16(rows, D, dev)
    for i, (r0, B, N) in enumerate(segs):
        for b in range(B):
            lo, hi = r0 + b * N, r0 + (b + 1) * N
            o = T._nan32(N, D, dev=dev)
            ops.attention_fwd16(qkv16.rows_slice(lo, hi), 1, N, H, HD, SCALE, out=o, out16=r16.rows_slice(lo, hi), products=1)
            assert torch.isfinite(o).all() and T._same_bits(outs[i][b * N:(b + 1) * N], o), f"segment {i} image {b}: fp32 out"
    assert torch.isfinite(s16.planes).all() and T._same_bits(s16.planes, r16.planes)


# ------------------------------------------------------------------------------------------ 4. containment and isolation
@pytest.mark.parametrize("N", M16.EDGE_N)
def test_h1_writes_nothing_outside_its_destinations(dev, N):
    """Guards bitwise unchanged, destinations fully written; B_f32 = 1 of 2 writes the fp32 out for the first image only and the
    planes for both.  qkv_lo is passed as NULL: the kernel does not read it."""
    from dupl_amd import ops
    B, H = 2, 12
    D = H * HD
    qkv16 = ops.split16(T._randn(B * N, 3 * D, 300 + N, 1.5).to(dev))
    ref_out = torch.empty(B * N, D, device=dev)
    ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out=ref_out, products=1)
    for bf in (B, 1):
        out = T._guarded_rows(bf * N, D, dev, f"fp32 out (B_f32 {bf})", behind=(B - bf) * N)
        big = T._nan_split16(B * N + 2 * T.GUARD_ROWS, D, dev)
        o16 = big.rows_slice(T.GUARD_ROWS, T.GUARD_ROWS + B * N)
        ops.L().dupl_attention_fwd16_prod(qkv16.hi, None, out.ptr(), o16.hi, o16.lo, None, B, N, H, HD, float(SCALE), bf, 0, 0, 1,
                                          ops._stream())
        out.check()
        T._check_planes(big, T.GUARD_ROWS, T.GUARD_ROWS + B * N, f"B_f32 {bf}")
        assert T._same_bits(out.view, ref_out[:bf * N])


@pytest.mark.parametrize("layout", ["step", "gaps"])
def test_h1_segs_writes_nothing_outside_its_destinations(dev, layout):
    from dupl_amd import ops, _lib
    H = 12
    D = H * HD
    segs, rows = T._layout_step(H) if layout == "step" else T._layout_gaps()
    qkv16 = ops.split16(T._randn(rows, 3 * D, 5, 1.5).to(dev))
    big = T._nan_split16(rows + 2 * T.GUARD_ROWS, D, dev)
    o16 = big.rows_slice(T.GUARD_ROWS, T.GUARD_ROWS + rows)
    arr = (_lib.AttnSeg * len(segs))()
    dests = []
    used = torch.zeros(rows, dtype=torch.bool)
    for i, (r0, B, N, want, _nl, b_f32) in enumerate(segs):
        bf = b_f32 or B
        out = T._guarded_rows(bf * N, D, dev, f"segment {i} fp32 out", behind=(B - bf) * N) if want else None
        if out is not None:
            dests.append(out)
        arr[i].row0, arr[i].B, arr[i].N, arr[i].B_f32 = r0, B, N, b_f32
        arr[i].out, arr[i].lse = (out.ptr() if out else None), None
        used[r0:r0 + B * N] = True
    ops.L().dupl_attention_fwd16_segs_prod(qkv16.hi, qkv16.lo, o16.hi, o16.lo, ctypes.cast(arr, ctypes.c_void_p), len(segs), H, HD,
                                           float(SCALE), 0, 0, 1, ops._stream())
    for d in dests:
        d.check()
    T._check_planes(big, T.GUARD_ROWS, T.GUARD_ROWS + rows, "segmented launch", used.to(dev))


@pytest.mark.parametrize("poison", ["nan", "decoy"])
@pytest.mark.parametrize("N", M16.EDGE_N)
def test_h1_reads_nothing_outside_its_own_image(dev, N, poison):
    """An image's out and planes are bit-identical whether the other image and the rows behind the slice hold the clean data, NaN,
    or decoys that would dominate the softmax."""
    from dupl_amd import ops
    B, H = 2, 12
    D = H * HD
    qkv = T._randn(B * N + min(T.TAIL, N), 3 * D, 500 + N, 1.5).to(dev)
    base = ops.split16(qkv)

    def run(p16):
        out = T._nan32(B * N, D, dev=dev)
        o16 = T._nan_split16(B * N, D, dev)
        ops.attention_fwd16(p16.rows_slice(0, B * N), B, N, H, HD, SCALE, out=out, out16=o16, products=1)
        return out, o16.planes

    out0, pl0 = run(base)
    assert torch.isfinite(out0).all() and torch.isfinite(pl0).all()
    for img in (0, 1):
        out, pl = run(T._poisoned_planes(ops, dev, base, qkv, B, N, D, img, poison))
        rs = slice(img * N, (img + 1) * N)
        assert T._same_bits(out[rs], out0[rs]), f"image {img}: fp32 out"
        assert T._same_bits(pl[:, rs], pl0[:, rs]), f"image {img}: planes"


# ------------------------------------------------------------------------------------------ 5. refusals
REFUSALS = ["fwd16-lse", "segs-lse", "fwd16-products0", "fwd16-products2", "fwd16-products4", "fwd16-products-1", "segs-products0",
            "segs-products2", "fwd16-hd32", "segs-hd32", "fwd16-mfma32", "fwd16-no-destination"]


@pytest.mark.parametrize("case", REFUSALS)
def test_h1_entry_points_refuse_bad_arguments_before_launching(dev, case):
    """Status -1 and the NaN-filled destinations keep their fill."""
    from dupl_amd import ops, _lib
    B, H, N = 1, 2, 33
    D = H * HD
    qkv16 = ops.split16(T._randn(B * N, 3 * D, 700, 1.0).to(dev))
    out, lse = T._nan32(B * N, D, dev=dev), T._nan32(B, H, N, dev=dev)
    o16 = T._nan_split16(B * N, D, dev)
    Lb = ops.L()

    def fwd16(out_p=out.data_ptr(), hi=o16.hi, lo=o16.lo, hd=HD, lse_p=None, mfma=0, products=1):
        Lb.dupl_attention_fwd16_prod(qkv16.hi, qkv16.lo, out_p, hi, lo, lse_p, B, N, H, hd, float(SCALE), 0, 0, mfma, products,
                                     ops._stream())

    def segs(hd=HD, lse_p=None, products=1):
        arr = (_lib.AttnSeg * 1)()
        arr[0].row0, arr[0].B, arr[0].N, arr[0].B_f32 = 0, B, N, 0
        arr[0].out, arr[0].lse = out.data_ptr(), lse_p
        Lb.dupl_attention_fwd16_segs_prod(qkv16.hi, qkv16.lo, o16.hi, o16.lo, ctypes.cast(arr, ctypes.c_void_p), 1, H, hd, float(SCALE),
                                          0, 0, products, ops._stream())

    call = {"fwd16-lse": lambda: fwd16(lse_p=lse.data_ptr()), "segs-lse": lambda: segs(lse_p=lse.data_ptr()),
            "fwd16-hd32": lambda: fwd16(hd=32), "segs-hd32": lambda: segs(hd=32), "fwd16-mfma32": lambda: fwd16(mfma=32),
            "fwd16-no-destination": lambda: fwd16(out_p=None, hi=None, lo=None)}
    for p in (0, 2, 4, -1):
        call[f"fwd16-products{p}"] = lambda p=p: fwd16(products=p)
        call[f"segs-products{p}"] = lambda p=p: segs(products=p)
    with pytest.raises(RuntimeError, match="status -1"):
        call[case]()
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("planes", o16.planes)):
        assert T._is_pattern(t), f"{case}: {name} was written"
