"""-m gpu: the split attention forward on v_mfma_f32_16x16x32_f16 (csrc/attn_split.hip attn_fwd16_m16_kernel, selected by
ops.ATTN16_TUNING["mfma"] = 16 or the `mfma` argument of dupl_attention_fwd16_mfma / dupl_attention_fwd16_segs_mfma).

  1  float64 bars of tests/test_attention_gpu.py (_fwd_bars, _planes_bar, both plane formats) at the shapes where THIS tiling goes
     wrong: one 16-query column tile and one over, the second column tile empty / partial, the key tile, the block, block totals
     that are no multiple of 8, one long case
  2  the lazy maximum decided on per-lane partial maxima: one spike that only ONE lane group of one column tile can see
  3  bit identities the step relies on: one segment = fwd16; an image's rows do not depend on B or on the segment layout
  4  containment and isolation (sections 4 and 5 of tests/test_attention_gpu.py) through the new entry points
  5  refusals: mfma outside {0, 16, 32}, and the existing refusals through the new entry points
  6  old against new: no systematic difference

Helpers and bars are imported from tests/test_attention_gpu.py, not copied.  Every output is pre-filled with its NaN patterns.

Mutation check (scratch build, not committed): with the ballot of the lazy maximum taken over `want && (lane >> 4) != 3` (lane
group 3 ignored) test_m16_spike_seen_by_one_lane_group[g3-ct1] fails (the probabilities overflow fp16: the output is NaN) while
[g0-ct0] passes."""
import contextlib
import ctypes

import pytest
import torch

import test_attention_gpu as T
from test_attention_gpu import HD, SCALE

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _mfma(v):
    from dupl_amd import ops
    old = ops.ATTN16_TUNING["mfma"]
    ops.ATTN16_TUNING["mfma"] = v
    try:
        yield
    finally:
        ops.ATTN16_TUNING["mfma"] = old


# ------------------------------------------------------------------------------------------ 1. forward shape sweep
FWD_CASES = [(2, 1, 12), (2, 15, 12), (2, 16, 12), (2, 17, 12),                                      # one 16-query tile and one over
             (2, 31, 12), (2, 32, 12), (2, 33, 12), (2, 47, 12), (2, 48, 12), (2, 49, 12),          # second column tile
             (1, 63, 12), (1, 64, 12), (1, 65, 12),                                                  # key tile
             (2, 127, 12), (2, 128, 12), (1, 129, 12),                                               # block
             (3, 197, 5), (1, 785, 7),                                                               # 30, 49 blocks
             (2, 1765, 12)]                                                                          # long (from the existing sweep)


@pytest.mark.parametrize("B,N,H", FWD_CASES, ids=[f"B{b}-N{n}-H{h}" for b, n, h in FWD_CASES])
def test_m16_shape_sweep(dev, B, N, H):
    qkv = T._randn(B * N, 3 * H * HD, B * 1000 + N + 7 * H, 1.5).to(dev)
    ref, ref_lse, _ = T.ref64(qkv, B, N, H, HD, SCALE)
    with _mfma(16):
        T._fwd_compare(dev, f"m16 fwd B{B} N{N} H{H}", qkv, B, N, H, ref, ref_lse)


# ------------------------------------------------------------------------------------------ 2. the lazy maximum on partial maxima
# (query, key): query 19 = column tile 1, c = 3; key 90 = tile 1, 32-key group 0, lane group 3 (keys 24 .. 31 of the group).
#               query 3 = column tile 0; key 65 = tile 1, lane group 0
SPIKES = {"g3-ct1": (19, 90), "g0-ct0": (3, 65)}


@pytest.mark.parametrize("which", list(SPIKES))
def test_m16_spike_seen_by_one_lane_group(dev, which):
    """N = 130 (three key tiles).  One query's largest score sits in ONE key of the second tile: k = 6 q (as
    test_fwd16_spike_on_the_last_key_of_a_partial_tile), 6 |q|^2 scale log2(e) ~ 69 above the running maximum in the base-2 domain,
    the threshold is 8.  Every other query is scaled by 0.1, so its score on that key (and on every other key) stays within ~3 of
    its running maximum: the move of the running maximum in tile 1 is triggered by the partial maximum of exactly one lane -- the
    spiked query's lane of the group that holds the key.  A ballot that missed that lane group would leave P = 2^66 (fp16 overflow).
    How that was checked: module docstring."""
    B, H, N = 1, 12, 130
    D = H * HD
    q, k = SPIKES[which]
    qkv = T._randn(B * N, 3 * D, 31, 1.0)
    keep = qkv[q, 0:D].clone()
    qkv[:, 0:D] *= 0.1
    qkv[q, 0:D] = keep
    qkv[k, D:2 * D] = 6.0 * keep
    qkv = qkv.to(dev)
    ref, ref_lse, _ = T.ref64(qkv, B, N, H, HD, SCALE)
    t = qkv.double().view(N, 3, H, HD)
    s2 = (t[:, 0].unsqueeze(1) * t[:, 1].unsqueeze(0)).sum(-1) * SCALE * 1.4426950408889634          # [query][key][H], base 2
    first = s2[:, :64].amax(1)                                                                          # running maximum after tile 0
    excess = s2[:, 64:128].amax(1) - first
    assert float(excess[q].min()) > 8.0 + 32.0
    others = torch.ones(N, dtype=torch.bool, device=dev)
    others[q] = False
    assert float(excess[others].max()) < 8.0 and float((s2[:, 128:].amax(1) - s2[:, :128].amax(1))[others].max()) < 8.0
    assert int(s2[q, :, 0].argmax()) == k
    with _mfma(16):
        out, _ = T._fwd_compare(dev, f"m16 spike {which}", qkv, B, N, H, ref, ref_lse)
    v_spike = qkv[k, 2 * D:].double()
    assert float((out[q].double() - v_spike).abs().max()) <= 0.02 * float(qkv[:, 2 * D:].abs().max())


# ------------------------------------------------------------------------------------------ 3. bit identities
def test_m16_one_segment_equals_fwd16(dev):
    with _mfma(16):
        T._segs_vs_batches(dev, 12, [(0, 2, 197, True, True, 0)], 394)
        T._segs_vs_batches(dev, 12, [(0, 2, 197, True, True, 1)], 394)


def test_m16_rows_of_an_image_do_not_depend_on_B_or_the_layout(dev):
    """The step layout in miniature (3 x 197 | 2 x 50 | 2 x 401 tokens, the longest last, fp32 out + lse for every image) as one
    segmented launch against ONE CALL PER IMAGE on rows_slices of the same planes: fp32 out, lse and planes bit-identical."""
    from dupl_amd import ops
    H = 12
    D = H * HD
    segs = [(0, 3, 197), (591, 2, 50), (691, 2, 401)]
    rows = 1493
    qkv16 = ops.split16(T._randn(rows, 3 * D, 77, 1.5).to(dev))
    with _mfma(16):
        s16 = T._nan_split16(rows, D, dev)
        outs = [T._nan32(B * N, D, dev=dev) for (_, B, N) in segs]
        lses = ops.attention_fwd16_segs(qkv16, [(r0, B, N, outs[i], True, 0) for i, (r0, B, N) in enumerate(segs)], H, HD, SCALE, out16=s16)
        r16 = T._nan_split16(rows, D, dev)
        for i, (r0, B, N) in enumerate(segs):
            for b in range(B):
                lo, hi = r0 + b * N, r0 + (b + 1) * N
                o = T._nan32(N, D, dev=dev)
                lse = ops.attention_fwd16(qkv16.rows_slice(lo, hi), 1, N, H, HD, SCALE, need_lse=True, out=o, out16=r16.rows_slice(lo, hi))
                assert torch.isfinite(o).all() and T._same_bits(outs[i][b * N:(b + 1) * N], o), f"segment {i} image {b}: fp32 out"
                assert T._same_bits(lses[i][b], lse[0]), f"segment {i} image {b}: lse"
    assert torch.isfinite(s16.planes).all() and T._same_bits(s16.planes, r16.planes)


# ------------------------------------------------------------------------------------------ 4. containment and isolation
EDGE_N = [17, 33, 65, 130, 197]


@pytest.mark.parametrize("N", EDGE_N)
def test_m16_writes_nothing_outside_its_destinations(dev, N):
    """test_fwd16_writes_nothing_outside_its_destinations through dupl_attention_fwd16_mfma(.., 16): guards bitwise unchanged,
    destinations fully written; B_f32 = 1 of 2 writes fp32 out / lse for the first image only and the planes for both."""
    from dupl_amd import ops
    B, H = 2, 12
    D = H * HD
    qkv16 = ops.split16(T._randn(B * N, 3 * D, 300 + N, 1.5).to(dev))
    ref_out = torch.empty(B * N, D, device=dev)
    with _mfma(16):
        ref_lse = ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, need_lse=True, out=ref_out)
    for bf in (B, 1):
        out = T._guarded_rows(bf * N, D, dev, f"fp32 out (B_f32 {bf})", behind=(B - bf) * N)
        lse = T._guarded_flat(bf * H * N, N, dev, f"lse (B_f32 {bf})", behind=(B - bf) * H * N)
        big = T._nan_split16(B * N + 2 * T.GUARD_ROWS, D, dev)
        o16 = big.rows_slice(T.GUARD_ROWS, T.GUARD_ROWS + B * N)
        ops.L().dupl_attention_fwd16_mfma(qkv16.hi, qkv16.lo, out.ptr(), o16.hi, o16.lo, lse.ptr(), B, N, H, HD, float(SCALE), bf, 0,
                                          16, ops._stream())
        out.check()
        lse.check()
        T._check_planes(big, T.GUARD_ROWS, T.GUARD_ROWS + B * N, f"B_f32 {bf}")
        assert T._same_bits(out.view, ref_out[:bf * N]) and T._same_bits(lse.view, ref_lse[:bf].reshape(-1))


@pytest.mark.parametrize("layout", ["step", "gaps"])
def test_m16_segs_writes_nothing_outside_its_destinations(dev, layout):
    """test_fwd16_segs_writes_nothing_outside_its_destinations (its layouts) through dupl_attention_fwd16_segs_mfma(.., 16)."""
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
    for i, (r0, B, N, want, nl, b_f32) in enumerate(segs):
        bf = b_f32 or B
        out = T._guarded_rows(bf * N, D, dev, f"segment {i} fp32 out", behind=(B - bf) * N) if want else None
        lse = T._guarded_flat(bf * H * N, N, dev, f"segment {i} lse", behind=(B - bf) * H * N) if nl else None
        dests += [d for d in (out, lse) if d is not None]
        arr[i].row0, arr[i].B, arr[i].N, arr[i].B_f32 = r0, B, N, b_f32
        arr[i].out, arr[i].lse = (out.ptr() if out else None), (lse.ptr() if lse else None)
        used[r0:r0 + B * N] = True
    ops.L().dupl_attention_fwd16_segs_mfma(qkv16.hi, qkv16.lo, o16.hi, o16.lo, ctypes.cast(arr, ctypes.c_void_p), len(segs), H, HD,
                                           float(SCALE), 0, 16, ops._stream())
    for d in dests:
        d.check()
    T._check_planes(big, T.GUARD_ROWS, T.GUARD_ROWS + rows, "segmented launch", used.to(dev))


@pytest.mark.parametrize("poison", ["nan", "decoy"])
@pytest.mark.parametrize("N", EDGE_N)
def test_m16_reads_nothing_outside_its_own_image(dev, N, poison):
    """test_fwd16_reads_nothing_outside_its_own_image with the new kernel: an image's out, lse and planes are bit-identical whether
    the other image and the rows behind the slice hold the clean data, NaN, or decoys that would dominate the softmax.  (The rows
    behind the slice are min(TAIL, N): _poisoned_planes fills them from one image's decoys.)"""
    from dupl_amd import ops
    B, H = 2, 12
    D = H * HD
    qkv = T._randn(B * N + min(T.TAIL, N), 3 * D, 500 + N, 1.5).to(dev)
    base = ops.split16(qkv)

    def run(p16):
        out = T._nan32(B * N, D, dev=dev)
        o16 = T._nan_split16(B * N, D, dev)
        lse = ops.attention_fwd16(p16.rows_slice(0, B * N), B, N, H, HD, SCALE, need_lse=True, out=out, out16=o16)
        return out, lse, o16.planes

    with _mfma(16):
        out0, lse0, pl0 = run(base)
        assert torch.isfinite(out0).all() and torch.isfinite(lse0).all() and torch.isfinite(pl0).all()
        for img in (0, 1):
            out, lse, pl = run(T._poisoned_planes(ops, dev, base, qkv, B, N, D, img, poison))
            rs = slice(img * N, (img + 1) * N)
            assert T._same_bits(out[rs], out0[rs]), f"image {img}: fp32 out"
            assert T._same_bits(lse[img], lse0[img]), f"image {img}: lse"
            assert T._same_bits(pl[:, rs], pl0[:, rs]), f"image {img}: planes"


# ------------------------------------------------------------------------------------------ 5. refusals
BAD_MFMA = [1, 8, 15, 17, 31, 33, 64, -16]
REFUSALS = [f"fwd16-mfma{m}" for m in BAD_MFMA] + [f"segs-mfma{m}" for m in BAD_MFMA] + [
    "segs-n0", "segs-n5", "fwd16-hd32", "segs-hd32", "fwd16-B_f32-above-B", "segs-B_f32-above-B", "fwd16-no-destination",
    "segs-no-destination", "segs-row0-negative", "fwd16-hi-without-lo", "segs-hi-without-lo", "fwd16-N0", "segs-N0"]


@pytest.mark.parametrize("case", REFUSALS)
def test_m16_entry_points_refuse_bad_arguments_before_launching(dev, case):
    """mfma outside {0, 16, 32} and the forward cases of test_launchers_refuse_bad_arguments_before_launching (with mfma = 16)
    through dupl_attention_fwd16_mfma / dupl_attention_fwd16_segs_mfma: status -1 and the NaN-filled destinations keep their fill."""
    from dupl_amd import ops, _lib
    B, H, N = 1, 2, 33
    D = H * HD
    qkv16 = ops.split16(T._randn(B * N, 3 * D, 700, 1.0).to(dev))
    out, lse = T._nan32(B * N, D, dev=dev), T._nan32(B, H, N, dev=dev)
    o16 = T._nan_split16(B * N, D, dev)
    Lb = ops.L()

    def fwd16(out_p=out.data_ptr(), hi=o16.hi, lo=o16.lo, B_=B, N_=N, hd=HD, bf=0, mfma=16):
        Lb.dupl_attention_fwd16_mfma(qkv16.hi, qkv16.lo, out_p, hi, lo, lse.data_ptr(), B_, N_, H, hd, float(SCALE), bf, 0, mfma,
                                     ops._stream())

    def segs(n=1, count=1, row0=0, B_=B, N_=N, bf=0, out_p=out.data_ptr(), hi=o16.hi, lo=o16.lo, hd=HD, mfma=16):
        arr = (_lib.AttnSeg * max(count, 1))()
        for i in range(max(count, 1)):
            arr[i].row0, arr[i].B, arr[i].N, arr[i].B_f32 = row0, B_, N_, bf
            arr[i].out, arr[i].lse = out_p, lse.data_ptr()
        Lb.dupl_attention_fwd16_segs_mfma(qkv16.hi, qkv16.lo, hi, lo, ctypes.cast(arr, ctypes.c_void_p), n, H, hd, float(SCALE), 0,
                                          mfma, ops._stream())

    call = {"segs-n0": lambda: segs(n=0), "segs-n5": lambda: segs(n=5, count=5),
            "fwd16-hd32": lambda: fwd16(hd=32), "segs-hd32": lambda: segs(hd=32),
            "fwd16-B_f32-above-B": lambda: fwd16(bf=B + 1), "segs-B_f32-above-B": lambda: segs(bf=B + 1),
            "fwd16-no-destination": lambda: fwd16(out_p=None, hi=None, lo=None),
            "segs-no-destination": lambda: segs(out_p=None, hi=None, lo=None),
            "segs-row0-negative": lambda: segs(row0=-1),
            "fwd16-hi-without-lo": lambda: fwd16(lo=None), "segs-hi-without-lo": lambda: segs(lo=None),
            "fwd16-N0": lambda: fwd16(N_=0), "segs-N0": lambda: segs(N_=0)}
    for m in BAD_MFMA:
        call[f"fwd16-mfma{m}"] = lambda m=m: fwd16(mfma=m)
        call[f"segs-mfma{m}"] = lambda m=m: segs(mfma=m)
    with pytest.raises(RuntimeError, match="status -1"):
        call[case]()
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("planes", o16.planes)):
        assert T._is_pattern(t), f"{case}: {name} was written"


# ------------------------------------------------------------------------------------------ 6. old against new
@pytest.mark.parametrize("N", [197, 785])
def test_m16_against_the_32x32x16_kernel(dev, N):
    """|out16 - out32| (and lse) inside the sum of both kernels' float64 errors: no new bar, a guard against a systematic
    difference.  Bit equality is not expected (the accumulation order differs)."""
    from dupl_amd import ops
    B, H = 2, 12
    D = H * HD
    qkv = T._randn(B * N, 3 * D, 900 + N, 1.5).to(dev)
    ref, ref_lse, _ = T.ref64(qkv, B, N, H, HD, SCALE)
    qkv16 = ops.split16(qkv)
    res = {}
    for m in (32, 16):
        out = T._nan32(B * N, D, dev=dev)
        with _mfma(m):
            lse = ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, need_lse=True, out=out)
        assert torch.isfinite(out).all() and torch.isfinite(lse).all()
        res[m] = (out, lse, float((out.double() - ref).abs().max()), float((lse.double() - ref_lse).abs().max()))
    d_out = float((res[16][0] - res[32][0]).abs().max())
    d_lse = float((res[16][1] - res[32][1]).abs().max())
    print(f"m16 vs m32 N{N}: |out16 - out32| {d_out:.2e} (errors vs float64 {res[16][2]:.2e} + {res[32][2]:.2e}); "
          f"|lse16 - lse32| {d_lse:.2e} ({res[16][3]:.2e} + {res[32][3]:.2e})")
    assert d_out <= res[16][2] + res[32][2]
    assert d_lse <= res[16][3] + res[32][3]
