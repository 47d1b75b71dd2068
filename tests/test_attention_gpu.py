"""-m gpu: the split attention kernels (csrc/attn_split.hip, csrc/attn_split_bwd.hip) and the exact-f32 attention kernels
(csrc/attn.hip) at their edges, through dupl_amd.ops / the C ABI.

  1  forward shape sweep against float64: one key, around one 64-key tile / one 32-query wave, exact multiples of the
     128-query block and one row over, the lengths a training step runs (1 765, 2 117), head counts whose block totals are not
     multiples of 8; two analytic cases (q = 0; all the mass on the last key of a partial tile)
  2  backward shape sweep against float64 autograd up to the 2 048-token limit, dout of very different magnitudes
  3  dupl_attention_fwd16_segs: bit identity with one dupl_attention_fwd16 per batch, and float64 directly
  4  containment: guard rows / entries around every destination stay bitwise unchanged, the destination is fully written
  5  isolation: the rows of the neighbouring image (NaN, or finite decoys) never reach an image's results
  6  refusals: bad arguments are rejected by the launchers before anything is launched
  7  the exact-f32 kernels (yardstick of every f16x3 bar, product path of the backward beyond 2 048 tokens) at those lengths

Bars are the project's standing ones (test_attention_fwd16_is_fp32_equivalent, test_attention_bwd16_is_fp32_equivalent,
test_attention_fwd_bwd); every test prints its measured errors next to the exact-f32 kernel's before it asserts.  The exact-f32
kernel's own error is first held to ITS standing bars (out 5e-6, lse 5e-6, dqkv 2e-5 of the reference's maximum) on the same
input, so a bar of the form "2 x the exact-f32 kernel's error" cannot widen unnoticed; the f32 kernels' own edges:
tests/test_attention_f32_gpu.py.

Cost on one MI355X, measured in one session: this module alone 4.4 s (92 tests; the slowest single test 0.9 s, the float64
references run on the device); the whole -m gpu suite 639 s without it (325 tests) and 617 s with it (417 tests) -- the
module is below the run-to-run spread of the suite.

Mutation check (scratch builds, not committed): with `if (b >= B_f32)` of attn_split.hip disabled, the containment tests of
section 4 fail at (2, 33), (2, 197) and on the step layout ("the guard behind the destination changed"); with the partial-tile
clamp min(.., N - 1) turned into min(.., N), the NaN cases of section 5 fail at N = 65, 130 and 197."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 64
SCALE = HD ** -0.5
NAN32, NAN16 = 0x7FC00000, 0x7E00          # the guard patterns (quiet NaNs), written and compared as integers


# ------------------------------------------------------------------------------------------ helpers
def ref64(qkv, B, N, H, hd, scale, dout=None):
    """The plain formula in float64 from the fp32 qkv, on qkv's device: softmax(q k^T scale) v, logsumexp, and (with dout) the
    autograd gradient with respect to qkv."""
    x = qkv.double().clone().requires_grad_(dout is not None)
    q, k, v = (x.view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)[i] for i in range(3))
    att = (q @ k.transpose(-1, -2)) * scale
    out = (att.softmax(-1) @ v).transpose(1, 2).reshape(B * N, H * hd)
    lse = torch.logsumexp(att, dim=-1)
    grad = None
    if dout is not None:
        out.backward(dout.double())
        grad = x.grad
    return out.detach(), lse.detach(), grad


def _randn(rows, cols, seed, std):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g) * std


def _nan32(*shape, dev):
    return torch.full(shape, NAN32, dtype=torch.int32, device=dev).view(torch.float32)


def _nan_split16(rows, cols, dev, exp=0):
    from dupl_amd import ops
    return ops.Split16(torch.full((2, rows, cols), NAN16, dtype=torch.int16, device=dev).view(torch.float16), exp)


def _recon(planes, exp):
    """fp32 value of hi / lo planes [2, rows, cols]: format 0 (exp 0) hi + lo / 2048, format 1 (hi + lo) / 2^exp."""
    if exp == 0:
        return planes[0].float() + planes[1].float() / 2048.0
    return (planes[0].float() + planes[1].float()) / float(2 ** exp)


def _same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _is_pattern(t):
    if t.numel() == 0:
        return True
    it, pat = {2: (torch.int16, NAN16), 4: (torch.int32, NAN32)}[t.element_size()]
    return bool((t.contiguous().view(it) == pat).all())


def _fwd_bars(tag, out, lse, o32, lse32, ref, ref_lse):
    """Output error relative to max |ref| <= 2 x the exact-f32 kernel's + 2e-7; lse absolute error <= 2 x the f32 kernel's + 1e-6."""
    sc = float(ref.abs().max())
    e16, e32 = float((out.double() - ref).abs().max()) / sc, float((o32.double() - ref).abs().max()) / sc
    l16, l32 = float((lse.double() - ref_lse).abs().max()), float((lse32.double() - ref_lse).abs().max())
    print(f"{tag}: out f16x3 {e16:.2e} f32 {e32:.2e} (bar {2.0 * e32 + 2e-7:.2e}); lse f16x3 {l16:.2e} f32 {l32:.2e} "
          f"(bar {2.0 * l32 + 1e-6:.2e})")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    # the yardstick itself first: the exact-f32 kernel meets its own standing bars (test_attention_fwd_bwd) on this input
    assert e32 < 5e-6 and l32 < 5e-6 * float(ref_lse.abs().max()), f"{tag}: the exact-f32 kernel misses its own bar"
    assert e16 <= 2.0 * e32 + 2e-7, tag
    assert l16 <= 2.0 * l32 + 1e-6, tag
    return sc


def _planes_bar(tag, out, o16):
    """The planes reconstruct the fp32 output to 2^-21 of its maximum."""
    sc = float(out.abs().max())
    e = float((_recon(o16.planes, o16.exp) - out).abs().max())
    print(f"{tag}: planes (format {int(o16.exp > 0)}) vs fp32 out {e / sc:.2e} of the maximum (bar {2.0 ** -21:.2e})")
    assert e <= 2.0 ** -21 * sc, tag


def _fwd_compare(dev, tag, qkv, B, N, H, ref, ref_lse):
    """fwd16 (fp32 out + lse + format 0 planes, then format 1 planes) on qkv against a float64 reference, bars of section 1."""
    from dupl_amd import ops
    D = H * HD
    o32, lse32 = ops.attention_fwd(qkv, B, N, H, HD, SCALE, need_lse=True)
    qkv16 = ops.split16(qkv)
    out = _nan32(B * N, D, dev=dev)
    o0 = _nan_split16(B * N, D, dev)
    lse = ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, need_lse=True, out=out, out16=o0)
    _fwd_bars(tag, out, lse, o32, lse32, ref, ref_lse)
    _planes_bar(tag, out, o0)
    o1 = _nan_split16(B * N, D, dev, ops.EXP_ACT)
    ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out16=o1)
    _planes_bar(tag, out, o1)
    return out, lse


# ------------------------------------------------------------------------------------------ 1. forward shape sweep
FWD_CASES = [(1, 1, 12), (3, 1, 5),                                                                   # one key, one query
             (2, 31, 12), (2, 33, 12), (1, 63, 12), (1, 65, 12),                                      # one key tile / one wave
             (2, 127, 12), (2, 128, 12), (1, 129, 12), (1, 192, 12), (1, 256, 12), (1, 257, 12),      # query blocks
             (1, 1024, 12), (2, 1765, 12), (1, 2048, 12), (1, 2117, 12),                              # long
             (1, 197, 1), (3, 197, 5), (1, 785, 7)]                                                   # 2, 30, 49 blocks


@pytest.mark.parametrize("B,N,H", FWD_CASES, ids=[f"B{b}-N{n}-H{h}" for b, n, h in FWD_CASES])
def test_fwd16_shape_sweep(dev, B, N, H):
    """dupl_attention_fwd16 against float64 at the shapes where a tiled kernel goes wrong."""
    qkv = _randn(B * N, 3 * H * HD, B * 1000 + N + 7 * H, 1.5).to(dev)
    ref, ref_lse, _ = ref64(qkv, B, N, H, HD, SCALE)
    _fwd_compare(dev, f"fwd B{B} N{N} H{H}", qkv, B, N, H, ref, ref_lse)


@pytest.mark.parametrize("N", [65, 785])
def test_fwd16_zero_queries_give_the_column_mean(dev, N):
    """q = 0: every score is 0, every probability 1 / N -- out is the column mean of v per head and lse = log N.  The reference
    is that mean in float64 (no softmax involved); bars of the shape sweep (the exact-f32 kernel on the same input sets the
    scale of what fp32 accumulation over N terms costs)."""
    B, H = 2, 12
    D = H * HD
    qkv = _randn(B * N, 3 * D, 40 + N, 1.5)
    qkv[:, :D] = 0.0
    qkv = qkv.to(dev)
    ref = qkv[:, 2 * D:].double().view(B, N, D).mean(1, keepdim=True).expand(B, N, D).reshape(B * N, D)
    ref_lse = torch.full((B, H, N), math.log(N), dtype=torch.float64, device=dev)
    _fwd_compare(dev, f"q=0 N{N}", qkv, B, N, H, ref, ref_lse)


@pytest.mark.parametrize("N", [65, 129])
def test_fwd16_spike_on_the_last_key_of_a_partial_tile(dev, N):
    """The mass sits in the partial tile: the LAST key (64 of 65, 128 of 129: the only key of its tile) is 6 x query 3 in
    every head, so query 3 puts > 0.99 of its probability there.  A mask or clamp that is off by one loses exactly this key."""
    B, H = 1, 12
    D = H * HD
    qkv = _randn(B * N, 3 * D, 21, 1.0)
    qkv[N - 1, D:2 * D] = 6.0 * qkv[3, 0:D]
    qkv = qkv.to(dev)
    ref, ref_lse, _ = ref64(qkv, B, N, H, HD, SCALE)
    t = qkv.double().view(N, 3, H, HD)
    p_last = ((t[3, 0] * t[:, 1]).sum(-1) * SCALE).softmax(0)[N - 1]          # [H]: query 3's probability of the last key
    assert float(p_last.min()) > 0.99
    out, _ = _fwd_compare(dev, f"spike N{N}", qkv, B, N, H, ref, ref_lse)
    # and in plain words: query 3's output is (almost) the last value row
    v_last = qkv[N - 1, 2 * D:].double()
    assert float((out[3].double() - v_last).abs().max()) <= 0.02 * float(qkv[:, 2 * D:].abs().max())


# ------------------------------------------------------------------------------------------ 2. backward shape sweep
def _bwd_compare(dev, tag, B, N, H, qkv, dout):
    """bwd16 against float64 autograd: each of dq / dk / dv relative to its own maximum <= 2 x the exact-f32 kernels' + 5e-7.
    Where the reference slice is exactly zero (dq, dk at N = 1) the errors are taken against the dv scale instead."""
    from dupl_amd import ops
    D = H * HD
    _, _, ref = ref64(qkv, B, N, H, HD, SCALE, dout)
    out32, lse32 = ops.attention_fwd(qkv, B, N, H, HD, SCALE, need_lse=True)
    d32 = ops.attention_bwd(qkv, out32, dout, lse32, B, N, H, HD, SCALE)
    qkv16 = ops.split16(qkv)
    out16 = _nan32(B * N, D, dev=dev)
    lse16 = ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, need_lse=True, out=out16)
    d16 = ops.attention_bwd16(qkv16, out16, dout, lse16, B, N, H, HD, SCALE)
    assert torch.isfinite(d16).all()
    # the yardstick itself first: the exact-f32 backward meets its own standing bar (test_attention_fwd_bwd) on this input
    g32 = float((d32.double() - ref).abs().max() / ref.abs().max())
    print(f"{tag}: exact-f32 dqkv {g32:.2e} of the reference's maximum (bar 2e-05)")
    assert g32 < 2e-5, f"{tag}: the exact-f32 kernels miss their own bar"
    sc_dv = float(ref[:, 2 * D:].abs().max())
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        sc = float(ref[:, sl].abs().max())
        if sc == 0.0:
            assert N == 1 and name != "dv"
            sc = sc_dv
        e16 = float((d16[:, sl].double() - ref[:, sl]).abs().max()) / sc
        e32 = float((d32[:, sl].double() - ref[:, sl]).abs().max()) / sc
        print(f"{tag} {name}: f16x3 {e16:.2e} f32 {e32:.2e} (bar {2.0 * e32 + 5e-7:.2e})")
        assert e16 <= 2.0 * e32 + 5e-7, f"{tag} {name}"
    return d16


BWD_CASES = [(1, 1, 12), (2, 32, 12), (2, 33, 12), (1, 65, 12), (2, 127, 12), (2, 128, 12), (1, 129, 12), (1, 256, 12),
             (1, 1024, 12), (1, 1765, 12), (1, 2047, 12), (1, 2048, 12), (3, 197, 5), (1, 785, 7)]


@pytest.mark.parametrize("B,N,H", BWD_CASES, ids=[f"B{b}-N{n}-H{h}" for b, n, h in BWD_CASES])
def test_bwd16_shape_sweep(dev, B, N, H):
    """dupl_attention_bwd16 against float64 autograd, gradient magnitudes of a real step (2e-5), up to the 2 048-token limit
    (lse / delta of a head live in LDS up to exactly that)."""
    g = torch.Generator().manual_seed(B * 100 + N + 7 * H)
    qkv = (torch.randn(B * N, 3 * H * HD, generator=g) * 1.2).to(dev)
    dout = (torch.randn(B * N, H * HD, generator=g) * 2e-5).to(dev)
    _bwd_compare(dev, f"bwd B{B} N{N} H{H}", B, N, H, qkv, dout)


@pytest.mark.parametrize("kind", ["times-1e-8", "std-1e-8", "std-1", "one-row-1e4"])
def test_bwd16_dout_magnitudes(dev, kind):
    """The dO planes are scaled by a power of two taken from max |dout|: the bar must hold for gradients of 2e-13, 1e-8 and 1
    in size, and when one row of dout is 1e4 times larger than the rest (the scale then follows that row, and the other rows
    sit 13 bits lower in their planes)."""
    B, N, H = 2, 197, 12
    g = torch.Generator().manual_seed(B * 100 + N)
    qkv = (torch.randn(B * N, 3 * H * HD, generator=g) * 1.2).to(dev)
    dout = torch.randn(B * N, H * HD, generator=g)
    if kind == "times-1e-8":
        dout = dout * 2e-5 * 1e-8
    elif kind == "std-1e-8":
        dout = dout * 1e-8
    elif kind == "one-row-1e4":
        dout = dout * 2e-5
        dout[N + 17] *= 1e4
    _bwd_compare(dev, f"bwd dout {kind}", B, N, H, qkv, dout.to(dev))


# ------------------------------------------------------------------------------------------ 3. the segmented launch
# token rows in buffer order; a segment = (row0, B, N, fp32 out wanted, lse wanted, b_f32)
def _layout_step(H):
    """The real step in miniature: [2 x 785: fp32 out + lse for the first image only | 2 x 197 planes | 2 x 1765 planes].  The
    longest batch is last in the buffer (the reordering is live), every segment has more than one query block; the block counts
    are 14 H, 4 H and 28 H: multiples of 8 at H = 12, none at H = 5 (the remainder branch of the per-segment XCD remap)."""
    return [(0, 2, 785, True, True, 1), (1570, 2, 197, False, False, 0), (1964, 2, 1765, False, False, 0)], 5494


def _layout_ties():
    """Four segments (the maximum), two of equal length (ties keep the caller's order), all with fp32 out and lse."""
    return [(0, 1, 130, True, True, 0), (130, 2, 64, True, True, 0), (258, 1, 130, True, True, 0), (388, 3, 50, True, True, 0)], 538


def _layout_gaps():
    """Segments passed in an order that is not their row order, 64 unused rows between them and at both ends of the buffer:
    rows 64 | 1 x 129 | 64 | 2 x 33 | 64 | 1 x 200 | 64."""
    return [(257, 2, 33, True, True, 0), (387, 1, 200, True, True, 1), (64, 1, 129, True, True, 0)], 651


def _segs_vs_batches(dev, H, segs, rows, exp=0, planes=True, seed=5):
    """ops.attention_fwd16_segs on one buffer against one ops.attention_fwd16 per batch on rows_slices of the same planes:
    planes (all rows of the buffer, untouched ones included), fp32 outputs and lse must be bit-identical."""
    from dupl_amd import ops
    D = H * HD
    qkv = _randn(rows, 3 * D, seed, 1.5).to(dev)
    qkv16 = ops.split16(qkv)
    s16 = _nan_split16(rows, D, dev, exp) if planes else None
    r16 = _nan_split16(rows, D, dev, exp) if planes else None
    outs = [_nan32((bf or B) * N, D, dev=dev) if want else None for (_, B, N, want, _, bf) in segs]
    lses = ops.attention_fwd16_segs(qkv16, [(r0, B, N, outs[i], nl, bf) for i, (r0, B, N, _, nl, bf) in enumerate(segs)],
                                    H, HD, SCALE, out16=s16)
    for i, (r0, B, N, want, nl, bf) in enumerate(segs):
        o = _nan32((bf or B) * N, D, dev=dev) if want else None
        lse = ops.attention_fwd16(qkv16.rows_slice(r0, r0 + B * N), B, N, H, HD, SCALE, need_lse=nl, out=o,
                                  out16=r16.rows_slice(r0, r0 + B * N) if planes else None, b_f32=bf)
        if want:
            assert torch.isfinite(o).all() and _same_bits(outs[i], o), f"segment {i}: fp32 out"
        if nl:
            assert lses[i].shape == ((bf or B), H, N) and torch.isfinite(lse).all() and _same_bits(lses[i], lse), f"segment {i}: lse"
        else:
            assert lses[i] is None
        if planes:
            assert torch.isfinite(s16.planes[:, r0:r0 + B * N]).all(), f"segment {i}: planes"
    if planes:
        assert _same_bits(s16.planes, r16.planes)
    return qkv, outs, lses, s16


@pytest.mark.parametrize("H", [12, 5])
def test_fwd16_segs_step_layout(dev, H):
    """Layout 1 at H = 12 and H = 5: bit identity with the per-batch launches, and the segmented results against float64
    directly -- the fp32 out / lse of the one image that has them with the bars of the shape sweep, the planes of every
    segment reconstructed (their own bar, 2^-21 of the maximum, added to the output bar)."""
    from dupl_amd import ops
    segs, rows = _layout_step(H)
    qkv, outs, lses, s16 = _segs_vs_batches(dev, H, segs, rows)
    D = H * HD
    for i, (r0, B, N, want, nl, bf) in enumerate(segs):
        x = qkv[r0:r0 + B * N].contiguous()
        ref, ref_lse, _ = ref64(x, B, N, H, HD, SCALE)
        o32, lse32 = ops.attention_fwd(x, B, N, H, HD, SCALE, need_lse=True)
        sc = float(ref.abs().max())
        e32 = float((o32.double() - ref).abs().max()) / sc
        ep = float((_recon(s16.planes[:, r0:r0 + B * N], 0).double() - ref).abs().max()) / sc
        print(f"segs H{H} segment {i} ({B} x {N}): planes vs float64 {ep:.2e}, f32 kernel {e32:.2e} (bar {2.0 * e32 + 2e-7 + 2.0 ** -21:.2e})")
        assert ep <= 2.0 * e32 + 2e-7 + 2.0 ** -21
        if want:
            k = (bf or B) * N
            _fwd_bars(f"segs H{H} segment {i} fp32", outs[i], lses[i], o32[:k], lse32[:bf or B], ref[:k], ref_lse[:bf or B])
        del ref, ref_lse, o32, lse32


def test_fwd16_segs_ties_and_the_maximum_count(dev):
    segs, rows = _layout_ties()
    _segs_vs_batches(dev, 12, segs, rows)


def test_fwd16_segs_one_segment_equals_fwd16(dev):
    _segs_vs_batches(dev, 12, [(0, 2, 197, True, True, 0)], 394)
    _segs_vs_batches(dev, 12, [(0, 2, 197, True, True, 1)], 394)


def test_fwd16_segs_caller_order_and_unused_rows(dev):
    """Layout 4: the unused rows of the output planes keep their fill (the comparison covers every row of the buffer)."""
    segs, rows = _layout_gaps()
    _, _, _, s16 = _segs_vs_batches(dev, 12, segs, rows)
    used = torch.zeros(rows, dtype=torch.bool)
    for (r0, B, N, _, _, _) in segs:
        used[r0:r0 + B * N] = True
    assert int((~used).sum()) == 4 * 64 and _is_pattern(s16.planes[:, (~used).to(dev)])


def test_fwd16_segs_format1_planes_and_no_planes(dev):
    """Layout 1 with the output planes in format 1, and a layout in which every segment has an fp32 output without planes."""
    from dupl_amd import ops
    segs, rows = _layout_step(12)
    _, outs, _, s16 = _segs_vs_batches(dev, 12, segs, rows, exp=ops.EXP_ACT)
    sc = float(outs[0].abs().max())
    assert float((_recon(s16.planes[:, :785], ops.EXP_ACT) - outs[0]).abs().max()) <= 2.0 ** -21 * sc
    segs, rows = _layout_ties()
    _segs_vs_batches(dev, 12, segs, rows, planes=False)


# ------------------------------------------------------------------------------------------ 4. containment
GUARD_ROWS = 128


class _Guarded:
    """A destination inside a larger pre-filled tensor: `full` (first dimension = rows / entries), data in [lo, hi)."""

    def __init__(self, full, lo, hi, name):
        self.full, self.lo, self.hi, self.name = full, lo, hi, name
        self.view = full[lo:hi]

    def ptr(self):
        return self.view.data_ptr()

    def check(self):
        assert _is_pattern(self.full[:self.lo]), f"{self.name}: the guard before the destination changed"
        assert _is_pattern(self.full[self.hi:]), f"{self.name}: the guard behind the destination changed"
        assert torch.isfinite(self.view).all(), f"{self.name}: not fully written"


def _guarded_rows(rows, cols, dev, name, behind=GUARD_ROWS):
    behind = max(behind, GUARD_ROWS)
    return _Guarded(_nan32(GUARD_ROWS + rows + behind, cols, dev=dev), GUARD_ROWS, GUARD_ROWS + rows, name)


def _guarded_flat(n, guard, dev, name, behind=0):
    behind = max(behind, guard)
    return _Guarded(_nan32(guard + n + behind, dev=dev), guard, guard + n, name)


def _check_planes(big, lo, hi, name, used=None):
    """big: Split16 with guard rows; [lo, hi) were handed to the kernel; used: bool mask over [lo, hi) of rows that must be written."""
    p = big.planes
    assert _is_pattern(p[:, :lo]) and _is_pattern(p[:, hi:]), f"{name}: guard rows of the planes changed"
    inner = p[:, lo:hi]
    if used is None:
        assert torch.isfinite(inner).all(), f"{name}: planes not fully written"
    else:
        assert torch.isfinite(inner[:, used]).all(), f"{name}: planes not fully written"
        assert _is_pattern(inner[:, ~used]), f"{name}: unused rows of the planes changed"


RAGGED = [(2, 33), (1, 129), (2, 197), (1, 785)]


@pytest.mark.parametrize("B,N", RAGGED, ids=[f"B{b}-N{n}" for b, n in RAGGED])
def test_fwd16_writes_nothing_outside_its_destinations(dev, B, N):
    """dupl_attention_fwd16 with fp32 out, lse and both planes inside NaN-filled tensors: >= 128 guard rows (N lse entries) on
    either side; behind a B_f32 < B prefix the guard is as large as what a kernel that ignored B_f32 would write."""
    from dupl_amd import ops
    H = 12
    D = H * HD
    qkv16 = ops.split16(_randn(B * N, 3 * D, 300 + N, 1.5).to(dev))
    ref_out = torch.empty(B * N, D, device=dev)
    ref_lse = ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, need_lse=True, out=ref_out)
    for bf in ([B] if B == 1 else [B, 1]):
        out = _guarded_rows(bf * N, D, dev, f"fp32 out (B_f32 {bf})", behind=(B - bf) * N)
        lse = _guarded_flat(bf * H * N, N, dev, f"lse (B_f32 {bf})", behind=(B - bf) * H * N)
        big = _nan_split16(B * N + 2 * GUARD_ROWS, D, dev)
        o16 = big.rows_slice(GUARD_ROWS, GUARD_ROWS + B * N)
        ops.L().dupl_attention_fwd16(qkv16.hi, qkv16.lo, out.ptr(), o16.hi, o16.lo, lse.ptr(), B, N, H, HD, float(SCALE), bf, 0,
                                     ops._stream())
        out.check()
        lse.check()
        _check_planes(big, GUARD_ROWS, GUARD_ROWS + B * N, f"B_f32 {bf}")
        assert _same_bits(out.view, ref_out[:bf * N]) and _same_bits(lse.view, ref_lse[:bf].reshape(-1))


def _segs_guarded(dev, H, segs, rows, seed=5):
    from dupl_amd import ops, _lib
    D = H * HD
    qkv16 = ops.split16(_randn(rows, 3 * D, seed, 1.5).to(dev))
    big = _nan_split16(rows + 2 * GUARD_ROWS, D, dev)
    o16 = big.rows_slice(GUARD_ROWS, GUARD_ROWS + rows)
    arr = (_lib.AttnSeg * len(segs))()
    dests = []
    used = torch.zeros(rows, dtype=torch.bool)
    for i, (r0, B, N, want, nl, b_f32) in enumerate(segs):
        bf = b_f32 or B
        out = _guarded_rows(bf * N, D, dev, f"segment {i} fp32 out", behind=(B - bf) * N) if want else None
        lse = _guarded_flat(bf * H * N, N, dev, f"segment {i} lse", behind=(B - bf) * H * N) if nl else None
        dests += [d for d in (out, lse) if d is not None]
        arr[i].row0, arr[i].B, arr[i].N, arr[i].B_f32 = r0, B, N, b_f32
        arr[i].out, arr[i].lse = (out.ptr() if out else None), (lse.ptr() if lse else None)
        used[r0:r0 + B * N] = True
    ops.L().dupl_attention_fwd16_segs(qkv16.hi, qkv16.lo, o16.hi, o16.lo, ctypes.cast(arr, ctypes.c_void_p), len(segs), H, HD,
                                      float(SCALE), 0, ops._stream())
    for d in dests:
        d.check()
    _check_planes(big, GUARD_ROWS, GUARD_ROWS + rows, "segmented launch", used.to(dev))


@pytest.mark.parametrize("layout", ["step", "gaps"])
def test_fwd16_segs_writes_nothing_outside_its_destinations(dev, layout):
    """Layouts 1 and 4 with every destination guarded: the fp32 out / lse of the 2 x 785 segment exist for its first image only
    (B_f32 = 1), the rows / entries its second image would occupy are guards; the planes of both images are written."""
    segs, rows = _layout_step(12) if layout == "step" else _layout_gaps()
    _segs_guarded(dev, 12, segs, rows)


def _bwd16_raw(ops, qkv16, out, dout, lse, delta_ptr, dqkv_ptr, B, N, H, hd=HD):
    """dupl_attention_bwd16 with the arguments ops.attention_bwd16 passes and the caller's delta / dqkv."""
    do16, _, alpha = ops.split_prepare(dout, scaled=True, want_rm=True, want_T=False, target_exp=4)
    alpha.check()
    ops.L().dupl_attention_bwd16(qkv16.hi, qkv16.lo, out.data_ptr(), dout.data_ptr(), do16.hi, do16.lo, int(alpha) - 4,
                                 lse.data_ptr(), delta_ptr, dqkv_ptr, B, N, H, hd, float(SCALE), None, ops._stream())
    torch.cuda.synchronize()          # do16 stays alive until the kernels have read it


@pytest.mark.parametrize("B,N", RAGGED, ids=[f"B{b}-N{n}" for b, n in RAGGED])
def test_bwd16_writes_nothing_outside_its_destinations(dev, B, N):
    """dupl_attention_bwd16 with dqkv (128 guard rows) and delta (N guard entries) inside NaN-filled tensors."""
    from dupl_amd import ops
    H = 12
    D = H * HD
    qkv16 = ops.split16(_randn(B * N, 3 * D, 400 + N, 1.2).to(dev))
    dout = _randn(B * N, D, 401 + N, 2e-5).to(dev)
    out = torch.empty(B * N, D, device=dev)
    lse = ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, need_lse=True, out=out)
    ref = ops.attention_bwd16(qkv16, out, dout, lse, B, N, H, HD, SCALE)
    dqkv = _guarded_rows(B * N, 3 * D, dev, "dqkv")
    delta = _guarded_flat(B * H * N, N, dev, "delta")
    _bwd16_raw(ops, qkv16, out, dout, lse, delta.ptr(), dqkv.ptr(), B, N, H)
    dqkv.check()
    delta.check()
    assert _same_bits(dqkv.view, ref)


# ------------------------------------------------------------------------------------------ 5. isolation
TAIL = 64          # rows that follow the rows_slice in the base buffer


def _poisoned_planes(ops, dev, base, qkv, B, N, D, img, poison):
    """A copy of the clean planes in which every row that is not image `img` -- the other image and the TAIL rows behind the
    slice -- holds NaN, or finite decoys: keys = 8 x the queries of image `img` (scores far above the real ones) and v = 1e3."""
    p = ops.Split16(base.planes.clone())
    other = 1 - img
    if poison == "nan":
        p.planes[:, other * N:(other + 1) * N] = torch.full((), NAN16, dtype=torch.int16, device=dev).view(torch.float16)
        p.planes[:, B * N:] = torch.full((), NAN16, dtype=torch.int16, device=dev).view(torch.float16)
    else:
        d = qkv[img * N:(img + 1) * N].clone()
        d[:, D:2 * D] = 8.0 * d[:, :D]
        d[:, 2 * D:] = 1e3
        d16 = ops.split16(d.contiguous())
        p.planes[:, other * N:(other + 1) * N] = d16.planes
        p.planes[:, B * N:] = d16.planes[:, :TAIL]
    assert _same_bits(p.planes[:, img * N:(img + 1) * N], base.planes[:, img * N:(img + 1) * N])
    return p


@pytest.mark.parametrize("poison", ["nan", "decoy"])
@pytest.mark.parametrize("N", [65, 130, 197])
def test_fwd16_reads_nothing_outside_its_own_image(dev, N, poison):
    """B = 2 on a rows_slice of a buffer with TAIL more rows.  An image's output, lse and planes are bit-identical whether the
    rest of the buffer holds the clean data, NaN, or decoys that would dominate the softmax: the clamped rows of the partial last
    key tile stay inside the image, and what is read past N there is masked."""
    from dupl_amd import ops
    B, H = 2, 12
    D = H * HD
    qkv = _randn(B * N + TAIL, 3 * D, 500 + N, 1.5).to(dev)
    base = ops.split16(qkv)

    def run(p16):
        out = _nan32(B * N, D, dev=dev)
        o16 = _nan_split16(B * N, D, dev)
        lse = ops.attention_fwd16(p16.rows_slice(0, B * N), B, N, H, HD, SCALE, need_lse=True, out=out, out16=o16)
        return out, lse, o16.planes

    out0, lse0, pl0 = run(base)
    assert torch.isfinite(out0).all() and torch.isfinite(lse0).all() and torch.isfinite(pl0).all()
    for img in (0, 1):
        out, lse, pl = run(_poisoned_planes(ops, dev, base, qkv, B, N, D, img, poison))
        rs = slice(img * N, (img + 1) * N)
        assert _same_bits(out[rs], out0[rs]), f"image {img}: fp32 out"
        assert _same_bits(lse[img], lse0[img]), f"image {img}: lse"
        assert _same_bits(pl[:, rs], pl0[:, rs]), f"image {img}: planes"


@pytest.mark.parametrize("poison", ["nan", "decoy"])
@pytest.mark.parametrize("N", [65, 130, 197])
def test_bwd16_reads_nothing_outside_its_own_image(dev, N, poison):
    """The same for the backward: q / k / v planes of the other image (and of the rows behind the slice) poisoned, out, lse and
    dout clean (the scaling of dout is global by design); the dqkv rows of the clean image are bit-identical."""
    from dupl_amd import ops
    B, H = 2, 12
    D = H * HD
    qkv = _randn(B * N + TAIL, 3 * D, 600 + N, 1.2).to(dev)
    dout = _randn(B * N, D, 601 + N, 2e-5).to(dev)
    base = ops.split16(qkv)
    out = torch.empty(B * N, D, device=dev)
    lse = ops.attention_fwd16(base.rows_slice(0, B * N), B, N, H, HD, SCALE, need_lse=True, out=out)
    d0 = ops.attention_bwd16(base.rows_slice(0, B * N), out, dout, lse, B, N, H, HD, SCALE)
    assert torch.isfinite(d0).all()
    for img in (0, 1):
        p16 = _poisoned_planes(ops, dev, base, qkv, B, N, D, img, poison)
        d = ops.attention_bwd16(p16.rows_slice(0, B * N), out, dout, lse, B, N, H, HD, SCALE)
        rs = slice(img * N, (img + 1) * N)
        assert _same_bits(d[rs], d0[rs]), f"image {img}: dqkv"


# ------------------------------------------------------------------------------------------ 6. refusals
REFUSALS = ["segs-n0", "segs-n5", "fwd16-hd32", "segs-hd32", "bwd16-hd32", "fwd16-B_f32-above-B", "segs-B_f32-above-B",
            "fwd16-no-destination", "segs-no-destination", "segs-row0-negative", "fwd16-hi-without-lo", "segs-hi-without-lo",
            "fwd16-N0", "segs-N0", "bwd16-N0", "bwd16-N2049"]


@pytest.mark.parametrize("case", REFUSALS)
def test_launchers_refuse_bad_arguments_before_launching(dev, case):
    """Every case is rejected by a check that precedes the launch (attn_fwd16_launch / dupl_attention_fwd16 /
    dupl_attention_bwd16): RuntimeError with status -1, and the NaN-filled destinations keep their fill."""
    from dupl_amd import ops, _lib
    B, H = 1, 2
    N = 2049 if case == "bwd16-N2049" else 33
    D = H * HD
    qkv16 = ops.split16(_randn(B * N, 3 * D, 700, 1.0).to(dev))
    out, lse = _nan32(B * N, D, dev=dev), _nan32(B, H, N, dev=dev)
    o16 = _nan_split16(B * N, D, dev)
    dqkv, delta = _nan32(B * N, 3 * D, dev=dev), _nan32(B, H, N, dev=dev)
    Lb = ops.L()

    def fwd16(out_p=out.data_ptr(), hi=o16.hi, lo=o16.lo, B_=B, N_=N, hd=HD, bf=0):
        Lb.dupl_attention_fwd16(qkv16.hi, qkv16.lo, out_p, hi, lo, lse.data_ptr(), B_, N_, H, hd, float(SCALE), bf, 0, ops._stream())

    def segs(n=1, count=1, row0=0, B_=B, N_=N, bf=0, out_p=out.data_ptr(), hi=o16.hi, lo=o16.lo, hd=HD):
        arr = (_lib.AttnSeg * max(count, 1))()
        for i in range(max(count, 1)):
            arr[i].row0, arr[i].B, arr[i].N, arr[i].B_f32 = row0, B_, N_, bf
            arr[i].out, arr[i].lse = out_p, lse.data_ptr()
        Lb.dupl_attention_fwd16_segs(qkv16.hi, qkv16.lo, hi, lo, ctypes.cast(arr, ctypes.c_void_p), n, H, hd, float(SCALE), 0,
                                     ops._stream())

    def bwd16(N_=N, hd=HD):
        src_out, dout = torch.zeros(B * N, D, device=dev), _randn(B * N, D, 701, 2e-5).to(dev)
        src_lse = torch.zeros(B, H, N, device=dev)
        _bwd16_raw(ops, qkv16, src_out, dout, src_lse, delta.data_ptr(), dqkv.data_ptr(), B, N_, H, hd)

    call = {"segs-n0": lambda: segs(n=0), "segs-n5": lambda: segs(n=5, count=5),
            "fwd16-hd32": lambda: fwd16(hd=32), "segs-hd32": lambda: segs(hd=32), "bwd16-hd32": lambda: bwd16(hd=32),
            "fwd16-B_f32-above-B": lambda: fwd16(bf=B + 1), "segs-B_f32-above-B": lambda: segs(bf=B + 1),
            "fwd16-no-destination": lambda: fwd16(out_p=None, hi=None, lo=None),
            "segs-no-destination": lambda: segs(out_p=None, hi=None, lo=None),
            "segs-row0-negative": lambda: segs(row0=-1),
            "fwd16-hi-without-lo": lambda: fwd16(lo=None), "segs-hi-without-lo": lambda: segs(lo=None),
            "fwd16-N0": lambda: fwd16(N_=0), "segs-N0": lambda: segs(N_=0), "bwd16-N0": lambda: bwd16(N_=0),
            "bwd16-N2049": lambda: bwd16()}[case]
    assert _lib.ATTN_SEGS_MAX == 4          # "segs-n5" is one more than the maximum
    with pytest.raises(RuntimeError, match="status -1"):
        call()
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("planes", o16.planes), ("dqkv", dqkv), ("delta", delta)):
        assert _is_pattern(t), f"{case}: {name} was written"
    if case == "bwd16-N2049":
        with pytest.raises(AssertionError):          # and the Python wrapper says so before the library is asked
            ops.attention_bwd16(qkv16, out, out, lse, B, N, H, HD, SCALE)


# ------------------------------------------------------------------------------------------ 7. the exact-f32 kernels
F32_CASES = [(1, 1765, 2, 64), (1, 2048, 2, 64), (1, 2117, 2, 64), (1, 2117, 1, 32), (2, 128, 2, 64), (1, 1, 2, 64), (1, 2117, 12, 64)]


@pytest.mark.parametrize("B,N,H,hd", F32_CASES, ids=[f"B{b}-N{n}-H{h}-hd{d}" for b, n, h, d in F32_CASES])
def test_f32_attention_at_the_lengths_it_serves(dev, B, N, H, hd):
    """dupl_attention_fwd / dupl_attention_bwd against float64 with the bars of test_attention_fwd_bwd (out 5e-6, lse 5e-6,
    dqkv 2e-5, each relative to the reference's maximum) at the CAM-scale lengths and beyond the split backward's limit.  A plain
    fp32 PyTorch evaluation of the formula on a CPU reaches out 1.6e-6, lse 2.7e-7, dqkv 9.5e-7 at these shapes."""
    from dupl_amd import ops
    D = H * hd
    scale = hd ** -0.5
    qkv = _randn(B * N, 3 * D, 11, 1.5).to(dev)
    dout = _randn(B * N, D, 12, 1.0).to(dev)
    ref, ref_lse, ref_grad = ref64(qkv, B, N, H, hd, scale, dout)
    out, lse = ops.attention_fwd(qkv, B, N, H, hd, scale, need_lse=True)
    dqkv = ops.attention_bwd(qkv, out, dout, lse, B, N, H, hd, scale)

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())

    eo, el, eg = rel(out, ref), rel(lse, ref_lse), rel(dqkv, ref_grad)
    print(f"f32 B{B} N{N} H{H} hd{hd}: out {eo:.2e} (bar 5e-6), lse {el:.2e} (bar 5e-6), dqkv {eg:.2e} (bar 2e-5)")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    assert eo < 5e-6 and el < 5e-6 and eg < 2e-5
