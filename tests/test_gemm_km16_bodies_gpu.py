"""GPU: the two bodies of the k-major backward GEMMs -- dupl_gemm16_desc.tile 24 (gemm_f16x3_km_body, v_mfma_f32_32x32x16_f16) and 26
(gemm_f16x3_km16_body, v_mfma_f32_16x16x32_f16) -- side by side, at the smallest shapes at which each mechanism engages: every
instantiation of gemm_f16x3_km_kernel and the grouped kernel, each through both tile ids.

Operands and the float64 reference are test_gemm_km16_gpu._operands (the values the planes REPRESENT; built once per shape and shared with
that module).  Bar of every GEMM check, the standing one: error over max |ref| <= 2 x the exact-f32 kernel's on the same values + 2e-7.
Every case also prints max |tile 26 - tile 24| / max |ref| (only the order of the sums inside a k-tile differs: a reported figure)."""
import pytest
import torch

from test_gemm_km16_gpu import _err, _operands

pytestmark = pytest.mark.gpu

BODIES = (24, 26)


def _tn(tile, **kw):
    from dupl_amd import ops
    return dict(ops.GEMM16_TUNING, tile=tile, **kw)


def _gelu_grad(p):
    return 0.5 * (1 + torch.erf(p / 2 ** 0.5)) + p * torch.exp(-0.5 * p * p) / (2 * torch.pi) ** 0.5


def _both(name, outs, want, e32):
    """The bar for both bodies' results, and the reported distance between them."""
    for tile in BODIES:
        e16 = _err(outs[tile], want)
        print(f"{name} tile {tile}: f16x3 {e16:.2e}  f32 {e32:.2e}")
        assert e16 <= 2.0 * e32 + 2e-7, (name, tile)
    d = float((outs[26].double() - outs[24].double()).abs().max()) / float(want.abs().max())
    print(f"{name}: max |t26 - t24| / max |ref| = {d:.2e}")


# ------------------------------------------------------------------------------------------ data gradients
@pytest.mark.parametrize("tokens", [1, 15, 17, 255, 257])
def test_dgrad_full_epilogue(dev, tokens):
    """dx = (dy . W) [* gelu'(pre)] with the producer amax: contraction exactly the pipeline depth (96) and one step more (128); a
    ragged column tile (8), one tile + 8, two tiles + 8; row tiles of 1 .. 257 rows.  The amax word is max |dx| exactly."""
    from dupl_amd import ops
    for n_out in (96, 128):
        for n_in in (8, 136, 264):
            o = _operands(tokens, n_out, n_in)
            for dgelu in (False, True):
                pre = o["pre"] if dgelu else None
                want = o["dy_r"] @ o["W_r"]
                if dgelu:
                    want = want * _gelu_grad(o["pre"].double().cpu())
                e32 = _err(ops.linear_dgrad(o["dy32"], o["W32"], dgelu_of=pre), want)
                outs = {}
                for tile in BODIES:
                    dx, _ = ops.linear16(o["dy16"].rows_slice(0, tokens), o["W16"], alpha=o["alpha"], dgelu_of=pre, b_kmajor=True,
                                         amax_for_next=True, tuning=_tn(tile))
                    ring = ops._scale_ring(dev)
                    assert dx._dupl_amax is ring[2]
                    word = ring[0][ring[1], 2].clone()
                    ops.split_prepare(dx, scaled=True, want_rm=True, want_T=False)      # (closes the reservation)
                    assert float(word) == float(dx.abs().max()) > 0, (tile, n_out, n_in, dgelu)
                    outs[tile] = dx
                _both(f"dgrad {tokens}x{n_in}x{n_out} dgelu={int(dgelu)}", outs, want, e32)


# (n_out = contraction length, slice count): 6 k-steps in two slices and 9 in three are the shortest that leave every slice the three
# k-steps of the prologue; < 0 = the equal-run cut
STREAM_K = ((192, 2), (192, -1), (288, 3), (288, -1))


@pytest.mark.parametrize("tokens", [17, 257])
def test_dgrad_stream_k_into_zeros(dev, tokens):
    """The linear-epilogue data gradient as a stream-K launch into a zero-filled dx: two and three aligned slices of three k-steps each,
    and the equal-run cut; one and two row tiles, a ragged and three column tiles."""
    from dupl_amd import ops
    for n_out, sk in STREAM_K:
        for n_in in (8, 264):
            o = _operands(tokens, n_out, n_in)
            want = o["dy_r"] @ o["W_r"]
            e32 = _err(ops.linear_dgrad(o["dy32"], o["W32"]), want)
            outs = {}
            for tile in BODIES:
                outs[tile] = ops.zeros((tokens, n_in), dev)
                ops.linear16(o["dy16"].rows_slice(0, tokens), o["W16"], out=outs[tile], accumulate=True, alpha=o["alpha"], b_kmajor=True,
                             tuning=_tn(tile, sk_slices=sk))
            _both(f"stream-K dgrad {tokens}x{n_in}x{n_out} sk_slices={sk}", outs, want, e32)


# ------------------------------------------------------------------------------------------ weight gradients
def _wgrad_single(o, out, det, tile, **kw):
    from dupl_amd import ops
    ops.set_deterministic(det)
    try:
        ops.linear16(o["dy16"], o["x16"], out=out, accumulate=True, alpha=o["alpha"], a_kmajor=True, b_kmajor=True, k_pad=o["Kp"],
                     tuning=_tn(tile, **kw))
    finally:
        ops.set_deterministic(0)
    return out


def _wgrad_f32(o, shape, dev):
    from dupl_amd import ops
    c32 = ops.zeros(shape, dev)
    ops.linear_wgrad(o["dy32"], o["x32"], c32, accumulate=True)
    return c32


# (n_out, n_in): one tile with both edges ragged (136 x 8), a ragged row tile over three column tiles, two row tiles over two and over
# three column tiles
GROUP = ((8, 264), (136, 8), (264, 136), (264, 264))


@pytest.mark.parametrize("more_rows", [False, True], ids=["exact", "more"])
@pytest.mark.parametrize("tokens", [1, 31, 33, 97])
def test_wgrad_single_launch(dev, tokens, more_rows):
    """dW += dy^T . x into zeros, both operands k-major: Kp = 96 / 128 pads dy with zero rows, x is clamped to its last valid row
    (exact) or goes on with 13 finite foreign rows (more).  The one-owner form (deterministic mode) twice is bit-identical."""
    for n_out, n_in in GROUP:
        o = _operands(tokens, n_out, n_in, more_rows)
        want = o["dy_r"].t() @ o["x_r"]
        e32 = _err(_wgrad_f32(o, (n_out, n_in), dev), want)
        for det in (0, 1):
            from dupl_amd import ops
            outs = {tile: _wgrad_single(o, ops.zeros((n_out, n_in), dev), det, tile) for tile in BODIES}
            _both(f"wgrad {n_out}x{n_in}x{tokens} det={det}", outs, want, e32)
            if det:
                for tile in BODIES:
                    again = _wgrad_single(o, ops.zeros((n_out, n_in), dev), 1, tile)
                    assert torch.equal(again.view(torch.int32), outs[tile].view(torch.int32)), (tile, n_out, n_in)


def test_wgrad_stream_k(dev):
    """The stream-K weight gradient (fp32 atomics) engages from Kp = 288 on (the shortest contraction that is split at all): 257 tokens,
    two aligned slices and the equal-run cut."""
    from dupl_amd import ops
    tokens = 257
    for n_out, n_in in ((136, 8), (264, 264)):
        o = _operands(tokens, n_out, n_in)
        assert o["Kp"] == 288
        want = o["dy_r"].t() @ o["x_r"]
        e32 = _err(_wgrad_f32(o, (n_out, n_in), dev), want)
        for sk in (2, -1):
            outs = {tile: _wgrad_single(o, ops.zeros((n_out, n_in), dev), 0, tile, sk_slices=sk) for tile in BODIES}
            _both(f"stream-K wgrad {n_out}x{n_in}x{tokens} sk_slices={sk}", outs, want, e32)


@pytest.mark.parametrize("more_rows", [False, True], ids=["exact", "more"])
@pytest.mark.parametrize("tokens", [1, 31, 33, 97])
def test_wgrad_grouped(dev, tokens, more_rows):
    """Four problems of different sizes as one grouped launch: the fp64 bar; bit-identical to each launched singly in deterministic mode
    on the same body; `fresh` into a NaN-filled target gives the bits of the accumulating form into zeros; without it a non-zero
    target receives exactly one fp32 add of those values."""
    from dupl_amd import ops
    os_ = [_operands(tokens, n_out, n_in, more_rows) for n_out, n_in in GROUP]

    def group(cs, tile, fresh=None):
        ops.wgrad16_group([(o["dy16"], o["x16"], c, o["alpha"]) for o, c in zip(os_, cs)], tuning=_tn(tile), fresh=fresh)
        return cs

    acc = {tile: group([ops.zeros(s, dev) for s in GROUP], tile) for tile in BODIES}
    gen = torch.Generator().manual_seed(tokens)
    for i, ((n_out, n_in), o) in enumerate(zip(GROUP, os_)):
        want = o["dy_r"].t() @ o["x_r"]
        e32 = _err(_wgrad_f32(o, (n_out, n_in), dev), want)
        _both(f"grouped wgrad {n_out}x{n_in}x{tokens}", {tile: acc[tile][i] for tile in BODIES}, want, e32)
    for tile in BODIES:
        for (n_out, n_in), o, c in zip(GROUP, os_, acc[tile]):
            assert torch.equal(c, _wgrad_single(o, ops.zeros((n_out, n_in), dev), 1, tile)), (tile, n_out, n_in)
        over = group([torch.full(s, float("nan"), device=dev) for s in GROUP], tile, fresh=[True] * 4)
        base = [(torch.randn(s, generator=gen) * 1e-4).to(dev) for s in GROUP]
        onto = group([b.clone() for b in base], tile)
        for c, a, b, t in zip(over, acc[tile], base, onto):
            assert torch.equal(c.view(torch.int32), a.view(torch.int32)), tile
            assert torch.equal(t, b + a), tile


# ------------------------------------------------------------------------------------------ a block walks more than one piece
# 9 tiles of 256 x 128 (3 row tiles x 3 column tiles; group 2: the last row group is ragged) on a grid of 8 blocks: the block of XCD 0
# walks two tiles (a next piece, then none), the others one.  Which block computes a tile does not enter its arithmetic.
WALK = dict(persist_blocks=8, group=2)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("tile", BODIES)
@pytest.mark.parametrize("dgelu", [False, True], ids=["linear", "dgelu"])
def test_walk_dgrad_full_epilogue(dev, tile, dgelu):
    """513 tokens x n_in 264 x n_out 96 on 8 blocks: bit-identical to the default grid, the amax word included."""
    from dupl_amd import ops
    o = _operands(513, 96, 264)
    pre = o["pre"] if dgelu else None
    got = {}
    for name, extra in (("default", dict(group=2)), ("walk", WALK)):
        dx, _ = ops.linear16(o["dy16"].rows_slice(0, 513), o["W16"], alpha=o["alpha"], dgelu_of=pre, b_kmajor=True, amax_for_next=True,
                             tuning=_tn(tile, **extra))
        ring = ops._scale_ring(dev)
        assert dx._dupl_amax is ring[2]
        word = ring[0][ring[1], 2].clone()
        ops.split_prepare(dx, scaled=True, want_rm=True, want_T=False)      # (closes the reservation)
        assert float(word) == float(dx.abs().max()) > 0
        got[name] = (dx, word)
    assert torch.equal(_bits(got["walk"][0]), _bits(got["default"][0]))
    assert torch.equal(_bits(got["walk"][1]), _bits(got["default"][1]))


@pytest.mark.parametrize("tile", BODIES)
def test_walk_wgrad_one_owner(dev, tile):
    """n_out 520 x n_in 264 over 97 tokens (Kp 128), the one-owner form (deterministic mode) on 8 blocks: bit-identical to the default grid."""
    from dupl_amd import ops
    o = _operands(97, 520, 264)
    assert o["Kp"] == 128
    base = _wgrad_single(o, ops.zeros((520, 264), dev), 1, tile, group=2)
    walk = _wgrad_single(o, ops.zeros((520, 264), dev), 1, tile, **WALK)
    assert float(base.abs().max()) > 0
    assert torch.equal(_bits(walk), _bits(base))


@pytest.mark.parametrize("sk", [0, -1], ids=["host-choice", "equal-runs"])
def test_walk_stream_k_equal_runs(dev, sk):
    """Contraction 288 = 9 k-steps, 9 tiles on 8 blocks: more tiles than blocks, so the host takes the equal-run cut (sk_slices 0) as it
    does when asked for it (-1).  Runs of 81 / 8 k-steps span tiles, and cuts that land within 2 k-steps of a tile's edge are moved.
    Data gradient into zeros and weight gradient, both bodies, the standing bar."""
    from dupl_amd import ops
    o = _operands(513, 288, 264)
    want = o["dy_r"] @ o["W_r"]
    e32 = _err(ops.linear_dgrad(o["dy32"], o["W32"]), want)
    outs = {}
    for tile in BODIES:
        outs[tile] = ops.zeros((513, 264), dev)
        ops.linear16(o["dy16"].rows_slice(0, 513), o["W16"], out=outs[tile], accumulate=True, alpha=o["alpha"], b_kmajor=True,
                     tuning=_tn(tile, sk_slices=sk, **WALK))
    _both(f"walk stream-K dgrad 513x264x288 sk_slices={sk}", outs, want, e32)
    o = _operands(257, 520, 264)
    assert o["Kp"] == 288
    want = o["dy_r"].t() @ o["x_r"]
    e32 = _err(_wgrad_f32(o, (520, 264), dev), want)
    outs = {tile: _wgrad_single(o, ops.zeros((520, 264), dev), 0, tile, sk_slices=sk, **WALK) for tile in BODIES}
    _both(f"walk stream-K wgrad 520x264x257 sk_slices={sk}", outs, want, e32)


def test_walk_stream_k_aligned_slices(dev):
    """sk_slices 2 with n_in 8: 3 tiles -> 6 (tile, slice) units on 8 blocks, two blocks return at once.  Slices of 5 and 4 k-steps."""
    from dupl_amd import ops
    o = _operands(513, 288, 8)
    want = o["dy_r"] @ o["W_r"]
    e32 = _err(ops.linear_dgrad(o["dy32"], o["W32"]), want)
    outs = {}
    for tile in BODIES:
        outs[tile] = ops.zeros((513, 8), dev)
        ops.linear16(o["dy16"].rows_slice(0, 513), o["W16"], out=outs[tile], accumulate=True, alpha=o["alpha"], b_kmajor=True,
                     tuning=_tn(tile, sk_slices=2, **WALK))
    _both("walk stream-K dgrad 513x8x288 sk_slices=2", outs, want, e32)
    o = _operands(257, 520, 8)
    want = o["dy_r"].t() @ o["x_r"]
    e32 = _err(_wgrad_f32(o, (520, 8), dev), want)
    outs = {tile: _wgrad_single(o, ops.zeros((520, 8), dev), 0, tile, sk_slices=2, **WALK) for tile in BODIES}
    _both("walk stream-K wgrad 520x8x257 sk_slices=2", outs, want, e32)


# ------------------------------------------------------------------------------------------ two streams
@pytest.mark.parametrize("tile", BODIES)
def test_bodies_are_deterministic_under_stream_concurrency(dev, tile):
    """Two launches of each instantiation on two streams at once reproduce their solo results bit for bit (the pattern of
    test_split_kernels_are_deterministic_under_stream_concurrency).  The stream-K forms run with two slices: two addends per element
    meet in the atomics, and an fp32 sum of two does not depend on their order."""
    from dupl_amd import ops
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    oa, ob = _operands(257, 192, 264), _operands(255, 192, 136)
    wa, wb = _operands(257, 264, 264), _operands(257, 264, 136)

    def dgrad_epi(o, tokens):
        out = torch.empty((tokens, o["W16"].cols), device=dev)
        return (lambda: ops.linear16(o["dy16"].rows_slice(0, tokens), o["W16"], alpha=o["alpha"], dgelu_of=o["pre"], b_kmajor=True, out=out,
                                     tuning=_tn(tile))), out

    def dgrad_sk(o, tokens):
        out = torch.empty((tokens, o["W16"].cols), device=dev)

        def run():
            out.zero_()
            ops.linear16(o["dy16"].rows_slice(0, tokens), o["W16"], out=out, accumulate=True, alpha=o["alpha"], b_kmajor=True,
                         tuning=_tn(tile, sk_slices=2))
        return run, out

    def wgrad(o, det, **kw):
        out = torch.empty((o["dy16"].cols, o["x16"].cols), device=dev)

        def run():
            out.zero_()
            _wgrad_single(o, out, det, tile, **kw)
        return run, out

    def grouped(os_):
        outs = [torch.empty((o["dy16"].cols, o["x16"].cols), device=dev) for o in os_]
        return (lambda: ops.wgrad16_group([(o["dy16"], o["x16"], c, o["alpha"]) for o, c in zip(os_, outs)], tuning=_tn(tile),
                                          fresh=[True] * len(os_))), outs

    pairs = [("dgrad epilogue", dgrad_epi(oa, 257), dgrad_epi(ob, 255)),
             ("dgrad stream-K", dgrad_sk(oa, 257), dgrad_sk(ob, 255)),
             ("wgrad stream-K", wgrad(wa, 0, sk_slices=2), wgrad(wb, 0, sk_slices=2)),
             ("wgrad one owner", wgrad(wa, 1), wgrad(wb, 1)),
             ("wgrad grouped", grouped([wa, wb]), grouped([wb, wa]))]
    for name, (ra, outa), (rb, outb) in pairs:
        la, lb = (outa if isinstance(outa, list) else [outa]), (outb if isinstance(outb, list) else [outb])
        ra()
        rb()
        torch.cuda.synchronize()
        solo = [c.clone() for c in la + lb]
        bad = 0
        for _ in range(4):
            with torch.cuda.stream(s1):
                for _ in range(3):
                    ra()
            with torch.cuda.stream(s2):
                for _ in range(3):
                    rb()
            torch.cuda.synchronize()
            bad += int(not all(torch.equal(c.view(torch.int32), r.view(torch.int32)) for c, r in zip(la + lb, solo)))
        print(f"tile {tile} {name}: {bad}/4 rounds deviate from the solo result")
        assert bad == 0, (tile, name)
