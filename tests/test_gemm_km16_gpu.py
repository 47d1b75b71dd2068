"""GPU: the k-major backward GEMMs (dupl_gemm16_desc.a_layout / b_layout) at the smallest shapes at which each of their mechanisms
engages, the overwrite form of the grouped weight gradients (DUPL_GEMM_C_FRESH) and the lazily zeroed gradient ranges built on it.

Reference of every GEMM check: a float64 matmul on the CPU of the values the operand planes REPRESENT ((hi + lo) 2^-exp, times the
inverse scale of scaled gradient planes), so that the operand split itself is not part of the error.  Bar (the standing one of
test_kmajor_backward_gemms_are_fp32_equivalent): error over max |ref| <= 2 x the exact-f32 kernel's on the same values + 2e-7."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


def _rep(p16, inv_scale: float = 1.0):
    """float64 CPU values of operand planes in format 1."""
    return (p16.planes[0].double() + p16.planes[1].double()).cpu() * (2.0 ** -p16.exp) * inv_scale


@functools.lru_cache(maxsize=None)
def _operands(tokens: int, n_out: int, n_in: int, more_rows: bool = False):
    """One Linear's backward operands as planes, and what they represent: dy [tokens, n_out] scaled format 1 planes with zero rows up
    to Kp; x [tokens (+ 13 foreign rows), n_in]; W [n_out, n_in]; pre [tokens, n_in].  Built once per shape, never modified."""
    from dupl_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * tokens + 10 * n_out + n_in)
    dy = (torch.randn(tokens, n_out, generator=g) * 2e-5 * (1.0 + 5.0 * (torch.rand(tokens, 1, generator=g) > 0.9))).to(dev)
    x_all = torch.randn(tokens + (13 if more_rows else 0), n_in, generator=g).to(dev)
    W = (torch.randn(n_out, n_in, generator=g) * 0.03).to(dev)
    pre = torch.randn(tokens, n_in, generator=g).to(dev)
    Kp = max(96, (tokens + 31) // 32 * 32)
    dy16, _, _ = ops.split_prepare(dy, scaled=True, want_rm=True, want_T=False, fmt1=True, rm_rows=Kp)
    x16, W16 = ops.split16(x_all, exp=ops.EXP_ACT), ops.split16(W, exp=ops.EXP_W)
    # the 1 / scale of the gradient planes in a word of its own: the ring slot split_prepare returned is reused 128 splits later
    inv = dy16.planes._dupl_scale[1:2].clone()
    torch.cuda.synchronize()
    dy_r = _rep(dy16, float(inv))[:tokens]
    x_r, W_r = _rep(x16)[:tokens], _rep(W16)
    return dict(dy16=dy16, alpha=inv.data_ptr(), inv=inv, x16=x16, W16=W16, pre=pre, Kp=Kp, dy_r=dy_r, x_r=x_r, W_r=W_r,
                dy32=dy_r.float().to(dev), x32=x_r.float().to(dev), W32=W_r.float().to(dev))


def _err(got, want):
    return float((got.double().cpu() - want).abs().max()) / float(want.abs().max())


# ------------------------------------------------------------------------------------------ data gradients
@pytest.mark.parametrize("tokens", [1, 15, 17, 255, 257])
def test_dgrad_full_epilogue(dev, tokens):
    """dx = (dy . W) [* gelu'(pre)] with the producer amax, W read k-major: contraction exactly the pipeline depth (96) and one step
    more (128), a ragged column tile (8), one tile + 8, two tiles + 8; row tiles of 1 .. 257 rows."""
    from dupl_amd import ops
    for n_out in (96, 128):
        for n_in in (8, 136, 264):
            o = _operands(tokens, n_out, n_in)
            for dgelu in (False, True):
                pre = o["pre"] if dgelu else None
                dx, _ = ops.linear16(o["dy16"].rows_slice(0, tokens), o["W16"], alpha=o["alpha"], dgelu_of=pre, b_kmajor=True,
                                     amax_for_next=True)
                ring = ops._scale_ring(dev)
                assert dx._dupl_amax is ring[2]
                word = ring[0][ring[1], 2].clone()
                ops.split_prepare(dx, scaled=True, want_rm=True, want_T=False)      # (closes the reservation)
                assert float(word) == float(dx.abs().max()) > 0, (n_out, n_in, dgelu)
                want = o["dy_r"] @ o["W_r"]
                if dgelu:
                    p = o["pre"].double().cpu()
                    want = want * (0.5 * (1 + torch.erf(p / 2 ** 0.5)) + p * torch.exp(-0.5 * p * p) / (2 * torch.pi) ** 0.5)
                dx32 = ops.linear_dgrad(o["dy32"], o["W32"], dgelu_of=pre)
                e16, e32 = _err(dx, want), _err(dx32, want)
                print(f"dgrad {tokens}x{n_in}x{n_out} dgelu={int(dgelu)}: f16x3 {e16:.2e}  f32 {e32:.2e}")
                assert e16 <= 2.0 * e32 + 2e-7, (n_out, n_in, dgelu)


@pytest.mark.parametrize("tokens", [1, 15, 17, 255, 257])
def test_dgrad_stream_k_into_zeros(dev, tokens):
    """The linear-epilogue data gradient as a stream-K launch into zeros: the library's cut and explicit slice counts -- one slice,
    two (which 3 k-steps cannot be cut into), and more units than the grid has blocks (both fall back to the library's choice)."""
    from dupl_amd import ops
    for n_out in (96, 384):
        for n_in in (8, 136, 264):
            o = _operands(tokens, n_out, n_in)
            want = o["dy_r"] @ o["W_r"]
            e32 = _err(ops.linear_dgrad(o["dy32"], o["W32"]), want)
            for sk in (0, 1, 2, 1000):
                dx = ops.zeros((tokens, n_in), dev)
                ops.linear16(o["dy16"].rows_slice(0, tokens), o["W16"], out=dx, accumulate=True, alpha=o["alpha"], b_kmajor=True,
                             tuning=dict(ops.GEMM16_TUNING, sk_slices=sk))
                e16 = _err(dx, want)
                print(f"stream-K dgrad {tokens}x{n_in}x{n_out} sk_slices={sk}: f16x3 {e16:.2e}  f32 {e32:.2e}")
                assert e16 <= 2.0 * e32 + 2e-7, (n_out, n_in, sk)


# ------------------------------------------------------------------------------------------ weight gradients
WGRAD_DIMS = (8, 136, 264)


def _wgrad_single(o, out, det):
    from dupl_amd import ops
    ops.set_deterministic(det)
    try:
        ops.linear16(o["dy16"], o["x16"], out=out, accumulate=True, alpha=o["alpha"], a_kmajor=True, b_kmajor=True, k_pad=o["Kp"])
    finally:
        ops.set_deterministic(0)
    return out


@pytest.mark.parametrize("more_rows", [False, True], ids=["exact", "more"])
@pytest.mark.parametrize("tokens", [1, 31, 33, 97])
def test_wgrad_single_launch(dev, tokens, more_rows):
    """dW += dy^T . x, both operands k-major, token counts whose zero-padded rows up to Kp = max(96, ceil32) matter; x planes that end
    exactly at `tokens` (clamped reads) or go on with finite foreign rows (dy is zero there: they must not reach dW).  Accumulated
    into zeros; the fixed-order form twice is bit-identical."""
    from dupl_amd import ops
    for n_out in WGRAD_DIMS:
        for n_in in WGRAD_DIMS:
            o = _operands(tokens, n_out, n_in, more_rows)
            want = o["dy_r"].t() @ o["x_r"]
            c32 = ops.zeros((n_out, n_in), dev)
            ops.linear_wgrad(o["dy32"], o["x32"], c32, accumulate=True)
            e32 = _err(c32, want)
            outs = [_wgrad_single(o, ops.zeros((n_out, n_in), dev), det) for det in (0, 1, 1)]
            for det, c in zip((0, 1), outs):
                e16 = _err(c, want)
                print(f"wgrad {n_out}x{n_in}x{tokens} det={det}: f16x3 {e16:.2e}  f32 {e32:.2e}")
                assert e16 <= 2.0 * e32 + 2e-7, (n_out, n_in, det)
            assert torch.equal(outs[1], outs[2]), "the fixed-order weight gradient must be bit-reproducible"


GROUP = ((8, 264), (136, 136), (264, 8), (264, 264))


@pytest.mark.parametrize("more_rows", [False, True], ids=["exact", "more"])
@pytest.mark.parametrize("tokens", [1, 31, 33, 97])
def test_wgrad_grouped(dev, tokens, more_rows):
    """Four problems as one grouped launch: the fp64 bar, bit-identical to the four launched singly in deterministic mode (the same
    whole-tile walk over all of K), and the OVERWRITE form (DUPL_GEMM_C_FRESH) into NaN-filled C bit-identical to the accumulating
    form into zeros -- also with only some problems of the group fresh."""
    from dupl_amd import ops
    os_ = [_operands(tokens, n_out, n_in, more_rows) for n_out, n_in in GROUP]

    def group(cs, fresh=None):
        ops.wgrad16_group([(o["dy16"], o["x16"], c, o["alpha"]) for o, c in zip(os_, cs)], fresh=fresh)
        return cs

    acc = group([ops.zeros(s, dev) for s in GROUP])
    for (n_out, n_in), o, c in zip(GROUP, os_, acc):
        want = o["dy_r"].t() @ o["x_r"]
        c32 = ops.zeros((n_out, n_in), dev)
        ops.linear_wgrad(o["dy32"], o["x32"], c32, accumulate=True)
        e16, e32 = _err(c, want), _err(c32, want)
        print(f"grouped wgrad {n_out}x{n_in}x{tokens}: f16x3 {e16:.2e}  f32 {e32:.2e}")
        assert e16 <= 2.0 * e32 + 2e-7, (n_out, n_in)
        assert torch.equal(c, _wgrad_single(o, ops.zeros((n_out, n_in), dev), 1)), (n_out, n_in)
    nan = lambda s: torch.full(s, float("nan"), device=dev)
    over = group([nan(s) for s in GROUP], fresh=[True] * 4)
    mixed = group([nan(s) if f else ops.zeros(s, dev) for s, f in zip(GROUP, (True, False, False, True))], fresh=[True, False, False, True])
    for c, a, m in zip(over, acc, mixed):
        assert torch.equal(c.view(torch.int32), a.view(torch.int32)) and torch.equal(m.view(torch.int32), a.view(torch.int32))
    # a fresh C is not read: the accumulating form on top of it doubles the values exactly
    twice = group(over)
    for c, a in zip(twice, acc):
        assert torch.equal(c, 2.0 * a)


def test_fill_ranges(dev):
    """dupl_fill_ranges: every listed range and nothing else -- unaligned ends, an empty range, ranges shorter than a float4."""
    from dupl_amd import ops
    n = 70001
    t = torch.full((n + 3,), 7.0, device=dev)[3:]          # (a base that is 4-byte, not 16-byte, aligned)
    rows = [(0, 1), (5, 5), (6, 9), (17, 4099), (4101, 4102), (30000, 70001)]
    ops.fill_ranges_(t, torch.tensor(rows, dtype=torch.int64).to(dev), 0.0)
    want = torch.full((n,), 7.0)
    for lo, hi in rows:
        want[lo:hi] = 0.0
    assert torch.equal(t.cpu(), want)
    ops.fill_ranges_(t, torch.empty((0, 2), dtype=torch.int64, device=dev), 3.0)      # an empty table (no address): nothing is written
    assert torch.equal(t.cpu(), want)


# ------------------------------------------------------------------------------------------ lazily zeroed gradient ranges
def _tiny_model(dev):
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.utils.optimizer import PolyWarmupAdamW
    from oracle import dupl_oracle as O
    model = siamese_network("tiny_test", num_classes=21, pretrained=False, aux_layer=-3)
    model.load_state_dict(O.make_siamese_params(O.VIT_TINY, 21, seed=5), strict=True)
    model.to(dev)
    model.enable_dual_stream(True)
    g = model.get_param_groups()
    opt = PolyWarmupAdamW(params=[{"params": g[i], "lr": 6e-5 * (1 if i < 2 else 10), "weight_decay": 0.01} for i in range(4)],
                          lr=6e-5, weight_decay=0.01, betas=(0.9, 0.999), warmup_iter=3, max_iter=20, warmup_ratio=1e-6,
                          power=0.9).bind(model.flat_storage)
    return model, opt


@pytest.fixture(scope="module")
def tiny(dev):
    """A tiny two-student model with its optimiser and one phase-B batch; backward(n) = n forward + backward passes in deterministic
    mode (the only mode in which two runs agree bit for bit).  The tests below change its gradients only, never its parameters."""
    import types
    from dupl_amd import ops, trainer
    from dupl_amd.model.PAR import PAR
    from oracle import dupl_oracle as O
    model, opt = _tiny_model(dev)
    par = PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]).to(dev)
    inputs, cls_label, img_box = O.synthetic_batch(3, 20, 128, seed=11)
    inputs, cls_dev = inputs.to(dev), cls_label.to(dev)
    store = model.flat_storage

    def backward(n=1):
        ops.set_deterministic(1)
        try:
            for _ in range(n):
                loss, _ = trainer.compute_losses(model, par, inputs, cls_dev, img_box, 5000, trainer.StepArgs(), cls_label_host=cls_label)
                loss.sum().backward()
        finally:
            ops.set_deterministic(0)
        store.wait_streams()
        torch.cuda.synchronize()

    def lazy_zero():
        store.grad.fill_(float("nan"))        # whatever a lazy range holds must not reach a gradient
        opt.zero_grad(lazy=True)

    t = types.SimpleNamespace(model=model, opt=opt, store=store, backward=backward, lazy_zero=lazy_zero)
    opt.zero_grad()
    backward()
    t.eager = store.grad.clone()              # the eager path's gradients, shared by the tests below
    assert bool(torch.isfinite(t.eager).all())
    return t


def _lazy_ranges(store):
    return [store._abs_range(s, k) for s in range(store.n_students) for k in store.lazy_keys()]


def test_lazy_zero_grad_gives_the_eager_gradients(tiny):
    st = tiny.store
    assert len(st.lazy_keys()) == 4 * st.cfg.depth
    tiny.lazy_zero()
    assert len(st._fresh) == 2 * 4 * st.cfg.depth
    lo, hi = _lazy_ranges(st)[0]
    assert bool(torch.isnan(st.grad[lo:hi]).all()) and float(st.grad[:lo].abs().max()) == 0.0
    tiny.backward()
    assert not st._fresh, "every block Linear weight receives its gradient from the grouped launch"
    assert torch.equal(st.grad.view(torch.int32), tiny.eager.view(torch.int32))


def test_second_backward_without_zero_grad_accumulates(tiny):
    st = tiny.store
    tiny.lazy_zero()
    tiny.backward(2)
    for lo, hi in _lazy_ranges(st):
        assert torch.equal(st.grad[lo:hi], 2.0 * tiny.eager[lo:hi])


def test_lazy_range_written_by_the_f32_route(tiny):
    """A site on the exact-f32 kernels accumulates: it fills its fresh range first.  Lazy and eager zeroing agree bit for bit."""
    from dupl_amd import engine
    st = tiny.store
    mode = engine.GEMM_MODE
    engine.set_gemm_mode("f32")
    try:
        tiny.opt.zero_grad()
        tiny.backward()
        eager = st.grad.clone()
        tiny.lazy_zero()
        tiny.backward()
    finally:
        engine.set_gemm_mode(mode)
    assert not st._fresh and bool(torch.isfinite(eager).all())
    assert torch.equal(st.grad.view(torch.int32), eager.view(torch.int32))


def test_step_without_a_backward_settles_fresh_ranges(dev):
    model, opt = _tiny_model(dev)
    st = model.flat_storage
    before = st.data.clone()
    st.grad.fill_(float("nan"))
    opt.zero_grad(lazy=True)
    assert st._fresh
    opt.step()
    torch.cuda.synchronize()
    assert not st._fresh
    assert float(st.grad.abs().max()) == 0.0 and torch.equal(st.data, before)      # (no segment has a gradient: nothing is updated)
    # a plain zero_grad() is the full fill and leaves nothing fresh: the .grad views may be written by hand next
    st.grad.fill_(float("nan"))
    opt.zero_grad(lazy=True)
    opt.zero_grad()
    assert not st._fresh and float(st.grad.abs().max()) == 0.0
