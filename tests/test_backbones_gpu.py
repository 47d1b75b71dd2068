"""-m gpu: the backbone family (DeiT-T/S, ViT-B at 384, ViT-L) on the hot path.

* forward of four members against the REFERENCE's outputs (tests/golden/<name>_fwd.npz, tools/gen_backbone_golden.py), both GEMM modes;
* a whole phase-B step of reduced-depth members (widths 192 / 384 / 1024, a 24 x 24 position grid) against the CPU oracle, every
  gradient tensor, both GEMM modes;
* each kernel family that sees the width, the number of heads or the depth, launch by launch against float64 at the shapes the
  family produces, with the bar of that kernel's existing test and every output inside a sentinel-guarded buffer;
* deterministic mode, the range guard's verdicts at width 1024, and the checkpoint loader.

The weights of the forward test are oracle.make_student_params(cfg, 21, seed=11), what the fixtures were written with; generating
the 304 M of ViT-L takes the host most of a minute, once for both GEMM modes."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from kernel_guard import Guard, Tally, nan_in, same_bits
from parity_util import assert_labels_equal_up_to_ties, head_decisions, oracle_pool_decisions, oracle_relu_masks

pytestmark = pytest.mark.gpu

TOL_FWD = 2e-4          # of the tensor's max-abs: the bar of test_vitb_forward_matches_reference
NC = 21
FWD_NAMES = ("deit_tiny_patch16_224", "deit_small_patch16_224", "vit_base_patch16_384", "vit_large_patch16_224")
WIDTHS = {192: 3, 384: 6, 1024: 16}                      # embed dim -> heads (head dim 64)
ROWS = (2 * 197, 2 * 37)                                 # ragged token counts: two images at 224^2 and at 96^2
GEMM_ROWS = ROWS + (4 * 785,)                            # and the step's own: 4 images at 448^2, where the launchers pick tile and split
HD = 64
SCALE = HD ** -0.5


@pytest.fixture
def gemm_mode(request):
    from dupl_amd import engine
    prev = engine.GEMM_MODE
    engine.set_gemm_mode(request.param)
    yield request.param
    engine.set_gemm_mode(prev)


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _oracle_cfg(cfg):
    from oracle import dupl_oracle as O
    return O.ViTConfig(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, patch=cfg.patch,
                       img_size=cfg.img_size, aux_layer=cfg.aux_layer, ln_eps=cfg.ln_eps, head_classes=cfg.head_classes)


# ================================================================================================ forward against the reference
@functools.lru_cache(maxsize=1)
def _golden_student(name):
    """The named student with the fixture's weights, on the device (one at a time: ViT-L is 1.2 GB)."""
    from dupl_amd.model.backbone import encoder_config
    from dupl_amd.model.model_dupl import network
    from oracle import dupl_oracle as O
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    net = network(name, num_classes=NC, pretrained=False, aux_layer=-3)
    net.load_state_dict(O.make_student_params(_oracle_cfg(encoder_config(name)), NC, seed=11), strict=True)
    return net.to(torch.device("cuda", 0))


@pytest.mark.parametrize("gemm_mode", ["f16x3", "f32"], indirect=True)
@pytest.mark.parametrize("name", FWD_NAMES)
def test_forward_matches_reference(dev, golden_dir, name, gemm_mode):
    from oracle import dupl_oracle as O
    g = np.load(os.path.join(golden_dir, name + "_fwd.npz"))
    net = _golden_student(name)
    xb, _, _ = O.synthetic_batch(2, 20, 224, seed=12)
    with torch.no_grad():
        cls, seg, x4, cls_aux = net(xb.to(dev))
        cam_aux, cam = net(xb.to(dev), cam_only=True)
    got = dict(cls=cls, seg=seg, x4_sub=x4[:, ::16], cls_aux=cls_aux, cam_aux=cam_aux, cam=cam)
    errs = {k: relerr(t, g[k]) for k, t in got.items()}
    print(f"{name} [{gemm_mode}] forward vs reference:", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, t in got.items():
        assert tuple(t.shape) == g[k].shape and errs[k] < TOL_FWD, (k, errs[k])
    if gemm_mode == "f16x3":
        s = net._store.guard.summary()
        assert s["sites_on_f32"] == 0, s


# ================================================================================================ whole step against the oracle
STEP_CONFIGS = {"192x3": dict(embed_dim=192, num_heads=3), "384x6": dict(embed_dim=384, num_heads=6),
                "1024x16": dict(embed_dim=1024, num_heads=16), "384x6-grid24": dict(embed_dim=384, num_heads=6, img_size=384)}


def _step_cfg(tag):
    from dupl_amd.engine import EncoderConfig
    return EncoderConfig(depth=4, **STEP_CONFIGS[tag])          # aux_layer = -3 needs at least 3 blocks


@functools.lru_cache(maxsize=None)
def _step_case(tag):
    """Weights, inputs and the oracle's step (losses, CAMs, labels, every gradient): computed once per configuration, read-only."""
    from oracle import dupl_oracle as O
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    ocfg = _oracle_cfg(_step_cfg(tag))
    pp = O.make_siamese_params(ocfg, NC, seed=3)
    inputs, cls_label, img_box = O.synthetic_batch(2, NC - 1, 96, seed=61)
    frozen = ("encoder.pos_embed", "encoder.head.weight", "encoder.head.bias")
    watch = [k for k in pp if k.split(".", 1)[1] not in frozen]
    leaf = {k: v.clone().requires_grad_(k in watch) for k, v in pp.items()}
    ref_loss, pc = O.train_step_losses(leaf, inputs, cls_label, img_box, 5000, ocfg, O.StepArgs())
    ref_loss.sum().backward()
    grads = {k: leaf[k].grad for k in watch}
    assert all(g is not None for g in grads.values())
    pc = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in pc.items()}
    return dict(ocfg=ocfg, pp=pp, inputs=inputs, cls_label=cls_label, img_box=img_box, watch=watch, grads=grads, pc=pc)


def _run_step(dev, tag, pp, inputs, cls_label, img_box):
    from dupl_amd import trainer
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.model.PAR import PAR
    model = siamese_network(_step_cfg(tag), num_classes=NC, pretrained=False, aux_layer=-3)
    model.load_state_dict(pp, strict=True)
    model.to(dev)
    model.enable_dual_stream(True)
    par = PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]).to(dev)

    def step():
        model.flat_storage.grad.zero_()
        loss, out = trainer.compute_losses(model, par, inputs.to(dev), cls_label.to(dev), img_box, 5000, trainer.StepArgs(),
                                           cls_label_host=cls_label)
        loss.sum().backward()
        model.flat_storage.wait_streams()
        torch.cuda.synchronize()
        return loss, out

    return model, step


def _grad(model, k):
    return model.flat_storage.view(0 if k.startswith("branch1.") else 1, k.split(".", 1)[1], grad=True).cpu()


@pytest.mark.parametrize("gemm_mode", ["f16x3", "f32"], indirect=True)
@pytest.mark.parametrize("tag", list(STEP_CONFIGS))
def test_reduced_depth_step_vs_oracle(dev, tag, gemm_mode):
    """The form of test_ragged_shapes_step_vs_oracle (2 images of 96 x 96, two streams, phase B) on family members at depth 4, with
    its bars -- losses 1e-4 max(1, |ref|), CAMs 1e-4, pseudo labels equal, refined labels equal up to proven ties -- and ALL gradient
    tensors through the comparison of test_full_size_vitb_step_vs_oracle: 2e-4 of the tensor's max on f16x3, 5e-4 on the exact-f32
    kernels, after the proven LargeFOV ReLU / global-max-pool decisions of the product are imposed on the oracle."""
    from oracle import dupl_oracle as O
    c = _step_case(tag)
    pp, pc, inputs, cls_label, img_box, watch = c["pp"], c["pc"], c["inputs"], c["cls_label"], c["img_box"], c["watch"]
    model, step = _run_step(dev, tag, pp, inputs, cls_label, img_box)
    loss, out = step()
    for k in ("loss", "cls_loss", "ptc_loss", "seg_loss", "sim_loss"):
        got, ref = float(out[k].reshape(-1)[0].item()), float(pc[k].reshape(-1)[0].item())
        print(f"{tag} [{gemm_mode}] {k}: oracle {ref:.6f} got {got:.6f}")
        assert abs(got - ref) <= 1e-4 * max(1.0, abs(ref)), (k, got, ref)
    for k in ("cams_1", "cams_aux_1", "cams_2", "cams_aux_2"):
        d = float((out[k].cpu() - pc[k]).abs().max())
        print(f"{tag} [{gemm_mode}] {k}: max-abs-diff {d:.2e}")
        assert d < 1e-4, k
    for k in ("pseudo_label_aux_1", "pseudo_label_aux_2"):
        assert torch.equal(out[k].cpu().long(), pc[k].long()), k
    for k in ("refined_1", "refined_2"):
        assert_labels_equal_up_to_ties(out[k], pc[k], pc["refined_margin_" + k[-1]], f"{tag} {k}", max_frac=1e-3)
    bar = 2e-4 if gemm_mode == "f16x3" else 5e-4
    errs = {k: float((_grad(model, k) - c["grads"][k]).abs().max() / c["grads"][k].abs().max().clamp_min(1e-30)) for k in watch}
    order = sorted(errs, key=errs.get)
    print(f"{tag} [{gemm_mode}] gradients: {len(errs)} tensors, median rel err {errs[order[len(order) // 2]]:.2e}, worst "
          f"{errs[order[-1]]:.2e} ({order[-1]}), bar {bar:.0e}")
    if any(not errs[k] < bar for k in order):
        # decisions at round-off level (a LargeFOV ReLU, the arg-max of a global max pool) may fall either way in two fp32
        # implementations: accepted only with proof, as in test_full_size_vitb_step_vs_oracle
        flips, masks, pools = head_decisions(model, pp, pc, inputs.to(dev))
        nflip = 0
        for br, (n6, n7, worst) in flips.items():
            print(f"{tag} {br} ReLU decisions that differ: conv6 {n6}, conv7 {n7}; largest |oracle pre-activation| {worst:.2e} of the layer max")
            assert worst < 1e-4, "a ReLU decision differs where the oracle's pre-activation is NOT at round-off level"
            nflip += n6 + n7
        leaf2 = {k: v.clone().requires_grad_(k in watch) for k, v in pp.items()}
        fh = inputs.shape[-1] // 16
        with oracle_relu_masks(masks) as used, oracle_pool_decisions(pools, fh * fh) as pst:
            ref2, _ = O.train_step_losses(leaf2, inputs, cls_label, img_box, 5000, c["ocfg"], O.StepArgs())
            ref2.sum().backward()
        assert used[0] == len(masks) and pst["used"] == len(pools) == 4
        print(f"{tag} pooling decisions that differ: {pst['flips']}; largest oracle margin {pst['worst_margin']:.2e} (bar 1e-5)")
        assert pst["worst_margin"] < 1e-5, "a pooling decision differs where the oracle's top-2 gap is NOT at round-off level"
        assert nflip + pst["flips"] > 0, "gradients above the bar without a single flipped decision"
        errs = {k: float((_grad(model, k) - leaf2[k].grad).abs().max() / leaf2[k].grad.abs().max().clamp_min(1e-30)) for k in watch}
        order = sorted(errs, key=errs.get)
        print(f"{tag} [{gemm_mode}] gradients with the product's decisions imposed: worst {errs[order[-1]]:.2e} ({order[-1]})")
    bad = [(k, errs[k]) for k in order if not errs[k] < bar]
    assert not bad, f"{len(bad)} gradient tensors above {bar:.0e}: {bad[:8]}"
    if gemm_mode == "f16x3" and tag == "1024x16":
        # sane weights (N(0, 0.02)): no site of the widest member is routed to the exact-f32 kernels
        guard = model.flat_storage.guard
        for s in (0, 1):
            sites = guard.sites(s)
            flat = [("patch", sites["patch"]), ("conv6", sites["conv6"]), ("conv7", sites["conv7"])]
            flat += [(f"blocks.{i}.{k}", v) for i, b in enumerate(sites["blocks"]) for k, v in b.items() if not k.endswith("_f1")]
            assert all(v is True or v == 1 for _, v in flat), [n for n, v in flat if not v]
        assert guard.summary()["sites_on_f32"] == 0, guard.summary()


def test_deterministic_mode_is_bit_reproducible_at_width_384(dev):
    """DUPL_DETERMINISTIC=1 (dupl_amd.set_deterministic): two identical steps of the 384 / 6 member give the same bits in every
    gradient and loss."""
    import dupl_amd
    c = _step_case("384x6")
    model, step = _run_step(dev, "384x6", c["pp"], c["inputs"], c["cls_label"], c["img_box"])
    dupl_amd.set_deterministic(True)
    try:
        l1, _ = step()
        l1, g1 = l1.detach().clone(), model.flat_storage.grad.clone()
        l2, _ = step()
        l2, g2 = l2.detach().clone(), model.flat_storage.grad.clone()
    finally:
        dupl_amd.set_deterministic(False)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    assert float(g1.abs().max()) > 0 and bool(torch.isfinite(g1).all())


def test_checkpoint_of_another_width_is_refused(dev):
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.tools import eval_seg
    small = siamese_network("deit_small_patch16_224", num_classes=NC, pretrained=False, aux_layer=-3)
    ckpt = {"module." + k: v.clone() for k, v in small.state_dict().items()}
    target = siamese_network("deit_small_patch16_224", num_classes=NC, pretrained=False, aux_layer=-3).to(dev)
    eval_seg.load_checkpoint(target, ckpt)
    assert all(torch.equal(v, target.state_dict()[k].cpu()) for k, v in small.state_dict().items())
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        assert bool(torch.isfinite(target(x, val=True)["branch1"][1]).all())
    base = siamese_network("deit_base_patch16_224", num_classes=NC, pretrained=False, aux_layer=-3).to(dev)
    with pytest.raises(ValueError, match="expected width 768.*found width 384"):
        eval_seg.load_checkpoint(base, ckpt)


# ================================================================================================ kernel sweep
def _pairs(D):
    """(n_out, n_in) of a block's four Linears: qkv, proj, fc1, fc2."""
    return [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)))


def _planes_nan(M, N, exp, dev):
    from dupl_amd import ops
    p = ops.split16_empty(M, N, dev, exp)
    p.planes.fill_(float("nan"))
    return p


@pytest.mark.parametrize("D", list(WIDTHS))
def test_forward_split_gemms_at_the_family_widths(dev, D):
    """Format 1 planes, both tiles the launcher can pick (18: 256 x 256, 22: 256 x 128) and its own choice (0), N in {D, 3D, 4D} and
    K in {D, 4D} (K = 192: six k-tiles), ragged M.  Bar of test_mfma16_tiles_are_fp32_equivalent: error vs float64 <= 2 x the exact-f32
    kernel's + 1e-7 for the result and the stored pre-activation, planes within 2^-21; the tiles agree bit for bit."""
    from dupl_amd import ops
    for N, K in _pairs(D):
        for M in GEMM_ROWS:
            g = _gen(M, N, K)
            x = torch.randn(M, K, generator=g).to(dev)
            W = (torch.randn(N, K, generator=g) * 0.05).to(dev)
            b = torch.randn(N, generator=g).to(dev)
            res = torch.randn(M, N, generator=g).to(dev)
            xs, Ws = ops.split16(nan_in(x, dev), exp=ops.EXP_ACT), ops.split16(nan_in(W, dev), exp=ops.EXP_W)
            ref = x.double() @ W.double().t() + b.double()
            want = F.gelu(ref) + res.double()
            sc = float(want.abs().max())
            pre32 = torch.empty(M, N, device=dev)
            y32 = ops.linear(x, W, b, gelu=True, res=res, store_pre=pre32)
            e32 = float((y32.double() - want).abs().max()) / sc
            e32p = float((pre32.double() - ref).abs().max()) / float(ref.abs().max())
            outs = {}
            for tile in (18, 22, 0):
                y, pre, y16 = Guard((M, N), dev), Guard((M, N), dev), _planes_nan(M, N, ops.EXP_ACT, dev)
                ops.GEMM16_TUNING["tile"] = tile
                try:
                    ops.linear16(xs, Ws, nan_in(b, dev), gelu=True, res=nan_in(res, dev), store_pre=pre.view, out=y.view, out16=y16)
                finally:
                    ops.GEMM16_TUNING["tile"] = 0
                yc, prec = y.cpu().to(dev), pre.cpu().to(dev)
                e16 = float((yc.double() - want).abs().max()) / sc
                e16p = float((prec.double() - ref).abs().max()) / float(ref.abs().max())
                print(f"fwd {M}x{N}x{K} tile {tile}: f16x3 {e16:.2e} (pre {e16p:.2e})  f32 {e32:.2e} (pre {e32p:.2e})")
                assert e16 <= 2.0 * e32 + 1e-7 and e16p <= 2.0 * e32 + 1e-7, (M, N, K, tile)
                rec = (y16.planes[0].float() + y16.planes[1].float()) / 2.0 ** ops.EXP_ACT
                assert float((rec - yc).abs().max()) <= 2.0 ** -21 * sc
                outs[tile] = (yc, prec, y16.planes)
            for t in (22, 0):
                assert all(torch.equal(a, b_) for a, b_ in zip(outs[18], outs[t])), (M, N, K, t)


@pytest.mark.parametrize("D", list(WIDTHS))
def test_kmajor_backward_gemms_at_the_family_widths(dev, D):
    """The k-major data gradients (GELU' epilogue, and the stream-K form into a zero-filled dx: at n_out = 192 its contraction has six
    k-tiles) and weight gradients (atomics and fixed order) of the four Linears, ragged token counts.  Bars of
    test_kmajor_backward_gemms_are_fp32_equivalent: <= 2 x the exact-f32 kernels' error + 2e-7 (+ 2.5e-10 per token in fixed order).
    At the step's 3 140 tokens the fixed-order weight gradient is held to 2 x the exact-f32 kernel's error IN DETERMINISTIC MODE + 2e-7
    instead: that run has the same single fp32 accumulator chain over all tokens (test_grouped_weight_gradients compares the same
    launch form that way), while the f32 kernel's default split-K cuts the token axis the deeper the fewer output tiles there are --
    at 192 / 384 columns into pieces so short that its error (2.5e-7 - 2.7e-7 measured) says nothing about a 3 140-term chain.  Against
    the split-K figure the per-token allowance, fitted at 768 columns, was missed at 192 <- 192 (1.68e-6, bar 1.53e-6) and 384 <- 384
    (1.53e-6, bar 1.49e-6); at 768 columns the same kernel gives the same 1.2e-6 - 1.6e-6 and passes only on the comparator's larger error."""
    from dupl_amd import ops
    for n_out, n_in in _pairs(D):
        for tokens in GEMM_ROWS:
            g = _gen(tokens, n_out, n_in)
            dy = (torch.randn(tokens, n_out, generator=g) * 2e-5 * (1.0 + 5.0 * (torch.rand(tokens, 1, generator=g) > 0.97))).to(dev)
            x_all = torch.randn(tokens + 77, n_in, generator=g).to(dev)
            x = x_all[:tokens]
            W = (torch.randn(n_out, n_in, generator=g) * 0.03).to(dev)
            pre = torch.randn(tokens, n_in, generator=g).to(dev)
            x16, W16 = ops.split16(x_all, exp=ops.EXP_ACT), ops.split16(nan_in(W, dev), exp=ops.EXP_W)
            Kp = max(96, (tokens + 31) // 32 * 32)
            dy16, _, alpha = ops.split_prepare(dy, scaled=True, want_rm=True, want_T=False, fmt1=True, rm_rows=Kp)
            tag = f"{tokens} tokens {n_out}<-{n_in}"
            # ---- data gradient through GELU'
            dx = Guard((tokens, n_in), dev)
            ops.linear16(dy16.rows_slice(0, tokens), W16, alpha=alpha, dgelu_of=nan_in(pre, dev), b_kmajor=True, out=dx.view)
            pd = pre.double()
            want = (dy.double() @ W.double()) * (0.5 * (1 + torch.erf(pd / 2 ** 0.5)) + pd * torch.exp(-0.5 * pd ** 2) / (2 * torch.pi) ** 0.5)
            dx32 = ops.linear_dgrad(dy, W, dgelu_of=pre)
            sc = float(want.abs().max())
            e16, e32 = float((dx.cpu().to(dev).double() - want).abs().max()) / sc, float((dx32.double() - want).abs().max()) / sc
            print(f"k-major dgrad {tag}: f16x3 {e16:.2e}  f32 {e32:.2e}")
            assert e16 <= 2.0 * e32 + 2e-7, tag
            # ---- stream-K data gradient (linear epilogue, fp32 atomics onto zeros), with the launcher's slice choice
            dxs = Guard((tokens, n_in), dev, init=torch.zeros(tokens, n_in))
            ops.linear16(dy16.rows_slice(0, tokens), W16, out=dxs.view, accumulate=True, alpha=alpha, b_kmajor=True)
            wantp = dy.double() @ W.double()
            dxp32 = ops.linear_dgrad(dy, W)
            scp = float(wantp.abs().max())
            es, ep32 = float((dxs.cpu().to(dev).double() - wantp).abs().max()) / scp, float((dxp32.double() - wantp).abs().max()) / scp
            print(f"k-major stream-K dgrad {tag}: f16x3 {es:.2e}  f32 {ep32:.2e}")
            assert es <= 2.0 * ep32 + 2e-7, tag
            # ---- weight gradient onto existing values
            c0 = torch.randn(n_out, n_in, generator=g) * 1e-4
            wantw = c0.to(dev).double() + dy.double().t() @ x.double()
            scw = float(wantw.abs().max())
            gw32 = c0.to(dev)
            ops.linear_wgrad(dy, x, gw32, accumulate=True)
            e32w = float((gw32.double() - wantw).abs().max()) / scw
            gw32d = c0.to(dev)
            ops.set_deterministic(1)
            try:
                ops.linear_wgrad(dy, x, gw32d, accumulate=True)
            finally:
                ops.set_deterministic(0)
            e32wd = float((gw32d.double() - wantw).abs().max()) / scw
            fixed = []
            for det in (0, 1, 1):
                gw = Guard((n_out, n_in), dev, init=c0)
                ops.set_deterministic(det)
                try:
                    ops.linear16(dy16, x16, out=gw.view, accumulate=True, alpha=alpha, a_kmajor=True, b_kmajor=True, k_pad=Kp)
                finally:
                    ops.set_deterministic(0)
                got = gw.cpu()
                e = float((got.to(dev).double() - wantw).abs().max()) / scw
                print(f"k-major wgrad {tag} det={det}: f16x3 {e:.2e}  f32 {e32w:.2e}  f32 in fixed order {e32wd:.2e}")
                if det and tokens not in ROWS:
                    assert e <= 2.0 * e32wd + 2e-7, (tag, det)
                else:
                    assert e <= 2.0 * e32w + 2e-7 + (2.5e-10 * tokens if det else 0.0), (tag, det)
                if det:
                    fixed.append(got)
            assert same_bits(fixed[0], fixed[1]), "the fixed-order weight gradient must be bit-reproducible"


@pytest.mark.parametrize("tokens", GEMM_ROWS)
@pytest.mark.parametrize("D", list(WIDTHS))
def test_grouped_weight_gradients_at_the_family_widths(dev, D, tokens):
    """The four weight gradients of a block as one grouped launch.  Bar of test_grouped_weight_gradients: no further from float64 than
    the exact-f32 kernel in deterministic mode + 2e-7; the launch is bit-reproducible, in deterministic mode too."""
    from dupl_amd import ops
    g = _gen(tokens, D)
    Kp = max(96, (tokens + 31) // 32 * 32)
    items, refs, c0s, f32s, keep = [], [], [], [], []
    for n_out, n_in in _pairs(D):
        dy = (torch.randn(tokens, n_out, generator=g) * 3e-5).to(dev)
        x = torch.randn(tokens + 5, n_in, generator=g).to(dev)
        c0 = torch.randn(n_out, n_in, generator=g) * 1e-4
        dy16, _, alpha = ops.split_prepare(dy, scaled=True, want_rm=True, want_T=False, fmt1=True, rm_rows=Kp)
        x16 = ops.split16(x, exp=ops.EXP_ACT)
        keep.append((dy, x, dy16, x16))
        items.append((dy16, x16, alpha))
        c0s.append(c0)
        refs.append(c0.to(dev).double() + dy.double().t() @ x[:tokens].double())
        c32 = c0.to(dev)
        ops.set_deterministic(1)
        try:
            ops.linear_wgrad(dy, x[:tokens], c32, accumulate=True)
        finally:
            ops.set_deterministic(0)
        f32s.append(c32)
    outs = []
    for rep in range(3):
        cs = [Guard(tuple(c.shape), dev, init=c) for c in c0s]
        ops.set_deterministic(int(rep == 2))
        try:
            ops.wgrad16_group([(dy16, x16, c.view, alpha) for (dy16, x16, alpha), c in zip(items, cs)])
        finally:
            ops.set_deterministic(0)
        outs.append([c.cpu() for c in cs])
    for i, ref in enumerate(refs):
        sc = float(ref.abs().max())
        e16 = float((outs[0][i].to(dev).double() - ref).abs().max()) / sc
        e32 = float((f32s[i].double() - ref).abs().max()) / sc
        print(f"grouped wgrad {tuple(ref.shape)} x {tokens}: f16x3 {e16:.2e}  f32 {e32:.2e}")
        assert e16 <= e32 + 2e-7, (D, tokens, i)
        assert same_bits(outs[0][i], outs[1][i]) and same_bits(outs[0][i], outs[2][i]), "the grouped launch must be bit-reproducible"


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("D", list(WIDTHS))
def test_layernorm_at_the_family_widths(dev, D, rows):
    """layernorm_fwd16 (fp32 out, mean, rstd and the planes in both formats) and layernorm_bwd (atomics and fixed order, with the
    residual gradient) against float64 with the row-wise bounds of test_layernorm_fwd_edges / test_layernorm_bwd_edges.  D = 192 runs
    on one float4 chunk per lane with a quarter of the lanes idle, D = 384 on the three-chunk instantiation with the third masked."""
    from dupl_amd import ops
    from kernel_guard import stream
    L = ops.L()
    eps = 1e-6
    T = Tally(f"ln {rows}x{D}")
    x, gamma, beta = R.ln_inputs(rows, D, rows * 7919 + D)
    ref = R.ln_fwd_ref(x, gamma, beta, eps)
    xd, gd, bd = nan_in(x, dev), nan_in(gamma, dev), nan_in(beta, dev)
    for e in (0, ops.EXP_ACT):
        y, m, r = Guard((rows, D), dev), Guard((rows,), dev), Guard((rows,), dev)
        planes = torch.full((2, rows + 2, D), -1234.0, dtype=torch.float16, device=dev)
        L.dupl_layernorm_fwd16(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.ptr, planes[0, 1].data_ptr(), planes[1, 1].data_ptr(),
                               m.ptr, r.ptr, rows, D, eps, 0, e, stream())
        y0, m0, r0 = y.cpu(), m.cpu(), r.cpu()
        T.add(f"y exp{e}", (y0.double() - ref.y).abs(), ref.y_bound)
        T.add(f"mean exp{e}", (m0.double() - ref.mean).abs(), ref.mean_bound)
        T.add(f"rstd exp{e}", (r0.double() - ref.rstd).abs(), ref.rstd_bound)
        p = planes.cpu()
        assert bool((p[:, 0] == -1234.0).all()) and bool((p[:, -1] == -1234.0).all()), "the kernel wrote outside its planes"
        assert same_bits(p[:, 1:-1].contiguous(), ops.split16(y.view, exp=e).planes.cpu()), f"planes exp {e}"
    # ---- backward
    xb, gb, dy, dres = R.ln_bwd_inputs(rows, D, rows * 7919 + D)
    xbd, gbd, dresd = nan_in(xb, dev), nan_in(gb, dev), nan_in(dres, dev)
    m, r, yb = Guard((rows,), dev), Guard((rows,), dev), Guard((rows, D), dev)
    L.dupl_layernorm_fwd(xbd.data_ptr(), gbd.data_ptr(), nan_in(torch.zeros(D), dev).data_ptr(), yb.ptr, m.ptr, r.ptr, rows, D, eps, stream())
    mean, rstd = m.cpu(), r.cpu()
    dg0, db0 = torch.randn(D, generator=_gen(D, 21)) * 0.5, torch.randn(D, generator=_gen(D, 22)) * 0.5
    bref = R.ln_bwd_ref(dy, xb, gb, mean, rstd, dres, dg0, db0)
    fixed = []
    for det in (0, 1, 1):
        dyg, dx = Guard((rows, D), dev, init=dy), Guard((rows, D), dev)
        dg, db = Guard((D,), dev, init=dg0), Guard((D,), dev, init=db0)
        L.dupl_layernorm_bwd(dyg.ptr, xbd.data_ptr(), gbd.data_ptr(), m.ptr, r.ptr, dresd.data_ptr(), dx.ptr, dg.ptr, db.ptr, rows, D,
                             None, None, 0, 0, None, det, stream())
        got = (dx.cpu(), dg.cpu(), db.cpu())
        assert same_bits(dyg.cpu(), dy), "dy is an input"
        T.add(f"dx det{det}", (got[0].double() - bref.dx).abs(), bref.dx_bound)
        T.add(f"dgamma det{det}", (got[1].double() - bref.dgamma).abs(), bref.dgamma_bound)
        T.add(f"dbeta det{det}", (got[2].double() - bref.dbeta).abs(), bref.dbeta_bound)
        if det:
            fixed.append(got)
    assert all(same_bits(a, b) for a, b in zip(*fixed)), "deterministic LayerNorm backward must be bit-reproducible"
    T.done()


def _ref64(qkv, B, N, H, dout=None):
    x = qkv.double().clone().requires_grad_(dout is not None)
    q, k, v = (x.view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)[i] for i in range(3))
    att = (q @ k.transpose(-1, -2)) * SCALE
    out = (att.softmax(-1) @ v).transpose(1, 2).reshape(B * N, H * HD)
    lse = torch.logsumexp(att, dim=-1)
    if dout is not None:
        out.backward(dout.double())
    return out.detach(), lse.detach(), x.grad


@pytest.mark.parametrize("N", [197, 37])
@pytest.mark.parametrize("H", list(WIDTHS.values()))
def test_split_attention_at_the_family_head_counts(dev, H, N):
    """attention_fwd16 and attention_bwd16 at H = 3, 6, 16 (B H ceil(N / 128) = 6 .. 64 blocks: far below the chip at H = 3, a
    remainder in the XCD deal), bars of test_fwd16_shape_sweep / test_bwd16_shape_sweep: out <= 2 x the exact-f32 kernel's error +
    2e-7, lse 2 x + 1e-6, planes 2^-21 of the maximum in both formats, dq / dk / dv 2 x + 5e-7."""
    from dupl_amd import ops
    B, D = 2, H * HD
    g = _gen(B, N, H)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.3).to(dev)
    dout = (torch.randn(B * N, D, generator=g) * 2e-5).to(dev)
    ref, ref_lse, ref_g = _ref64(qkv, B, N, H, dout)
    o32, lse32 = ops.attention_fwd(qkv, B, N, H, HD, SCALE, need_lse=True)
    d32 = ops.attention_bwd(qkv, o32, dout, lse32, B, N, H, HD, SCALE)
    qkv16 = ops.split16(nan_in(qkv, dev))
    out = Guard((B * N, D), dev)
    o0 = _planes_nan(B * N, D, 0, dev)
    lse = ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, need_lse=True, out=out.view, out16=o0)
    outc = out.cpu().to(dev)
    sc = float(ref.abs().max())
    e16, e32 = float((outc.double() - ref).abs().max()) / sc, float((o32.double() - ref).abs().max()) / sc
    l16, l32 = float((lse.double() - ref_lse).abs().max()), float((lse32.double() - ref_lse).abs().max())
    print(f"attention H{H} N{N}: out f16x3 {e16:.2e} f32 {e32:.2e}; lse f16x3 {l16:.2e} f32 {l32:.2e}")
    assert bool(torch.isfinite(lse).all()) and e16 <= 2.0 * e32 + 2e-7 and l16 <= 2.0 * l32 + 1e-6
    assert float((o0.planes[0].float() + o0.planes[1].float() / 2048.0 - outc).abs().max()) <= 2.0 ** -21 * sc
    o1 = _planes_nan(B * N, D, ops.EXP_ACT, dev)
    ops.attention_fwd16(qkv16, B, N, H, HD, SCALE, out16=o1)
    assert float(((o1.planes[0].float() + o1.planes[1].float()) / 2.0 ** ops.EXP_ACT - outc).abs().max()) <= 2.0 ** -21 * sc
    d16 = ops.attention_bwd16(qkv16, outc, dout, lse, B, N, H, HD, SCALE)
    assert bool(torch.isfinite(d16).all())
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        s_ = float(ref_g[:, sl].abs().max())
        b16 = float((d16[:, sl].double() - ref_g[:, sl]).abs().max()) / s_
        b32 = float((d32[:, sl].double() - ref_g[:, sl]).abs().max()) / s_
        print(f"attention H{H} N{N} {name}: f16x3 {b16:.2e} f32 {b32:.2e}")
        assert b16 <= 2.0 * b32 + 5e-7, name


@pytest.mark.parametrize("H", list(WIDTHS.values()))
def test_segmented_attention_at_the_family_head_counts(dev, H):
    """attention_fwd16_segs over [2 x 197 with fp32 out + lse of the first image | 2 x 37 | 1 x 401] (4 H, 2 H and 4 H blocks: no
    multiple of 8 at H = 3): bit-identical to one attention_fwd16 per batch, planes of every segment within the forward bar
    (+ 2^-21) of float64, rows between the segments untouched."""
    from dupl_amd import ops
    D = H * HD
    segs = [(0, 2, 197, True, True, 1), (394 + 16, 2, 37, False, False, 0), (394 + 16 + 74 + 16, 1, 401, False, False, 0)]
    rows = segs[-1][0] + 401 + 16
    qkv = (torch.randn(rows, 3 * D, generator=_gen(rows, H)) * 1.5).to(dev)
    qkv16 = ops.split16(qkv)
    s16, r16 = _planes_nan(rows, D, 0, dev), _planes_nan(rows, D, 0, dev)
    outs = [Guard(((bf or B) * N, D), dev) if want else None for (_, B, N, want, _, bf) in segs]
    lses = ops.attention_fwd16_segs(qkv16, [(r0, B, N, outs[i].view if outs[i] else None, nl, bf) for i, (r0, B, N, _, nl, bf) in enumerate(segs)],
                                    H, HD, SCALE, out16=s16)
    used = torch.zeros(rows, dtype=torch.bool)
    for i, (r0, B, N, want, nl, bf) in enumerate(segs):
        used[r0:r0 + B * N] = True
        o = Guard(((bf or B) * N, D), dev) if want else None
        lse = ops.attention_fwd16(qkv16.rows_slice(r0, r0 + B * N), B, N, H, HD, SCALE, need_lse=nl, out=o.view if o else None,
                                  out16=r16.rows_slice(r0, r0 + B * N), b_f32=bf)
        if want:
            assert same_bits(outs[i].cpu(), o.cpu()) and same_bits(lses[i].cpu(), lse.cpu()), f"segment {i}"
        xs = qkv[r0:r0 + B * N].contiguous()
        ref, _, _ = _ref64(xs, B, N, H)
        o32 = ops.attention_fwd(xs, B, N, H, HD, SCALE)
        o32 = o32[0] if isinstance(o32, tuple) else o32
        sc = float(ref.abs().max())
        e32 = float((o32.double() - ref).abs().max()) / sc
        rec = s16.planes[0, r0:r0 + B * N].float() + s16.planes[1, r0:r0 + B * N].float() / 2048.0
        ep = float((rec.double() - ref).abs().max()) / sc
        print(f"segs H{H} segment {i} ({B} x {N}): planes vs float64 {ep:.2e}, f32 kernel {e32:.2e}")
        assert ep <= 2.0 * e32 + 2e-7 + 2.0 ** -21, i
    sp, rp = s16.planes.cpu(), r16.planes.cpu()
    assert bool(torch.isnan(sp[:, ~used]).all()), "rows between the segments were written"
    assert same_bits(sp[:, used].contiguous(), rp[:, used].contiguous())
