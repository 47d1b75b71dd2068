"""CPU checks of tests/par_ref.py and tests/optim_ref.py, the yardsticks of tests/test_par_refine_kernels_gpu.py and
tests/test_adamw_gmm_kernels_gpu.py: the float64 references agree with torch / the oracle, torch's own fp32 evaluation passes every
bound (not too tight), each classic mistake fails on the cases the GPU suite uses (not too loose), the test images are well
conditioned, and the AdamW emulation's fused multiply-add rounds once.  The fp32 oracle's deviation from affinity64 -- the number
the kernel's affinity bound is 4 x of -- is printed per case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optim_ref as R
import par_ref as P
from kernel_guard import ratio_report
from parity_util import assert_labels_equal_up_to_ties


# ============================================================================================== affinity
def test_references_agree_with_the_oracles_par_at_the_workloads_dilations():
    from oracle import dupl_oracle as O
    assert tuple(O.PAR_DILATIONS) == P.DILATIONS and tuple(O.PAR_OFFSETS) == P.OFFSETS
    imgs = P.textured_images(2, 40, 52, seed=3)
    pos = P.oracle_pos32(P.DILATIONS)
    ref = P.affinity64(imgs, P.DILATIONS, pos)
    got = O.par_affinity(imgs)[:, 0]
    dev = float((got.double() - ref).abs().max())
    print(f"oracle fp32 affinity vs affinity64, 40x52, 6 dilations: max deviation {dev:.3e}")
    assert dev < 2e-5 and float(ref.sum(1).sub(1.0 + float(pos.double().sum())).abs().max()) < 1e-12
    assert torch.equal(P.neighbours64(imgs, P.DILATIONS), O.par_neighbors(imgs.double()))
    masks = torch.rand(2, 3, 40, 52, generator=torch.Generator().manual_seed(4))
    one = O.par_forward(imgs, masks, num_iter=1)                       # fp32: its own affinity, one propagation
    out, S = P.propagate64(got, masks, [0, 1], [3, 3], P.DILATIONS)
    assert ratio_report("oracle fp32 propagate", (one.double() - out).abs(), P.propagate_bound(S, 48)) < 1.0


@pytest.mark.parametrize("ndil,h,w", P.AFF_CASES)
def test_affinity_cases_are_conditioned_and_mistakes_fail(ndil, h, w):
    imgs, dil, dev = P.affinity_case(ndil, h, w)
    pos = P.oracle_pos32(dil)
    ref = P.affinity64(imgs, dil, pos)
    bound = P.affinity_bound(ref, dev)
    print(f"affinity case ndil {ndil} plane {h}x{w}: fp32 oracle max deviation from affinity64 {dev:.3e}; kernel bound "
          f"4 x that = {4 * dev:.3e}, floor 8 ulp = {float((8 * P.G.ulp32(ref)).max()):.3e}")
    assert np.isfinite(dev) and dev < 2e-5, "the fp32 formulation itself is off: the case is badly conditioned"
    wrong = {"reflect": dict(border="reflect"), "dy/dx swapped": dict(swap=True), "biased std": dict(unbiased=False)}
    if (h, w) == (1, 1):
        # every neighbour is the centre: the numerator is exactly 0 whatever the deviation, the affinity is uniform, and no
        # variant can differ; the standard deviation is 0 by construction, not by lack of texture
        assert float((ref - (1.0 / (8 * ndil) + pos.double().view(1, -1, 1, 1))).abs().max()) < 1e-15
        for kw in wrong.values():
            assert torch.equal(P.affinity64(imgs, dil, pos, **kw), ref)
        return
    sd_min = float(P.neighbourhood_sd(imgs, dil).min())
    print(f"    smallest neighbourhood standard deviation {sd_min:.3f} (floor {P.SD_FLOOR})")
    assert sd_min >= P.SD_FLOOR
    for name, kw in wrong.items():
        r = ratio_report(f"    {name}", (P.affinity64(imgs, dil, pos, **kw) - ref).abs(), bound)
        assert r > 1.0, f"{name} passes the bound on this case"


def test_constant_image_reference_is_uniform():
    for ndil in P.AFF_NDIL:
        dil = P.DILATIONS[:ndil]
        pos = P.oracle_pos32(dil)
        ref = P.affinity64(torch.full((1, 3, 5, 7), 0.3), dil, pos)
        assert float((ref - (1.0 / (8 * ndil) + pos.double().view(1, -1, 1, 1))).abs().max()) < 1e-15


# ============================================================================================== propagate
@pytest.mark.parametrize("ndil,h,w", P.PROP_CASES)
def test_propagate_bound_holds_for_torch_fp32_and_catches_the_wrong_affinity(ndil, h, w):
    aff, masks, dil = P.propagate_case(ndil, h, w)
    out, S = P.propagate64(aff, masks, P.PROP_JOB_IMG, P.PROP_JOB_K, dil)
    bound = P.propagate_bound(S, 8 * ndil)
    wrong, _ = P.propagate64(aff, masks, P.PROP_JOB_IMG, P.PROP_JOB_K, dil, own_affinity=True)
    worst_wrong = 0.0
    for j, K in enumerate(P.PROP_JOB_K):
        assert bool(torch.isfinite(out[j, :K]).all()) and bool(torch.isnan(out[j, K:]).all())
        nb = P.neighbours64(masks[j, :K], dil).float()                                  # exact: the values are fp32
        got = (nb * aff[P.PROP_JOB_IMG[j]].float()).sum(dim=1)
        assert ratio_report(f"torch fp32, job {j}", (got.double() - out[j, :K]).abs(), bound[j, :K], quiet=True) < 1.0
        if j % 3 != P.PROP_JOB_IMG[j]:
            worst_wrong = max(worst_wrong, ratio_report("", (wrong[j, :K] - out[j, :K]).abs(), bound[j, :K], quiet=True))
    print(f"propagate {h}x{w}, {ndil} dilations: the affinity of job j instead of job_img[j] is off by {worst_wrong:.1f} bounds")
    assert worst_wrong > 1.0
    j0, k0 = P.PROP_SAME_PLANE[0]
    for j, k in P.PROP_SAME_PLANE[1:]:
        assert P.PROP_JOB_IMG[j] == P.PROP_JOB_IMG[j0] and k < P.PROP_JOB_K[j] and torch.equal(out[j, k], out[j0, k0])


# ============================================================================================== refine_pre
@pytest.mark.parametrize("use_map", [False, True], ids=["scalar", "map"])
@pytest.mark.parametrize("ds", P.PRE_SCALES)
@pytest.mark.parametrize("H,W", P.PRE_SIZES)
def test_refine_pre64_is_interpolate_softmax_and_torch_fp32_passes(H, W, ds, use_map):
    cams, thr_map, thr = P.refine_pre_case(H, W)
    keys = torch.tensor(P.PRE_KEYS, dtype=torch.int32)
    ref, bound = P.refine_pre64(cams, thr_map if use_map else None, None if use_map else thr, P.PRE_JOB_IMG, P.PRE_JOB_K, keys, ds)
    h, w = H // ds, W // ds
    worst = 0.0
    for j, (b, K) in enumerate(zip(P.PRE_JOB_IMG, P.PRE_JOB_K)):
        bg = thr_map[b] if use_map else torch.full((H, W), float(thr[j]))
        stack = torch.cat([bg[None], cams[b, keys[j, 1:K].long() - 1]])[None]            # (1, K, H, W)
        want = F.interpolate(stack.double(), size=[h, w], mode="bilinear", align_corners=False).softmax(dim=1)[0]
        assert float((ref[j, :K] - want).abs().max()) < 1e-13 and bool((ref[j, K:] == 0).all())
        got = F.interpolate(stack, size=[h, w], mode="bilinear", align_corners=False).softmax(dim=1)[0]
        worst = max(worst, ratio_report("", (got.double() - ref[j, :K]).abs(), bound[j, :K], quiet=True))
        if K == 1:
            assert bool((ref[j, 0] == 1.0).all())
    print(f"refine_pre ({H},{W}) / {ds}, {'map' if use_map else 'scalar'}: torch fp32 worst err / bound {worst:.3f}")
    assert worst < 1.0
    # not too loose: a down-scaling that samples at the nearest pixel instead of blending is caught wherever it is not the identity
    if ds > 1 and use_map:
        near = F.interpolate(cams.double(), size=[h, w], mode="nearest")
        j, b, K = 2, P.PRE_JOB_IMG[2], P.PRE_JOB_K[2]
        v = torch.cat([F.interpolate(thr_map[None, [b]].double(), size=[h, w], mode="nearest")[0], near[b, keys[j, 1:K].long() - 1]])
        assert ratio_report("", (v.softmax(0) - ref[j, :K]).abs(), bound[j, :K], quiet=True) > 1.0


# ============================================================================================== refine_post
@pytest.mark.parametrize("ignore", P.POST_IGNORE)
@pytest.mark.parametrize("hw,HW", P.POST_SIZES)
def test_refine_post64_is_interpolate_argmax_and_its_tie_set_is_within_the_cap(hw, HW, ignore):
    (h, w), (H, W) = hw, HW
    masks, keys, box = P.refine_post_case(h, w), torch.tensor(P.POST_KEYS, dtype=torch.int32), P.post_boxes(H, W)
    lab, margin, bound = P.refine_post64(masks, P.POST_JOB_IMG, P.POST_JOB_K, keys, box, ignore, H, W)
    tol = 2.0 * float(bound.max())
    assert 0 < tol < 1e-5, "two fp32 blends of values <= 1 differ by far less than parity_util's TIE_TOL"
    n_tie = int((margin < tol).sum())
    print(f"refine_post {hw}->{HW}: {n_tie} pixels of {lab.numel()} have a float64 margin below {tol:.2e}")
    assert n_tie <= P.tie_cap(lab.numel()), "pick another seed: the float64 reference alone leaves too many near-ties"
    got = torch.full_like(lab, ignore)
    for j, (b, K) in enumerate(zip(P.POST_JOB_IMG, P.POST_JOB_K)):
        y0, y1, x0, x1 = (int(t) for t in box[b])
        up64 = F.interpolate(masks[j, :K][None].double(), size=(H, W), mode="bilinear", align_corners=False)[0]
        want = torch.full((H, W), ignore, dtype=torch.int64)
        want[y0:y1, x0:x1] = keys[j].long()[up64.argmax(0)][y0:y1, x0:x1]
        assert torch.equal(lab[j], want)
        up32 = F.interpolate(masks[j, :K][None], size=(H, W), mode="bilinear", align_corners=False)[0]
        got[j, y0:y1, x0:x1] = keys[j].long()[up32.argmax(0)][y0:y1, x0:x1]
        inside = torch.zeros(H, W, dtype=torch.bool)
        inside[y0:y1, x0:x1] = True
        assert bool(torch.isinf(margin[j][~inside]).all()) and (K > 1 or bool(torch.isinf(margin[j]).all()))
    assert_labels_equal_up_to_ties(got, lab, margin, f"torch fp32 refine_post {hw}->{HW}", tol=tol)
    assert bool((lab[P.POST_JOB_IMG.index(1)] == ignore).all()), "an empty box leaves only ignore"
    assert int((lab[P.POST_JOB_IMG.index(2)] != ignore).sum()) == 1, "the one-pixel box"
    assert bool((lab[P.POST_JOB_IMG.index(4)][H - 1] == ignore).all())
    wrong, _, _ = P.refine_post64(masks, P.POST_JOB_IMG, P.POST_JOB_K, keys, box, ignore, H, W, box_inclusive=True)
    with pytest.raises(AssertionError):
        assert_labels_equal_up_to_ties(wrong, lab, margin, "upper box edges included", tol=tol)


def test_forced_ties_go_to_the_first_channel_and_last_wins_fails():
    masks, job_img, job_K, keys, box, (H, W) = P.forced_tie_case()
    lab, margin, bound = P.refine_post64(masks, job_img, job_K, keys, box, 255, H, W)
    assert bool((margin == 0).all()), "every pixel is a true tie"
    assert bool((lab[0] == 4).all()) and bool((lab[1] == 11).all())
    up32 = F.interpolate(masks[0][None], size=(H, W), mode="bilinear", align_corners=False)[0]
    assert torch.equal(up32.double(), P.G.bilinear64(masks[0], H, W, False)), "the fp32 blend of this case is exact"
    last, _, _ = P.refine_post64(masks, job_img, job_K, keys, box, 255, H, W, last_wins=True)
    assert bool((last[0] == 11).all()) and bool((last[1] == 4).all()) and not torch.equal(last, lab)


# ============================================================================================== refine_merge
@pytest.mark.parametrize("ignore", P.MERGE_IGNORE)
def test_refine_merge_int_is_the_references_two_assignments(ignore):
    a, b = P.merge_table(ignore, 16)
    out = P.refine_merge_int(a, b, ignore)
    fa, fb = a.float(), b.float()
    want = fa.clone()
    want[fa == 0] = ignore
    want[(fa + fb) == 0] = 0
    assert torch.equal(out.float(), want)
    if ignore == 255:
        assert out.tolist() == [0, 255, 255, 255, 1, 1, 1, 1, 7, 7, 7, 7, 255, 255, 255, 255]
    if ignore == -1:                     # a + b == 0 also where a = 1 meets b = ignore: the second assignment decides
        assert out.tolist() == [0, -1, -1, -1, 1, 1, 1, 0, 7, 7, 7, 7, -1, 0, -1, -1]
    if ignore == 0:
        assert out.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 7, 7, 7, 7, 0, 0, 0, 0]
    for off in range(16):
        a1, b1 = P.merge_table(ignore, 1, off)
        assert int(a1) == int(a[off]) and int(b1) == int(b[off])


# ============================================================================================== AdamW emulation
def test_fma32_rounds_once_where_rounding_twice_gives_the_other_answer():
    f = np.float32
    e = f(2.0 ** -23)
    # a * b = -(1 - 2^-46);  c = 2^24 + 2 (odd mantissa): the exact sum 2^24 + 1 + 2^-46 lies just ABOVE the float32 midpoint
    # 2^24 + 1; float64 (ulp 2^-28 here) rounds it ONTO the midpoint, and the cast then goes to the even neighbour 2^24
    up = (-(f(1) + e), f(1) - e, f(2.0 ** 24 + 2))
    # a * b = 1 - 2^-46;  c = 2^24 + 2: the exact sum 2^24 + 3 - 2^-46 lies just BELOW the midpoint 2^24 + 3; rounding twice lands
    # on it and goes to the even neighbour 2^24 + 4
    down = (f(1) + e, f(1) - e, f(2.0 ** 24 + 2))
    for (a, b, c), right, twice in ((up, 2.0 ** 24 + 2, 2.0 ** 24), (down, 2.0 ** 24 + 2, 2.0 ** 24 + 4)):
        assert float(R.fma32_exact(a, b, c)) == right
        assert float(R.fma32_twice_rounded(a, b, c)) == twice != right
        assert float(R.fma32(a, b, c)) == right
    # and on operands of the kernel's own magnitudes, against exact rational arithmetic
    r = np.random.RandomState(0)
    a = np.concatenate([np.full(300, 0.9, f), np.full(300, 0.999, f), r.standard_normal(400).astype(f)])
    b = (r.standard_normal(1000) * 10.0 ** r.uniform(-6, 3, 1000)).astype(f)
    c = (b * (f(1) - a) * (1 + r.standard_normal(1000) * 1e-3) * r.choice([-1, 1], 1000)).astype(f)
    got = R.fma32(a, b, c)
    for i in range(1000):
        assert got[i] == R.fma32_exact(a[i], b[i], c[i]), (a[i], b[i], c[i])
    assert float(R.fma32(f(np.inf), f(1), f(1))) == np.inf and np.isnan(R.fma32(f(np.inf), f(1), f(-np.inf)))
    assert np.isnan(R.fma32(f(np.nan), f(1), f(1))) and float(R.fma32(f(0), f(5), f(0))) == 0.0


def test_adamw_emulation_follows_torch_and_refuses_subnormals():
    from oracle import dupl_oracle as O
    for n in R.ADAMW_N:
        for first in (True, False):
            p, g, m, v, step = R.adamw_case(n, first)
            for scale in R.ADAMW_SCALES:
                p2, g2, m2, v2 = R.adamw_ref(p, g, m, v, step, grad_scale=scale, **R.HYPER)
                assert R.same_bits_or_both_nan(g2, g * np.float32(scale) if np.float32(scale) != 1 else g)
                tp, tg, tm, tv = (torch.from_numpy(t.copy()) for t in (p, g2, m, v))
                O.adamw_update(tp, tg, tm, tv, step, R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"], R.HYPER["wd"])
                fin = np.isfinite(g2)
                # a sanity check, not the yardstick: torch forms 1 - beta in double (0.001), the kernel in fp32 from the rounded
                # beta (1.f - 0.999f = 0.00099998712, 1.3e-5 off), and torch's lerp / addcdiv round differently
                # -- so each is compared relative to the magnitude of the terms it is summed from
                k = R.host_scalars(step=step, **R.HYPER)
                with np.errstate(all="ignore"):
                    scale_m = np.abs(m) + np.abs(g2)
                    scale_p = np.abs(p) + float(k["step_size"]) * np.abs(m2 / (np.sqrt(v2) / k["bc2_sqrt"] + k["eps"]))
                for mine, theirs, scale in ((p2, tp, scale_p), (m2, tm, scale_m), (v2, tv, v2)):
                    assert (np.abs(mine[fin].astype(np.float64) - theirs.numpy()[fin]) <= 2e-5 * scale[fin] + 1e-38).all()
    seen = np.concatenate([R.adamw_case(n, False)[1] for n in R.ADAMW_N])
    assert np.isinf(seen).any() and np.isnan(seen).any() and (seen == 0).any()
    a = np.abs(seen[np.isfinite(seen) & (seen != 0)])
    assert a.min() <= 1.001e-6 and a.max() >= 999.0
    one = np.ones(4, np.float32)
    with pytest.raises(ValueError):
        R.adamw_ref(one, one * np.float32(1e-41), one, one, 1, **R.HYPER)
    with pytest.raises(ValueError):      # an intermediate: (1 - b2) g g
        R.adamw_ref(one, one * np.float32(3e-18), one, one, 1, **R.HYPER)
    # a NaN and an inf gradient stay inside their own element
    p, g, m, v, step = R.adamw_case(1031, False)
    clean = np.where(np.isfinite(g), g, np.float32(1.0))
    pa, _, ma, va = R.adamw_ref(p, g, m, v, step, **R.HYPER)
    pb, _, mb, vb = R.adamw_ref(p, clean, m, v, step, **R.HYPER)
    fin = np.isfinite(g)
    assert (~fin).sum() >= 2 and np.array_equal(pa[fin], pb[fin]) and np.array_equal(ma[fin], mb[fin]) and np.isnan(pa[~fin]).all()


def test_adamw_stride_case_emulates_in_seconds_without_subnormals():
    import time
    p, g, m, v, step = R.adamw_case(R.ADAMW_STRIDE_N, False)
    t0 = time.time()
    p2, _, m2, v2 = R.adamw_ref(p, g, m, v, step, grad_scale=1.0 / 3.0, **R.HYPER)
    print(f"vectorised emulation of {R.ADAMW_STRIDE_N} elements: {time.time() - t0:.1f} s")
    assert R.ADAMW_STRIDE_N > 8192 * 256 * 4 and p2.shape == p.shape


def test_the_gpu_cases_tell_a_contracted_final_subtraction_from_the_written_one():
    """what the kernel computed before its roundings were pinned: p * decay fused into the final subtraction (one rounding instead
    of two).  The cases of the GPU suite must see the difference, or bit-exactness against adamw_ref would pin nothing."""
    f = np.float32
    differ = 0
    for n in R.ADAMW_N[-2:]:
        p, g, m, v, step = R.adamw_case(n, False)
        p2, _, m2, v2 = R.adamw_ref(p, g, m, v, step, **R.HYPER)
        k = R.host_scalars(step=step, **R.HYPER)
        with np.errstate(all="ignore"):
            fused = R.fma32(k["decay"], p, -(k["step_size"] * (m2 / (np.sqrt(v2) / k["bc2_sqrt"] + k["eps"]))).astype(f))
        fin = np.isfinite(p2)
        assert np.abs(fused[fin].astype(np.float64) - p2[fin]).max() <= np.spacing(np.abs(p2[fin])).max()      # the last bit only
        differ += int((fused[fin].view(np.int32) != p2[fin].view(np.int32)).sum())
    print(f"a fused p * decay - step changes the last bit of {differ} of {sum(R.ADAMW_N[-2:])} parameters")
    assert differ >= 20
