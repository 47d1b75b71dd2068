"""The pseudo-label kernels of csrc/par.hip (par_affinity, par_propagate, refine_pre, refine_post, refine_merge) at their edges:
fewer than six dilations, planes smaller than a dilation, one row / one column, an h * w that ends inside a 256-lane block, job
tables that are not the identity, job_K < Kmax over more than one channel chunk, every down-scale, boxes that are empty / one
pixel / flush with the border, true ties, both ignore values and the second trip of refine_merge's stride loop -- each against the
float64 references and bounds of tests/par_ref.py, which tests/test_par_ref_host.py checks first (same case lists).

Technique (tests/kernel_guard.py): outputs live inside sentinel-guarded buffers, inputs inside NaN slack, and every element a kernel
is told to skip (channels >= job_K) is NaN, so a finite result proves it was not read.  The refusal tests only pass arguments a
launcher rejects before launching.  Host-guaranteed preconditions (a key 0 in a foreground slot, a box outside the image, a job_img
out of range) are not tried.  Tolerance tests print their worst err / bound."""
import ctypes

import numpy as np
import pytest
import torch

import par_ref as P
from kernel_guard import _ALIVE, Guard, Tally, nan_in, ratio_report, same_bits, stream
from parity_util import assert_labels_equal_up_to_ties

pytestmark = pytest.mark.gpu
ERR_ARG = -1


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _ALIVE.clear()


def _i32(v, dev):
    return torch.as_tensor(np.asarray(v), dtype=torch.int32).to(dev)


def _dil(d):
    return (ctypes.c_int32 * len(d))(*d)


def _pos(dil, dev):
    from dupl_amd import ops
    pos = torch.from_numpy(ops.par_pos_term(list(dil)))
    return pos, nan_in(pos, dev)


# =========================================================================================== affinity
def _affinity(dev, imgs, dil):
    from dupl_amd import ops
    B, _, h, w = imgs.shape
    pos, pos_d = _pos(dil, dev)
    out = Guard((B, 8 * len(dil), h, w), dev)
    ops.L().dupl_par_affinity(nan_in(imgs, dev).data_ptr(), out.ptr, ctypes.cast(_dil(dil), ctypes.c_void_p), len(dil), pos_d.data_ptr(),
                              B, h, w, stream())
    return out.cpu(), pos


@pytest.mark.parametrize("ndil,h,w", P.AFF_CASES)
def test_affinity_against_float64_within_four_oracle_deviations(dev, ndil, h, w):
    """B = 3 different images (one per blockIdx.y), nn in {8, 16, 48}, planes down to 1 x 1: |kernel - affinity64| <= max(4 x the
    fp32 oracle's own deviation from affinity64 on this input, 8 ulp).  On most of these planes most neighbours clamp; on 1 x 1 all
    of them are the centre."""
    imgs, dil, dev_oracle = P.affinity_case(ndil, h, w)
    got, pos = _affinity(dev, imgs, dil)
    ref = P.affinity64(imgs, dil, pos)
    assert bool(torch.isfinite(got).all())
    print(f"fp32 oracle deviation on this input {dev_oracle:.3e}")
    assert ratio_report(f"affinity ndil {ndil} {h}x{w}", (got.double() - ref).abs(), P.affinity_bound(ref, dev_oracle)) < 1.0


@pytest.mark.parametrize("ndil", P.AFF_NDIL)
def test_affinity_of_a_constant_image_is_exactly_uniform(dev, ndil):
    """every difference is exactly 0, so whatever the deviation comes to the result is fl(fl(1 / nn) + pos[n]) in every plane"""
    dil = P.DILATIONS[:ndil]
    for (h, w), val in (((5, 7), 0.3), ((1, 1), 0.9), ((23, 25), 0.0), ((1, 257), 1.0)):
        got, pos = _affinity(dev, torch.full((2, 3, h, w), val), dil)
        want = (np.float32(1) / np.float32(8 * ndil) + pos.numpy()).astype(np.float32)
        assert same_bits(got, torch.from_numpy(want).view(1, -1, 1, 1).expand(2, -1, h, w).contiguous()), (h, w, val)


def test_affinity_refusals(dev):
    from dupl_amd import ops
    raw = ops.L().dupl_par_affinity.raw
    imgs = nan_in(torch.zeros(1, 3, 4, 4), dev)
    out = Guard((1, 48, 4, 4), dev)
    _, pos_d = _pos(P.DILATIONS, dev)
    d7 = ctypes.cast(_dil((1, 2, 4, 8, 12, 24, 30)), ctypes.c_void_p)
    d6 = ctypes.cast(_dil(P.DILATIONS), ctypes.c_void_p)
    for ndil, h, d in ((7, 4, d7), (0, 4, d6), (6, 0, d6)):
        assert raw(imgs.data_ptr(), out.ptr, d, ndil, pos_d.data_ptr(), 1, h, 4, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert out.untouched()


# =========================================================================================== propagate
def _propagate_once(dev, aff_d, masks_d, job_img_d, job_K_d, dil):
    from dupl_amd import ops
    njobs, Kmax, h, w = masks_d.shape
    out = Guard((njobs, Kmax, h, w), dev)
    ops.L().dupl_par_propagate(aff_d.data_ptr(), masks_d.data_ptr(), out.ptr, job_img_d.data_ptr(), job_K_d.data_ptr(),
                               ctypes.cast(_dil(dil), ctypes.c_void_p), len(dil), njobs, Kmax, h, w, stream())
    return out.cpu()


@pytest.mark.parametrize("ndil,h,w", P.PROP_CASES)
def test_propagate_one_iteration(dev, ndil, h, w):
    """Kmax = 9, job_K = 1 .. 9 (chunks of 4 + 4 + 1 and every chunk width), jobs 0 .. 8 on images [2, 0, 1, ...]; channels >= job_K
    of the input are NaN and must not reach a channel < job_K; error <= nn * 2^-24 * sum |a| |M|; the same plane as channel 0, 3,
    5, 4 and 8 of three jobs on one image comes out bit-identical (same sums in the same order whatever the chunk).  Nothing is
    asserted about channels >= job_K of the result: they are unspecified."""
    aff, masks, dil = P.propagate_case(ndil, h, w)
    got = _propagate_once(dev, nan_in(aff, dev), nan_in(masks, dev), _i32(P.PROP_JOB_IMG, dev), _i32(P.PROP_JOB_K, dev), dil)
    ref, S = P.propagate64(aff, masks, P.PROP_JOB_IMG, P.PROP_JOB_K, dil)
    bound = P.propagate_bound(S, 8 * ndil)
    t = Tally(f"propagate {h}x{w} nn {8 * ndil}")
    for j, K in enumerate(P.PROP_JOB_K):
        assert bool(torch.isfinite(got[j, :K]).all()), f"job {j}: a poisoned channel >= job_K reached a live one"
        t.add(f"job {j}", (got[j, :K].double() - ref[j, :K]).abs(), bound[j, :K])
    t.done()
    j0, k0 = P.PROP_SAME_PLANE[0]
    for j, k in P.PROP_SAME_PLANE[1:]:
        assert same_bits(got[j, k], got[j0, k0]), f"job {j} channel {k} differs from job {j0} channel {k0}"


def test_propagate_wrapper_iterates_single_steps(dev):
    """ops.par_propagate(num_iter) equals num_iter single launches bit for bit in the channels < job_K; num_iter = 0 hands the input
    tensor back untouched"""
    from dupl_amd import ops
    aff, masks, dil = P.propagate_case(6, 23, 25)
    aff_d, ji, jk = nan_in(aff, dev), _i32(P.PROP_JOB_IMG, dev), _i32(P.PROP_JOB_K, dev)
    step = masks
    singles = [masks]
    for _ in range(3):
        step = _propagate_once(dev, aff_d, nan_in(step, dev), ji, jk, dil)
        singles.append(step)
    for it in (0, 1, 2, 3):
        m_d = nan_in(masks, dev)
        res = ops.par_propagate(aff_d, m_d, ji, jk, list(dil), it)
        torch.cuda.synchronize()
        if it == 0:
            assert res is m_d and same_bits(m_d.cpu(), masks)
        for j, K in enumerate(P.PROP_JOB_K):
            assert same_bits(res[j, :K].cpu(), singles[it][j, :K]), (it, j)


def test_propagate_refusals(dev):
    """h <= 0 and w <= 0 (which used to launch a zero-sized grid), njobs = 0 and seven dilations: DUPL_ERR_ARG, nothing launched"""
    from dupl_amd import ops
    raw = ops.L().dupl_par_propagate.raw
    aff, m = nan_in(torch.zeros(1, 48, 4, 4), dev), nan_in(torch.zeros(1, 2, 4, 4), dev)
    out = Guard((1, 2, 4, 4), dev)
    ji, jk = _i32([0], dev), _i32([2], dev)
    d7 = ctypes.cast(_dil((1, 2, 4, 8, 12, 24, 30)), ctypes.c_void_p)
    d6 = ctypes.cast(_dil(P.DILATIONS), ctypes.c_void_p)
    for d, ndil, njobs, h, w in ((d6, 6, 1, 0, 4), (d6, 6, 1, 4, 0), (d6, 6, 1, -1, 4), (d6, 6, 0, 4, 4), (d7, 7, 1, 4, 4)):
        assert raw(aff.data_ptr(), m.data_ptr(), out.ptr, ji.data_ptr(), jk.data_ptr(), d, ndil, njobs, 2, h, w, stream()) == ERR_ARG, \
            (ndil, njobs, h, w)
    torch.cuda.synchronize()
    assert out.untouched()


# =========================================================================================== refine_pre
@pytest.mark.parametrize("use_map", [False, True], ids=["scalar", "map"])
@pytest.mark.parametrize("ds", P.PRE_SCALES)
@pytest.mark.parametrize("H,W", P.PRE_SIZES)
def test_refine_pre(dev, H, W, ds, use_map):
    """every down_scale on sizes that are and are not multiples of it; scalar threshold per job / threshold map per image; keys out
    of order from C = 20 with repeats across jobs; jobs on images that are not their own index; K = 1 gives exactly 1; channels
    beyond K (Kmax = 6 > K) stay exactly 0"""
    from dupl_amd import ops
    cams, thr_map, thr = P.refine_pre_case(H, W)
    keys = torch.tensor(P.PRE_KEYS, dtype=torch.int32)
    ref, bound = P.refine_pre64(cams, thr_map if use_map else None, None if use_map else thr, P.PRE_JOB_IMG, P.PRE_JOB_K, keys, ds)
    njobs, Kmax, h, w = ref.shape
    out = Guard((njobs, Kmax, h, w), dev, init=torch.zeros(njobs, Kmax, h, w))          # ops.refine_pre hands the kernel zeros
    # every table stays in a local until the launch has finished: a temporary's memory would be handed to the next allocation
    cams_d, map_d, thr_d = nan_in(cams, dev), nan_in(thr_map, dev), nan_in(thr, dev)
    ji, jk, keys_d = _i32(P.PRE_JOB_IMG, dev), _i32(P.PRE_JOB_K, dev), keys.to(dev)
    ops.L().dupl_refine_pre(cams_d.data_ptr(), map_d.data_ptr() if use_map else None, None if use_map else thr_d.data_ptr(),
                            ji.data_ptr(), jk.data_ptr(), keys_d.data_ptr(), njobs, Kmax, out.ptr, P.PRE_C, H, W, h, w, stream())
    got = out.cpu()
    t = Tally(f"refine_pre ({H},{W}) / {ds} {'map' if use_map else 'scalar'}")
    for j, K in enumerate(P.PRE_JOB_K):
        t.add(f"job {j}", (got[j, :K].double() - ref[j, :K]).abs(), bound[j, :K])
        assert bool((got[j, K:] == 0).all()), f"job {j}: a channel beyond K was written"
        if K == 1:
            assert bool((got[j, 0] == 1.0).all())
    t.done()
    if (H, W, ds) == (33, 50, 2):                            # the wrapper: same launch, its own zeroed output
        res = ops.refine_pre(cams_d, map_d if use_map else None, None if use_map else thr_d, ji, jk, keys_d, down_scale=ds)
        assert same_bits(res.cpu(), got)


# =========================================================================================== refine_post
def _post(dev, masks, job_img, job_K, keys, box, ignore, H, W):
    from dupl_amd import ops
    njobs, Kmax, h, w = masks.shape
    out = Guard((njobs, H, W), dev)
    masks_d, ji, jk, keys_d, box_d = nan_in(masks, dev), _i32(job_img, dev), _i32(job_K, dev), keys.to(dev), box.to(dev)   # alive until
    ops.L().dupl_refine_post(masks_d.data_ptr(), ji.data_ptr(), jk.data_ptr(), keys_d.data_ptr(), njobs, Kmax, box_d.data_ptr(),  # the sync
                             float(ignore), out.ptr, h, w, H, W, stream())
    got = out.cpu()
    del ji, jk, keys_d, box_d
    return got


@pytest.mark.parametrize("ignore", P.POST_IGNORE)
@pytest.mark.parametrize("hw,HW", P.POST_SIZES)
def test_refine_post(dev, hw, HW, ignore):
    """labels equal refine_post64 up to proven ties (a mismatching pixel must have a float64 margin below twice the fp32 blend's
    bound; the share of excused pixels is capped); keys not increasing; boxes full / empty / one pixel / flush with the right and
    bottom border / all but the last row; channels >= K are NaN"""
    (h, w), (H, W) = hw, HW
    masks, keys, box = P.refine_post_case(h, w), torch.tensor(P.POST_KEYS, dtype=torch.int32), P.post_boxes(H, W)
    got = _post(dev, masks, P.POST_JOB_IMG, P.POST_JOB_K, keys, box, ignore, H, W)
    lab, margin, bound = P.refine_post64(masks, P.POST_JOB_IMG, P.POST_JOB_K, keys, box, ignore, H, W)
    assert bool((got == got.round()).all())
    assert_labels_equal_up_to_ties(got, lab, margin, f"refine_post {hw}->{HW} ignore {ignore}", tol=2.0 * float(bound.max()))
    outside = torch.isinf(margin) & (torch.tensor(P.POST_JOB_K).view(-1, 1, 1) > 1)
    assert bool((got[outside] == ignore).all()), "outside the box only ignore"
    assert bool((got[P.POST_JOB_IMG.index(1)] == ignore).all()), "the empty box"


def test_refine_post_true_ties_go_to_the_first_channel(dev):
    masks, job_img, job_K, keys, box, (H, W) = P.forced_tie_case()
    got = _post(dev, masks, job_img, job_K, keys, box, 255, H, W)
    assert bool((got[0] == 4).all()), "increasing keys: the lower key of the tied pair"
    assert bool((got[1] == 11).all()), "the first channel of the tied pair, whatever its key"
    lab, _, _ = P.refine_post64(masks, job_img, job_K, keys, box, 255, H, W)
    assert torch.equal(got.long(), lab)


# =========================================================================================== refine_merge
@pytest.mark.parametrize("ignore", P.MERGE_IGNORE)
@pytest.mark.parametrize("n", P.MERGE_N)
def test_refine_merge(dev, n, ignore):
    """exact over the full table of (a, b) in {0, 1, 7, ignore}^2; n = 4096 * 256 + 257 takes the stride loop's second trip;
    ignore_index = 0 as the reference's two assignments define it"""
    from dupl_amd import ops
    for off in (range(16) if n == 1 else (0, 5)):
        a, b = P.merge_table(ignore, n, off)
        out = Guard((n,), dev)
        ops.L().dupl_refine_merge(nan_in(a.float(), dev).data_ptr(), nan_in(b.float(), dev).data_ptr(), out.ptr, float(ignore), n, stream())
        assert torch.equal(out.cpu(), P.refine_merge_int(a, b, ignore).float()), (n, ignore, off)
