"""Plain float64 references for the pseudo-label kernels of csrc/par.hip (par_affinity, par_propagate, refine_pre, refine_post,
refine_merge), the bounds a correct fp32 kernel may differ from them by, and the case lists that tests/test_par_ref_host.py (CPU)
and tests/test_par_refine_kernels_gpu.py (MI355X) both iterate.  Everything is gathers over whole axes, torch on the CPU.

Bounds (u = 2^-24, the unit round-off of float32):

* propagate.  out = sum_n a_n M_n accumulated as acc <- fma(a_n, M_n, acc), n ascending, nn terms.  Every step commits one
  rounding, acc_n = (a_n M_n + acc_{n-1}) (1 + d_n), |d_n| <= u, so term n carries the factor prod_{i >= n} (1 + d_i) and
      |out_fp32 - out| <= ((1 + u)^nn - 1) sum_n |a_n| |M_n|.
  Jeannerod & Rump (2013) sharpen (1 + u)^nn - 1 to nn u for inner products in any order, with or without fused multiply-adds
  (round-to-nearest errors are bounded by u / (1 + u), not u): the bound is  nn * 2^-24 * sum_n |a_n| |M_n|  per element, absent
  underflow (propagate_case floors its affinity at 2^-60, so no product is near the subnormal range).

* refine_pre.  Channel values v_k are bilinear down-scalings (error e_k <= glue_ref.bilinear_bound, exact for the scalar threshold)
  followed by softmax_k.  With E = max_k e_k and D = max_k (max_j v_j - v_k): the argument fl(v_k - mx) is off by at most
  2 E + u D; expf is good to 2 ulp = 4 u; so each exponential has relative error <= expm1(2 E + u D) + 4 u; the sum of K
  positive terms adds (K - 1) u, the division u, and numerator and denominator errors add:
      |s_fp32 - s_k| <= s_k * (2 expm1(2 E + u D) + (K + 8) u).
  The exponentials must not underflow: refine_pre64 asserts D < 80.

* affinity.  t = |d| / sd / 0.3 is ill-conditioned wherever the neighbourhood standard deviation is small: there is no useful
  a-priori bound.  The yardstick is the reference formulation itself: oracle.dupl_oracle.par_affinity (torch fp32, replicate pad,
  dilated gathers) deviates from affinity64 by some maximum on the same input; a kernel may deviate by at most 4 x that (one more
  reordering of the same fp32 sums), with a floor of 8 ulp of the output (affinity_bound).  The test images have texture
  everywhere, and the host suite asserts SD_FLOOR on the smallest neighbourhood standard deviation of every one of them."""
from __future__ import annotations

import functools
import math

import torch

import glue_ref as G

U = 2.0 ** -24
OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))      # (dy, dx) in units of the dilation
DILATIONS = (1, 2, 4, 8, 12, 24)                                                      # the workload's
# smallest neighbourhood standard deviation a test image may have.  Values are below 1, so fp32 commits about 2^-24 in x - mean:
# relative to a deviation of 0.01 that is 6e-6, far from losing the quantity, and real images (smooth regions) go lower still.
SD_FLOOR = 0.01


# ============================================================================================== neighbours
def _border_index(i: torch.Tensor, n: int, border: str) -> torch.Tensor:
    if border == "replicate":
        return i.clamp(0, n - 1)
    assert border == "reflect"                      # the classic mistake: mirror without repeating the edge sample
    if n == 1:
        return torch.zeros_like(i)
    period = 2 * (n - 1)
    i = i % period
    return torch.where(i > n - 1, period - i, i)


def neighbours64(x: torch.Tensor, dilations, border: str = "replicate", swap: bool = False) -> torch.Tensor:
    """(..., h, w) -> (..., 8 * len(dilations), h, w): neighbour n = 8 i + k of a pixel is the pixel at OFFSETS[k] * dilations[i],
    indices clamped into the plane (replicate padding).  `border` / `swap` exist so that the host suite can feed the wrong rules
    (mirror padding; dy and dx exchanged) through the same code."""
    x = x.double()
    h, w = x.shape[-2:]
    ys, xs = torch.arange(h), torch.arange(w)
    outs = []
    for d in dilations:
        for oy, ox in OFFSETS:
            if swap:
                oy, ox = ox, oy
            outs.append(x.index_select(-2, _border_index(ys + oy * d, h, border)).index_select(-1, _border_index(xs + ox * d, w, border)))
    return torch.stack(outs, dim=-3)


# ============================================================================================== affinity
def neighbourhood_sd(imgs: torch.Tensor, dilations, unbiased: bool = True, **kw) -> torch.Tensor:
    nb = neighbours64(imgs, dilations, **kw)                             # (B, 3, nn, h, w)
    nn = nb.shape[2]
    dev = nb - nb.mean(dim=2, keepdim=True)
    return ((dev * dev).sum(dim=2) / (nn - 1 if unbiased else nn)).sqrt()


def affinity64(imgs: torch.Tensor, dilations, pos: torch.Tensor, border: str = "replicate", swap: bool = False,
               unbiased: bool = True) -> torch.Tensor:
    """(B, 3, h, w) images, pos (nn,) -> (B, nn, h, w): softmax_n(-mean_c((|I_n - I| / (sd_c + 1e-8) / 0.3)^2)) + pos[n], sd_c the
    unbiased standard deviation of the nn neighbours of channel c."""
    x = imgs.double()
    nb = neighbours64(x, dilations, border, swap)
    sd = neighbourhood_sd(x, dilations, unbiased, border=border, swap=swap).unsqueeze(2) + 1e-8
    t = (nb - x.unsqueeze(2)).abs() / sd / 0.3
    a = -(t * t).mean(dim=1)
    return torch.softmax(a, dim=1) + pos.double().view(1, -1, 1, 1)


def oracle_pos32(dilations) -> torch.Tensor:
    """the position term exactly as the fp32 oracle adds it"""
    from oracle import dupl_oracle as O
    return 0.01 * O.par_pos_affinity(tuple(dilations))


def oracle_affinity_deviation(imgs: torch.Tensor, dilations) -> float:
    """max |oracle.par_affinity (torch fp32) - affinity64| on the same image and the same position term"""
    from oracle import dupl_oracle as O
    got = O.par_affinity(imgs.float(), tuple(dilations))[:, 0]
    return float((got.double() - affinity64(imgs, dilations, oracle_pos32(dilations))).abs().max())


def affinity_bound(ref: torch.Tensor, oracle_dev: float) -> torch.Tensor:
    """per element: 4 x the fp32 oracle's own maximum deviation on this input, at least 8 ulp of the output"""
    return torch.maximum(torch.full_like(ref, 4.0 * oracle_dev), 8.0 * G.ulp32(ref))


def textured_images(B: int, h: int, w: int, seed: int) -> torch.Tensor:
    """(B, 3, h, w) float32 in [0.1, 0.9] with texture everywhere and a wide spread of |difference| / deviation: per channel a
    triangle wave along its own oblique direction (period 16 px: adjacent pixels differ by about 0.06 to 0.1 in x AND in y, so a
    plane of one row or one column is textured too) plus uniform noise of +-0.01.  A checkerboard or white noise would not do:
    with w1 = 0.3 the affinity of a neighbour one deviation away is already exp(-11), the softmax saturates and hides errors."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.arange(h).view(1, 1, h, 1).double(), torch.arange(w).view(1, 1, 1, w).double()
    ax = torch.tensor([1.0, 0.7, -0.6]).view(1, 3, 1, 1).double()
    ay = torch.tensor([0.6, -1.0, 0.9]).view(1, 3, 1, 1).double()
    phase = (ax * x + ay * y) / 16.0 + 0.37 * torch.arange(B).view(B, 1, 1, 1).double() + 0.21 * torch.arange(3).view(1, 3, 1, 1).double()
    tri = 2.0 * ((phase - phase.floor()) - 0.5).abs()
    noise = torch.rand(B, 3, h, w, generator=g, dtype=torch.float64) - 0.5
    return (0.11 + 0.78 * tri + 0.02 * noise).float()


AFF_PLANES = [(1, 1), (1, 257), (300, 1), (5, 7), (16, 17), (23, 25), (40, 52)]
AFF_NDIL = [1, 2, 6]
AFF_B = 3
AFF_CASES = [(nd, h, w) for nd in AFF_NDIL for (h, w) in AFF_PLANES]


@functools.lru_cache(maxsize=None)
def affinity_case(ndil: int, h: int, w: int):
    """(images, dilations, oracle deviation): computed once, shared, never modified"""
    dil = DILATIONS[:ndil]
    imgs = textured_images(AFF_B, h, w, seed=100 * ndil + 7 * h + w)
    return imgs, dil, oracle_affinity_deviation(imgs, dil)


# ============================================================================================== propagate
def propagate64(aff: torch.Tensor, masks: torch.Tensor, job_img, job_K, dilations, own_affinity: bool = False):
    """One iteration.  aff (B, nn, h, w), masks (njobs, Kmax, h, w) -> (out, S), both (njobs, Kmax, h, w) float64:
    out[j, k] = sum_n aff[job_img[j], n] * neighbour_n(masks[j, k]) for k < job_K[j], S the same sum of absolute values (the bound is
    nn * 2^-24 * S); channels >= job_K[j] are NaN in both: the kernel leaves them unspecified.  own_affinity: the classic mistake,
    job j reads aff[j]."""
    njobs, Kmax = masks.shape[:2]
    out = torch.full(masks.shape, float("nan"), dtype=torch.float64)
    S = out.clone()
    for j in range(njobs):
        K = int(job_K[j])
        a = aff[(j if own_affinity else int(job_img[j])) % aff.shape[0]].double()          # (nn, h, w)
        nb = neighbours64(masks[j, :K], dilations)                                          # (K, nn, h, w)
        out[j, :K] = (nb * a).sum(dim=1)
        S[j, :K] = (nb * a).abs().sum(dim=1)
    return out, S


def propagate_bound(S: torch.Tensor, nn: int) -> torch.Tensor:
    return nn * U * S


PROP_KMAX = 9
PROP_JOB_K = list(range(1, 10))
PROP_JOB_IMG = [2, 0, 1, 2, 0, 1, 2, 0, 1]
PROP_CASES = [(6, 5, 7), (6, 23, 25), (6, 1, 257), (2, 16, 17), (1, 300, 1)]
# the same plane as (job, channel): jobs 2, 5, 8 all read image 1; chunk position / chunk width: 0 of 3, 3 of 4, 1 of 2, 0 of 4, 0 of 1
PROP_SAME_PLANE = [(2, 0), (5, 3), (5, 5), (8, 4), (8, 8)]


@functools.lru_cache(maxsize=None)
def propagate_case(ndil: int, h: int, w: int):
    """(aff fp32 (3, nn, h, w), masks fp32 (9, 9, h, w) with NaN in the channels >= job_K, dilations)"""
    dil = DILATIONS[:ndil]
    imgs = textured_images(3, h, w, seed=5 * h + w + ndil)
    # an affinity like the kernel's own output; the far dilations' position terms are below 1e-38, so it is floored at 2^-60 to
    # keep every product clear of the subnormal range (the bound assumes no underflow)
    aff = affinity64(imgs, dil, oracle_pos32(dil)).float().clamp_min(2.0 ** -60)
    g = torch.Generator().manual_seed(31 * h + w)
    masks = 0.01 + 0.99 * torch.rand(len(PROP_JOB_K), PROP_KMAX, h, w, generator=g)
    shared = masks[2, 0].clone()
    for j, k in PROP_SAME_PLANE:
        masks[j, k] = shared
    for j, K in enumerate(PROP_JOB_K):
        masks[j, K:] = float("nan")
    assert float(aff.min()) * 0.01 > 2.0 ** -100
    return aff, masks, dil


# ============================================================================================== refine_pre
def refine_pre64(cams: torch.Tensor, thr_map, thr, job_img, job_K, keys: torch.Tensor, down_scale: int):
    """cams (B, C, H, W); thr_map (B, H, W) or None; thr (njobs,) scalars or None -> (masks, bound), (njobs, Kmax, h, w) float64 with
    (h, w) = (H // down_scale, W // down_scale): channel 0 is the background threshold of image job_img[j] (the map, down-scaled, or
    the job's scalar), channel k >= 1 is cams[job_img[j], keys[j, k] - 1] down-scaled (bilinear, align_corners False); softmax over
    the job's K channels; channels >= K are exactly 0."""
    B, C, H, W = cams.shape
    njobs, Kmax = keys.shape
    h, w = H // down_scale, W // down_scale
    masks = torch.zeros(njobs, Kmax, h, w, dtype=torch.float64)
    bound = torch.zeros_like(masks)
    for j in range(njobs):
        K, b = int(job_K[j]), int(job_img[j])
        if K > 1:
            planes = cams[b, (keys[j, 1:K].long() - 1)]                                      # (K - 1, H, W)
            v = G.bilinear64(planes, h, w, False)
            e = G.bilinear_bound(planes, h, w, False).expand_as(v)
        else:
            v = e = torch.zeros(0, h, w, dtype=torch.float64)
        if thr_map is not None:
            v0, e0 = G.bilinear64(thr_map[b][None], h, w, False), G.bilinear_bound(thr_map[b][None], h, w, False).expand(1, h, w)
        else:
            v0, e0 = torch.full((1, h, w), float(thr[j]), dtype=torch.float64), torch.zeros(1, h, w, dtype=torch.float64)
        v, e = torch.cat([v0, v]), torch.cat([e0, e])
        s = torch.softmax(v, dim=0)
        E = e.amax(dim=0, keepdim=True)
        D = (v.amax(dim=0, keepdim=True) - v).amax(dim=0, keepdim=True)
        assert float(D.max()) < 80.0, "an exponential would underflow: outside what the bound covers"
        masks[j, :K] = s
        bound[j, :K] = s * (2.0 * torch.expm1(2.0 * E + U * D) + (K + 8) * U)
    return masks, bound


PRE_SIZES = [(8, 8), (9, 11), (33, 50), (7, 130)]
PRE_SCALES = [1, 2, 3, 4]
PRE_C, PRE_B, PRE_KMAX = 20, 3, 6
PRE_JOB_IMG = [2, 0, 2, 1, 0]
PRE_JOB_K = [1, 3, 4, 2, 5]
# column 0 is the background slot; foreground keys are classes 1..C, out of order, repeated across jobs; slots >= K are never read
PRE_KEYS = [[0, 1, 1, 1, 1, 1], [0, 17, 3, 1, 1, 1], [0, 20, 3, 11, 1, 1], [0, 17, 1, 1, 1, 1], [0, 9, 20, 2, 1, 1]]


@functools.lru_cache(maxsize=None)
def refine_pre_case(H: int, W: int):
    """(cams fp32 (B, C, H, W) in [0, 1], thr_map fp32 (B, H, W), thr fp32 (njobs,))"""
    g = torch.Generator().manual_seed(13 * H + W)
    cams = torch.rand(PRE_B, PRE_C, H, W, generator=g)
    thr_map = 0.45 + 0.3 * torch.rand(PRE_B, H, W, generator=g)
    thr = torch.tensor([0.3, 0.65, 0.5, 0.7, 0.25])
    return cams, thr_map, thr


# ============================================================================================== refine_post
def refine_post64(masks: torch.Tensor, job_img, job_K, keys: torch.Tensor, box: torch.Tensor, ignore: int, H: int, W: int,
                  last_wins: bool = False, box_inclusive: bool = False):
    """masks (njobs, Kmax, h, w) -> (labels int64 (njobs, H, W), margin float64, bound float64): the job's K channels up-scaled to
    (H, W) (bilinear, align_corners False), FIRST maximum over k, label keys[j, k]; outside the half-open box
    [y0, y1) x [x0, x1) of image job_img[j] the label is `ignore`.  margin: top-1 minus top-2 of the up-scaled stack (+inf outside
    the box and for K = 1); bound: what one fp32 up-scaled value may be off by (glue_ref.bilinear_bound, largest over the channels).
    last_wins / box_inclusive: the classic mistakes (last maximum; upper edges included)."""
    njobs, Kmax, h, w = masks.shape
    labels = torch.full((njobs, H, W), int(ignore), dtype=torch.int64)
    margin = torch.full((njobs, H, W), math.inf, dtype=torch.float64)
    bound = torch.zeros((njobs, H, W), dtype=torch.float64)
    Y, X = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    for j in range(njobs):
        K, b = int(job_K[j]), int(job_img[j])
        up = G.bilinear64(masks[j, :K], H, W, False)                                         # (K, H, W)
        y0, y1, x0, x1 = (int(t) for t in box[b])
        inside = (Y >= y0) & (Y <= y1 if box_inclusive else Y < y1) & (X >= x0) & (X <= x1 if box_inclusive else X < x1)
        is_max = up == up.amax(dim=0)
        if last_wins:
            arg = K - 1 - (is_max.flip(0).long().cumsum(0) == 0).sum(0)
        else:
            arg = (is_max.long().cumsum(0) == 0).sum(0)                 # how many channels precede the first maximum
        labels[j] = torch.where(inside, keys[j].long()[arg], labels[j])
        if K > 1:
            t2 = up.topk(2, dim=0).values
            margin[j] = torch.where(inside, t2[0] - t2[1], margin[j])
        bound[j] = G.bilinear_bound(masks[j, :K], H, W, False).amax(dim=0).expand(H, W)
    return labels, margin, bound


POST_SIZES = [((4, 4), (8, 8)), ((3, 5), (10, 16)), ((1, 1), (5, 3)), ((16, 25), (33, 50))]
POST_IGNORE = [255, -1]
POST_KMAX = 5
POST_JOB_IMG = [4, 0, 1, 2, 3, 0]
POST_JOB_K = [4, 5, 3, 1, 2, 3]
POST_KEYS = [[0, 7, 3, 12, 1], [0, 19, 2, 20, 5], [0, 6, 4, 1, 1], [0, 1, 1, 1, 1], [0, 15, 1, 1, 1], [0, 20, 9, 1, 1]]   # not increasing


def post_boxes(H: int, W: int) -> torch.Tensor:
    """one box per image: full; empty (y0 == y1); one pixel; flush with the right / bottom border; all but the last row"""
    ye = min(2, H - 1)
    return torch.tensor([[0, H, 0, W], [ye, ye, 0, W], [H // 2, H // 2 + 1, W // 2, W // 2 + 1], [H // 2, H, W // 2, W],
                         [0, H - 1, 0, W]], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def refine_post_case(h: int, w: int):
    """masks fp32 (njobs, Kmax, h, w): a softmax over the job's K channels, NaN beyond"""
    g = torch.Generator().manual_seed(1 + 17 * h + w)
    m = torch.full((len(POST_JOB_K), POST_KMAX, h, w), float("nan"))
    for j, K in enumerate(POST_JOB_K):
        m[j, :K] = torch.softmax(2.0 * torch.randn(K, h, w, generator=g), dim=0)
    return m


def forced_tie_case():
    """(masks (2, 4, 4, 4), job_img, job_K, keys, box, (H, W)): scale 2 (the taps' weights are 1/4 and 3/4) and values on the 2^-8
    grid, so the fp32 blend is exact; channels 1 and 3 are the same plane and hold the largest values, so every pixel is a true tie
    between them: the first wins.  Job 0's keys increase (the lower key wins); job 1's do not (the first channel's key wins)."""
    g = torch.Generator().manual_seed(5)
    lowv = torch.randint(0, 128, (4, 4, 4), generator=g).float() / 256.0
    top = (128 + torch.randint(0, 129, (4, 4), generator=g)).float() / 256.0
    one = lowv.clone()
    one[1], one[3] = top, top
    masks = torch.stack([one, one])
    keys = torch.tensor([[0, 4, 9, 11], [0, 11, 9, 4]], dtype=torch.int32)
    box = torch.tensor([[0, 8, 0, 8]], dtype=torch.int32)
    return masks, [0, 0], [4, 4], keys, box, (8, 8)


def tie_cap(numel: int, max_frac: float = 1e-4) -> int:
    """parity_util.assert_labels_equal_up_to_ties' cap on the number of excused pixels"""
    return max(2, int(max_frac * numel))


# ============================================================================================== refine_merge
def refine_merge_int(a: torch.Tensor, b: torch.Tensor, ignore: int) -> torch.Tensor:
    """the two assignments of the reference's merge, on integers: out = a; out[a == 0] = ignore; out[a + b == 0] = 0"""
    a, b = a.long(), b.long()
    out = a.clone()
    out[a == 0] = ignore
    out[(a + b) == 0] = 0
    return out


MERGE_N = [1, 255, 257, 4096 * 256 + 257]       # the last is past the capped grid's first trip
MERGE_IGNORE = [255, -1, 0]


def merge_table(ignore: int, n: int, offset: int = 0):
    """(a, b) int64 of length n cycling through the full table of {0, 1, 7, ignore}^2, starting at `offset`"""
    vals = torch.tensor([0, 1, 7, ignore])
    i = (torch.arange(n) + offset) % 16
    return vals[i // 4], vals[i % 4]
