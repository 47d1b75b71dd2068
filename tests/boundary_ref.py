"""numpy / scipy reference of ops.seg_boundary (csrc/boundary.hip), in the filter / erosion formulation -- not the kernel's separable
row / column search:
  dist(L) <= r   <=>  maximum_filter(L, 2r+1, mode='nearest') != minimum_filter(L, 2r+1, mode='nearest')
      (a (2r+1)-window, replicated at the border so that the border itself adds no label, holds two different values);
  the dist_b band of class c at distance d  <=>  mask & ~binary_erosion(mask, ones((3,3)), iterations=d, border_value=0)
      (mask_to_boundary of the Boundary IoU paper's code: cv2's 3x3 erode of the zero-padded mask is the Chebyshev ball).
`brute_*` are the O((HW)^2) definitions themselves, for maps of a few dozen pixels (tests/test_boundary_host.py)."""
import math

import numpy as np
from scipy import ndimage


def biou_dist(H, W):
    """0.02 of the diagonal, halves rounded up, at least 1, at most 64."""
    return max(1, min(64, int(math.floor(0.02 * math.sqrt(H * H + W * W) + 0.5))))


def dist_map(L, R):
    """dist(L) capped at R + 1, int64 (H,W)."""
    L = np.asarray(L, dtype=np.int64)
    out = np.full(L.shape, R + 1, dtype=np.int64)
    for r in range(R, 0, -1):
        near = ndimage.maximum_filter(L, size=2 * r + 1, mode="nearest") != ndimage.minimum_filter(L, size=2 * r + 1, mode="nearest")
        out[near] = r
    return out


def band_hist(gt, pred, nc, R):
    gt, pred = np.asarray(gt, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    ok = (gt >= 0) & (gt < nc) & (pred >= 0) & (pred < nc)
    b = dist_map(gt, R) - 1
    out = np.zeros((R + 1, nc, nc), dtype=np.int64)
    np.add.at(out, (b[ok], gt[ok], pred[ok]), 1)
    return out


def boundary_band(mask, d):
    """mask_to_boundary: the pixels of mask within Chebyshev distance d of its complement, the outside of the image included."""
    mask = np.asarray(mask, dtype=bool)
    if not mask.any():
        return mask
    return mask & ~ndimage.binary_erosion(mask, structure=np.ones((3, 3), dtype=bool), iterations=int(d), border_value=0)


def biou_counts(gt, pred, nc, d):
    """(3, nc) int64: I, G, P over the pixels with valid gt and valid pred."""
    gt, pred = np.asarray(gt, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    ok = (gt >= 0) & (gt < nc) & (pred >= 0) & (pred < nc)
    out = np.zeros((3, nc), dtype=np.int64)
    for c in range(nc):
        g = boundary_band(gt == c, d) & ok
        p = boundary_band(pred == c, d) & ok
        out[0, c], out[1, c], out[2, c] = (g & p).sum(), g.sum(), p.sum()
    return out


def reference(gt, pred, nc, R, d=0):
    """(band_hist, biou counters or None, dist_gt, dist_pred) as ops.seg_boundary(..., want_dist=True) returns them."""
    return (band_hist(gt, pred, nc, R), biou_counts(gt, pred, nc, d) if d > 0 else None,
            dist_map(gt, R).astype(np.uint8), dist_map(pred, R).astype(np.uint8))


def scores_from_hist(hist):
    hist = np.asarray(hist, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.diag(hist).sum() / hist.sum()
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
    valid = hist.sum(axis=1) > 0
    return {"pAcc": acc, "miou": np.nanmean(iu[valid]) if valid.any() else float("nan")}


def boundary_scores(pairs, nc, widths, R=32):
    """The "boundary" dict eval_seg reports, from a list of (gt, pred) host maps: per-image d = biou_dist(H, W), counters summed."""
    hist = np.zeros((R + 1, nc, nc), dtype=np.int64)
    cnt = np.zeros((3, nc), dtype=np.int64)
    for gt, pred in pairs:
        H, W = np.asarray(gt).shape
        hist += band_hist(gt, pred, nc, R)
        cnt += biou_counts(gt, pred, nc, biou_dist(H, W))
    I, G, P = (v.astype(np.float64) for v in cnt)
    with np.errstate(divide="ignore", invalid="ignore"):
        iu = I / (G + P - I)
    present = G > 0
    trimap = {}
    for r in widths:
        s = scores_from_hist(hist[:r].sum(0))
        trimap[int(r)] = {"miou": s["miou"], "pAcc": s["pAcc"]}
    return {"biou": float(np.nanmean(iu[present])) if present.any() else float("nan"), "biou_iou": dict(zip(range(nc), iu)),
            "trimap": trimap}


# ---------------------------------------------------------------------------------------------------------------- brute force
def brute_dist(L, R, border=False):
    """The definition: for every pixel the nearest pixel inside the image with another label, Chebyshev, capped at R + 1; with
    border=True the outside of the image counts as another label."""
    L = np.asarray(L, dtype=np.int64)
    H, W = L.shape
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.full((H, W), R + 1, dtype=np.int64)
    for y in range(H):
        for x in range(W):
            cheb = np.maximum(np.abs(ys - y), np.abs(xs - x))
            other = L != L[y, x]
            best = cheb[other].min() if other.any() else R + 1
            if border:
                best = min(best, min(x, y, W - 1 - x, H - 1 - y) + 1)
            out[y, x] = min(best, R + 1)
    return out


def brute(gt, pred, nc, R, d):
    gt, pred = np.asarray(gt, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    H, W = gt.shape
    big = max(R, d, H, W)
    dg, dgb, dpb = brute_dist(gt, R), brute_dist(gt, big, True), brute_dist(pred, big, True)
    hist = np.zeros((R + 1, nc, nc), dtype=np.int64)
    cnt = np.zeros((3, nc), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            g, p = gt[y, x], pred[y, x]
            if not (0 <= g < nc and 0 <= p < nc):
                continue
            hist[dg[y, x] - 1, g, p] += 1
            gb, pb = dgb[y, x] <= d, dpb[y, x] <= d
            cnt[0, g] += gb and pb and g == p
            cnt[1, g] += gb
            cnt[2, p] += pb
    return hist, cnt, dg, brute_dist(pred, R)
