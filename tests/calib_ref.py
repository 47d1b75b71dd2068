"""Float64 reference of dupl_seg_calib (include/dupl_hip.h, csrc/seg_calib.hip), independent of the kernels, and the host binning of
fp32 confidences by the header's formula.

The reference takes the header's SAMPLING -- the fp32 source index and weights of the bilinear taps (r = fma(scale, o + 0.5, -0.5)
with the fp32 scale in / out, clamped at 0), and the fp32 inverse temperature -- and does every value computation in float64: the
scaled logits, the taps, the soft-max, the mean of two students, the log and the Brier score.  A pixel is AMBIGUOUS when its
float64 confidence lies within EPS of a bin edge or its two largest probabilities are closer than EPS, at any temperature of the
call: fp32 may then bin or decide it either way.  EPS = 2e-6 is >= 6 x the 1e-7 probability error csrc/seg_pixel.h documents for
its exp, plus the rounding of the mean."""
import numpy as np

EPS = 2e-6
AMBIGUOUS_CAP = 0.005        # at most this share of a case's pixels may be set aside


def inv_temperature(T):
    """the fp32 1 / T (ops.inv_temperature's definition, written again)"""
    return float(np.float32(1.0) / np.float32(T))


def logits(shape, seed, scale=2.0):
    """seeded N(0, scale^2) fp32 logits"""
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def gt_for(C, H, W, seed):
    """a seeded ground truth over [0, C) with the three kinds of skipped values planted: 255, -1 and C"""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, C, (H, W)).astype(np.int64)
    r = rng.random((H, W))
    gt[r < 0.04] = 255
    gt[(r >= 0.04) & (r < 0.06)] = -1
    gt[(r >= 0.06) & (r < 0.08)] = C
    return gt


def _src(out, inn):
    """the header's source index: (i0, i1, weight of i1) per output coordinate, the fp32 arithmetic of the kernels"""
    scale = np.float32(inn) / np.float32(out)
    o = np.arange(out, dtype=np.float64)
    r = np.float32(np.float64(scale) * (o + 0.5) - 0.5)          # the product is exact in float64: one rounding, as the fma
    r = np.maximum(r, np.float32(0.0))
    i0 = np.minimum(r.astype(np.int64), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = (r - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, l1.astype(np.float64)


def upsample(v, H, W):
    """(C,h,w) float64 -> (C,H,W): bilinear, align_corners False; the values themselves when the sizes agree"""
    C, h, w = v.shape
    if (h, w) == (H, W):
        return v
    y0, y1, ly = _src(H, h)
    x0, x1, lx = _src(W, w)
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = (1 - lx) * v[:, y0][:, :, x0] + lx * v[:, y0][:, :, x1]
    bot = (1 - lx) * v[:, y1][:, :, x0] + lx * v[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def _log_softmax(u):
    m = u.max(0, keepdims=True)
    return u - m - np.log(np.exp(u - m).sum(0, keepdims=True))


def pixel_scores(a, b, size, temperature=1.0, is_prob=False):
    """-> p (C,H,W) float64 of one temperature: the soft-max of the up-sampled scaled logits, the mean of the two students', or the
    given probabilities (their mean); and logp (C,H,W), the log of it computed in the logit domain for one student"""
    H, W = size
    if is_prob:
        p = a.astype(np.float64) if b is None else 0.5 * (a.astype(np.float64) + b.astype(np.float64))
        with np.errstate(divide="ignore"):
            return p, np.log(np.maximum(p, np.finfo(np.float32).tiny))
    k = np.float64(np.float32(inv_temperature(temperature)))
    la = _log_softmax(upsample(a.astype(np.float64) * k, H, W))
    if b is None:
        return np.exp(la), la
    p = 0.5 * (np.exp(la) + np.exp(_log_softmax(upsample(b.astype(np.float64) * k, H, W))))
    return p, np.log(np.maximum(p, np.finfo(np.float32).tiny))


def reference(a, b, size, gt, temperatures=(1.0,), nbins=15, is_prob=False):
    """-> dict(bins (T,nbins,3) float64: pixels, correct, sum of conf; cls (T,C,3) the same per predicted class; sums (T,4): valid,
    correct, sum of nll, sum of brier -- all over the pixels with 0 <= gt < C; ambiguous (H,W) bool: see the module docstring)"""
    C = a.shape[0]
    H, W = size
    T = len(temperatures)
    valid = (gt >= 0) & (gt < C)
    g = np.where(valid, gt, 0)
    bins, cls, sums = np.zeros((T, nbins, 3)), np.zeros((T, C, 3)), np.zeros((T, 4))
    amb = np.zeros((H, W), dtype=bool)
    for t, temp in enumerate(temperatures):
        p, logp = pixel_scores(a, b, size, temp, is_prob)
        win = p.argmax(0)
        conf = p.max(0)
        if C > 1:
            top2 = np.partition(p, C - 2, axis=0)[C - 2:]
            amb |= (top2[1] - top2[0]) < EPS
        e = conf * nbins
        k = np.rint(e)
        amb |= (np.abs(e - k) < EPS * nbins) & (k >= 1) & (k <= nbins - 1)
        b_ = np.minimum(np.floor(e).astype(np.int64), nbins - 1)
        ok = (win == g) & valid
        nll = -np.take_along_axis(logp, g[None], 0)[0]
        brier = (p * p).sum(0) - 2.0 * np.take_along_axis(p, g[None], 0)[0] + 1.0
        for arr, idx, n in ((bins, b_, nbins), (cls, win, C)):
            arr[t, :, 0] = np.bincount(idx[valid], minlength=n)
            arr[t, :, 1] = np.bincount(idx[ok], minlength=n)
            arr[t, :, 2] = np.bincount(idx[valid], weights=conf[valid], minlength=n)
        sums[t] = [valid.sum(), ok.sum(), nll[valid].sum(), brier[valid].sum()]
    return {"bins": bins, "cls": cls, "sums": sums, "ambiguous": amb & valid, "valid": valid}


def bin_conf32(conf, nbins):
    """the header's bin of an fp32 confidence: min((int)(conf * (float)nbins), nbins - 1), the product in fp32"""
    assert conf.dtype == np.float32
    return np.minimum((conf * np.float32(nbins)).astype(np.int64), nbins - 1)


def host_counters(label, conf, gt, C, nbins):
    """What one temperature of dupl_seg_calib must hold, from dupl_seg_decide's label (H,W) uint8 and conf (H,W) fp32 on the scaled
    logits: bins (nbins,3), cls (C,3) int64 -- pixels, pixels with label == gt, sum of (int64)rint(conf * 2^24) -- and (valid, correct)."""
    valid = (gt >= 0) & (gt < C)
    lab = label.astype(np.int64)
    ok = valid & (lab == gt)
    q = np.rint(conf * np.float32(16777216.0)).astype(np.int64)
    b = bin_conf32(conf, nbins)
    out = []
    for idx, n in ((b, nbins), (lab, C)):
        arr = np.zeros((n, 3), dtype=np.int64)
        arr[:, 0] = np.bincount(idx[valid], minlength=n)
        arr[:, 1] = np.bincount(idx[ok], minlength=n)
        np.add.at(arr[:, 2], idx[valid], q[valid])
        out.append(arr)
    return out[0], out[1], np.array([valid.sum(), ok.sum()], dtype=np.int64)


def ece(bins_t):
    """sum_b n_b / n |acc_b - conf_b| of one temperature's (nbins,3) float table (sum of conf in natural units)"""
    n = bins_t[:, 0].sum()
    full = bins_t[:, 0] > 0
    return float(np.sum(np.abs(bins_t[full, 1] - bins_t[full, 2]) / n))


def best_temperature(temperatures, nll):
    """(T_grid, T_fit, at_edge): the temperature of least nll, the vertex of the parabola through it and its neighbours in log T
    (numpy's polyfit), T_grid at an end of the sorted grid"""
    order = np.argsort(temperatures, kind="stable")
    T, y = np.asarray(temperatures, dtype=np.float64)[order], np.asarray(nll, dtype=np.float64)[order]
    j = int(np.argmin(y))
    if j == 0 or j == len(T) - 1:
        return float(T[j]), float(T[j]), True
    c2, c1, _ = np.polyfit(np.log(T[j - 1:j + 2]) - np.log(T[j]), y[j - 1:j + 2], 2)
    return float(T[j]), float(T[j] * np.exp(-c1 / (2.0 * c2))), False


# the shapes of the GPU tests: (C, h, w, H, W); the smallest at which each path of the kernel can go wrong
IDENTITY = [(21, 37, 53, 37, 53), (24, 37, 53, 37, 53), (25, 37, 53, 37, 53), (81, 37, 53, 37, 53), (1, 37, 53, 37, 53)]
RESIZED = [(81, 7, 9, 37, 53), (3, 7, 9, 37, 53), (81, 28, 28, 70, 130), (21, 40, 40, 17, 23)]
EDGES = [(21, 37, 1, 37, 1), (21, 1, 53, 1, 53), (21, 5, 65, 5, 65), (5, 3, 4, 1, 65), (5, 4, 3, 37, 1)]
# against float64: (shape, students, is_prob) x nbins 15 and 64 at T = 1, 0.5, 2, 4 (is_prob: T = 1)
F64_TEMPS = (1.0, 0.5, 2.0, 4.0)
F64_CASES = ([(s, n, False) for s in [(3, 37, 53, 37, 53), (21, 37, 53, 37, 53), (25, 37, 53, 37, 53), (81, 37, 53, 37, 53),
                                      (81, 7, 9, 37, 53), (3, 7, 9, 37, 53), (81, 28, 28, 70, 130), (21, 40, 40, 17, 23)] for n in (1, 2)] +
             [((21, 37, 53, 37, 53), n, True) for n in (1, 2)])


def case_inputs(shape, students, is_prob=False, seed=0):
    """(a, b or None, gt) of a test case: N(0, 2^2) logits (soft-maxed in float64 and rounded to fp32 for is_prob), gt_for's ground truth"""
    C, h, w, H, W = shape
    base = 1000 * seed + 7 * C + h + 3 * H
    ins = [logits((C, h, w), base + k) for k in range(students)]
    if is_prob:
        ins = [np.exp(_log_softmax(z.astype(np.float64))).astype(np.float32) for z in ins]
    return ins[0], (ins[1] if students == 2 else None), gt_for(C, H, W, base + 5)


def f64_case(shape, students, is_prob, nbins):
    """-> (a, b, gt with the ambiguous pixels set to 255, reference on that gt, share of the valid pixels set aside)"""
    a, b, gt = case_inputs(shape, students, is_prob)
    temps = (1.0,) if is_prob else F64_TEMPS
    first = reference(a, b, shape[3:], gt, temps, nbins, is_prob)
    share = float(first["ambiguous"].sum()) / float(shape[3] * shape[4])
    gt2 = np.where(first["ambiguous"], 255, gt)
    return a, b, gt2, reference(a, b, shape[3:], gt2, temps, nbins, is_prob), share


PLANTED = (21, 96, 128)      # the planted temperature: z ~ N(0, 3^2), gt ~ softmax(z / 2)


def planted(students=1, seed=11):
    """-> (list of `students` independent logit draws (C,H,W) fp32, gt (H,W) sampled from softmax(z_0 / 2) with a fixed seed)"""
    C, H, W = PLANTED
    zs = [logits((C, H, W), seed + k, scale=3.0) for k in range(students)]
    p = np.exp(_log_softmax(zs[0].astype(np.float64) / 2.0))
    u = np.random.default_rng(seed + 100).random((1, H, W))
    gt = np.minimum((np.cumsum(p, 0) < u).sum(0), C - 1).astype(np.int64)
    return zs, gt
