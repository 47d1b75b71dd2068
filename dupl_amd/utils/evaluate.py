"""Segmentation / classification scores (reference: utils/evaluate.py).

Same functions and return values as the reference (`multilabel_score`, `_fast_hist`, `scores`, `pseudo_scores`) for
host arrays, plus `ConfusionMatrix`: the histogram the reference rebuilds on the host from lists of per-image numpy maps
(`scores(gts, preds)` at the end of validation) is accumulated on the device instead, image by image
(csrc/eval.hip::confusion_kernel); only nc*nc counters are copied back.  `BoundaryMatrix` (beyond the reference) does the same
for the scores at the object boundaries: the trimap confusion matrices and the Boundary IoU counters (csrc/boundary.hip)."""
import numpy as np
import torch

from .. import ops


def multilabel_score(y_true, y_pred):
    """evaluate.py:4-6 = sklearn.metrics.f1_score of one multi-hot vector: 2TP / (2TP + FP + FN), 0 when undefined."""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    tp = float(((y_true == 1) & (y_pred == 1)).sum())
    fp = float(((y_true == 0) & (y_pred == 1)).sum())
    fn = float(((y_true == 1) & (y_pred == 0)).sum())
    den = 2 * tp + fp + fn
    return 2 * tp / den if den > 0 else 0.0


def _fast_hist(label_true, label_pred, num_classes):
    """evaluate.py:9-16."""
    mask = (label_true >= 0) & (label_true < num_classes)
    hist = np.bincount(num_classes * label_true[mask].astype(int) + label_pred[mask], minlength=num_classes ** 2)
    return hist.reshape(num_classes, num_classes)


def scores_from_hist(hist):
    """evaluate.py:22-36: {"pAcc", "mAcc", "miou" (over classes present in the ground truth), "iou": {class: IoU}}."""
    hist = np.asarray(hist, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
    valid = hist.sum(axis=1) > 0
    return {"pAcc": acc, "mAcc": acc_cls, "miou": np.nanmean(iu[valid]), "iou": dict(zip(range(hist.shape[0]), iu))}


def scores(label_trues, label_preds, num_classes=21):
    """evaluate.py:18-36 for lists of host arrays."""
    hist = np.zeros((num_classes, num_classes))
    for lt, lp in zip(label_trues, label_preds):
        hist += _fast_hist(np.asarray(lt).flatten(), np.asarray(lp).flatten(), num_classes)
    return scores_from_hist(hist)


def pseudo_scores(label_trues, label_preds, num_classes=21):
    """evaluate.py:38-62: predictions equal to 255 are excluded (truth set to 255, prediction to 0)."""
    hist = np.zeros((num_classes, num_classes))
    for lt, lp in zip(label_trues, label_preds):
        lt, lp = np.array(lt).flatten(), np.array(lp).flatten()
        lt[lp == 255] = 255
        lp[lp == 255] = 0
        hist += _fast_hist(lt, lp, num_classes)
    return scores_from_hist(hist)


class ConfusionMatrix:
    """Device-resident (nc, nc) int64 histogram; update(gt, pred) with int64 device tensors of equal shape."""

    def __init__(self, num_classes, device):
        self.num_classes = int(num_classes)
        self.hist = torch.zeros((self.num_classes, self.num_classes), device=device, dtype=torch.int64)

    def update(self, gt, pred):
        ops.confusion_accum(gt, pred, self.hist)

    def scores(self):
        return scores_from_hist(self.hist.cpu().numpy())


class EnsembleMatrix:
    """Device-resident (3, nc, nc) int64 histograms -- student 1, student 2, the mean of their class probabilities -- and the
    (2,) int64 counters (pixels with valid gt, pixels on which the two students agree), filled image by image by the fused pass
    ops.seg_ensemble (csrc/seg_ens.hip): rows 0 and 1 are what two ConfusionMatrix.update calls on the students' own predictions give."""

    def __init__(self, num_classes, device):
        self.num_classes = int(num_classes)
        self.hist = torch.zeros((3, self.num_classes, self.num_classes), device=device, dtype=torch.int64)
        self.counts = torch.zeros((2,), device=device, dtype=torch.int64)

    def update(self, a, b, gt):
        """a, b: the students' accumulated logits (1,C,h,w) or (C,h,w); gt (1,H,W) or (H,W) int64; the logits are up-sampled to gt's size."""
        ops.seg_ensemble(a, b, gt.shape[-2:], gt=gt.reshape(gt.shape[-2:]), hist=self.hist, counts=self.counts)

    def scores(self):
        """[student 1, student 2, ensemble] score dicts."""
        return [scores_from_hist(h) for h in self.hist.cpu().numpy()]

    def agreement(self):
        """The share of the valid pixels on which the two students predict the same class (nan before any valid pixel)."""
        n, same = (int(v) for v in self.counts.cpu())
        return same / n if n else float("nan")


class ThresholdSweep:
    """Device-resident (T, nc, nc) int64 histograms, one confusion matrix per background threshold, filled by the fused pass
    ops.cam_eval (csrc/cam_eval.hip): T thresholds cost the same pass over the label grid as one."""

    def __init__(self, num_classes, thresholds, device):
        self.num_classes = int(num_classes)
        self.thresholds = [float(t) for t in ops.check_thresholds(thresholds)]
        self.hist = torch.zeros((len(self.thresholds), self.num_classes, self.num_classes), device=device, dtype=torch.int64)

    def update(self, cam, cls_label, gt, label_at=None, want_value=False):
        """cam (B,C,h,w), cls_label (B,C), gt (B,H,W) int64 -> (label at thresholds[label_at] or None, max value or None)."""
        return ops.cam_eval(cam, cls_label, gt.shape[-2:], self.thresholds, gt=gt, hist=self.hist, label_at=label_at,
                            want_value=want_value)

    def scores(self):
        return [scores_from_hist(h) for h in self.hist.cpu().numpy()]

    def best(self):
        """(threshold, score dict) of the highest mIoU; the lowest such threshold on equal mIoU."""
        sc = self.scores()
        i = max(range(len(sc)), key=lambda k: (sc[k]["miou"], -k))
        return self.thresholds[i], sc[i]


BOUNDARY_MAX_DIST = 64      # DUPL_SEG_BOUNDARY_MAX_DIST: the farthest distance the boundary kernel searches


def biou_dist(H, W):
    """The Boundary IoU band width of an (H,W) image: the published code's dilation_ratio = 0.02 of the image diagonal, rounded to
    the nearest integer with halves rounded up (375 x 500: 12.5 -> 13), at least 1, clipped to the kernel's maximum distance
    BOUNDARY_MAX_DIST = 64 (reached by images with a diagonal of 3175 pixels and more)."""
    d = int(np.floor(0.02 * np.sqrt(float(H) * float(H) + float(W) * float(W)) + 0.5))
    return max(1, min(BOUNDARY_MAX_DIST, d))


class BoundaryMatrix:
    """Device-resident boundary counters, filled image by image by the fused pass ops.seg_boundary (csrc/boundary.hip):
    hist (max_dist + 1, nc, nc) int64 -- the confusion matrix split by the distance of the pixel to the nearest ground-truth label
    change (bin r - 1 = distance r, the last bin everything farther than max_dist) -- and biou (3, nc) int64, the Boundary IoU
    counters I, G, P (Cheng et al., CVPR 2021) at the per-image distance biou_dist(H, W).  Both are plain sums: all-reduce them."""

    def __init__(self, num_classes, device, max_dist=32):
        self.num_classes, self.max_dist = int(num_classes), int(max_dist)
        if not 1 <= self.max_dist <= BOUNDARY_MAX_DIST:
            raise ValueError(f"max_dist must be 1 .. {BOUNDARY_MAX_DIST}, got {max_dist}")
        self.hist = torch.zeros((self.max_dist + 1, self.num_classes, self.num_classes), device=device, dtype=torch.int64)
        self.biou = torch.zeros((3, self.num_classes), device=device, dtype=torch.int64)

    def update(self, gt, pred):
        """gt, pred: (H,W) or (1,H,W) int64 device tensors of one image."""
        H, W = gt.shape[-2:]
        ops.seg_boundary(gt.reshape(H, W), pred.reshape(H, W), num_classes=self.num_classes, max_dist=self.max_dist,
                         biou_dist=biou_dist(H, W), band_hist=self.hist, biou=self.biou)

    def scores(self):
        """The plain scores: the bins summed are the confusion matrix."""
        return scores_from_hist(self.hist.sum(0).cpu().numpy())

    def trimap_scores(self, widths):
        """{r: score dict of the pixels at most r away from a ground-truth label change} for every r of widths (1 .. max_dist)."""
        h = self.hist.cpu().numpy()
        out = {}
        for r in widths:
            if not 1 <= int(r) <= self.max_dist:
                raise ValueError(f"trimap width must be 1 .. {self.max_dist}, got {r}")
            out[int(r)] = scores_from_hist(h[:int(r)].sum(0))
        return out

    def boundary_iou(self):
        """{"biou": the nan-mean over the classes with ground-truth boundary pixels (G > 0), as miou uses only classes present in the
        ground truth; nan when there is none, "iou": {class: I / (G + P - I)}}."""
        I, G, P = (v.astype(np.float64) for v in self.biou.cpu().numpy())
        with np.errstate(divide="ignore", invalid="ignore"):
            iu = I / (G + P - I)
        present = G > 0
        return {"biou": float(np.nanmean(iu[present])) if present.any() else float("nan"), "iou": dict(zip(range(len(iu)), iu))}


CALIB_MAX_T, CALIB_MAX_BINS = 16, 64      # DUPL_SEG_CALIB_MAX_T, DUPL_SEG_CALIB_MAX_BINS


class CalibrationMatrix:
    """Device-resident calibration counters of one score column, filled image by image by the fused pass ops.seg_calibration
    (csrc/seg_calib.hip) at every temperature of `temperatures` at once: bins (T, nbins, 3), cls (T, nc, 3) and sums (T, 4) int64
    (pixels, correct pixels and fixed-point sums, as the op documents them).  All are plain sums: all-reduce them.  The confidence
    they bin is, bit for bit, what tools/predict --temperature T writes."""

    def __init__(self, num_classes, device, temperatures=(1.0,), nbins=15):
        self.num_classes, self.nbins = int(num_classes), int(nbins)
        self.temperatures = tuple(float(t) for t in temperatures)
        if not 1 <= len(self.temperatures) <= CALIB_MAX_T:
            raise ValueError(f"1 .. {CALIB_MAX_T} temperatures go through one pass, got {len(self.temperatures)}")
        if not 1 <= self.nbins <= CALIB_MAX_BINS:
            raise ValueError(f"nbins must be 1 .. {CALIB_MAX_BINS}, got {nbins}")
        for t in self.temperatures:
            ops.inv_temperature(t)
        T = len(self.temperatures)
        self.bins = torch.zeros((T, self.nbins, 3), device=device, dtype=torch.int64)
        self.cls = torch.zeros((T, self.num_classes, 3), device=device, dtype=torch.int64)
        self.sums = torch.zeros((T, 4), device=device, dtype=torch.int64)

    def tensors(self):
        return [self.bins, self.cls, self.sums]

    def update(self, gt, a, b=None, size=None, is_prob=False):
        """gt (H,W) or (1,H,W) int64; a (and b): the logits (1,C,h,w) or (C,h,w) of one or two students, up-sampled to `size`
        (None: gt's size); is_prob: probabilities at gt's size, scored at T = 1 only (temperatures must be (1.0,))."""
        H, W = gt.shape[-2:]
        ops.seg_calibration(a, b, (H, W) if size is None else size, gt=gt.reshape(H, W), temperatures=self.temperatures,
                            nbins=self.nbins, is_prob=is_prob, bins=self.bins, cls=self.cls, sums=self.sums)

    def scores(self):
        """One dict per temperature: T, n, ece = sum_b n_b / n |acc_b - conf_b|, mce (the largest gap of a non-empty bin), nll, brier,
        acc, mean_conf, reliability [{n, acc, conf} per bin], risk_coverage [{min_conf, coverage, acc} for k = 0 .. nbins - 1: the
        pixels in bins >= k, what --min_conf k / nbins keeps up to the fp32 rounding of conf * nbins], classes {predicted class:
        {n, precision, mean_conf}}.  Empty bins and classes give nan."""
        bins, cls, sums = (t.cpu().numpy().astype(np.float64) for t in self.tensors())
        out = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for t, T in enumerate(self.temperatures):
                n = sums[t, 0]
                nb, okb, cfb = bins[t, :, 0], bins[t, :, 1], bins[t, :, 2] / float(1 << 24)
                acc_b, conf_b = okb / nb, cfb / nb
                gap = np.abs(acc_b - conf_b)
                full = nb > 0
                keep_n, keep_ok = np.cumsum(nb[::-1])[::-1], np.cumsum(okb[::-1])[::-1]
                nc, okc, cfc = cls[t, :, 0], cls[t, :, 1], cls[t, :, 2] / float(1 << 24)
                out.append({
                    "T": T, "n": int(n),
                    "ece": float(np.sum(nb[full] / n * gap[full])) if n else float("nan"),
                    "mce": float(gap[full].max()) if full.any() else float("nan"),
                    "nll": float(sums[t, 2] / float(1 << 20) / n), "brier": float(sums[t, 3] / float(1 << 24) / n),
                    "acc": float(sums[t, 1] / n), "mean_conf": float(cfb.sum() / n) if n else float("nan"),
                    "reliability": [{"n": int(nb[k]), "acc": float(acc_b[k]), "conf": float(conf_b[k])} for k in range(self.nbins)],
                    "risk_coverage": [{"min_conf": k / self.nbins, "coverage": float(keep_n[k] / n), "acc": float(keep_ok[k] / keep_n[k])}
                                      for k in range(self.nbins)],
                    "classes": {c: {"n": int(nc[c]), "precision": float(okc[c] / nc[c]), "mean_conf": float(cfc[c] / nc[c])}
                                for c in range(self.num_classes)},
                })
        return out

    def best_temperature(self, scores=None):
        """{"T_grid": the temperature of the grid with the least mean NLL (the lowest such on equal NLL), "T_fit": the vertex of the
        parabola through it and its two neighbours in log T -- T_grid itself where the minimum sits at an end of the grid, "at_edge":
        whether it does (the sweep should then be widened), "index": T_grid's index in `temperatures`}."""
        sc = self.scores() if scores is None else scores
        order = sorted(range(len(sc)), key=lambda i: sc[i]["T"])
        nll = [sc[i]["nll"] for i in order]
        if any(np.isnan(v) for v in nll):
            return {"T_grid": float("nan"), "T_fit": float("nan"), "at_edge": True, "index": None}
        j = min(range(len(order)), key=lambda k: (nll[k], k))
        Tg = sc[order[j]]["T"]
        edge = j == 0 or j == len(order) - 1
        fit = Tg
        if not edge:
            x0, x1, x2 = (float(np.log(sc[order[k]]["T"])) for k in (j - 1, j, j + 1))
            y0, y1, y2 = nll[j - 1], nll[j], nll[j + 1]
            den = (x1 - x0) * (y1 - y2) - (x1 - x2) * (y1 - y0)
            if den != 0.0:
                fit = float(np.exp(x1 - 0.5 * ((x1 - x0) ** 2 * (y1 - y2) - (x1 - x2) ** 2 * (y1 - y0)) / den))
        return {"T_grid": Tg, "T_fit": fit, "at_edge": edge, "index": order[j]}
