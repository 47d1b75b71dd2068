"""Offline multi-scale + flip segmentation inference and DenseCRF post-processing (reference: tools/eval_seg_voc.py:38-193 and
tools/eval_seg_coco_ddp.py:54-256).

    python -m dupl_amd.tools.eval_seg --model_path work_dir/checkpoints/checkpoint.pth ...   (needs a data loader)

`msc_seg_logits` is the per-image core: for every scale the two students run on [x_s; flip(x_s)], the low-resolution
logits are up-sampled to the label size, the flipped half is flipped back and added, and the scales are combined with
an element-wise max -- fused into one accumulate kernel per scale (csrc/eval.hip::msc_seg_accum_kernel), so the
(3, 2, C, H, W) stack the reference builds is never materialised.  `load_checkpoint` reads the reference's checkpoint
format (torch.save(model.state_dict()) of the DDP-wrapped model: keys prefixed `module.`, train_final_voc.py:514-519).
With `--crf 1` the reference's `crf_proc` follows on the device (`crf_proc` below): DenseCRF(10, 1, 1, 4, 121, 5) on the better
student's saved logits, `seg_crf` scores and the prediction PNGs.  It is the exact mean-field update (utils/dcrf.py of this
package, csrc/crf.hip), not pydensecrf's lattice approximation, and its scores have not been compared with pydensecrf's.
Beyond the reference, `--ensemble 1` also scores the mean of the two students' class probabilities: per image one fused pass
(ops.seg_ensemble, csrc/seg_ens.hip) up-samples both students' logits and fills the three confusion matrices and the students'
agreement counters; `--crf_branch ens` runs the CRF stage on that mean.  `--boundary 1` also scores every column at the object
boundaries: per image and column one fused pass (ops.seg_boundary, csrc/boundary.hip) splits the confusion matrix by the Chebyshev
distance to the nearest ground-truth label change and fills the Boundary IoU counters (Cheng et al., CVPR 2021); the trimap mIoU of
every `--trimap_widths` width (DeepLab's trimap score) and the Boundary IoU are printed under the table, returned under the key
"boundary" of every score dict and, with `--crf 1`, reported for seg_crf too, so the CRF's effect at the boundary reads off one run.
`--crf_method {exact,lattice}` chooses the CRF stage's inference (utils/dcrf.py).  `--calibration 1` scores whether the confidence
tools/predict publishes means anything: per image and column one fused pass (ops.seg_calibration, csrc/seg_calib.hip) bins the
winner's confidence against the ground truth at every temperature of `--temp_sweep` at once -- ECE, MCE, NLL, Brier, reliability
bins, risk-coverage and the temperature of least NLL, printed under the boundary lines, returned under the key "calibration" and
written in full to `--calib_json`; with `--crf 1` the CRF's marginals are scored at T = 1.  The confidence scored at T is, bit for
bit, what `predict --temperature T` writes.  Without these flags nothing changes."""
from collections import OrderedDict

import torch

from .. import ops
from ..model.backbone import FAMILY
from ..utils import evaluate
from ..utils.pyutils import format_tabs


def load_checkpoint(model, path_or_state):
    """tools/eval_seg_voc.py:173-178: strip the DDP `module.` prefix and load strictly."""
    sd = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, str) else path_or_state
    new = OrderedDict((k.replace("module.", ""), v) for k, v in sd.items())
    # a checkpoint of another --backbone: say so in one line (strict loading would list every tensor of every block)
    want = model.state_dict()
    for k, v in new.items():
        if k.endswith("encoder.cls_token") and k in want and v.shape[-1] != want[k].shape[-1]:
            raise ValueError(f"checkpoint is of another backbone: expected width {want[k].shape[-1]} "
                             f"(--backbone {getattr(model, '_ctor', ('?',))[0]}), found width {v.shape[-1]} ({k})")
    depth = {m: 1 + max((int(k.split(".")[3]) for k in d if k.startswith("branch1.encoder.blocks.")), default=-1)
             for m, d in (("expected", want), ("found", new))}
    if depth["expected"] != depth["found"] and depth["found"] > 0:
        raise ValueError(f"checkpoint is of another backbone: expected depth {depth['expected']} "
                         f"(--backbone {getattr(model, '_ctor', ('?',))[0]}), found depth {depth['found']}")
    model.load_state_dict(new, strict=True)
    return model


def msc_seg_logits(model, inputs, out_size, scales=(1.0, 1.5, 1.25)):
    """inputs (1,3,h,w) on the device -> (seg_1, seg_2), each (1,C1,H,W): eval_seg_voc.py:52-75."""
    assert inputs.shape[0] == 1
    core = model.module if hasattr(model, "module") else model
    _, _, h, w = inputs.shape
    H, W = int(out_size[0]), int(out_size[1])
    accs = None
    with torch.no_grad():
        for i, sc in enumerate(scales):
            # F.interpolate(inputs, [int(h*sc), int(w*sc)]) and cat([x, x.flip(-1)]) in one kernel (flip_cat)
            cat = ops.resize_bilinear(inputs.contiguous().float(), int(h * sc), int(w * sc), flip_cat=True)
            res = core(cat)
            segs = (res["branch1"][1], res["branch2"][1])
            if accs is None:
                C1 = segs[0].shape[1]
                accs = [torch.empty((1, C1, H, W), device=inputs.device, dtype=torch.float32) for _ in range(2)]
            for acc, s in zip(accs, segs):
                ops.msc_seg_accum_(acc, s, mode=(0 if i == 0 else 1))
    return accs[0], accs[1]


def msc_seg_logits_coco(model, inputs, scales=(1.0, 1.25, 1.5), size=448):
    """tools/eval_seg_coco_ddp.py:76-119: the image is first resized to size x size; per scale the logits of
    [x_s; flip(x_s)] are resized to the scale-1 logit size, the flipped half is flipped back and added, and the scales
    are SUMMED (VOC takes the max at label size).  -> (seg_1, seg_2), each (1,C1,size/16,size/16); the caller up-samples
    the sum to the label size (ops.upsample_argmax)."""
    assert inputs.shape[0] == 1
    core = model.module if hasattr(model, "module") else model
    x = ops.resize_bilinear(inputs.contiguous().float(), size, size)
    accs = None
    order = [1.0] + [float(s) for s in scales if float(s) != 1.0]      # the reference always starts with scale 1
    with torch.no_grad():
        for i, sc in enumerate(order):
            cat = ops.resize_bilinear(x, int(size * sc), int(size * sc), flip_cat=True)
            res = core(cat)
            segs = (res["branch1"][1], res["branch2"][1])
            if accs is None:
                C1, hs, ws = segs[0].shape[1:]
                accs = [torch.empty((1, C1, hs, ws), device=x.device, dtype=torch.float32) for _ in range(2)]
            for acc, s in zip(accs, segs):
                ops.msc_seg_accum_(acc, s, mode=(0 if i == 0 else 2))
    return accs[0], accs[1]


def _ensemble_update(em, bms, seg, labels):
    """One image into the EnsembleMatrix; with boundary matrices the same fused pass also hands back the ensemble's prediction for bms[2]."""
    if not bms:
        return em.update(seg[0], seg[1], labels)
    gt = labels.reshape(labels.shape[-2:])
    pred, _ = ops.seg_ensemble(seg[0], seg[1], gt.shape, gt=gt, hist=em.hist, counts=em.counts, want_pred=True)
    bms[2].update(gt, pred)


def _ensemble_scores(em):
    """[student 1, student 2, ensemble] of an EnsembleMatrix; the ensemble's dict also carries "agree", the share of the valid
    pixels on which the two students predict the same class."""
    sc = em.scores()
    sc[2]["agree"] = em.agreement()
    return sc


def parse_trimap_widths(text):
    """--trimap_widths: "1,2,4" -> (1, 2, 4); positive integers, ascending, at most evaluate.BOUNDARY_MAX_DIST."""
    import argparse
    try:
        widths = tuple(int(v) for v in str(text).strip("()[] ").split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"trimap widths are integers separated by commas, got {text!r}")
    if not widths or widths[0] < 1 or widths[-1] > evaluate.BOUNDARY_MAX_DIST or any(b <= a for a, b in zip(widths, widths[1:])):
        raise argparse.ArgumentTypeError(f"trimap widths must be ascending integers in 1 .. {evaluate.BOUNDARY_MAX_DIST}, got {text!r}")
    return widths


def boundary_scores(bm, widths):
    """The "boundary" entry of a score dict, from a filled evaluate.BoundaryMatrix: {"biou": mean Boundary IoU, "biou_iou": {class: value},
    "trimap": {width: {"miou", "pAcc"} of the pixels at most `width` away from a ground-truth label change}}."""
    b = bm.boundary_iou()
    return {"biou": b["biou"], "biou_iou": b["iou"],
            "trimap": {r: {"miou": s["miou"], "pAcc": s["pAcc"]} for r, s in bm.trimap_scores(widths).items()}}


def format_boundary(scores, name_list):
    """One line per column: the Boundary IoU and the trimap mIoU per width (x 100, as the table above it)."""
    return "\n".join(f"boundary {n}: BIoU {100 * s['boundary']['biou']:.3f} | trimap mIoU " +
                     " ".join(f"@{r} {100 * t['miou']:.3f}" for r, t in s["boundary"]["trimap"].items())
                     for s, n in zip(scores, name_list))


def parse_temp_sweep(text):
    """--temp_sweep "LO:HI:N" -> the temperatures of one pass: 1.0 first, then the geometric grid LO .. HI of N points (rounded to 12
    significant digits, so 0.5:4:13 holds 2.0 itself) without its own 1.0.  0 < LO < HI, 2 <= N <= 15: with T = 1 at most
    evaluate.CALIB_MAX_T = 16 temperatures."""
    import argparse
    try:
        lo, hi, n = str(text).strip().split(":")
        lo, hi, n = float(lo), float(hi), int(n)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a temperature sweep is LO:HI:N, got {text!r}")
    if not (0.0 < lo < hi < float("inf")) or not 2 <= n <= evaluate.CALIB_MAX_T - 1:
        raise argparse.ArgumentTypeError(f"a temperature sweep needs 0 < LO < HI and 2 <= N <= {evaluate.CALIB_MAX_T - 1}, got {text!r}")
    grid = [float(f"{lo * (hi / lo) ** (i / (n - 1)):.12g}") for i in range(n)]
    return (1.0,) + tuple(t for t in grid if t != 1.0)


def calibration_scores(cm):
    """The "calibration" entry of a score dict, from a filled evaluate.CalibrationMatrix: {"temperatures", "nbins", "scores": one
    dict per temperature (CalibrationMatrix.scores; index 0 is T = 1), "best": CalibrationMatrix.best_temperature}."""
    sc = cm.scores()
    return {"temperatures": list(cm.temperatures), "nbins": cm.nbins, "scores": sc, "best": cm.best_temperature(sc)}


def format_calibration(scores, name_list):
    """One line per column: the scores at T = 1, then the temperature of least NLL with ECE and NLL there."""
    lines = []
    for s, n in zip(scores, name_list):
        c = s["calibration"]
        one, best = c["scores"][0], c["best"]
        line = (f"calibration {n}: ECE {one['ece']:.4f} MCE {one['mce']:.4f} NLL {one['nll']:.4f} Brier {one['brier']:.4f} "
                f"conf {one['mean_conf']:.4f} acc {one['acc']:.4f} at T=1")
        if len(c["scores"]) > 1 and best["index"] is not None:
            at = c["scores"][best["index"]]
            line += f" | best T {best['T_grid']:.4g} (fit {best['T_fit']:.4g}): ECE {at['ece']:.4f} NLL {at['nll']:.4f}"
            if best["at_edge"]:
                line += " -- at the end of the sweep: widen --temp_sweep"
        lines.append(line)
    return "\n".join(lines)


def _calibration_matrices(calibration, n, num_classes, dev):
    return [evaluate.CalibrationMatrix(num_classes, dev, **calibration) for _ in range(n)] if calibration else None


def _calibration_update(cals, seg, labels):
    """One image into every column's CalibrationMatrix: each student alone, then (a third matrix) the two together."""
    for k in range(2):
        cals[k].update(labels, seg[k])
    if len(cals) > 2:
        cals[2].update(labels, seg[0], seg[1])


def _boundary_matrices(boundary, n, num_classes, dev):
    return [evaluate.BoundaryMatrix(num_classes, dev, max_dist=max(boundary)) for _ in range(n)] if boundary else None


def validate_coco(model, data_loader, args, num_classes=81, cat_list=None, process_group=None, keep_logits=None, ensemble=False,
                  boundary=None, calibration=None):
    """eval_seg_coco_ddp._validate on this rank's shard of the loader (the reference splits the val set round-robin over
    the ranks, tools/eval_seg_coco_ddp.py:239-245, and every rank scores its own shard).  With `process_group` (or an
    initialised default group) the per-rank confusion matrices are additionally summed over the ranks -- nc^2 int64
    counters, the only exchange of the evaluation path -- so that every rank returns the scores of the WHOLE set.
    ensemble=True: one fused pass per image (ops.seg_ensemble) up-samples both students' logits, scores each student and the mean
    of their class probabilities -> (seg_score_1, seg_score_2, seg_score_ens); the students' scores are the same counts.
    boundary=widths: every column also feeds an evaluate.BoundaryMatrix and its score dict gains "boundary" (boundary_scores).
    calibration={"temperatures", "nbins"}: every column also feeds an evaluate.CalibrationMatrix -- the up-sampling form, from the
    low-resolution logits -- and its score dict gains "calibration" (calibration_scores)."""
    import torch.distributed as dist
    from ..utils.train_helper import _device_of, _fetch
    dev = _device_of(model)
    cms = [evaluate.ConfusionMatrix(num_classes, dev) for _ in range(2)]
    em = evaluate.EnsembleMatrix(num_classes, dev) if ensemble else None
    bms = _boundary_matrices(boundary, 3 if ensemble else 2, num_classes, dev)
    cals = _calibration_matrices(calibration, 3 if ensemble else 2, num_classes, dev)
    model.eval()
    scales = getattr(args, "scales", (1.0, 1.25, 1.5))
    for data in data_loader:
        inputs, labels, _ = _fetch(data, dev)
        seg = msc_seg_logits_coco(model, inputs, scales, getattr(args, "crop_size", 448))
        H, W = labels.shape[1:]
        if ensemble:
            _ensemble_update(em, bms, seg, labels)
        if cals:
            _calibration_update(cals, seg, labels)
        for k in range(2):
            if not ensemble or bms:
                pred = ops.upsample_argmax(seg[k], H, W)
            if not ensemble:
                cms[k].update(labels, pred)
            if bms:
                bms[k].update(labels, pred)
            if keep_logits is not None:          # eval_seg_coco_ddp.py:127-128 saves the summed low-resolution logits
                keep_logits(data[0], k + 1, seg[k])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
        for t in (([em.hist, em.counts] if ensemble else [c.hist for c in cms]) + [t for b in bms or [] for t in (b.hist, b.biou)] +
                  [t for c in cals or [] for t in c.tensors()]):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
    sc = _ensemble_scores(em) if ensemble else [c.scores() for c in cms]
    for s, b in zip(sc, bms or []):
        s["boundary"] = boundary_scores(b, boundary)
    for s, c in zip(sc, cals or []):
        s["calibration"] = calibration_scores(c)
    if cat_list is not None:
        print(format_tabs(sc, ["Seg_1", "Seg_2", "Seg_ens"][:len(sc)], cat_list=cat_list))
        if bms:
            print(format_boundary(sc, ["Seg_1", "Seg_2", "Seg_ens"]))
        if cals:
            print(format_calibration(sc, ["Seg_1", "Seg_2", "Seg_ens"]))
    return tuple(sc)


def validate(model, data_loader, args, num_classes=21, cat_list=None, keep_logits=None, ensemble=False, boundary=None,
             calibration=None):
    """eval_seg_voc._validate: multi-scale seg predictions of both students over a loader of
    (name, inputs (1,3,h,w), labels (1,H,W), cls_label) -> (seg_score_1, seg_score_2).
    keep_logits(name, branch, logits) is called with the (1,C1,H,W) device logits (the reference np.save()s them for the
    CRF stage).  ensemble=True: one fused pass per image (ops.seg_ensemble) scores each student and the mean of their class
    probabilities -> (seg_score_1, seg_score_2, seg_score_ens); the students' scores are the same counts.
    boundary=widths: every column also feeds an evaluate.BoundaryMatrix and its score dict gains "boundary" (boundary_scores).
    calibration={"temperatures", "nbins"}: every column also feeds an evaluate.CalibrationMatrix -- the identity form, the logits are
    at label size -- and its score dict gains "calibration" (calibration_scores)."""
    from ..utils.train_helper import _device_of, _fetch
    dev = _device_of(model)
    cms = [evaluate.ConfusionMatrix(num_classes, dev) for _ in range(2)]
    em = evaluate.EnsembleMatrix(num_classes, dev) if ensemble else None
    bms = _boundary_matrices(boundary, 3 if ensemble else 2, num_classes, dev)
    cals = _calibration_matrices(calibration, 3 if ensemble else 2, num_classes, dev)
    model.eval()
    for data in data_loader:
        inputs, labels, _ = _fetch(data, dev)
        seg = msc_seg_logits(model, inputs, labels.shape[1:], getattr(args, "scales", (1.0, 1.5, 1.25)))
        if ensemble:
            _ensemble_update(em, bms, seg, labels)
        if cals:
            _calibration_update(cals, seg, labels)
        for k in range(2):
            if not ensemble or bms:
                pred = ops.argmax_channels(seg[k])
            if not ensemble:
                cms[k].update(labels, pred)
            if bms:
                bms[k].update(labels, pred)
            if keep_logits is not None:
                keep_logits(data[0], k + 1, seg[k])
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        # main() shards the split over the ranks for both datasets: the score is of the summed confusion matrices
        for t in (([em.hist, em.counts] if ensemble else [c.hist for c in cms]) + [t for b in bms or [] for t in (b.hist, b.biou)] +
                  [t for c in cals or [] for t in c.tensors()]):
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
    sc = _ensemble_scores(em) if ensemble else [c.scores() for c in cms]
    for s, b in zip(sc, bms or []):
        s["boundary"] = boundary_scores(b, boundary)
    for s, c in zip(sc, cals or []):
        s["calibration"] = calibration_scores(c)
    if cat_list is not None and (not dist.is_initialized() or dist.get_rank() == 0):
        print(format_tabs(sc, ["Seg_1", "Seg_2", "Seg_ens"][:len(sc)], cat_list=cat_list))
        if bms:
            print(format_boundary(sc, ["Seg_1", "Seg_2", "Seg_ens"]))
        if cals:
            print(format_calibration(sc, ["Seg_1", "Seg_2", "Seg_ens"]))
    return tuple(sc)


def crf_proc(branch, names, image_path, label_of, logits_dir, segs_dir, segs_rgb_dir, num_classes, dev, process_group=None,
             boundary=None, method=None, calibration=None):
    """tools/eval_seg_voc.py:94-153 / tools/eval_seg_coco_ddp.py:142-202 on the device, over this rank's `names`: per image the
    saved logits of `branch` are resized to the JPEG's size, softmax + DenseCRF(10, 1, 1, 4, 121, 5) + argmax run on the device,
    the label PNG (and the palette PNG) are written and a device ConfusionMatrix is accumulated; with several ranks the
    matrices are summed.  image_path(name) -> JPEG path; label_of(name, image) -> (H,W) ground truth.  Returns the scores.
    branch "ens": both students' saved logits go through ops.seg_ensemble and the CRF runs on the mean of their probabilities.
    method "exact" / "lattice": the CRF's inference (None = utils.dcrf.METHOD).  boundary=widths: the predictions also feed an
    evaluate.BoundaryMatrix and the returned dict gains "boundary" (boundary_scores).  calibration={"nbins", ...}: the CRF's marginals
    also feed an evaluate.CalibrationMatrix as probabilities, at T = 1 only (they are not a soft-max of the logits, no temperature
    is fitted for them), and the returned dict gains "calibration" (calibration_scores)."""
    import os
    import numpy as np
    import torch.distributed as dist
    from PIL import Image
    from ..utils import imutils
    from ..utils.dcrf import DenseCRF
    post = DenseCRF(iter_max=10, pos_xy_std=1, pos_w=1, bi_xy_std=121, bi_rgb_std=5, bi_w=4)
    if method is not None:
        post.method = method
    cm = evaluate.ConfusionMatrix(num_classes, dev)
    bm = evaluate.BoundaryMatrix(num_classes, dev, max_dist=max(boundary)) if boundary else None
    cal = evaluate.CalibrationMatrix(num_classes, dev, temperatures=(1.0,), nbins=calibration["nbins"]) if calibration else None
    for d in (segs_dir, segs_rgb_dir):
        if d:
            os.makedirs(d, exist_ok=True)
    def saved(b, name):
        z = np.load(os.path.join(logits_dir, b, name + ".npy"), allow_pickle=True).item()["msc_seg"]
        return torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(dev)

    for name in names:
        with Image.open(image_path(name)) as im:
            image = np.ascontiguousarray(np.array(im.convert("RGB")), dtype=np.uint8)
        H, W, _ = image.shape
        if branch == "ens":       # the mean of the two students' class probabilities at the JPEG's size, one fused pass
            _, prob = ops.seg_ensemble(saved("branch1", name), saved("branch2", name), (H, W), want_prob=True)
            Q = post(torch.from_numpy(image).to(dev), prob)
        else:
            logit = ops.resize_bilinear(saved(branch, name), H, W)
            Q = post.from_logits(torch.from_numpy(image).to(dev), logit[0])
        pred = ops.argmax_channels(Q[None])[0]
        label = torch.from_numpy(np.ascontiguousarray(label_of(name, image)).astype(np.int64)).to(dev)
        cm.update(label, pred)
        if bm is not None:
            bm.update(label, pred)
        if cal is not None:
            cal.update(label, Q, is_prob=True)
        pred = pred.cpu().numpy().astype(np.uint8)
        Image.fromarray(pred).save(os.path.join(segs_dir, name + ".png"))
        if segs_rgb_dir:
            Image.fromarray(imutils.encode_cmap(pred).astype(np.uint8)).save(os.path.join(segs_rgb_dir, name + ".png"))
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
        for t in [cm.hist] + ([bm.hist, bm.biou] if bm is not None else []) + (cal.tensors() if cal is not None else []):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
    sc = cm.scores()
    if bm is not None:
        sc["boundary"] = boundary_scores(bm, boundary)
    if cal is not None:
        sc["calibration"] = calibration_scores(cal)
    return sc


def build_parser(dataset: str = "voc"):
    """The flags of tools/eval_seg_voc.py:26-36 (dataset "voc") or tools/eval_seg_coco_ddp.py:31-46 ("coco"): same names and
    defaults (tests/golden/cli_flags.json), plus --dataset, --save_logits and --crf."""
    import argparse
    import os
    voc_ = dataset == "voc"
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", default=dataset, choices=("voc", "coco"))
    p.add_argument("--infer_set", default="val" if voc_ else "val_part", type=str)
    p.add_argument("--pooling", default="gmp", type=str)
    p.add_argument("--model_path", default="your_model_dir/checkpoints.pth", type=str)
    p.add_argument("--backbone", default="deit_base_patch16_224" if voc_ else "vit_base_patch16_224", type=str,
                   help="the checkpoint's backbone: " + " | ".join(FAMILY))
    if voc_:
        p.add_argument("--data_folder", default="your_voc_dir", type=str, help="dataset folder")
    else:
        p.add_argument("--img_folder", default="your_coco_dir", type=str, help="image folder")
        p.add_argument("--label_folder", default="your_coco_seg_dir", type=str, help="label folder")
        p.add_argument("--backend", default="nccl")
        p.add_argument("--crop_size", default=448, type=int)
    p.add_argument("--list_folder", default="datasets/voc" if voc_ else "datasets/coco", type=str)
    p.add_argument("--num_classes", default=21 if voc_ else 81, type=int)
    p.add_argument("--ignore_index", default=255, type=int)
    p.add_argument("--scales", default=[1.0, 1.5, 1.25] if voc_ else [1.0, 1.25, 1.5], help="multi-scale list")
    p.add_argument("--save_logits", default=1, type=int,
                   help="write <run>/segs/logits/<infer_set>/branch{1,2}/<name>.npy = {'msc_seg': ...} like the reference does for "
                        "its DenseCRF stage; --crf 1 reads them back")
    p.add_argument("--crf", default=0, type=int,
                   help="1: run the reference's crf_proc on the device after the inference (DenseCRF(10, 1, 1, 4, 121, 5) on the "
                        "better student's saved logits; needs --save_logits 1): prints the seg_crf table, writes "
                        "<run>/segs/seg_preds/<infer_set>/<name>.png (+ the palette PNGs)")
    p.add_argument("--ensemble", default=0, type=int, choices=(0, 1),
                   help="1: also score the mean of the two students' class probabilities (one fused pass per image, ops.seg_ensemble): "
                        "a third table column Seg_ens, 'Seg_ens mIoU' and the students' agreement 'agree' in the last line")
    p.add_argument("--crf_branch", default="auto", choices=("auto", "1", "2", "ens"),
                   help="what --crf 1 post-processes: auto = the highest mIoU (of the two students, or with --ensemble 1 of the "
                        "students and the ensemble; on equal mIoU the students' rule, then the ensemble last), 1 / 2 = that "
                        "student, ens = the ensemble (needs --ensemble 1)")
    p.add_argument("--crf_method", default=None, choices=("exact", "lattice"),
                   help="the inference of the --crf 1 stage, for every --crf_branch: exact = the exact mean-field update, lattice = the "
                        "permutohedral-lattice approximation (utils/dcrf.py); default: utils.dcrf.METHOD")
    p.add_argument("--boundary", default=0, type=int, choices=(0, 1),
                   help="1: also score every column at the object boundaries (one fused pass per image and column, ops.seg_boundary): "
                        "a line per column with the Boundary IoU and the trimap mIoU per --trimap_widths width, '<column> BIoU' in the "
                        "last line, a 'boundary' entry in every returned score dict; with --crf 1 for seg_crf too")
    p.add_argument("--trimap_widths", default="1,2,4,8,16,32", type=parse_trimap_widths,
                   help="the trimap widths --boundary 1 reports: positive integers, ascending, at most 64")
    p.add_argument("--calibration", default=0, type=int, choices=(0, 1),
                   help="1: also score every column's confidence calibration (one fused pass per image and column, ops.seg_calibration): "
                        "a line per column with ECE, MCE, NLL, Brier, mean confidence and accuracy at T = 1 and the temperature of least "
                        "NLL, '<column> ECE' in the last line, a 'calibration' entry in every returned score dict; with --crf 1 the CRF's "
                        "marginals at T = 1 too.  The temperature goes into predict --temperature")
    p.add_argument("--calib_bins", default=15, type=int, help="the confidence bins of --calibration 1: 1 .. 64")
    p.add_argument("--temp_sweep", default="0.5:4:13", type=parse_temp_sweep,
                   help="the temperatures --calibration 1 sweeps in its one pass, LO:HI:N: a geometric grid of N <= 15 points beside T = 1")
    p.add_argument("--calib_json", default=None, type=str,
                   help="--calibration 1: write every column's full calibration dict (reliability bins, risk-coverage, classes, per "
                        "temperature) to this JSON file")
    p.add_argument("--nograd_gemm", default=os.environ.get("DUPL_NOGRAD_GEMM", "f16x3"), choices=("f16x3", "f16"),
                   help="GEMMs and attention of the no-grad encoder passes (multi-scale CAM, validation, inference): f16x3 = three f16 products, "
                        "fp32-equivalent (default); f16 = one product on the hi planes, fp32 accumulation (engine.set_nograd_gemm_mode; "
                        "experimental)")
    return p


ENS_NEEDS_FLAG = "--crf_branch ens post-processes the ensemble of the two students: it requires --ensemble 1"


def check_branch_args(args):
    """Refuse flag combinations that cannot be served, before anything is loaded."""
    if args.crf_branch == "ens" and not args.ensemble:
        raise SystemExit(ENS_NEEDS_FLAG)
    if not 1 <= getattr(args, "calib_bins", 15) <= evaluate.CALIB_MAX_BINS:
        raise SystemExit(f"--calib_bins must be 1 .. {evaluate.CALIB_MAX_BINS}, got {args.calib_bins}")


def calibration_spec(args):
    """The calibration= argument of validate / validate_coco / crf_proc from the flags; None without --calibration 1."""
    return {"temperatures": tuple(args.temp_sweep), "nbins": int(args.calib_bins)} if args.calibration else None


def pick_crf_branch(choice, s1, s2, ens=None):
    """The logits crf_proc runs on: "branch1", "branch2" or "ens".  auto without an ensemble score is the reference's rule
    (eval_seg_voc.py:185-188: student 1 only when strictly better); auto with one takes the highest mIoU of the three, and on
    equal mIoU the earliest of branch1, branch2, ens."""
    if choice in ("1", "2"):
        return "branch" + choice
    if choice == "ens":
        return "ens"
    if ens is None:
        return "branch1" if s1["miou"] > s2["miou"] else "branch2"
    cand = [("branch1", s1["miou"]), ("branch2", s2["miou"]), ("ens", ens["miou"])]
    best = cand[0]
    for c in cand[1:]:
        if c[1] > best[1]:
            best = c
    return best[0]


def main(argv=None):
    """tools/eval_seg_voc.py:154-193 (`validate`) / tools/eval_seg_coco_ddp.py:205-256: build the val loader, load the
    reference-format checkpoint strictly, run the multi-scale + flip inference of both students, print the score tables; with
    --crf 1 go on to crf_proc; under torch.distributed.run the split is sharded round-robin over the ranks (for the CRF stage
    too) and the confusion matrices are summed."""
    import os
    import numpy as np
    import torch.distributed as dist
    from torch.utils.data import DataLoader, Subset
    from ..datasets import voc, coco
    from ..datasets.device_loader import DeviceValLoader, raw_collate
    from ..model.model_dupl import siamese_network
    import argparse
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--dataset", default="voc", choices=("voc", "coco"))
    is_voc = pre.parse_known_args(argv)[0].dataset == "voc"
    args = build_parser("voc" if is_voc else "coco").parse_args(argv)
    check_branch_args(args)
    from .. import engine
    engine.set_nograd_gemm_mode(args.nograd_gemm)
    if isinstance(args.scales, str):
        args.scales = [float(v) for v in args.scales.strip("()[] ").split(",")]
    args.scales = tuple(args.scales)
    if args.crf and not args.save_logits:
        raise SystemExit("--crf 1 reads the logits that --save_logits 1 writes (segs/logits/<infer_set>/branch{1,2}): "
                         "run with --save_logits 1")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(getattr(args, "backend", "nccl"))
    if is_voc:
        ds = voc.VOC12SegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.infer_set, stage="val",
                                 aug=False, ignore_index=args.ignore_index, num_classes=args.num_classes)
    else:
        ds = coco.CocoSegDataset(img_dir=args.img_folder, label_dir=args.label_folder, name_list_dir=args.list_folder,
                                 split=args.infer_set, stage="val", aug=False, ignore_index=args.ignore_index)
    if world > 1:
        ds = Subset(ds, list(range(dist.get_rank(), len(ds), world)))        # eval_seg_coco_ddp.py:239-245
    loader = DeviceValLoader(DataLoader(ds, batch_size=1, shuffle=False, num_workers=8, pin_memory=False, drop_last=False,
                                        collate_fn=raw_collate), dev)
    model = siamese_network(backbone=args.backbone, num_classes=args.num_classes, pretrained=False, aux_layer=-3)
    load_checkpoint(model, args.model_path)
    model.to(dev)
    model.eval()
    base_dir = args.model_path.split("checkpoints")[0]
    logits_dir = os.path.join(base_dir, "segs/logits", args.infer_set)
    keep = None
    if args.save_logits:
        for b in ("branch1", "branch2"):
            os.makedirs(os.path.join(logits_dir, b), exist_ok=True)

        def keep(name, branch, logits):
            nm = name[0] if isinstance(name, (tuple, list)) else name
            np.save(os.path.join(logits_dir, f"branch{branch}", str(nm) + ".npy"), {"msc_seg": logits.cpu().numpy()})

    boundary = args.trimap_widths if args.boundary else None
    calibration = calibration_spec(args)
    extra = {"calibration": calibration} if calibration else {}
    with torch.no_grad():
        if is_voc:
            sc = validate(model, loader, args, args.num_classes, voc.class_list, keep_logits=keep, ensemble=bool(args.ensemble),
                          boundary=boundary, **extra)
        else:
            sc = validate_coco(model, loader, args, args.num_classes, coco.class_list, keep_logits=keep, ensemble=bool(args.ensemble),
                               boundary=boundary, **extra)
    s1, s2 = sc[0], sc[1]
    ens = sc[2] if args.ensemble else None
    last = {"Seg_1 mIoU": s1["miou"], "Seg_2 mIoU": s2["miou"]}
    if ens is not None:
        last.update({"Seg_ens mIoU": ens["miou"], "agree": ens["agree"]})
    if boundary:
        last.update({f"{n} BIoU": s["boundary"]["biou"] for n, s in zip(("Seg_1", "Seg_2", "Seg_ens"), sc)})
    calib_out = {}
    if calibration:
        last.update({f"{n} ECE": s["calibration"]["scores"][0]["ece"] for n, s in zip(("Seg_1", "Seg_2", "Seg_ens"), sc)})
        calib_out = {n: s["calibration"] for n, s in zip(("Seg_1", "Seg_2", "Seg_ens"), sc)}
    # crf_proc (eval_seg_voc.py:185-188): the student with the higher mIoU unless --crf_branch / --ensemble say otherwise
    branch = pick_crf_branch(args.crf_branch, s1, s2, ens)
    rank0 = int(os.environ.get("RANK", "0")) == 0

    def write_calib_json():
        if calibration and args.calib_json and rank0:
            import json
            with open(args.calib_json, "w") as f:
                json.dump(calib_out, f, indent=1)

    if not args.crf:
        write_calib_json()
        if rank0:
            over = "both students' logits under " + logits_dir if branch == "ens" else f"{logits_dir}/{branch}"
            print({**last, "next": f"DenseCRF over {over} (reference: crf_proc, CPU)"})
        return tuple(sc)
    # images sharded like the logits pass
    base = ds.dataset if world > 1 else ds
    names = [str(n) for n in base.name_list][(dist.get_rank() if world > 1 else 0)::world]
    test_set = "test" in args.infer_set
    if is_voc:
        image_path = lambda n: os.path.join(base.img_dir, n + ".jpg")
        label_path = lambda n: os.path.join(base.label_dir, n + ".png")
        rgb_dir = os.path.join(base_dir, "segs/seg_preds_rgb", args.infer_set)
    else:
        image_path = lambda n: base._paths(n)[0]
        label_path = lambda n: base._paths(n)[1]
        rgb_dir = os.path.join(base_dir, "segs", args.infer_set)

    def label_of(name, image):
        if test_set:
            return image[:, :, 0]
        return voc._read_label(label_path(name))

    if rank0:
        print("crf post-processing...")
    with torch.no_grad():
        crf = crf_proc(branch, names, image_path, label_of, logits_dir, os.path.join(base_dir, "segs/seg_preds", args.infer_set),
                       rgb_dir, args.num_classes, dev, boundary=boundary, method=args.crf_method, **extra)
    if rank0:
        print(format_tabs([crf], ["seg_crf"], cat_list=voc.class_list if is_voc else coco.class_list))
        if boundary:
            print(format_boundary([crf], ["seg_crf"]))
            last["seg_crf BIoU"] = crf["boundary"]["biou"]
        if calibration:
            print(format_calibration([crf], ["seg_crf"]))
            last["seg_crf ECE"] = crf["calibration"]["scores"][0]["ece"]
        print({**last, "seg_crf mIoU": crf["miou"]})
    if calibration:
        calib_out["seg_crf"] = crf["calibration"]
        write_calib_json()
    return tuple(sc) + (crf,)


if __name__ == "__main__":
    main()
