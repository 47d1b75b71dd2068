"""Segment arbitrary images with a trained checkpoint (beyond the reference, whose inference tools all need a VOC / COCO folder
layout, a split list and cls_labels_onehot.npy around the images):

    python -m dupl_amd.tools.predict --model_path work_dir/checkpoints/checkpoint.pth --input photos/ --out_dir out/

Per image: the multi-scale + flip inference of tools/eval_seg (`msc_seg_logits`), optionally over sliding windows
(`msc_seg_logits_windowed`: ops.window_gather cuts the windows of the resized image and of its flip straight from the source, the two
students run on chunks of `window_batch` windows, ops.window_merge averages the overlapping logits on the canvas that
ops.msc_seg_accum_ consumes), optionally DenseCRF, then ONE pass that turns the logits into the label map, the per-pixel confidence,
the rejection of low-confidence pixels and the per-class statistics (ops.seg_decide), optionally the connected regions of that map (ops.seg_regions: --regions 1 lists the objects with class, area, box
and mean confidence; --min_region N first absorbs the regions of fewer than N pixels into their surroundings,
ops.seg_regions_clean), and one integer pass for the palette overlay (ops.seg_paint).  Nothing but the PNGs' pixels, 2 (C+1)
counters and, when asked for, the region table travel to the host.  `--temperature T` (the temperature eval_seg --calibration 1
reports) multiplies the logits by the fp32 1 / T before that pass: the confidence written is then the one eval_seg scored at T."""
import argparse
import json
import os
import time

import numpy as np
import torch

from .. import ops
from ..model.backbone import FAMILY
from . import eval_seg

PATCH = 16
IMAGE_EXT = (".jpg", ".jpeg", ".png", ".bmp")


def plan_windows(n_tokens, win_tokens, stride_tokens):
    """Start tokens of the windows along one axis of n_tokens tokens: one window of n tokens at 0 when n <= win, otherwise 0, stride,
    2 stride, ... while start + win < n, then n - win (the last window ends at n)."""
    n, win, stride = int(n_tokens), int(win_tokens), int(stride_tokens)
    assert n >= 1 and win >= 1 and 1 <= stride <= win
    if n <= win:
        return [0]
    starts = []
    s = 0
    while s + win < n:
        starts.append(s)
        s += stride
    if not starts or starts[-1] != n - win:
        starts.append(n - win)
    return starts


def check_window_args(window, stride):
    """window 0 = the whole image; otherwise window and stride are multiples of 16 with 16 <= stride <= window."""
    window, stride = int(window), int(stride)
    if window == 0:
        return
    if window < PATCH or window % PATCH:
        raise ValueError(f"--window must be 0 (whole image) or a multiple of {PATCH} (the patch size), got {window}")
    if stride % PATCH or not PATCH <= stride <= window:
        raise ValueError(f"--stride must be a multiple of {PATCH} with {PATCH} <= stride <= window ({window}): a larger stride "
                         f"would leave tokens uncovered; got {stride}")


def default_stride(window):
    """about two thirds of the window, a multiple of 16"""
    return max(PATCH, (2 * int(window) // 3) // PATCH * PATCH)


def scale_plan(h, w, scale, window, stride):
    """(Hs, Ws), the token grid PatchEmbed keeps, and the window starts (tokens) along both axes of one scale."""
    Hs, Ws = int(h * scale), int(w * scale)
    th, tw = Hs // PATCH, Ws // PATCH
    if window == 0:
        return (Hs, Ws), (th, tw), [0], [0]
    return (Hs, Ws), (th, tw), plan_windows(th, window // PATCH, stride // PATCH), plan_windows(tw, window // PATCH, stride // PATCH)


def windows_per_scale(h, w, scales, window, stride):
    out = []
    for sc in scales:
        _, _, rows, cols = scale_plan(h, w, sc, window, stride)
        out.append(len(rows) * len(cols))
    return out


def msc_seg_logits_windowed(model, inputs, out_size, scales=(1.0, 1.5, 1.25), window=448, stride=320, window_batch=8):
    """eval_seg.msc_seg_logits with every scale run over sliding windows of `window` pixels every `stride` pixels: inputs (1,3,h,w)
    on the device -> (seg_1, seg_2), each (1,C1,H,W).  The overlapping windows' logits are averaged at logit resolution.  A scale
    that one window covers takes msc_seg_logits's whole-image route (the same bits)."""
    assert inputs.shape[0] == 1
    check_window_args(window, stride)
    if window == 0:
        return eval_seg.msc_seg_logits(model, inputs, out_size, scales)
    window_batch = int(window_batch)
    if window_batch < 1:
        raise ValueError(f"window_batch must be at least 1, got {window_batch}")
    core = model.module if hasattr(model, "module") else model
    _, _, h, w = inputs.shape
    H, W = int(out_size[0]), int(out_size[1])
    x = inputs.contiguous().float()
    accs = None
    with torch.no_grad():
        for i, sc in enumerate(scales):
            (Hs, Ws), (th, tw), rows, cols = scale_plan(h, w, sc, window, stride)
            if len(rows) == 1 and len(cols) == 1:
                res = core(ops.resize_bilinear(x, Hs, Ws, flip_cat=True))
                canvas = (res["branch1"][1], res["branch2"][1])
            else:
                wth, wtw = min(th, window // PATCH), min(tw, window // PATCH)
                org = [(r, c) for r in rows for c in cols]
                batch = ops.window_gather(x, Hs, Ws, [(r * PATCH, c * PATCH) for r, c in org], wth * PATCH, wtw * PATCH)
                logits = None
                for j in range(0, batch.shape[0], window_batch):
                    res = core(batch[j:j + window_batch])
                    segs = (res["branch1"][1], res["branch2"][1])
                    if logits is None:
                        logits = [torch.empty((batch.shape[0],) + tuple(s.shape[1:]), device=x.device, dtype=torch.float32) for s in segs]
                    for dst, s in zip(logits, segs):
                        dst[j:j + s.shape[0]].copy_(s)
                canvas = tuple(ops.window_merge(t, org, th, tw) for t in logits)
            if accs is None:
                C1 = canvas[0].shape[1]
                accs = [torch.empty((1, C1, H, W), device=x.device, dtype=torch.float32) for _ in range(2)]
            for acc, s in zip(accs, canvas):
                ops.msc_seg_accum_(acc, s, mode=(0 if i == 0 else 1))
    return accs[0], accs[1]


_PALETTES = {}


def device_palette(dev):
    """imutils.colormap() (256,3) uint8 on the device, once per device."""
    from ..utils import imutils
    key = str(dev)
    if key not in _PALETTES:
        _PALETTES[key] = torch.from_numpy(np.ascontiguousarray(imutils.colormap())).to(dev)
    return _PALETTES[key]


def predict_image(model, image_u8, *, scales=(1.0, 1.5, 1.25), branch="ens", window=0, stride=0, window_batch=8, crf=False,
                  min_conf=0.0, ignore_index=255, alpha=0.6, contour=False, tint_background=False, contour_rgb=(255, 255, 255),
                  crf_method="exact", min_region=0, regions=False, connectivity=8, max_regions=4096, temperature=1.0):
    """image_u8 (H,W,3) uint8 (numpy or tensor) -> dict(label (H,W) uint8, conf (H,W) fp32, overlay (H,W,3) uint8 -- device tensors --,
    stats (2, C+1) int64 on the host: ops.seg_decide's, windows: the windows per scale).  branch 1 / 2: that student, "ens": the
    mean of the two students' class probabilities.  crf: DenseCRF with crf_proc's parameters on the chosen student's logits or on
    the ensemble's probabilities, then the decision on its marginals; crf_method "exact" (the dense mean-field update) or "lattice"
    (the permutohedral approximation, utils/dcrf.py).
    min_region > 0: the connected regions (connectivity 4 / 8) of fewer than min_region pixels are absorbed by their surroundings
    (ops.seg_regions_clean) before painting; label, overlay and stats then describe the cleaned map (the rejected pixels stay), and
    `cleaned` = {regions, pixels} says what moved.  regions: also region (H,W) int32 (device), n_regions and region_table, the first
    max_regions rows of ops.seg_regions's table on the host.  With neither, the dict has the keys above and no region op runs.
    temperature T != 1: the accumulated logits of the chosen branch (of both, for "ens") are multiplied by ops.inv_temperature(T)
    before the decision -- the confidence is then, bit for bit, the one eval_seg --calibration 1 scored at T (the label of a single
    student does not change); at exactly 1.0 no op is added.  Refused together with crf (TEMPERATURE_WITH_CRF)."""
    from ..datasets.device_loader import DeviceTransform
    from ..utils.train_helper import _device_of
    branch = str(branch)
    if branch not in ("1", "2", "ens"):
        raise ValueError(f"branch must be 1, 2 or ens, got {branch}")
    if crf_method not in ("exact", "lattice"):
        raise ValueError(f"crf_method must be exact or lattice, got {crf_method}")
    if int(min_region) < 0:
        raise ValueError(f"min_region must be at least 0, got {min_region}")
    if int(connectivity) not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    if int(max_regions) < 1:
        raise ValueError(f"max_regions must be at least 1, got {max_regions}")
    temperature = float(temperature)
    inv_t = ops.inv_temperature(temperature)
    if crf and temperature != 1.0:
        raise ValueError(TEMPERATURE_WITH_CRF)
    if window and not stride:
        stride = default_stride(window)
    check_window_args(window, stride)
    dev = _device_of(model)
    raw = torch.as_tensor(np.ascontiguousarray(image_u8) if isinstance(image_u8, np.ndarray) else image_u8)
    assert raw.dtype == torch.uint8 and raw.dim() == 3 and raw.shape[2] == 3, "image_u8: (H,W,3) uint8"
    raw = raw.contiguous().to(dev)
    H, W, _ = raw.shape
    inputs = DeviceTransform(dev).val_item(raw)[None]
    seg = msc_seg_logits_windowed(model, inputs, (H, W), scales, window, stride, window_batch)
    C = seg[0].shape[1]
    if temperature != 1.0:                     # nothing else reads the accumulated logits: scaled in place
        for k in ((0, 1) if branch == "ens" else (int(branch) - 1,)):
            ops.scale_(seg[k], inv_t)
    stats = torch.zeros((2, C + 1), device=dev, dtype=torch.int64)
    kw = dict(min_conf=min_conf, ignore_index=ignore_index, stats=stats)
    if crf:
        from ..utils.dcrf import DenseCRF
        post = DenseCRF(iter_max=10, pos_xy_std=1, pos_w=1, bi_xy_std=121, bi_rgb_std=5, bi_w=4)
        post.method = crf_method
        if branch == "ens":
            Q = post(raw, ops.seg_ensemble(seg[0], seg[1], (H, W), want_prob=True)[1])
        else:
            Q = post.from_logits(raw, seg[int(branch) - 1][0])
        label, conf = ops.seg_decide(Q, is_prob=True, **kw)
    elif branch == "ens":
        label, conf = ops.seg_decide(seg[0], seg[1], **kw)
    else:
        label, conf = ops.seg_decide(seg[int(branch) - 1], **kw)
    extra = {}
    if int(min_region) > 0:
        # the cleaned map's statistics replace the decision's; the regions are counted in full here (the cap is on the list only)
        stats = torch.zeros((2, C + 1), device=dev, dtype=torch.int64)
        label, region, n, table, changed = ops.seg_regions_clean(label, min_area=int(min_region), connectivity=connectivity,
                                                                 ignore_index=ignore_index, max_regions=H * W, conf=conf, stats=stats)
        changed = changed.cpu()
        extra["cleaned"] = {"regions": int(changed[0]), "pixels": int(changed[1])}
        if regions:
            extra.update(region=region, n_regions=n, region_table=table[:int(max_regions)].cpu())
    elif regions:
        region, n, table = ops.seg_regions(label, conf, connectivity=connectivity, ignore_index=ignore_index,
                                           max_regions=int(max_regions), num_classes=C)
        extra.update(region=region, n_regions=n, region_table=table.cpu())
    overlay = ops.seg_paint(label, device_palette(dev), raw, alpha256=int(round(float(alpha) * 256)), tint_background=tint_background,
                            contour=contour, contour_rgb=contour_rgb)
    return {"label": label, "conf": conf, "overlay": overlay, "stats": stats.cpu(),
            "windows": windows_per_scale(H, W, scales, window, stride), **extra}


TEMPERATURE_WITH_CRF = ("--temperature cannot be combined with --crf 1: the CRF's marginals are not a soft-max of these logits, and "
                        "eval_seg --calibration 1 fits no temperature for them")


def class_summary(stats, names, n_pixels):
    """stats (2, C+1) of ops.seg_decide -> ([{id, name, pixels, share, mean_conf} per class present], rejected pixels)."""
    st = np.asarray(stats, dtype=np.int64)
    C = st.shape[1] - 1
    out = []
    for c in range(C):
        n = int(st[0, c])
        if n:
            out.append({"id": c, "name": names[c] if c < len(names) else f"class{c}", "pixels": n, "share": n / n_pixels,
                        "mean_conf": int(st[1, c]) / float(1 << 24) / n})
    return out, int(st[0, C])


def region_summary(table, names, min_pixels=1):
    """rows of ops.seg_regions's table (class, area, y0, x0, y1, x1, conf_sum, first_index) -> [{id, class, name, pixels,
    box: [x0, y0, x1, y1] (inclusive), mean_conf} per region of at least min_pixels pixels], in id order."""
    out = []
    for i, row in enumerate(np.asarray(table, dtype=np.int64).reshape(-1, 8)):
        c, n = int(row[0]), int(row[1])
        if n >= int(min_pixels):
            out.append({"id": i, "class": c, "name": names[c] if c < len(names) else f"class{c}", "pixels": n,
                        "box": [int(row[3]), int(row[2]), int(row[5]), int(row[4])], "mean_conf": int(row[6]) / float(1 << 24) / n})
    return out


def class_names(spec):
    from ..datasets import coco, voc
    if spec == "voc":
        return list(voc.class_list)
    if spec == "coco":
        return list(coco.class_list)
    with open(spec) as f:
        return [ln.strip() for ln in f if ln.strip()]


def list_inputs(path):
    """a file, a folder (its images, sorted), or a text file with one path per line (relative to the text file)"""
    if os.path.isdir(path):
        found = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(IMAGE_EXT))
    elif path.lower().endswith(".txt"):
        base = os.path.dirname(os.path.abspath(path))
        with open(path) as f:
            found = [ln.strip() if os.path.isabs(ln.strip()) else os.path.join(base, ln.strip()) for ln in f if ln.strip()]
    else:
        found = [path]
    if not found:
        raise SystemExit(f"--input {path}: no images found ({', '.join(IMAGE_EXT)})")
    return found


def build_parser():
    p = argparse.ArgumentParser(description="segment arbitrary images with a DuPL checkpoint")
    p.add_argument("--model_path", default="your_model_dir/checkpoints.pth", type=str)
    p.add_argument("--backbone", default="deit_base_patch16_224", type=str, help="the checkpoint's backbone: " + " | ".join(FAMILY))
    p.add_argument("--num_classes", default=21, type=int)
    p.add_argument("--input", required=True, type=str, help="an image, a folder of images, or a .txt file with one path per line")
    p.add_argument("--out_dir", required=True, type=str)
    p.add_argument("--scales", default="1.0,1.5,1.25", type=str, help="multi-scale list")
    p.add_argument("--branch", default="ens", choices=("1", "2", "ens"), help="student 1, student 2, or the mean of their probabilities")
    p.add_argument("--window", default=0, type=int, help="sliding window in pixels, a multiple of 16; 0 = the whole image (as eval_seg)")
    p.add_argument("--stride", default=0, type=int, help="window step in pixels, a multiple of 16, 16 <= stride <= window; "
                                                          "0 = about two thirds of the window")
    p.add_argument("--window_batch", default=8, type=int, help="windows per encoder pass")
    p.add_argument("--crf", default=0, type=int, choices=(0, 1), help="1: DenseCRF(10, 1, 1, 4, 121, 5) before the decision")
    p.add_argument("--crf_method", default=None, choices=("exact", "lattice"),
                   help="how --crf 1 evaluates the DenseCRF messages: exact = the dense sum over all pixel pairs (default), lattice = "
                        "the permutohedral-lattice approximation (O(N) per message); summary.json records it when given")
    p.add_argument("--min_conf", default=0.0, type=float, help="pixels whose confidence is below this get the label 255")
    p.add_argument("--temperature", default=None, type=float,
                   help="divide the logits by T before the soft-max (eval_seg --calibration 1 reports the T of least NLL): changes the "
                        "confidence -- what --min_conf, mean_conf and conf/<stem>.png see --, not a single student's labels; default 1 = off; "
                        "not with --crf 1; summary.json records it when given")
    p.add_argument("--alpha", default=0.6, type=float, help="weight of the class colour in the overlay, 0 .. 1")
    p.add_argument("--contour", default=0, type=int, choices=(0, 1), help="1: draw the class boundaries in white")
    p.add_argument("--tint_background", default=0, type=int, choices=(0, 1), help="1: blend the background's colour in as well")
    p.add_argument("--class_names", default="voc", type=str, help="voc, coco, or a file with one name per line")
    p.add_argument("--nograd_gemm", default=os.environ.get("DUPL_NOGRAD_GEMM", "f16x3"), choices=("f16x3", "f16"),
                   help="GEMMs and attention of the no-grad encoder passes: f16x3 = three f16 products, fp32-equivalent (default); "
                        "f16 = one product on the hi planes (engine.set_nograd_gemm_mode; experimental)")
    p.add_argument("--min_region", default=0, type=int, help="absorb connected regions of fewer than N pixels into their surroundings "
                                                             "before painting; 0 = off")
    p.add_argument("--regions", default=0, type=int, choices=(0, 1), help="1: list the connected regions (class, pixels, box, mean "
                                                                          "confidence) per image in summary.json")
    p.add_argument("--region_min_pixels", default=1, type=int, help="--regions 1: list only regions of at least this many pixels")
    p.add_argument("--max_regions", default=4096, type=int, help="--regions 1: cap on the regions listed per image (regions_total "
                                                                 "still gives the true count)")
    p.add_argument("--connectivity", default=8, type=int, choices=(4, 8), help="pixel neighbourhood of --min_region and --regions")
    p.add_argument("--save_conf", default=0, type=int, choices=(0, 1), help="1: also write conf/<stem>.png = floor(255 conf)")
    return p


def parse_args(argv=None):
    """The flags, checked before anything is loaded."""
    args = build_parser().parse_args(argv)
    args.crf_method_given = args.crf_method is not None          # summary.json records the method only when the flag is given
    args.crf_method = args.crf_method or "exact"
    args.temperature_given = args.temperature is not None        # summary.json records the temperature only when the flag is given
    args.temperature = 1.0 if args.temperature is None else args.temperature
    args.scales = tuple(float(v) for v in str(args.scales).strip("()[] ").split(",") if v.strip())
    if not args.scales:
        raise SystemExit("--scales: at least one scale")
    if args.window and not args.stride:
        args.stride = default_stride(args.window)
    try:
        check_window_args(args.window, args.stride)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.window_batch < 1:
        raise SystemExit(f"--window_batch must be at least 1, got {args.window_batch}")
    if not 0.0 <= args.alpha <= 1.0:
        raise SystemExit(f"--alpha must lie in 0 .. 1, got {args.alpha}")
    if not 1 <= args.num_classes <= 255:
        raise SystemExit(f"--num_classes must be 1 .. 255 (the label PNG keeps 255 for rejected pixels), got {args.num_classes}")
    if args.min_region < 0:
        raise SystemExit(f"--min_region must be at least 0, got {args.min_region}")
    if args.region_min_pixels < 1:
        raise SystemExit(f"--region_min_pixels must be at least 1, got {args.region_min_pixels}")
    if args.max_regions < 1:
        raise SystemExit(f"--max_regions must be at least 1, got {args.max_regions}")
    try:
        ops.inv_temperature(args.temperature)
    except ValueError as e:
        raise SystemExit(f"--temperature: {e}")
    if args.temperature != 1.0 and args.crf:
        raise SystemExit(TEMPERATURE_WITH_CRF)
    return args


def main(argv=None):
    from PIL import Image
    from .. import engine
    from ..model.model_dupl import siamese_network
    from ..utils import imutils
    args = parse_args(argv)
    names = class_names(args.class_names)
    paths = list_inputs(args.input)
    engine.set_nograd_gemm_mode(args.nograd_gemm)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    model = siamese_network(backbone=args.backbone, num_classes=args.num_classes, pretrained=False, aux_layer=-3)
    eval_seg.load_checkpoint(model, args.model_path)
    model.to(dev)
    model.eval()
    for sub in ("labels", "overlay") + (("conf",) if args.save_conf else ()):
        os.makedirs(os.path.join(args.out_dir, sub), exist_ok=True)
    flat_palette = imutils.colormap().flatten().tolist()
    summary = []
    t0 = time.time()
    for path in paths:
        stem = os.path.splitext(os.path.basename(path))[0]
        with Image.open(path) as im:
            image = np.ascontiguousarray(np.array(im.convert("RGB")), dtype=np.uint8)
        H, W, _ = image.shape
        r = predict_image(model, image, scales=args.scales, branch=args.branch, window=args.window, stride=args.stride,
                          window_batch=args.window_batch, crf=bool(args.crf), min_conf=args.min_conf, alpha=args.alpha,
                          contour=bool(args.contour), tint_background=bool(args.tint_background), crf_method=args.crf_method,
                          **({"min_region": args.min_region, "regions": bool(args.regions), "connectivity": args.connectivity,
                              "max_regions": args.max_regions} if args.min_region or args.regions else {}),
                          **({"temperature": args.temperature} if args.temperature != 1.0 else {}))
        png = Image.fromarray(r["label"].cpu().numpy())        # mode L; attaching the palette makes it an index image (mode P)
        png.putpalette(flat_palette)
        png.save(os.path.join(args.out_dir, "labels", stem + ".png"))
        Image.fromarray(r["overlay"].cpu().numpy()).save(os.path.join(args.out_dir, "overlay", stem + ".png"))
        if args.save_conf:
            conf8 = (r["conf"] * 255.0).floor().clamp_(0, 255).to(torch.uint8)
            Image.fromarray(conf8.cpu().numpy()).save(os.path.join(args.out_dir, "conf", stem + ".png"))
        classes, rejected = class_summary(r["stats"], names, H * W)
        summary.append({"image": os.path.basename(path), "size": [H, W], "windows_per_scale": r["windows"], "classes": classes,
                        "rejected_pixels": rejected})
        if args.min_region:
            summary[-1].update(min_region=args.min_region, cleaned=r["cleaned"])
        found = ", ".join(f"{c['name']} {100 * c['share']:.1f}%" for c in classes)
        print(f"{os.path.basename(path)}: {H}x{W}, windows {r['windows']}, {found}; rejected {rejected}")
        if args.regions:
            summary[-1].update(regions_total=r["n_regions"], regions=region_summary(r["region_table"], names, args.region_min_pixels))
            tab = r["region_table"].numpy()
            per = np.bincount(tab[:, 0], minlength=1)[1:] if len(tab) else []
            listed = ", ".join(f"{names[c + 1] if c + 1 < len(names) else f'class{c + 1}'} {int(k)}" for c, k in enumerate(per) if k)
            print(f"{os.path.basename(path)}: {r['n_regions']} regions" + (f" ({listed})" if listed else ""))
    torch.cuda.synchronize()
    dt = time.time() - t0
    with open(os.path.join(args.out_dir, "summary.json"), "w") as f:
        json.dump({"scales": list(args.scales), "branch": args.branch, "window": args.window, "stride": args.stride if args.window else 0,
                   "crf": int(args.crf), **({"crf_method": args.crf_method} if args.crf_method_given else {}),
                   "min_conf": args.min_conf, **({"temperature": args.temperature} if args.temperature_given else {}),
                   **({"min_region": args.min_region, "cleaned": {k: sum(e["cleaned"][k] for e in summary) for k in ("regions", "pixels")}}
                      if args.min_region else {}),
                   "images": summary}, f, indent=1)
    print(f"{len(paths)} images in {dt:.2f} s: {len(paths) / dt:.2f} images/s")
    return summary


if __name__ == "__main__":
    main()
