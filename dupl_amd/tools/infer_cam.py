"""Offline CAM inference over a split: seed quality and the background threshold (reference: tools/infer_cam_voc.py:38-141).

    python -m dupl_amd.tools.infer_cam --model_path work_dir/checkpoints/checkpoint.pth --data_folder VOC2012 \
        --infer_set train --sweep 0.05:0.95:0.05

Per image (batch 1) the input is resized to 448^2, the multi-scale CAMs of one student are computed
(cam_helper.multi_scale_cam2_siamese) and everything after them is one fused pass per CAM set over the label grid
(ops.cam_eval, csrc/cam_eval.hip): up-sampling of the classes present, label map at --bkg_thre, the max value for the jet
overlay, and the confusion matrices of every threshold of the sweep at once.  The matrices stay on the device until the end.
The reference script does not run as shipped (it declares --data_folder twice, reads args.list_folder without declaring it and
imports a model module that does not exist); this is its evident intent, with --list_folder, --branch, --scales, --sweep,
--save_img and --save_labels added.  Under torch.distributed.run the split is sharded round-robin over the ranks and the
histograms are all-reduced as in eval_seg.main -- untested beyond one rank."""
import os

import torch

from .. import ops
from ..utils import cam_helper, evaluate
from ..utils.pyutils import format_tabs
from .eval_seg import load_checkpoint
from ..model.backbone import FAMILY


def build_parser():
    """The flags of tools/infer_cam_voc.py:22-35 with their names and defaults, plus the ones listed in the module docstring."""
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument("--bkg_thre", default=0.5, type=float, help="background threshold of the score table and the label PNGs")
    p.add_argument("--model_path", default="your_model_path/checkpoint.pth", type=str, help="model_path")
    p.add_argument("--backbone", default="vit_base_patch16_224", type=str, help="the checkpoint's backbone: " + " | ".join(FAMILY))
    p.add_argument("--pooling", default="gmp", type=str, help="pooling choice for patch tokens")
    p.add_argument("--data_folder", default="your_voc_dir", type=str, help="dataset folder")
    p.add_argument("--num_classes", default=21, type=int, help="number of classes")
    p.add_argument("--ignore_index", default=255, type=int, help="random index")
    p.add_argument("--infer_set", default="train", type=str, help="infer_set")
    p.add_argument("--list_folder", default="datasets/voc", type=str, help="folder of <split>.txt and cls_labels_onehot.npy")
    p.add_argument("--branch", default=1, type=int, choices=(1, 2), help="the student whose CAMs are scored")
    p.add_argument("--scales", default="1.0,0.5,1.5", type=str, help="multi-scale list of the CAM forward")
    p.add_argument("--sweep", default="", type=str,
                   help="LO:HI:STEP, e.g. 0.05:0.95:0.05: score every background threshold of the range in the same pass")
    p.add_argument("--save_img", default=1, type=int, help="write the jet overlays to cam_img/ and cam_img_aux/")
    p.add_argument("--save_labels", default=0, type=int,
                   help="write the label map at --bkg_thre to cam_labels/<set>/<name>.png (+ cam_labels_rgb/)")
    # (no attribute unless given: the namespace of a plain run stays the reference's flag set; nograd_gemm_mode() supplies the default)
    p.add_argument("--nograd_gemm", default=argparse.SUPPRESS, choices=("f16x3", "f16"),
                   help="GEMMs and attention of the no-grad encoder passes (multi-scale CAM, validation, inference): f16x3 = three f16 products, "
                        "fp32-equivalent (default); f16 = one product on the hi planes, fp32 accumulation (engine.set_nograd_gemm_mode; "
                        "experimental)")
    return p


def nograd_gemm_mode(args) -> str:
    """--nograd_gemm of a parsed command line; when the flag was not given, DUPL_NOGRAD_GEMM or f16x3."""
    return getattr(args, "nograd_gemm", os.environ.get("DUPL_NOGRAD_GEMM", "f16x3"))


def parse_scales(text):
    if isinstance(text, (tuple, list)):
        return tuple(float(v) for v in text)
    return tuple(float(v) for v in str(text).strip("()[] ").split(",") if v.strip())


def sweep_thresholds(sweep: str, bkg_thre: float):
    """"LO:HI:STEP" -> the ascending float32 thresholds LO, LO + STEP, ... <= HI, with bkg_thre inserted when it is not one of
    them -> (thresholds, index of bkg_thre).  An empty sweep is the single threshold bkg_thre."""
    import numpy as np
    b = float(np.float32(bkg_thre))
    if not sweep:
        return [b], 0
    try:
        lo, hi, step = (float(v) for v in sweep.split(":"))
    except ValueError:
        raise SystemExit(f"--sweep takes LO:HI:STEP, got {sweep!r}")
    if not (step > 0 and 0 <= lo <= hi <= 1):
        raise SystemExit(f"--sweep needs 0 <= LO <= HI <= 1 and STEP > 0, got {sweep!r}")
    n = int(np.floor((hi - lo) / step + 1e-9)) + 1
    thr = sorted({float(np.float32(lo + i * step)) for i in range(n)} | {b})
    if len(thr) > 64:
        raise SystemExit(f"--sweep {sweep}: {len(thr)} thresholds, at most 64 fit one pass")
    return thr, thr.index(b)


def infer_cams(model, loader, args, thresholds=None, label_at=0, on_image=None, process_group=None):
    """tools/infer_cam_voc.py:38-97 (`_validate`) on this rank's loader of (name, inputs (1,3,h,w), labels (1,H,W), cls_label):
    -> (sweep_cam, sweep_aux), two evaluate.ThresholdSweep over `thresholds` (default: args.bkg_thre alone).
    on_image(name, inputs, which, label, value) is called per image and CAM set ("cam" / "aux_cam") with the (1,H,W) uint8 label
    map at thresholds[label_at] and the (1,H,W) fp32 max value, both on the device."""
    import torch.distributed as dist
    from ..utils.train_helper import _device_of, _fetch
    dev = _device_of(model)
    thresholds = [float(args.bkg_thre)] if thresholds is None else thresholds
    sweeps = [evaluate.ThresholdSweep(args.num_classes, thresholds, dev) for _ in range(2)]
    scales = parse_scales(getattr(args, "scales", (1.0, 0.5, 1.5)))
    branch = int(getattr(args, "branch", 1))
    model.eval()
    with torch.no_grad():
        for data in loader:
            inputs, labels, cls_label = _fetch(data, dev)
            x = ops.resize_bilinear(inputs, 448, 448)
            cams = cam_helper.multi_scale_cam2_siamese(model, inputs=x, scales=scales, branch=branch)
            for which, cam, sw in zip(("cam", "aux_cam"), cams, sweeps):
                label, value = sw.update(cam, cls_label, labels, label_at=label_at, want_value=on_image is not None)
                if on_image is not None:
                    on_image(data[0], inputs, which, label, value)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
        for sw in sweeps:
            dist.all_reduce(sw.hist, op=dist.ReduceOp.SUM, group=process_group)
    return sweeps[0], sweeps[1]


def main(argv=None):
    """tools/infer_cam_voc.py:100-148: build the loader of --infer_set, load the reference-format checkpoint, run infer_cams,
    write overlays / label PNGs below model_path.split("checkpoint")[0], print the cam / aux_cam table at --bkg_thre, the
    sweep lines and the summary dict."""
    import numpy as np
    import torch.distributed as dist
    from PIL import Image
    from torch.utils.data import DataLoader, Subset
    from ..datasets import voc
    from ..datasets.device_loader import DeviceValLoader, raw_collate
    from ..model.model_dupl import siamese_network
    from ..utils import imutils
    args = build_parser().parse_args(argv)
    from .. import engine
    engine.set_nograd_gemm_mode(nograd_gemm_mode(args))
    thresholds, at = sweep_thresholds(args.sweep, args.bkg_thre)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl")
    ds = voc.VOC12SegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.infer_set, stage="val",
                             aug=False, ignore_index=args.ignore_index, num_classes=args.num_classes)
    if world > 1:
        ds = Subset(ds, list(range(dist.get_rank(), len(ds), world)))
    loader = DeviceValLoader(DataLoader(ds, batch_size=1, shuffle=False, num_workers=8, pin_memory=False, drop_last=False,
                                        collate_fn=raw_collate), dev)
    model = siamese_network(backbone=args.backbone, num_classes=args.num_classes, pretrained=False, aux_layer=-3)
    load_checkpoint(model, args.model_path)
    model.to(dev)
    model.eval()
    base_dir = args.model_path.split("checkpoint")[0]
    dirs = {"cam": os.path.join(base_dir, "cam_img", args.infer_set), "aux_cam": os.path.join(base_dir, "cam_img_aux", args.infer_set),
            "labels": os.path.join(base_dir, "cam_labels", args.infer_set), "labels_rgb": os.path.join(base_dir, "cam_labels_rgb", args.infer_set)}
    for key in (("cam", "aux_cam") if args.save_img else ()) + (("labels", "labels_rgb") if args.save_labels else ()):
        os.makedirs(dirs[key], exist_ok=True)

    def on_image(name, inputs, which, label, value):
        nm = str(name[0] if isinstance(name, (tuple, list)) else name)
        if args.save_img:
            # the reference blends the aux colour with itself (infer_cam_voc.py:86): the truncated colour alone
            rgb = ops.cam_overlay(value, inputs if which == "cam" else None, alpha=0.6)
            Image.fromarray(rgb[0].cpu().numpy()).save(os.path.join(dirs[which], nm + ".jpg"))
        if args.save_labels and which == "cam":
            lab = label[0].cpu().numpy()
            Image.fromarray(lab).save(os.path.join(dirs["labels"], nm + ".png"))
            Image.fromarray(imutils.encode_cmap(lab).astype(np.uint8)).save(os.path.join(dirs["labels_rgb"], nm + ".png"))

    sw_cam, sw_aux = infer_cams(model, loader, args, thresholds, at, on_image if (args.save_img or args.save_labels) else None)
    if int(os.environ.get("RANK", "0")) != 0:
        return None
    sc_cam, sc_aux = sw_cam.scores(), sw_aux.scores()
    print(format_tabs([sc_cam[at], sc_aux[at]], ["cam", "aux_cam"], cat_list=voc.class_list))
    last = {"cam mIoU": sc_cam[at]["miou"], "aux_cam mIoU": sc_aux[at]["miou"]}
    if args.sweep:
        for t, a, b in zip(thresholds, sc_cam, sc_aux):
            print(f"bkg_thre {t:.4f}: cam mIoU {a['miou'] * 100:.3f}  aux_cam mIoU {b['miou'] * 100:.3f}")
        for key, sw in (("cam", sw_cam), ("aux_cam", sw_aux)):
            t, s = sw.best()
            last[f"{key} best_bkg_thre"], last[f"{key} best mIoU"] = t, s["miou"]
    print(last)
    return last


if __name__ == "__main__":
    main()
