#!/usr/bin/env python
"""Digests of what one training step computes, for checking that a restructuring of the engine's launch schedule changes no bit:
per case one phase-B step (ms-CAM, both students' forward / backward on two streams, PAR refinement, every loss) in deterministic
mode -- the only mode in which two runs of the same schedule agree bit for bit -- and the sha256 of every loss, the four CAM tensors,
the refined and pseudo label maps and the whole flat gradient buffer, plus the step's peak allocated memory.  Uses the public model
API only, so the same file, copied into the tools/ of an older tree, runs there unmodified and the two outputs can be compared line
by line:

    python tools/step_digest.py [--cases a,b,...] > new.jsonl"""
import argparse
import gc
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dupl_amd  # noqa: E402
from dupl_amd import engine, trainer  # noqa: E402
from dupl_amd.model.model_dupl import siamese_network  # noqa: E402
from dupl_amd.model.PAR import PAR  # noqa: E402
from oracle import dupl_oracle as O  # noqa: E402

KEEP = ("loss", "cls_loss", "ptc_loss", "seg_loss", "sim_loss", "cams_1", "cams_aux_1", "cams_2", "cams_aux_2", "refined_1", "refined_2",
        "pseudo_label_aux_1")
# case -> (backbone, oracle config, images, image size, switches); a switch names a module attribute of the engine or one of its modes
BASE = ("deit_base_patch16_224", O.VIT_BASE, 2, 96)
TINY = ("tiny_test", O.VIT_TINY, 3, 128)
CASES = {
    "a": BASE + ({},),                          # defaults: merged pass, segmented attention, k-major backward, grouped weight gradients
    "b": BASE + ({"MERGED_PASS": 0},),          # cam_logits_shared + cam_logits_multi
    "c": BASE + ({"KM_BWD": False},),           # transposed-planes backward
    "d": BASE + ({"FMT1": False},),
    "e": BASE + ({"NOGRAD_GEMM": "f16"},),
    "f": TINY + ({"GEMM_MODE": "f32"},),        # the exact-f32 encoder, saving and merged
    "g": TINY + ({},),                          # head dim 32: the f32 attention inside the planes encoder
}


def sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def settled_grad(model):
    """The flat gradient buffer as a reader must see it: ranges a lazy zero_grad left unwritten read as zeros (a tree without lazy
    ranges has nothing to settle)."""
    store = model.flat_storage
    if hasattr(store, "settle_grads"):
        store.settle_grads()
        torch.cuda.synchronize()
    return store.grad


def zero_grad(model):
    """What trainer.train_step's zero_grad leaves: where the tree zeroes lazily, the lazy ranges hold NaN, so that a range nobody
    overwrote or settled shows in the digest."""
    store = model.flat_storage
    if hasattr(store, "zero_grad"):
        store.grad.fill_(float("nan"))
        store.zero_grad(lazy=True)
    else:
        store.grad.zero_()


def build(backbone, cfg, dev):
    model = siamese_network(backbone, num_classes=21, pretrained=False, aux_layer=-3)
    model.load_state_dict(O.make_siamese_params(cfg, 21, seed=5), strict=True)
    model.to(dev)
    model.enable_dual_stream(True)
    return model


def step(backbone, cfg, B, S, dev):
    model = build(backbone, cfg, dev)
    par = PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]).to(dev)
    inputs, cls_label, img_box = O.synthetic_batch(B, 20, S, seed=11)
    zero_grad(model)
    loss, out = trainer.compute_losses(model, par, inputs.to(dev), cls_label.to(dev), img_box, 5000, trainer.StepArgs(),
                                       cls_label_host=cls_label)
    loss.sum().backward()
    model.flat_storage.wait_streams()
    torch.cuda.synchronize()
    d = {k: sha(out[k]) for k in KEEP}
    d["grad"] = sha(settled_grad(model))
    return d


def eval_paths(dev):
    """Case h: the no-grad forwards (training / val branch, cam_only, the stand-alone decoder) and forward_features with autograd."""
    backbone, cfg, B, S, _ = CASES["a"]
    model = build(backbone, cfg, dev)
    x = O.synthetic_batch(B, 20, S, seed=11)[0].to(dev)
    d = {}
    with torch.no_grad():
        for br, outs in model(x, val=True).items():
            for name, t in zip(("cls", "seg", "x4", "cls_aux"), outs):
                d[f"{br}.{name}"] = sha(t)
        for name, t in zip(("cam_aux_1", "cam_1", "cam_aux_2", "cam_2"), model(x, cam_only=True)):
            d[name] = sha(t)
        d["decoder"] = sha(model.branch1.decoder(model(x, val=True, branch=1)[2]))
    zero_grad(model)
    outs = model.branch1.encoder(x)
    R = [O.hash_normal(f"rf{i}", tuple(o.shape), seed=2).to(dev) for i, o in enumerate(outs)]
    sum((o * r).sum() for o, r in zip(outs, R)).backward()
    torch.cuda.synchronize()
    for name, t in zip(("ff.cls", "ff.tokens", "ff.aux"), outs):
        d[name] = sha(t)
    d["ff.grad"] = sha(settled_grad(model))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c,d,e,f,g,h")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dupl_amd.set_deterministic(True)
    for case in a.cases.split(","):
        switches = CASES[case][4] if case in CASES else {}
        prev = {k: getattr(engine, k) for k in switches}
        for k, v in switches.items():
            setattr(engine, k, v)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        try:
            d = step(*CASES[case][:4], dev) if case in CASES else eval_paths(dev)
        finally:
            for k, v in prev.items():
                setattr(engine, k, v)
        print(json.dumps({"case": case, "peak_bytes": torch.cuda.max_memory_allocated(), "digests": d}), flush=True)


if __name__ == "__main__":
    main()
