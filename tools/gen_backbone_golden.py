"""Golden fixtures for the backbone family (authoring machine only: needs the reference tree; CPU only).

Run:  python tools/gen_backbone_golden.py

For each family member that the reference exports and this package registers, the REFERENCE's
`network(backbone=name, num_classes=21)` is built (oracle.gen_golden.import_reference: the reference is only called) and
`oracle.make_student_params(cfg, 21, seed=11)` is loaded into it strictly.  Written:

  tests/golden/backbones.json     per name: the factory's hyper-parameters, read off the reference's encoder, and the ordered
                                  state_dict keys with their shapes
  tests/golden/<name>_fwd.npz     for FWD_NAMES: the reference's outputs on synthetic_batch(2, 20, 224, seed=12), the fields of
                                  vitb_224.npz (cls, seg, x4_sub = x4[:, ::16], cls_aux, cam_aux, cam)

The oracle (generic over ViTConfig) is run on the same weights and inputs and must give the reference's outputs exactly
(0.0), as oracle/gen_golden.py establishes for ViT-B: that pins the oracle at the new widths and grids.
"""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import dupl_oracle as O  # noqa: E402
from oracle import gen_golden as G  # noqa: E402

NAMES = ("deit_tiny_patch16_224", "deit_small_patch16_224", "deit_base_patch16_384", "vit_base_patch16_384",
         "vit_large_patch16_224", "vit_large_patch16_384")
FWD_NAMES = ("deit_tiny_patch16_224", "deit_small_patch16_224", "vit_base_patch16_384", "vit_large_patch16_224")
NC = 21


def hyper_parameters(enc) -> dict:
    """What the reference's factory built, read off the module itself."""
    blk = enc.blocks[0]
    D = enc.embed_dim
    gh, gw = enc.patch_embed.img_size[0] // enc.patch_embed.patch_size[0], enc.patch_embed.img_size[1] // enc.patch_embed.patch_size[1]
    assert gh == gw and enc.pos_embed.shape[1] == gh * gw + 1
    return dict(embed_dim=D, depth=len(enc.blocks), num_heads=blk.attn.num_heads, mlp_ratio=blk.mlp.fc1.out_features // D,
                patch=enc.patch_embed.patch_size[0], img_size=enc.patch_embed.img_size[0], grid=gh,
                qkv_bias=blk.attn.qkv.bias is not None, ln_eps=blk.norm1.eps, head_classes=enc.head.out_features)


def main():
    torch.set_num_threads(8)
    R = G.import_reference()
    table = {}
    xb, _, _ = O.synthetic_batch(2, 20, 224, seed=12)
    for name in NAMES:
        net = R["network"](name, num_classes=NC, pretrained=False, aux_layer=-3)
        hp = hyper_parameters(net.encoder)
        cfg = O.ViTConfig(embed_dim=hp["embed_dim"], depth=hp["depth"], num_heads=hp["num_heads"], mlp_ratio=hp["mlp_ratio"],
                          patch=hp["patch"], img_size=hp["img_size"], ln_eps=hp["ln_eps"], head_classes=hp["head_classes"])
        sp = O.make_student_params(cfg, NC, seed=11)
        net.load_state_dict(sp, strict=True)
        net.eval()
        table[name] = dict(hp, state_dict=[[k, list(v.shape)] for k, v in net.state_dict().items()])
        assert [k for k, _ in table[name]["state_dict"]] == list(sp), name
        print(f"{name}: {hp}, {len(sp)} tensors, {sum(v.numel() for v in sp.values()) / 1e6:.1f} M elements")
        if name not in FWD_NAMES:
            continue
        with torch.no_grad():
            rb = net(xb)
            rbc = net(xb, cam_only=True)
            ob = O.network_forward(sp, xb, cfg)
            obc = O.network_forward(sp, xb, cfg, cam_only=True)
        for a, b_, n in zip(ob + obc, rb + rbc, ("cls", "seg", "x4", "cls_aux", "cam_aux", "cam")):
            err = (a.double() - b_.double()).abs().max().item()
            print(f"    {n}: oracle vs reference {err:.1e}")
            assert err == 0.0, (name, n, err)
        G.npz(name + "_fwd", cls=rb[0], seg=rb[1], x4_sub=rb[2][:, ::16], cls_aux=rb[3], cam_aux=rbc[0], cam=rbc[1])
    path = os.path.join(G.GOLD, "backbones.json")
    with open(path, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
