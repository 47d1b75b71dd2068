"""Backbone factories on the path (reference: model/backbone/__init__.py, deit.py:68-109,356-368, vit.py:1092-1145).

The family is every reference factory that is a plain `VisionTransformer` with patch 16, head dim 64, `qkv_bias=True`,
`mlp_ratio=4` and LayerNorm eps 1e-6: DeiT-T/S/B, ViT-B and ViT-L, with a 224 (14 x 14) or 384 (24 x 24) position-embedding grid.
Members differ in width, depth, number of heads and grid; two names of the same shape (`deit_base_patch16_224` /
`vit_base_patch16_224`, and the two base-384 names) differ only in which pretrained file the reference fetches.  There is no
network here, so `pretrained` must be falsy or a path to a local state_dict.  Every other name the reference exports is
refused, with the reason (`_REFUSED`).
`tiny_test` is the 4-layer/96-dim configuration the golden vectors were generated with.
"""
import dataclasses
import re

from ...engine import EncoderConfig

_REGISTRY = {
    "deit_base_patch16_224": dict(),
    "vit_base_patch16_224": dict(),
    "deit_tiny_patch16_224": dict(embed_dim=192, depth=12, num_heads=3),
    "deit_small_patch16_224": dict(embed_dim=384, depth=12, num_heads=6),
    "deit_base_patch16_384": dict(img_size=384),
    "vit_base_patch16_384": dict(img_size=384),
    "vit_large_patch16_224": dict(embed_dim=1024, depth=24, num_heads=16),
    "vit_large_patch16_384": dict(embed_dim=1024, depth=24, num_heads=16, img_size=384),
    "tiny_test": dict(embed_dim=96, depth=4, num_heads=3, head_classes=10),
}

# the reference's factories: those behind --backbone (everything but the golden-vector model)
FAMILY = tuple(k for k in _REGISTRY if k != "tiny_test")

# why a name the reference exports is not served: (pattern, reason), first match wins
_REFUSED = (
    (r"_distilled_", "a DistilledVisionTransformer: forward_features returns a 4-tuple that the reference's own `network` "
                     "cannot consume"),
    (r"_patch(?!16_)\d+_", "its patch size is not 16"),
    (r"_dino$|^dino_", "loads its weights from an absolute path of the authors' machine"),
    (r"_(with_attn|with_aff|mct|memo|mask(_v\d+)?)$", "another model class (attention / affinity / multi-class-token / memory / "
                                                      "mask variants of the VisionTransformer), not the encoder DuPL trains"),
    (r"resnet", "a hybrid CNN + transformer; the engine embeds 16 x 16 patches with one convolution"),
    (r"^vit_small_patch16_224$", "head dim 96 (768 / 8) and no qkv bias; the split attention serves head dim 64 with qkv bias"),
    (r"^vit_huge_", "head dim 80 (1280 / 16); the split attention serves head dim 64"),
)


def refusal_reason(backbone: str):
    """Why `backbone` is refused, or None for a name the reference does not export either."""
    for pat, why in _REFUSED:
        if re.search(pat, backbone):
            return why
    return None


def encoder_config(backbone, aux_layer=None) -> EncoderConfig:
    """The EncoderConfig of a registered name.  An EncoderConfig itself passes through (a member of the family at a reduced
    depth, for tests and experiments); the engine's own checks decide which kernels its shapes take."""
    if isinstance(backbone, EncoderConfig):
        return backbone if aux_layer is None else dataclasses.replace(backbone, aux_layer=aux_layer)
    if backbone not in _REGISTRY:
        why = refusal_reason(str(backbone))
        raise ValueError(f"backbone {backbone!r} is not on the DuPL hot path"
                         + (f": {why}" if why else " (the reference exports no such factory)")
                         + f".  The family that works is the plain patch-16 VisionTransformers with head dim 64, qkv bias and "
                           f"mlp_ratio 4: {', '.join(FAMILY)} (and tiny_test, the golden-vector model)")
    kw = dict(_REGISTRY[backbone])
    if aux_layer is not None:
        kw["aux_layer"] = aux_layer
    return EncoderConfig(**kw)


def load_pretrained_encoder(encoder_module, path: str, patch: int = 16):
    """The reference's two pretrained-weight routes, fed from a LOCAL file (no network here):

    * deit.py:73-78,88-93,101-108,361-367 (`deit_tiny/small_patch16_224`, `deit_base_patch16_224/384`):
      `torch.hub.load_state_dict_from_url(...)["model"]` then a STRICT `model.load_state_dict` -> a `{"model": state_dict}` file;
    * vit.py:1098-1100,1110-1111,1132-1133,1143-1144 (`vit_base_patch16_224/384`, `vit_large_patch16_224/384`, ImageNet-21k
      init): timm 0.4.12 `load_pretrained(model, num_classes=model.num_classes, in_chans=3[, filter_fn=_conv_filter])`: a FLAT
      state_dict (the `jx_vit_*` files), `_conv_filter` (vit.py:1058-1065) reshapes a manually-patchified
      `patch_embed.proj.weight` (D, 3*p*p) to the conv layout (D, 3, p, p); the encoder keeps its 1000-way `head`, so timm
      leaves the classifier in and loads strictly.

    Both are strict in the reference; a file with missing / unexpected keys (distilled DeiT, `module.`-prefixed, a
    whole-`network` checkpoint) therefore raises here too instead of silently training from random init.  A 384 factory's own
    file carries a 577-row `pos_embed` (24 x 24 + cls), which is that factory's parameter shape and loads as is; the resize to a
    run's token grid starts from there.  A file of another width or position grid raises with both shapes named."""
    import torch
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    out = {}
    for k, v in sd.items():
        if "patch_embed.proj.weight" in k and v.dim() == 2:      # _conv_filter
            v = v.reshape(v.shape[0], 3, patch, patch)
        out[k] = v
    want = {k: tuple(v.shape) for k, v in encoder_module.state_dict().items()}
    bad = [(k, tuple(out[k].shape), want[k]) for k in ("pos_embed", "cls_token", "patch_embed.proj.weight")
           if k in out and k in want and tuple(out[k].shape) != want[k]]
    if bad:
        k, got, exp = bad[0]
        raise ValueError(f"pretrained file {path!r} is for another backbone: {k} is {got} in the file, {exp} in this model "
                         f"(embed dim {want['cls_token'][-1]}, {want['pos_embed'][1]} position rows); pass the file of the "
                         f"--backbone in use")
    encoder_module.load_state_dict(out, strict=True)
