"""The backbone family behind --backbone, on the host: registry vs the reference's factories (tests/golden/backbones.json, written
by tools/gen_backbone_golden.py from the reference's own modules), refused names, pretrained routes, copy / pickle, and the
gradient-exchange / in-backward-update plans at depth 24."""
import copy
import json
import os
import pickle

import pytest
import torch

FAMILY = ("deit_tiny_patch16_224", "deit_small_patch16_224", "deit_base_patch16_384", "vit_base_patch16_384",
          "vit_large_patch16_224", "vit_large_patch16_384")
# every other factory the reference's model/backbone/__init__.py exports, and the hybrid / patch-32 factories of its vit.py
REFUSED = ("vit_small_patch16_224", "deit_tiny_distilled_patch16_224", "deit_small_distilled_patch16_224",
           "deit_base_distilled_patch16_224", "deit_base_distilled_patch16_384", "deit_base_patch16_224_dino",
           "deit_base_patch16_224_with_attn", "deit_base_patch16_224_mct", "deit_base_patch16_224_memo", "deit_base_patch16_224_mask",
           "deit_base_patch16_224_mask_v1", "deit_base_patch16_224_with_aff", "vit_base_patch32_384", "vit_large_patch32_384",
           "vit_small_resnet26d_224", "vit_base_resnet50d_224")
NC = 21


@pytest.fixture(scope="module")
def table(golden_dir):
    with open(os.path.join(golden_dir, "backbones.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", FAMILY)
def test_encoder_config_has_the_reference_factorys_hyper_parameters(table, name):
    from dupl_amd.model.backbone import encoder_config
    cfg, ref = encoder_config(name), table[name]
    assert ref["qkv_bias"] is True and ref["embed_dim"] // ref["num_heads"] == 64       # what makes a factory a family member
    for k in ("embed_dim", "depth", "num_heads", "mlp_ratio", "patch", "img_size", "grid", "ln_eps", "head_classes"):
        assert getattr(cfg, k) == ref[k], (name, k, getattr(cfg, k), ref[k])
    assert cfg.head_dim == 64 and cfg.aux_layer == -3
    assert encoder_config(name, aux_layer=-1).aux_layer == -1


def test_the_existing_names_are_unchanged():
    from dupl_amd.engine import EncoderConfig
    from dupl_amd.model.backbone import encoder_config
    assert encoder_config("deit_base_patch16_224") == encoder_config("vit_base_patch16_224") == EncoderConfig()
    assert encoder_config("tiny_test") == EncoderConfig(embed_dim=96, depth=4, num_heads=3, head_classes=10)


@pytest.mark.parametrize("name", FAMILY)
def test_state_dict_keys_and_shapes_are_the_references(table, name, monkeypatch):
    from dupl_amd.model import model_dupl
    # keys and shapes only: the reference initialisation is skipped, so the flat buffers of the 2 x 304 M-parameter ViT-L pair stay
    # untouched zero pages
    monkeypatch.setattr(model_dupl, "_reference_init", lambda store, student: None)
    model = model_dupl.siamese_network(name, num_classes=NC, pretrained=False, aux_layer=-3)
    want = [(br + k, tuple(shp)) for br in ("branch1.", "branch2.") for k, shp in table[name]["state_dict"]]
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    # the same keys with the same shapes (a strict load does not depend on the order; the module tree registers `blocks` first) ...
    assert len(got) == len(want) and dict(got) == dict(want)
    # ... and the flat storage's parameter list is in the reference's own order
    from dupl_amd.engine import student_param_shapes
    assert [[k, list(shp)] for k, shp in student_param_shapes(model.branch1._cfg, NC).items()] == table[name]["state_dict"]
    groups = model.get_param_groups()
    n_groups = sum(p.numel() for g in groups for p in g)
    n_params = sum(p.numel() for p in model.parameters())
    assert n_groups == n_params and len({id(p) for g in groups for p in g}) == sum(len(g) for g in groups)
    depth = table[name]["depth"]
    assert [len(g) for g in groups] == [2 * (6 + 8 * depth), 2 * (4 * depth + 2), 4, 6]
    assert model.branch1.encoder.embed_dim == table[name]["embed_dim"] and len(model.branch2.encoder.blocks) == depth


@pytest.mark.parametrize("name", REFUSED + ("no_such_backbone",))
def test_other_reference_factories_stay_refused_with_the_reason(name):
    from dupl_amd.model.backbone import encoder_config, refusal_reason
    from dupl_amd.model.model_dupl import network
    with pytest.raises(ValueError) as e:
        encoder_config(name)
    msg = str(e.value)
    assert repr(name) in msg and "deit_small_patch16_224" in msg and "vit_large_patch16_224" in msg      # a working family member
    if name != "no_such_backbone":
        assert refusal_reason(name) and refusal_reason(name) in msg
    with pytest.raises(ValueError):
        network(name, num_classes=NC, pretrained=False)


def test_refusal_reasons_name_the_property_that_rules_the_factory_out():
    from dupl_amd.model.backbone import refusal_reason
    assert "head dim 96" in refusal_reason("vit_small_patch16_224") and "qkv bias" in refusal_reason("vit_small_patch16_224")
    assert "4-tuple" in refusal_reason("deit_base_distilled_patch16_384")
    assert "absolute path" in refusal_reason("deit_base_patch16_224_dino")
    for n in ("deit_base_patch16_224_with_attn", "deit_base_patch16_224_mct", "deit_base_patch16_224_memo",
              "deit_base_patch16_224_mask", "deit_base_patch16_224_mask_v1", "deit_base_patch16_224_with_aff"):
        assert "another model class" in refusal_reason(n), n
    assert "hybrid" in refusal_reason("vit_base_resnet50d_224") and "patch size" in refusal_reason("vit_large_patch32_384")
    for n in FAMILY + ("deit_base_patch16_224", "vit_base_patch16_224"):
        assert refusal_reason(n) is None, n


# ---------------------------------------------------------------------------------------------------- pretrained routes
def _encoder_state(cfg, rows=None, seed=5):
    """A synthetic encoder state_dict of `cfg`'s shapes (optionally with another number of pos_embed rows)."""
    from dupl_amd.engine import student_param_shapes
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in student_param_shapes(cfg, NC).items():
        if k.startswith("encoder."):
            if k == "encoder.pos_embed" and rows is not None:
                shp = (1, rows, shp[2])
            sd[k[len("encoder."):]] = torch.randn(shp, generator=g) * 0.02
    return sd


def _shallow(name, depth=3):
    """The named factory's width, heads and grid at a reduced depth: the pretrained routes do not depend on the depth."""
    import dataclasses
    from dupl_amd.model.backbone import encoder_config
    return dataclasses.replace(encoder_config(name), depth=depth)


@pytest.mark.parametrize("route", ["deit", "timm", "timm_patchified"])
def test_pretrained_routes_load_a_local_file_strictly(tmp_path, route):
    from dupl_amd.model.model_dupl import network, siamese_network
    name = "deit_small_patch16_224" if route == "deit" else "vit_large_patch16_224"
    cfg = _shallow(name)
    sd = _encoder_state(cfg)
    saved = dict(sd)
    if route == "timm_patchified":      # vit.py:1058-1065 (_conv_filter): a manually patchified stem weight
        saved["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"].reshape(cfg.embed_dim, -1)
    path = str(tmp_path / "w.pth")
    torch.save({"model": saved} if route == "deit" else saved, path)
    net = network(cfg, num_classes=NC, pretrained=path, aux_layer=-3)
    for k, v in sd.items():
        assert torch.equal(net.state_dict()["encoder." + k], v), k
    pair = siamese_network(cfg, num_classes=NC, pretrained=path, aux_layer=-3)
    for br in ("branch1.", "branch2."):
        assert torch.equal(pair.state_dict()[br + "encoder.blocks.2.mlp.fc2.weight"], sd["blocks.2.mlp.fc2.weight"])
    # strict like the reference: a missing tensor raises, nothing is left at its random init silently
    del saved["blocks.1.attn.qkv.bias"]
    torch.save({"model": saved} if route == "deit" else saved, path)
    with pytest.raises(RuntimeError, match="blocks.1.attn.qkv.bias"):
        network(cfg, num_classes=NC, pretrained=path, aux_layer=-3)


def test_a_384_file_loads_its_577_position_rows_as_they_are(tmp_path):
    from dupl_amd.model.model_dupl import network
    cfg = _shallow("vit_base_patch16_384")
    sd = _encoder_state(cfg)
    assert sd["pos_embed"].shape == (1, 577, 768)
    path = str(tmp_path / "w384.pth")
    torch.save(sd, path)
    net = network(cfg, num_classes=NC, pretrained=path, aux_layer=-3)
    assert torch.equal(net.encoder.pos_embed, sd["pos_embed"])
    path224 = str(tmp_path / "w224.pth")
    torch.save(_encoder_state(cfg, rows=197), path224)
    with pytest.raises(ValueError) as e:
        network(cfg, num_classes=NC, pretrained=path224, aux_layer=-3)
    assert "(1, 197, 768)" in str(e.value) and "(1, 577, 768)" in str(e.value)


def test_a_file_of_another_width_raises_with_both_shapes(tmp_path):
    from dupl_amd.model.model_dupl import network, siamese_network
    path = str(tmp_path / "small.pth")
    torch.save({"model": _encoder_state(_shallow("deit_small_patch16_224"))}, path)
    base = _shallow("deit_base_patch16_224")
    for ctor in (network, siamese_network):
        with pytest.raises(ValueError) as e:
            ctor(base, num_classes=NC, pretrained=path, aux_layer=-3)
        assert "384" in str(e.value) and "768" in str(e.value)


# ---------------------------------------------------------------------------------------------------- copy / pickle
@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_copies_keep_the_backbone_and_its_shapes(how):
    from dupl_amd.model.model_dupl import network, siamese_network
    name = "deit_tiny_patch16_224"
    for ctor in (siamese_network, network):
        m = ctor(name, num_classes=NC, pretrained=False, aux_layer=-3)
        c = copy.deepcopy(m) if how == "deepcopy" else pickle.loads(pickle.dumps(m))
        assert c._ctor == m._ctor == (name, NC, -3)
        a, b = m.state_dict(), c.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        first = c.branch1 if ctor is siamese_network else c
        assert first._cfg.embed_dim == 192 and first._cfg.num_heads == 3 and first.encoder.embed_dim == 192
        assert b[("branch1." if ctor is siamese_network else "") + "encoder.blocks.11.attn.qkv.weight"].shape == (576, 192)


# ---------------------------------------------------------------------------------------------------- exchange / update plans
def _assert_tiles_once(pieces, lo, hi, what):
    pieces = sorted(pieces)
    assert pieces[0][0] == lo and pieces[-1][1] == hi, (what, pieces[0], pieces[-1], lo, hi)
    assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(pieces, pieces[1:])), what


@pytest.mark.parametrize("name", ["vit_large_patch16_224", "vit_large_patch16_384"])
def test_exchange_and_update_plans_cover_depth_24_exactly_once(name):
    """ddp.GradReducer's bucket plan and PolyWarmupAdamW's in-backward plan (begin_step: store.grad_buckets(s)) are derived from the
    parameter list: at depth 24 both tile each student's trainable range exactly once, every trigger is an event the backward pass
    emits ("heads", a block index, "stem"), in the order it emits them, and every trainable tensor lies inside one piece."""
    from dupl_amd.ddp import GradReducer
    from dupl_amd.engine import FlatStorage, SEG_FROZEN, param_segment
    from dupl_amd.model.backbone import encoder_config
    cfg = encoder_config(name)
    store = FlatStorage(cfg, NC, 2)          # zero pages: nothing is touched
    red = GradReducer(store)
    emitted = ["heads"] + list(reversed(range(cfg.depth))) + ["stem"]
    for s in (0, 1):
        lo, hi = store.trainable_range(s)
        for what, plan in (("reducer", red.plan[s]), ("optimiser", store.grad_buckets(s)), ("one block per bucket", store.grad_buckets(s, 1)),
                           ("five blocks per bucket", store.grad_buckets(s, 5))):
            _assert_tiles_once([(a, b) for a, b, _ in plan], lo, hi, (name, s, what))
            trig = [t for _, _, t in plan]
            assert all(t in emitted for t in trig), (what, trig)
            pos = [emitted.index(t) for t in trig]
            assert pos == sorted(pos) and trig[0] == "heads" and trig[-2:] == ["stem", "stem"], (what, trig)
            # a block's tensors are final when the plan says so: the piece triggered by block i holds blocks >= i only
            for a, b, t in plan:
                if isinstance(t, int):
                    blocks = [i for i in range(cfg.depth) if a <= s * store.student_numel + store.block_range(i)[0] < b]
                    assert blocks and min(blocks) == t, (what, t, blocks)
            for key, (off, n) in store.layout.items():
                if param_segment(key) != SEG_FROZEN:
                    o = s * store.student_numel + off
                    assert sum(1 for a, b, _ in plan if a <= o and o + n <= b) == 1, (what, key)
        assert len(red.plan[s]) == 1 + 11 + 2       # heads, blocks 22, 20, ... 2, stem (blocks 0-1 + embedding), norm
        _assert_tiles_once(red.student_buckets(s), lo, hi, (name, s, "size buckets"))


# ---------------------------------------------------------------------------------------------------- entry points
def test_parsers_and_aliases_take_the_new_names():
    """train_final_voc.py / train_final_coco.py, eval_seg and infer_cam accept every family member and name the family in --help; the
    reference's own import lines (install_reference_aliases: process-wide sys.modules entries, hence a child process) build it."""
    import subprocess
    import sys
    from dupl_amd import train_main
    from dupl_amd.tools import eval_seg, infer_cam
    parsers = [train_main.build_parser("voc"), train_main.build_parser("coco"), eval_seg.build_parser("voc"),
               eval_seg.build_parser("coco"), infer_cam.build_parser()]
    for p in parsers:
        text = " ".join(p.format_help().split())
        for name in FAMILY:
            assert p.parse_args(["--backbone", name]).backbone == name
            assert name in text, name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import dupl_amd; dupl_amd.install_reference_aliases()\n"
            "from model.model_dupl import network\n"
            "from model.backbone import encoder_config\n"
            "n = network('deit_tiny_patch16_224', num_classes=21, pretrained=False, aux_layer=-3)\n"
            "assert n.encoder.embed_dim == 192 and len(n.encoder.blocks) == 12 and n.in_channels == [192] * 4\n"
            "assert encoder_config('vit_large_patch16_384').grid == 24\n"
            "print('ALIASES_OK')\n") % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "ALIASES_OK" in r.stdout, r.stdout + r.stderr


def test_a_checkpoint_of_another_width_is_refused_with_both_widths():
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.tools import eval_seg
    small = siamese_network(_shallow("deit_small_patch16_224"), num_classes=NC, pretrained=False, aux_layer=-3)
    ckpt = {"module." + k: v.clone() for k, v in small.state_dict().items()}      # train_final_voc.py:514-519: the DDP wrapper's keys
    again = siamese_network(_shallow("deit_small_patch16_224"), num_classes=NC, pretrained=False, aux_layer=-3)
    eval_seg.load_checkpoint(again, ckpt)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in small.state_dict().items())
    base = siamese_network(_shallow("deit_base_patch16_224"), num_classes=NC, pretrained=False, aux_layer=-3)
    with pytest.raises(ValueError) as e:
        eval_seg.load_checkpoint(base, ckpt)
    assert "expected width 768" in str(e.value) and "found width 384" in str(e.value)
    deep = siamese_network(_shallow("deit_small_patch16_224", depth=4), num_classes=NC, pretrained=False, aux_layer=-3)
    with pytest.raises(ValueError, match="expected depth 4.*found depth 3"):
        eval_seg.load_checkpoint(deep, ckpt)
