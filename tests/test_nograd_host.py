"""The public surface of the opt-in single-product mode of the no-grad encoder passes, without a GPU: the --nograd_gemm flag of the
training scripts, tools/eval_seg and tools/infer_cam (default f16x3, choices f16x3 | f16) and engine.set_nograd_gemm_mode.
tools/infer_cam leaves the attribute out of the namespace when the flag is not given (its plain namespace is pinned to the reference's
flag set by tests/test_infer_cam_host.py) and supplies the default through infer_cam.nograd_gemm_mode."""
import pytest


def _value(ns):
    from dupl_amd.tools import infer_cam
    return infer_cam.nograd_gemm_mode(ns)


def _parsers():
    from dupl_amd import train_main
    from dupl_amd.tools import eval_seg, infer_cam
    return {"train voc": train_main.build_parser("voc"), "train coco": train_main.build_parser("coco"),
            "eval_seg voc": eval_seg.build_parser("voc"), "eval_seg coco": eval_seg.build_parser("coco"),
            "infer_cam": infer_cam.build_parser()}


def test_nograd_gemm_flag_defaults_and_choices(monkeypatch):
    monkeypatch.delenv("DUPL_NOGRAD_GEMM", raising=False)
    for name, p in _parsers().items():
        assert _value(p.parse_args([])) == "f16x3", name
        assert p.parse_args(["--nograd_gemm", "f16"]).nograd_gemm == "f16", name
        assert p.parse_args(["--nograd_gemm", "f16x3"]).nograd_gemm == "f16x3", name
        for bad in ("f32", "bf16", "F16", ""):
            with pytest.raises(SystemExit):
                p.parse_args(["--nograd_gemm", bad])


def test_nograd_gemm_flag_default_follows_the_environment(monkeypatch):
    monkeypatch.setenv("DUPL_NOGRAD_GEMM", "f16")
    for name, p in _parsers().items():
        assert _value(p.parse_args([])) == "f16", name


def test_set_nograd_gemm_mode_accepts_the_two_modes_only():
    from dupl_amd import engine
    prev = engine.NOGRAD_GEMM
    try:
        for mode in ("f16", "f16x3"):
            engine.set_nograd_gemm_mode(mode)
            assert engine.NOGRAD_GEMM == mode
        for bad in ("f32", "bf16", "F16", "", None, 1):
            with pytest.raises(ValueError):
                engine.set_nograd_gemm_mode(bad)
            assert engine.NOGRAD_GEMM == "f16x3"
    finally:
        engine.set_nograd_gemm_mode(prev)


def test_single_product_only_for_passes_that_save_nothing():
    """nograd_products: 1 only under "f16", GEMM_MODE "f16x3" and save=False."""
    from dupl_amd import engine
    prev, prev_g = engine.NOGRAD_GEMM, engine.GEMM_MODE
    try:
        engine.set_gemm_mode("f16x3")
        engine.set_nograd_gemm_mode("f16x3")
        assert engine.nograd_products(False) == 3 and engine.nograd_products(True) == 3
        engine.set_nograd_gemm_mode("f16")
        assert engine.nograd_products(False) == 1 and engine.nograd_products(True) == 3
        engine.set_gemm_mode("f32")
        assert engine.nograd_products(False) == 3
    finally:
        engine.set_gemm_mode(prev_g)
        engine.set_nograd_gemm_mode(prev)
