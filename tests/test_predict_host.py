"""The host side of label-less inference (tools/predict, ops.seg_decide / seg_paint / window_gather / window_merge): the C
descriptors and their mirrors, the window plan, the numpy references the GPU suite leans on (tests/seg_render_ref.py) pinned against
independent evaluations on the CPU, and the flags with what they refuse."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import seg_ensemble_ref as ER
import seg_render_ref as R

ENTRIES = {"dupl_seg_decide": ("SegDecideDesc", "dupl_seg_decide_desc"), "dupl_seg_paint": ("SegPaintDesc", "dupl_seg_paint_desc"),
           "dupl_window_gather": ("WindowGatherDesc", "dupl_window_gather_desc"),
           "dupl_window_merge": ("WindowMergeDesc", "dupl_window_merge_desc")}


def test_header_prototypes_lib_entries_and_descriptors_agree():
    import __graft_entry__ as ge
    ge.build()
    from dupl_amd import _lib
    protos = _lib.parse_header()
    L = _lib.lib()
    assert L.dupl_abi_version() == 4                               # the exports are additive
    checks = []
    for fn, (mirror, cname) in ENTRIES.items():
        M = getattr(_lib, mirror)
        assert protos[fn] == [ctypes.POINTER(M), ctypes.c_void_p], fn
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), fn) and getattr(L, fn).raw.argtypes == protos[fn]
        fields = [n for n, _ in M._fields_]
        checks.append((M, fields))
        assert fields[0] == "struct_size" and M().struct_size == ctypes.sizeof(M)
    body = ""
    for (M, fields), (_, cname) in zip(checks, ENTRIES.values()):
        body += f'printf("%zu", sizeof({cname})); ' + " ".join(f'printf(" %zu", offsetof({cname}, {n}));' for n in fields) + ' printf("\\n"); '
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dupl_hip.h"\nint main(void) { ' + body +
           'printf("%d %d\\n", DUPL_SEG_DECIDE_MAX_C, DUPL_WINDOW_MAX); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sz.c"), os.path.join(td, "sz")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(_lib.HEADER), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for (M, fields), ln in zip(checks, lines):
        out = [int(v) for v in ln.split()]
        assert out[0] == ctypes.sizeof(M), M.__name__
        assert out[1:] == [getattr(M, n).offset for n in fields], M.__name__
    assert [int(v) for v in lines[-1].split()] == [_lib.SEG_DECIDE_MAX_C, _lib.WINDOW_MAX]


@pytest.mark.parametrize("n,win,stride", R.PLAN_CASES)
def test_plan_windows_covers_every_token(n, win, stride):
    from dupl_amd.tools.predict import plan_windows
    starts = plan_windows(n, win, stride)
    size = min(n, win)
    assert starts == sorted(set(starts)) and starts[0] == 0
    assert all(0 <= s and s + size <= n for s in starts)            # never leaves the grid
    assert starts[-1] + size == n                                   # the last window ends at n
    covered = np.zeros(n, dtype=bool)
    for s in starts:
        covered[s:s + size] = True
    assert covered.all()
    if n <= win:
        assert starts == [0]
    else:
        assert all(b - a <= stride for a, b in zip(starts, starts[1:]))
        assert starts[:-1] == list(range(0, n - win, stride))


def test_window_and_stride_refusals():
    from dupl_amd.tools import predict
    for ok in ((0, 0), (0, 7), (16, 16), (448, 320), (64, 48), (64, 64)):
        predict.check_window_args(*ok)
    for bad in ((8, 8), (450, 320), (64, 40), (64, 0), (64, 80), (64, 8), (-16, 16)):
        with pytest.raises(ValueError) as ei:
            predict.check_window_args(*bad)
        assert "multiple of 16" in str(ei.value)
    assert predict.default_stride(448) == 288 and predict.default_stride(16) == 16 and predict.default_stride(64) % 16 == 0
    assert predict.windows_per_scale(160, 208, (1.0, 1.5), 64, 48) == [3 * 4, 5 * 6]
    assert predict.windows_per_scale(160, 208, (1.0, 1.5), 0, 0) == [1, 1]
    assert predict.windows_per_scale(60, 64, (1.0,), 64, 48) == [1]


def test_flags_defaults_and_refusals(tmp_path):
    from dupl_amd.tools import predict
    base = ["--input", str(tmp_path), "--out_dir", str(tmp_path / "o")]
    a = predict.parse_args(base)
    assert a.window == 0 and a.stride == 0 and a.window_batch == 8 and a.branch == "ens" and a.crf == 0 and a.min_conf == 0.0
    assert a.scales == (1.0, 1.5, 1.25) and a.alpha == 0.6 and a.contour == 0 and a.tint_background == 0 and a.save_conf == 0
    assert a.num_classes == 21 and a.class_names == "voc" and a.nograd_gemm in ("f16x3", "f16")
    a = predict.parse_args(base + ["--window", "448", "--scales", "(1.0, 0.5)", "--branch", "2"])
    assert a.window == 448 and a.stride == 288 and a.scales == (1.0, 0.5) and a.branch == "2"
    a = predict.parse_args(base + ["--window", "448", "--stride", "320", "--window_batch", "4"])
    assert (a.window, a.stride, a.window_batch) == (448, 320, 4)
    for bad, word in ((["--window", "450"], "--window"), (["--window", "64", "--stride", "40"], "--stride"),
                      (["--window", "64", "--stride", "80"], "--stride"), (["--window_batch", "0"], "--window_batch"),
                      (["--alpha", "1.5"], "--alpha"), (["--num_classes", "256"], "--num_classes")):
        with pytest.raises(SystemExit) as ei:
            predict.parse_args(base + bad)
        assert word in str(ei.value), bad
    for bad in (["--branch", "3"], ["--crf", "2"], []):
        with pytest.raises(SystemExit):
            predict.parse_args((base if bad else []) + bad)
    # refused by main before a device or a checkpoint is touched
    with pytest.raises(SystemExit) as ei:
        predict.main(base + ["--window", "100"])
    assert "multiple of 16" in str(ei.value)
    assert predict.class_names("voc")[15] == "person" and len(predict.class_names("coco")) == 81
    (tmp_path / "names.txt").write_text("sky\nroad\n\n")
    assert predict.class_names(str(tmp_path / "names.txt")) == ["sky", "road"]
    (tmp_path / "b.JPG").write_bytes(b"")
    (tmp_path / "a.png").write_bytes(b"")
    (tmp_path / "list.txt").write_text("a.png\n")
    assert [os.path.basename(p) for p in predict.list_inputs(str(tmp_path))] == ["a.png", "b.JPG"]
    assert predict.list_inputs(str(tmp_path / "list.txt")) == [str(tmp_path / "a.png")]
    assert predict.list_inputs(str(tmp_path / "a.png")) == [str(tmp_path / "a.png")]
    st = np.array([[6, 0, 3, 1], [6 << 23, 0, 3 << 24, 5]], dtype=np.int64)
    classes, rejected = predict.class_summary(st, ["bg", "x"], 10)
    assert rejected == 1 and [c["id"] for c in classes] == [0, 2] and classes[1]["name"] == "class2"
    assert classes[0] == {"id": 0, "name": "bg", "pixels": 6, "share": 0.6, "mean_conf": 0.5} and classes[1]["mean_conf"] == 1.0


@pytest.mark.parametrize("case", R.MERGE_CASES, ids=lambda c: f"C{c[0]}-{c[1][0]}x{c[1][1]}-w{c[2]}s{c[3]}")
def test_merge_reference_is_the_explicit_loop(case):
    C, (hs, ws), win, stride = case
    lg, org = R.merge_inputs(C, hs, ws, win, stride)
    got = R.merge_ref(lg.numpy(), org, hs, ws)
    nW, wth, wtw = len(org), lg.shape[2], lg.shape[3]
    want = torch.zeros(2, C, hs, ws)
    for f in range(2):
        for y in range(hs):
            for x in range(ws):
                s, n = torch.zeros(C), 0
                for k, (r0, c0) in enumerate(org):
                    if r0 <= y < r0 + wth and c0 <= x < c0 + wtw:
                        s = s + lg[f * nW + k, :, y - r0, x - c0]
                        n += 1
                assert n >= 1                                          # the plan covers every token
                want[f, :, y, x] = s / torch.tensor(float(n))
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32))
    assert len(org) > 1


@pytest.mark.parametrize("H,W", R.PAINT_SHAPES)
def test_paint_reference_is_the_rounded_float64_blend(H, W):
    from dupl_amd.utils import imutils
    pal = imutils.colormap()
    label, image = R.paint_inputs(H, W)
    if H * W > 100:
        assert {0, 255} <= set(np.unique(label).tolist())
    assert np.array_equal(R.paint_ref(label, pal), imutils.encode_cmap(label))
    for alpha in R.PAINT_ALPHAS:
        for tint in (False, True):
            blend = np.floor((image.astype(np.float64) * (256 - alpha) + pal[label].astype(np.float64) * alpha) / 256.0 + 0.5)
            if not tint:
                blend[label == 0] = image[label == 0]
            assert np.array_equal(R.paint_ref(label, pal, image, alpha, tint), blend.astype(np.uint8)), (alpha, tint)
            got = R.paint_ref(label, pal, image, alpha, tint, contour=True, contour_rgb=(1, 2, 3))
            m = np.zeros((H, W), dtype=bool)
            for y in range(H):
                for x in range(W):
                    m[y, x] = (x + 1 < W and label[y, x] != label[y, x + 1]) or (y + 1 < H and label[y, x] != label[y + 1, x])
            assert np.array_equal(got[m], np.broadcast_to(np.array([1, 2, 3], dtype=np.uint8), got[m].shape))
            assert np.array_equal(got[~m], blend.astype(np.uint8)[~m])
    assert np.array_equal(R.paint_ref(label, pal, image, 0, True), image) and np.array_equal(R.paint_ref(label, pal, image, 256, True), pal[label])


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decide_reference_against_the_ensemble_reference_and_torch(shape):
    import torch.nn.functional as F
    C, h, w, H, W = shape
    a, b, _, ref = ER.case(shape)
    win2, conf2, margin2 = R.decide_case(shape, True)
    assert np.array_equal(win2, ref["pred"]) and np.array_equal(conf2, ref["e"].max(0)) and np.array_equal(margin2, ref["margin"])
    win1, conf1, _ = R.decide_case(shape, False)
    up = F.interpolate(a.double(), size=(H, W), mode="bilinear", align_corners=False)[0]
    assert np.array_equal(win1, ref["pred1"]) and np.array_equal(win1, up.argmax(0).numpy())
    assert float((torch.from_numpy(conf1) - torch.softmax(up, 0).max(0).values).abs().max()) <= 1e-13
    assert conf1.min() >= 1.0 / C - 1e-12 and conf1.max() <= 1.0 and conf2.max() <= 1.0
    # probabilities: the values themselves, or their mean
    winp, confp, _ = R.decide64(ref["e"], None, H, W, is_prob=True)
    assert np.array_equal(winp, win2) and np.array_equal(confp, conf2)
    p1 = torch.softmax(up, 0).numpy()
    winm, confm, _ = R.decide64(p1, ref["e"], H, W, is_prob=True)
    assert np.array_equal(confm, (0.5 * (p1 + ref["e"])).max(0)) and np.array_equal(winm, (0.5 * (p1 + ref["e"])).argmax(0))
    # rejection and the statistics on a known case
    c32 = conf2.astype(np.float32)
    lab, rej = R.labels_of(win2, c32, 0.6, 255)
    assert np.array_equal(lab == 255, c32 < np.float32(0.6)) and np.array_equal(lab[~rej], win2[~rej].astype(np.uint8))
    st = R.stats_ref(win2, c32, rej, C)
    assert st[0].sum() == H * W and st[0, C] == int(rej.sum())
    assert st[1].sum() == int(np.rint(c32.astype(np.float64) * R.Q24).sum())       # the fp32 product is exact
    for c in np.unique(win2[~rej]):
        assert st[0, c] == int(((win2 == c) & ~rej).sum())
