"""Connected regions, the host side: the reference of tests/regions_ref.py against itself (scipy against a flood fill, the cleaning
pass on hand-built maps), the C ABI's declarations, the ctypes mirrors, tools/predict's flags and region_summary."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import regions_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in RR.CASES if c[0][0] * c[0][1] <= 97 * 131]


@pytest.mark.skipif(RR.ndimage is None, reason="scipy is not installed: the flood fill is the only reference")
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("case", SMALL, ids=RR.case_id)
def test_scipy_reference_is_the_flood_fill(case, connectivity):
    lab, conf = RR.case(*case)
    a = RR.label_ref(lab, connectivity, case[2], conf)
    b = RR.flood_ref(lab, connectivity, case[2], conf)
    assert a[1] == b[1]
    for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
        assert np.array_equal(x, y)
    region, n, table, stats = a
    H, W = case[0]
    assert int(table[:, 1].sum()) == int((region >= 0).sum()) == H * W - int(stats[0, case[2]])
    assert np.array_equal(table[:, 7], np.sort(table[:, 7])) and len(np.unique(table[:, 7])) == n


def test_patterns_have_the_regions_they_are_built_for():
    for shape in RR.SHAPES:
        H, W = shape
        count = lambda name, conn: RR.label_ref(RR.case(shape, name, RR.CLASSES[name])[0], conn, RR.CLASSES[name])[1]
        assert count("uniform", 4) == count("uniform", 8) == 1
        assert count("all_ignore", 8) == 0
        assert count("checker", 4) == H * W
        assert count("checker", 8) == (2 if min(H, W) > 1 else H * W)        # a one-pixel-wide map has no diagonals
        for conn in (4, 8):
            lab = RR.case(shape, "serpentine", 2)[0]
            region, _, table, _ = RR.label_ref(lab, conn, 2)
            assert len(np.unique(region[lab == 1])) == 1 and int(table[region[0, 0], 1]) == int((lab == 1).sum())
        lab = RR.case(shape, "diag", 2)[0]
        assert len(np.unique(RR.label_ref(lab, 8, 2)[0][lab == 1])) == 1
        assert len(np.unique(RR.label_ref(lab, 4, 2)[0][lab == 1])) == min(H, W)
        if H >= 33 and W >= 33:
            lab = RR.case(shape, "comb", 4)[0]
            for conn in (4, 8):
                region = RR.label_ref(lab, conn, 4)[0]
                assert len(np.unique(region[lab == 2])) == 1 and len(np.unique(region[lab == 3])) == 1
    assert RR.label_ref(RR.case((375, 500), "random3", 3)[0], 8, 3)[1] > 2000


def _clean(rows, min_area, conn=8, classes=4, **kw):
    lab = np.array(rows, np.uint8)
    out, changed = RR.clean_ref(lab, min_area, conn, classes, **kw)
    return lab, out, changed


def test_cleaning_reference_on_hand_built_maps():
    # a 3-pixel island inside one class is absorbed
    lab, out, ch = _clean([[1, 1, 1, 1, 1], [1, 2, 2, 2, 1], [1, 1, 1, 1, 1]], 4)
    assert np.array_equal(out, np.ones_like(lab)) and list(ch) == [1, 3]
    assert np.array_equal(_clean(lab, 3)[1], lab) and list(_clean(lab, 3)[2]) == [0, 0]
    assert np.array_equal(_clean(lab, 1)[1], lab)
    # majority: the island straddles the boundary and touches class 3 on four pixel pairs, class 1 on two
    lab, out, ch = _clean([[1, 1, 3, 3, 3, 3],
                           [1, 1, 2, 2, 3, 3],
                           [1, 1, 1, 3, 3, 3],
                           [1, 1, 1, 3, 3, 3]], 3)
    assert list(out[1]) == [1, 1, 3, 3, 3, 3] and list(ch) == [1, 2]
    # a tie goes to the lower class: three pairs each
    lab, out, ch = _clean([[1, 1, 3, 3], [1, 2, 2, 3], [1, 1, 3, 3]], 3)
    assert list(out[1]) == [1, 1, 1, 3] and list(ch) == [1, 2]
    # an island that touches only the image edge and ignored pixels stays
    lab, out, ch = _clean([[2, 2, 255, 1, 1], [255, 255, 255, 1, 1], [1, 1, 1, 1, 1]], 3)
    assert np.array_equal(out, lab) and list(ch) == [0, 0]
    # two adjacent small islands do not vote for each other: 2 has two pairs with 1 and one with 0, 3 has one with 1 and two with 0
    lab, out, ch = _clean([[1, 1, 1, 1, 1, 1],
                           [1, 1, 2, 3, 0, 0],
                           [0, 0, 0, 0, 0, 0],
                           [0, 0, 0, 0, 0, 0]], 2, conn=4)
    assert out[1, 2] == 1 and out[1, 3] == 0 and list(ch) == [2, 2]
    # ignored pixels never change, and small regions beyond max_regions stay
    lab, out, ch = _clean([[1, 2, 1, 1, 255, 1, 1, 2, 1]], 2)
    assert list(out[0]) == [1, 1, 1, 1, 255, 1, 1, 1, 1] and list(ch) == [2, 2]
    lab, out, ch = _clean([[1, 2, 1, 1, 255, 1, 1, 2, 1]], 2, max_regions=4)
    assert list(out[0]) == [1, 1, 1, 1, 255, 1, 1, 2, 1] and list(ch) == [1, 1]


def test_header_library_and_mirrors():
    from dupl_amd import _lib
    src = open(_lib.HEADER).read()
    protos = _lib.parse_header()
    assert "dupl_seg_regions" in protos and "dupl_seg_regions_clean" in protos
    assert protos["dupl_seg_regions"][0] is ctypes.POINTER(_lib.SegRegionsDesc)
    assert protos["dupl_seg_regions_clean"][0] is ctypes.POINTER(_lib.SegRegionsCleanDesc)
    for name in ("dupl_seg_regions_workspace", "dupl_seg_regions_clean_workspace"):
        assert re.search(r"int64_t\s+" + name + r"\s*\(", src)
    L = _lib.lib()
    assert L.dupl_abi_version() == 4
    for name in ("dupl_seg_regions", "dupl_seg_regions_clean", "dupl_seg_regions_workspace", "dupl_seg_regions_clean_workspace"):
        assert hasattr(L.cdll, name)
    assert f"#define DUPL_SEG_REGIONS_MAX_C {_lib.SEG_REGIONS_MAX_C}" in src and f"#define DUPL_SEG_REGIONS_COLS {_lib.SEG_REGIONS_COLS}" in src
    # the size queries run on the host: the formula of the header, and <= 0 on a bad descriptor
    d = _lib.SegRegionsDesc(H=375, W=500, C=21, connectivity=8, ignore_index=255, max_regions=7)
    up = lambda v: (v + 255) // 256 * 256
    assert L.dupl_seg_regions_workspace(ctypes.byref(d)) == 2 * up(4 * 187500) + up(4 * (184 + 1))
    d.connectivity = 5
    assert L.dupl_seg_regions_workspace(ctypes.byref(d)) <= 0
    c = _lib.SegRegionsCleanDesc(H=10, W=10, C=3, max_regions=7, min_area=4)
    assert L.dupl_seg_regions_clean_workspace(ctypes.byref(c)) == up(4 * (7 * 3 + 93)) + up(4 * 7)
    c.struct_size += 8
    assert L.dupl_seg_regions_clean_workspace(ctypes.byref(c)) <= 0


def test_ctypes_mirrors_have_the_headers_sizes(tmp_path):
    from dupl_amd import _lib
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dupl_hip.h"\nint main(void) {\n'
                    '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(dupl_seg_regions_desc), offsetof(dupl_seg_regions_desc, label),\n'
                    '         offsetof(dupl_seg_regions_desc, workspace_bytes), sizeof(dupl_seg_regions_clean_desc),\n'
                    '         offsetof(dupl_seg_regions_clean_desc, min_area), offsetof(dupl_seg_regions_clean_desc, workspace_bytes));\n'
                    '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(["which", c], capture_output=True).returncode == 0
               or os.path.exists(c)), None)
    assert cc is not None, "no C compiler"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R, K = _lib.SegRegionsDesc, _lib.SegRegionsCleanDesc
    assert got == [ctypes.sizeof(R), R.label.offset, R.workspace_bytes.offset, ctypes.sizeof(K), K.min_area.offset, K.workspace_bytes.offset]
    assert _lib.SegRegionsDesc().struct_size == ctypes.sizeof(R) and _lib.SegRegionsCleanDesc().struct_size == ctypes.sizeof(K)


def test_predict_parser_carries_the_region_flags():
    from dupl_amd.tools import predict
    base = ["--input", "x.png", "--out_dir", "out"]
    a = predict.parse_args(base)
    assert (a.min_region, a.regions, a.region_min_pixels, a.max_regions, a.connectivity) == (0, 0, 1, 4096, 8)
    assert not a.min_region and not a.regions                     # everything off without the flags
    a = predict.parse_args(base + ["--min_region", "32", "--regions", "1", "--region_min_pixels", "9", "--max_regions", "10", "--connectivity", "4"])
    assert (a.min_region, a.regions, a.region_min_pixels, a.max_regions, a.connectivity) == (32, 1, 9, 10, 4)
    for bad in (["--connectivity", "5"], ["--min_region", "-1"], ["--regions", "2"], ["--max_regions", "0"], ["--region_min_pixels", "0"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
    import inspect
    sig = inspect.signature(predict.predict_image).parameters
    assert [sig[k].default for k in ("min_region", "regions", "connectivity", "max_regions")] == [0, False, 8, 4096]


def test_region_summary_on_a_hand_written_table():
    from dupl_amd.tools import predict
    names = ["background", "aeroplane", "bicycle"]
    table = np.array([[0, 100, 0, 0, 9, 9, 50 << 24, 0],
                      [2, 4, 3, 5, 4, 6, 3 << 24, 35],
                      [7, 1, 9, 9, 9, 9, 1 << 23, 99]], np.int64)
    got = predict.region_summary(table, names, 1)
    assert got == [{"id": 0, "class": 0, "name": "background", "pixels": 100, "box": [0, 0, 9, 9], "mean_conf": 0.5},
                   {"id": 1, "class": 2, "name": "bicycle", "pixels": 4, "box": [5, 3, 6, 4], "mean_conf": 0.75},
                   {"id": 2, "class": 7, "name": "class7", "pixels": 1, "box": [9, 9, 9, 9], "mean_conf": 0.5}]
    assert [r["id"] for r in predict.region_summary(table, names, 4)] == [0, 1]
    assert predict.region_summary(np.zeros((0, 8), np.int64), names, 1) == []
