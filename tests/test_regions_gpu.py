"""Connected regions on the GPU: dupl_seg_regions / dupl_seg_regions_clean (csrc/regions.hip), their ops.* wrappers and the two uses
in tools/predict, against tests/regions_ref.py.  Everything is integer: every comparison is exact equality.  The label sits in a
0xA5-slack uint8 buffer (tests/seg_render_ref.py's U8Guard; the 97 x 131 cases on an odd byte address), conf in a NaN-slack buffer,
every output in a sentinel-slack buffer (tests/kernel_guard.py).

  1. region, n_regions, table and stats equal the reference on every case x both connectivities; the slack is intact;
  2. two runs, and a run on another stream, are bit-identical;
  3. the cap: region and n_regions stay complete, the table rows below max_regions are the reference's, the rest is untouched;
  4. every subset of {table, stats, conf} (and a call without region) gives the bits of the full call for what it returns;
  5. on ops.seg_decide's label and conf, stats is seg_decide's stats;
  6. cleaning: label_out, changed and the second labelling equal the reference; label_out aliased onto label; the ValueError;
  7. bad arguments return -1 and write nothing;
  8. predict_image and the command line."""
import ctypes
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import kernel_guard as KG
import regions_ref as RR
import seg_ensemble_ref as ER
import seg_render_ref as R

pytestmark = pytest.mark.gpu

TABLE_PAT = KG.SENT[torch.int64][1]


@functools.lru_cache(maxsize=None)
def ref(case, conn, with_conf=True):
    """the reference of one case, computed once and shared; treat as read-only"""
    lab, conf = RR.case(*case)
    return RR.label_ref(lab, conn, case[2], conf if with_conf else None)


class Call:
    """One raw dupl_seg_regions call on guarded buffers; outputs not in `want` are NULL."""

    def __init__(self, case, conn, dev, want=("region", "n", "table", "stats"), with_conf=True, max_regions=None, lab=None, **over):
        from dupl_amd import _lib, ops
        (H, W), _, C = case
        lab_np, conf_np = RR.case(*case)
        lab_np = lab_np if lab is None else lab
        self.cap = min(65536, H * W) if max_regions is None else max_regions
        self.label = R.U8Guard((H, W), dev, init=np.array(lab_np), front=67 if (H, W) == RR.ODD_ADDRESS else 64)
        self.conf = KG.nan_in(torch.from_numpy(np.array(conf_np)), dev)
        self.region = KG.Guard((H, W), dev, torch.int32)
        self.n = KG.Guard((1,), dev, torch.int32)
        self.table = KG.Guard((max(self.cap, 1), 8), dev, torch.int64)
        self.stats = KG.Guard((2, C + 1), dev, torch.int64, init=torch.zeros((2, C + 1), dtype=torch.int64))
        kw = dict(H=H, W=W, C=C, connectivity=conn, ignore_index=RR.IGNORE, max_regions=self.cap, label=self.label.ptr,
                  conf=self.conf.data_ptr() if with_conf else None)
        for k in want:
            kw[{"n": "n_regions"}.get(k, k)] = getattr(self, k).ptr
        d = _lib.SegRegionsDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        d.max_regions = max(self.cap, 0)                                    # the size query refuses a bad descriptor too
        nbytes = _lib.lib().dupl_seg_regions_workspace(ctypes.byref(d))
        assert nbytes > 0
        self.ws = torch.empty((nbytes // 8 + 1,), device=dev, dtype=torch.int64)
        d.workspace, d.workspace_bytes, d.max_regions = self.ws.data_ptr(), self.ws.numel() * 8, self.cap
        for k, v in over.items():
            setattr(d, k, v)
        self.status = _lib.lib().dupl_seg_regions.raw(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()

    def outputs_untouched(self):
        return all(getattr(self, k).untouched() for k in ("region", "n", "table")) and not bool(self.stats.cpu().any())

    def check(self, want, rows=None):
        """region, n, the table rows below the cap and stats against the reference tuple; the other rows untouched; slack intact"""
        region, n, table, stats = want
        assert self.status == 0 and self.label.intact()
        assert int(self.n.cpu()[0]) == n
        assert np.array_equal(self.region.cpu().numpy(), region.astype(np.int32))
        got = self.table.cpu().numpy()
        k = min(n, self.cap) if rows is None else rows
        assert np.array_equal(got[:k], table[:k])
        assert bool((got[k:] == TABLE_PAT).all())
        assert np.array_equal(self.stats.cpu().numpy(), stats)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("case", RR.CASES, ids=RR.case_id)
def test_regions_table_and_stats_are_the_reference(dev, case, conn):
    r = Call(case, conn, dev)
    want = ref(case, conn)
    r.check(want)
    print(f"{RR.case_id(case)} / {conn}: {want[1]} regions, table rows {min(want[1], r.cap)}")


REPEAT = [c for c in RR.CASES if c[0] in ((97, 131), (375, 500)) and c[1] in ("random3", "checker", "blobs", "serpentine")]


@pytest.mark.parametrize("case", REPEAT, ids=RR.case_id)
def test_runs_are_bit_identical_on_any_stream(dev, case):
    for conn in (4, 8):
        a, b = Call(case, conn, dev), Call(case, conn, dev)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            c = Call(case, conn, dev)
        for o in (b, c):
            assert o.status == 0
            for k in ("region", "n", "stats"):
                assert torch.equal(getattr(o, k).cpu(), getattr(a, k).cpu()), k
            rows = min(int(a.n.cpu()[0]), a.cap)
            assert torch.equal(o.table.cpu()[:rows], a.table.cpu()[:rows])


CAPPED = [((s, p, RR.CLASSES[p]), conn) for s in ((33, 65), (97, 131)) for p, conn in (("checker", 4), ("random3", 4), ("random3", 8))]


@pytest.mark.parametrize("case,conn", CAPPED, ids=lambda v: RR.case_id(v) if isinstance(v, tuple) else str(v))
def test_the_cap_limits_the_table_only(dev, case, conn):
    want = ref(case, conn)
    n = want[1]
    assert n > 8
    for cap in (1, 7, n - 1):
        r = Call(case, conn, dev, max_regions=cap)
        r.check(want, rows=cap)


SUBSET_CASES = [((97, 131), "blobs", 21), ((33, 65), "random21_ignore", 21)]


@pytest.mark.parametrize("case", SUBSET_CASES, ids=RR.case_id)
def test_every_subset_of_the_optional_parts(dev, case):
    for conn in (4, 8):
        full = ref(case, conn)
        bare = ref(case, conn, False)
        assert not bare[2][:, 6].any() and not bare[3][1].any() and np.array_equal(bare[2][:, :6], full[2][:, :6])
        for table, stats, conf in itertools.product((False, True), repeat=3):
            want = ("region", "n") + (("table",) if table else ()) + (("stats",) if stats else ())
            r = Call(case, conn, dev, want=want, with_conf=conf)
            exp = full if conf else bare
            r.check((exp[0], exp[1], exp[2], exp[3] if stats else np.zeros_like(exp[3])), rows=None if table else 0)
        # without the region map: n, table and stats alone; and n alone
        r = Call(case, conn, dev, want=("n", "table", "stats"))
        assert r.status == 0 and r.region.untouched() and int(r.n.cpu()[0]) == full[1]
        assert np.array_equal(r.table.cpu().numpy()[:full[1]], full[2]) and np.array_equal(r.stats.cpu().numpy(), full[3])
        r = Call(case, conn, dev, want=("n",))
        assert r.status == 0 and r.region.untouched() and r.table.untouched() and int(r.n.cpu()[0]) == full[1]


@pytest.mark.parametrize("shape", (ER.SHAPES[1], ER.SHAPES[3]), ids=lambda s: "x".join(map(str, s)))
def test_stats_are_seg_decides_stats(dev, shape):
    from dupl_amd import ops
    C, h, w, H, W = shape
    a, b, _, _ = ER.case(shape)
    st = torch.zeros((2, C + 1), device=dev, dtype=torch.int64)
    median = float(ops.seg_decide(a.to(dev), b.to(dev), (H, W), want_label=False)[1].median())      # about half the pixels rejected
    label, conf = ops.seg_decide(a.to(dev), b.to(dev), (H, W), min_conf=median, stats=st)
    rejected = int(st[0, C])
    assert 0 < rejected < H * W
    for conn in (4, 8):
        mine = torch.zeros_like(st)
        region, n, table = ops.seg_regions(label, conf, connectivity=conn, stats=mine)
        assert torch.equal(mine, st)
        assert int(table[:, 1].sum()) == H * W - rejected and n == table.shape[0]
        want = RR.label_ref(label.cpu().numpy(), conn, C, conf.cpu().numpy())
        assert n == want[1] and np.array_equal(region.cpu().numpy(), want[0]) and np.array_equal(table.cpu().numpy(), want[2])
        # num_classes alone, and the default of 256 classes: the same regions (no label reaches C)
        for kw in (dict(num_classes=C), dict()):
            r2, n2, t2 = ops.seg_regions(label, connectivity=conn, **kw)
            assert n2 == n and torch.equal(r2, region) and torch.equal(t2[:, :6], table[:, :6]) and not bool(t2[:, 6].any())
    for kw in (dict(connectivity=5), dict(ignore_index=256), dict(max_regions=0), dict(num_classes=0), dict(num_classes=C + 1, stats=st)):
        with pytest.raises(ValueError):
            ops.seg_regions(label, **kw)


CLEAN_CASES = [((97, 131), "blobs", 21), ((375, 500), "blobs", 21), ((97, 131), "random21_ignore", 21), ((375, 500), "random21_ignore", 21)]


def _clean_raw(lab_np, C, conn, min_area, dev, alias):
    """one raw dupl_seg_regions_clean call after ops' labelling; label_out is the label buffer itself when alias"""
    from dupl_amd import _lib, ops
    H, W = lab_np.shape
    label = R.U8Guard((H, W), dev, init=lab_np, front=67)
    out = label if alias else R.U8Guard((H, W), dev, front=65)
    region, n_dev, table = ops._seg_regions(label.view, None, conn, RR.IGNORE, H * W, None, C)
    changed = KG.Guard((2,), dev, torch.int64)
    d = _lib.SegRegionsCleanDesc(H=H, W=W, C=C, max_regions=table.shape[0], min_area=min_area, label=label.ptr, region=region.data_ptr(),
                                 n_regions=n_dev.data_ptr(), table=table.data_ptr(), label_out=out.ptr, changed=changed.ptr)
    ws = torch.empty((_lib.lib().dupl_seg_regions_clean_workspace(ctypes.byref(d)) // 8 + 1,), device=dev, dtype=torch.int64)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    status = _lib.lib().dupl_seg_regions_clean.raw(ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    return status, out, changed


@pytest.mark.parametrize("case", CLEAN_CASES, ids=RR.case_id)
def test_cleaning_is_the_reference(dev, case):
    from dupl_amd import ops
    (H, W), _, C = case
    lab_np, conf_np = RR.case(*case)
    label = R.U8Guard((H, W), dev, init=lab_np, front=67).view
    conf = torch.from_numpy(conf_np).to(dev)
    for conn in (4, 8):
        for min_area in (1, 2, 16, 400):
            want_lab, want_changed = RR.clean_ref(lab_np, min_area, conn, C)
            stats = torch.zeros((2, C + 1), device=dev, dtype=torch.int64)
            out, region, n, table, changed = ops.seg_regions_clean(label, min_area=min_area, connectivity=conn, max_regions=H * W,
                                                                   conf=conf, stats=stats)
            assert np.array_equal(out.cpu().numpy(), want_lab) and np.array_equal(changed.cpu().numpy(), want_changed)
            assert np.array_equal(label.cpu().numpy(), lab_np)                       # the input is not written
            second = RR.label_ref(want_lab, conn, C, conf_np)
            assert n == second[1] and np.array_equal(region.cpu().numpy(), second[0]) and np.array_equal(table.cpu().numpy(), second[2])
            assert np.array_equal(stats.cpu().numpy(), second[3])
            if min_area == 1:
                assert np.array_equal(want_lab, lab_np) and not want_changed.any()
            elif case[1] == "blobs" or min_area == 2:                               # (i.i.d. labels have no region of 16 pixels to vote)
                assert want_changed[0] > 0
            print(f"{RR.case_id(case)} / {conn} min_area {min_area}: {want_changed[0]} regions, {want_changed[1]} pixels relabelled; {n} regions left")
            if H * W < 20000 or min_area == 16:
                for alias in (False, True):
                    status, raw, ch = _clean_raw(lab_np, C, conn, min_area, dev, alias)
                    assert status == 0 and np.array_equal(raw.cpu().numpy(), want_lab) and np.array_equal(ch.cpu().numpy(), want_changed)


def test_cleaning_refuses_more_regions_than_max_regions(dev):
    from dupl_amd import ops
    case = ((97, 131), "random21_ignore", 21)
    lab_np, _ = RR.case(*case)
    label = torch.from_numpy(lab_np.copy()).to(dev)
    n = ref(case, 8)[1]
    with pytest.raises(ValueError, match=rf"{n} regions.*max_regions = {n - 1}"):
        ops.seg_regions_clean(label, min_area=4, max_regions=n - 1)
    assert ops.seg_regions_clean(label, min_area=4, max_regions=n)[2] < n
    with pytest.raises(ValueError):
        ops.seg_regions_clean(label, min_area=-1)
    # at the C level the small regions beyond the table stay, and the kept / small decision is exact for every region
    H, W = lab_np.shape
    cap = n // 2
    from dupl_amd import _lib
    region, n_dev, table = ops._seg_regions(label, None, 8, RR.IGNORE, cap, None, 21)
    out = R.U8Guard((H, W), dev, front=65)
    changed = KG.Guard((2,), dev, torch.int64)
    d = _lib.SegRegionsCleanDesc(H=H, W=W, C=21, max_regions=cap, min_area=4, label=label.data_ptr(), region=region.data_ptr(),
                                 n_regions=n_dev.data_ptr(), table=table.data_ptr(), label_out=out.ptr, changed=changed.ptr)
    ws = torch.empty((_lib.lib().dupl_seg_regions_clean_workspace(ctypes.byref(d)) // 8 + 1,), device=dev, dtype=torch.int64)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    assert _lib.lib().dupl_seg_regions_clean.raw(ctypes.byref(d), ops._stream()) == 0
    want_lab, want_changed = RR.clean_ref(lab_np, 4, 8, 21, max_regions=cap)
    assert np.array_equal(out.cpu().numpy(), want_lab) and np.array_equal(changed.cpu().numpy(), want_changed)
    assert not np.array_equal(want_lab, RR.clean_ref(lab_np, 4, 8, 21)[0])


def test_bad_arguments_are_refused_and_write_nothing(dev):
    from dupl_amd import _lib
    case = ((33, 65), "random3", 3)
    size = ctypes.sizeof(_lib.SegRegionsDesc)
    for kw in (dict(connectivity=5), dict(H=0), dict(max_regions=0), dict(label=None), dict(struct_size=size - 8), dict(struct_size=size + 8),
               dict(struct_size=0), dict(W=-1), dict(C=0), dict(C=257), dict(ignore_index=256), dict(max_regions=-1), dict(reserved0=1),
               dict(workspace=None), dict(workspace_bytes=1024)):
        r = Call(case, 8, dev, **kw)
        assert r.status == -1 and r.outputs_untouched(), kw
    r = Call(case, 8, dev, want=())
    assert r.status == -1 and r.outputs_untouched()
    assert Call(case, 8, dev).status == 0
    # the cleaning entry point
    from dupl_amd import ops
    lab_np, _ = RR.case(*case)
    label = torch.from_numpy(lab_np.copy()).to(dev)
    region, n_dev, table = ops._seg_regions(label, None, 8, RR.IGNORE, 33 * 65, None, 3)
    csize = ctypes.sizeof(_lib.SegRegionsCleanDesc)
    for kw in (dict(struct_size=csize + 8), dict(H=0), dict(C=0), dict(max_regions=0), dict(min_area=-1), dict(label=None), dict(region=None),
               dict(n_regions=None), dict(table=None), dict(label_out=None), dict(changed=None), dict(workspace=None), dict(workspace_bytes=8)):
        out = R.U8Guard((33, 65), dev)
        changed = KG.Guard((2,), dev, torch.int64)
        d = _lib.SegRegionsCleanDesc(H=33, W=65, C=3, max_regions=table.shape[0], min_area=4, label=label.data_ptr(), region=region.data_ptr(),
                                     n_regions=n_dev.data_ptr(), table=table.data_ptr(), label_out=out.ptr, changed=changed.ptr)
        ws = torch.empty((_lib.lib().dupl_seg_regions_clean_workspace(ctypes.byref(d)) // 8 + 1,), device=dev, dtype=torch.int64)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        for k, v in kw.items():
            setattr(d, k, v)
        assert _lib.lib().dupl_seg_regions_clean.raw(ctypes.byref(d), ops._stream()) == -1, kw
        torch.cuda.synchronize()
        assert out.untouched() and changed.untouched(), kw


# ------------------------------------------------------------------------------------------------------------- the model level
@pytest.fixture(scope="module")
def tiny(dev):
    """the tiny seeded model of tests/test_predict_gpu.py, built the same way"""
    from dupl_amd.model.model_dupl import siamese_network
    from oracle import dupl_oracle as O
    pp = O.make_siamese_params(O.VIT_TINY, 21, seed=2)
    pp = {k: (v * 6.0 if ("classifier.weight" in k or k.endswith("decoder.conv8.weight")) else v) for k, v in pp.items()}
    model = siamese_network("tiny_test", num_classes=21, pretrained=False, aux_layer=-3)
    model.load_state_dict(pp, strict=True)
    model.to(dev)
    model.eval()
    return model


def _picture(H, W, seed):
    g = np.random.RandomState(seed)
    return np.ascontiguousarray(g.randint(0, 256, size=((H + 15) // 16, (W + 15) // 16, 3)).astype(np.uint8).repeat(16, 0).repeat(16, 1)[:H, :W])


def test_predict_image_cleans_and_lists_regions(dev, tiny):
    from dupl_amd.tools import predict
    # the first seeded picture whose plain prediction has a region under 32 pixels to absorb, under both connectivities, and
    # rejected pixels that must stay (the seeded model's maps are smooth: not every picture has such a region)
    for H, W, seed in ((75, 100, 12), (48, 64, 11), (75, 100, 5), (160, 208, 6), (160, 208, 7), (160, 208, 8)):
        image = _picture(H, W, seed)
        plain = predict.predict_image(tiny, image, scales=(1.0, 1.5), min_conf=0.3)
        lab0, conf = plain["label"].cpu().numpy(), plain["conf"].cpu().numpy()
        if all(RR.clean_ref(lab0, 32, conn, 21)[1][0] > 0 for conn in (4, 8)) and 0 < int(plain["stats"][0, 21]) < H * W:
            break
    else:
        pytest.fail("no candidate picture has a region under 32 pixels: the test would show nothing")
    print(f"picture {H}x{W} seed {seed}: {int(plain['stats'][0, 21])} pixels rejected")
    assert set(plain) == {"label", "conf", "overlay", "stats", "windows"}
    for conn in (8, 4):
        r = predict.predict_image(tiny, image, scales=(1.0, 1.5), min_conf=0.3, min_region=32, regions=True, connectivity=conn)
        assert set(r) == set(plain) | {"region", "n_regions", "region_table", "cleaned"}
        want_lab, want_changed = RR.clean_ref(lab0, 32, conn, 21)
        assert want_changed[0] > 0
        assert np.array_equal(r["label"].cpu().numpy(), want_lab) and np.array_equal(r["conf"].cpu().numpy(), conf)
        assert r["cleaned"] == {"regions": int(want_changed[0]), "pixels": int(want_changed[1])}
        region, n, table, stats = RR.label_ref(want_lab, conn, 21, conf)
        assert np.array_equal(r["stats"].numpy(), stats) and int(stats[0, 21]) == int(plain["stats"][0, 21])
        assert r["n_regions"] == n and np.array_equal(r["region"].cpu().numpy(), region) and np.array_equal(r["region_table"].numpy(), table[:4096])
        assert not torch.equal(r["overlay"], plain["overlay"])
    only = predict.predict_image(tiny, image, scales=(1.0, 1.5), min_conf=0.3, regions=True, max_regions=3)
    assert set(only) == set(plain) | {"region", "n_regions", "region_table"} and torch.equal(only["label"], plain["label"])
    region, n, table, _ = RR.label_ref(lab0, 8, 21, conf)
    assert only["n_regions"] == n > 3 and np.array_equal(only["region_table"].numpy(), table[:3]) and torch.equal(only["stats"], plain["stats"])
    cleaned = predict.predict_image(tiny, image, scales=(1.0, 1.5), min_conf=0.3, min_region=32)
    assert set(cleaned) == set(plain) | {"cleaned"}


def test_predict_command_line_with_regions(dev, tiny, tmp_path):
    from PIL import Image
    from dupl_amd.tools import predict
    imgs = tmp_path / "photos"
    imgs.mkdir()
    sizes = {"a": (48, 64), "b": (75, 100)}
    for i, (nm, (H, W)) in enumerate(sizes.items()):
        Image.fromarray(_picture(H, W, 11 + i)).save(imgs / (nm + ".png"))
    ckpt = str(tmp_path / "checkpoint.pth")
    torch.save({k: v.detach().cpu() for k, v in tiny.state_dict().items()}, ckpt)
    common = ["--model_path", ckpt, "--backbone", "tiny_test", "--num_classes", "21", "--input", str(imgs), "--scales", "1.0,1.5"]
    predict.main(common + ["--out_dir", str(tmp_path / "o1"), "--min_region", "32", "--regions", "1"])
    summ = json.load(open(tmp_path / "o1" / "summary.json"))
    assert summ["min_region"] == 32 and set(summ["cleaned"]) == {"regions", "pixels"}
    assert summ["cleaned"]["pixels"] == sum(e["cleaned"]["pixels"] for e in summ["images"]) > 0
    names = predict.class_names("voc")
    for e in summ["images"]:
        H, W = sizes[e["image"][0]]
        lab = np.array(Image.open(tmp_path / "o1" / "labels" / (e["image"][0] + ".png")))
        region, n, table, _ = RR.label_ref(lab, 8, 21)
        assert e["min_region"] == 32 and e["regions_total"] == n and [g["id"] for g in e["regions"]] == list(range(min(n, 4096)))
        assert sum(c["pixels"] for c in e["classes"]) + e["rejected_pixels"] == H * W
        for c in e["classes"]:
            assert c["pixels"] == int((lab == c["id"]).sum())
        for g in e["regions"]:
            x0, y0, x1, y1 = g["box"]
            inside = int((region[y0:y1 + 1, x0:x1 + 1] == g["id"]).sum())
            assert inside == g["pixels"] == int((region == g["id"]).sum()) and g["class"] == int(lab[region == g["id"]][0])
            assert g["name"] == names[g["class"]] and 0.0 < g["mean_conf"] <= 1.0
        assert min(g["pixels"] for g in e["regions"]) >= 1
    predict.main(common + ["--out_dir", str(tmp_path / "o2")])
    plain = json.load(open(tmp_path / "o2" / "summary.json"))
    new = {"min_region", "cleaned", "regions", "regions_total"}
    assert not new & set(plain) and all(not new & set(e) for e in plain["images"])
    assert set(summ) - set(plain) == {"min_region", "cleaned"} and set(summ["images"][0]) - set(plain["images"][0]) == new
    big = predict.main(common + ["--out_dir", str(tmp_path / "o3"), "--regions", "1", "--region_min_pixels", "50", "--max_regions", "5",
                                 "--connectivity", "4"])
    for e in big:
        assert len(e["regions"]) <= 5 and all(g["pixels"] >= 50 for g in e["regions"]) and "cleaned" not in e
        lab = np.array(Image.open(tmp_path / "o3" / "labels" / (e["image"][0] + ".png")))
        assert e["regions_total"] == RR.label_ref(lab, 4, 21)[1]
