"""dupl_seg_calib (csrc/seg_calib.hip) on the GPU, ops.seg_calibration and evaluate.CalibrationMatrix.  Every input lives in a
NaN-slack buffer, every counter in a sentinel-slack buffer (tests/kernel_guard.py).

  1. EXACT: bins, cls and sums[:, :2] equal the host binning (tests/calib_ref.py::host_counters) of ops.seg_decide on logits that
     ops.scale_ multiplied by ops.inv_temperature(T), per temperature, with no tolerance and no excluded pixel -- the definition is
     that composition.  Shapes: every path of the kernel (registers / sweeps either side of 24 channels, the staged footprint,
     taps through L1, cls privatised or not either side of T C = 1472, probabilities), one-pixel-wide grids, one lane past a tile,
     several tiles per workgroup; T in {1, 2, 16}, nbins in {1, 15, 64}; gt with 255, -1 and C.
  2. each output alone, accumulation, two runs bit-equal, an all-ignored gt; the packed 32-bit halves of the privatised cells on a
     1024 x 2048 image whose pixels all land in one bin and one class.
  3. AGAINST FLOAT64 (tests/calib_ref.py::reference, independent of seg_decide): with the pixels the reference itself calls
     ambiguous set aside (at most 0.5 %; tests/test_calibration_host.py asserts the actual shares) the pixel counters are exact, and
     mean NLL and mean Brier are within 5e-6 max(1, |ref|).  Worst measured on an MI355X: see test_against_float64's docstring.
  4. a planted temperature is found."""
import ctypes

import numpy as np
import pytest
import torch

import calib_ref as CR
import kernel_guard as KG

pytestmark = pytest.mark.gpu

T1, T2 = (1.0,), (1.0, 0.7)
T16 = (1.0,) + tuple(float(f"{0.4 * 12.5 ** (i / 14):.12g}") for i in range(15))
CLS_PRIV = 1472              # SC_CLS_CELLS of csrc/seg_calib.hip: 16 x 92 is privatised, 16 x 93 goes through global atomics
IDENT, BIG = (37, 53, 37, 53), (3, 28, 28, 600, 900)      # BIG: 2250 tiles on 2048 workgroups, every tile staged

EXACT = ([((21,) + IDENT, 1, T16, 15), ((21,) + IDENT, 2, T2, 64), ((21,) + IDENT, 1, T1, 1), ((21,) + IDENT, 2, T16, 15),
          ((24,) + IDENT, 1, T2, 15), ((24,) + IDENT, 2, T1, 1), ((25,) + IDENT, 1, T2, 15), ((25,) + IDENT, 2, T2, 64),
          ((81,) + IDENT, 1, T16, 15), ((81,) + IDENT, 2, T2, 64), ((1,) + IDENT, 1, T2, 15), ((1,) + IDENT, 2, T2, 15),
          ((92,) + IDENT, 1, T16, 15), ((93,) + IDENT, 1, T16, 15), ((93,) + IDENT, 2, T16, 64), ((255,) + IDENT, 1, T2, 15),
          ((3, 7, 9, 37, 53), 1, T16, 64), ((3, 7, 9, 37, 53), 2, T16, 15), (BIG, 1, T2, 15), (BIG, 2, T2, 15)] +
         [(s, n, T2, 15) for s in CR.RESIZED for n in (1, 2)] + [(s, n, T2, 15) for s in CR.EDGES for n in (1, 2)])
assert len(T16) == 16 and 16 * 92 == CLS_PRIV


def _id(c):
    s, n, temps, nbins = c
    return f"{s[0]}c-{s[1]}x{s[2]}-{s[3]}x{s[4]}-{n}s-T{len(temps)}-b{nbins}"


class Calib:
    """One raw dupl_seg_calib call on guarded buffers; outputs not in `want` are NULL, `into` adds to an earlier call's counters."""

    def __init__(self, ins, size, gt, dev, temps=T1, nbins=15, is_prob=False, want=("bins", "cls", "sums"), into=None, fill=0):
        from dupl_amd import _lib, ops
        C, h, w = ins[0].shape
        H, W = size
        T = len(temps)
        self.ins = [KG.nan_in(torch.from_numpy(t), dev) for t in ins]
        self.gt = torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
        self.shapes = dict(bins=(T, nbins, 3), cls=(T, C, 3), sums=(T, 4))
        for k, shp in self.shapes.items():
            setattr(self, k, getattr(into, k) if into is not None else
                    KG.Guard(shp, dev, torch.int64, init=torch.full(shp, fill, dtype=torch.int64)))
        inv = (ctypes.c_float * T)(*[ops.inv_temperature(t) for t in temps])
        d = _lib.SegCalibDesc(C=C, h=h, w=w, H=H, W=W, is_prob=int(is_prob), T=T, nbins=nbins, a=self.ins[0].data_ptr(),
                              b=self.ins[1].data_ptr() if len(self.ins) > 1 else None, gt=self.gt.data_ptr(),
                              inv_temp=ctypes.cast(inv, ctypes.c_void_p).value, **{k: getattr(self, k).ptr for k in want})
        self.status = _lib.lib().dupl_seg_calib.raw(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()

    def out(self, k):
        return getattr(self, k).cpu().numpy()


def composed(ins, size, gt, dev, temps, nbins, is_prob=False):
    """The counters by their definition: scale_ -> seg_decide -> read-back -> host binning, once per temperature."""
    from dupl_amd import ops
    C = ins[0].shape[0]
    bins, cls, sums = (np.zeros((len(temps), n, k), dtype=np.int64) for n, k in ((nbins, 3), (C, 3), (2, 1)))
    for t, temp in enumerate(temps):
        z = [torch.from_numpy(v).to(dev).clone() for v in ins]
        if not is_prob:
            z = [ops.scale_(v, ops.inv_temperature(temp)) for v in z]
        label, conf = ops.seg_decide(z[0], z[1] if len(z) > 1 else None, size, is_prob=is_prob)
        bins[t], cls[t], s = CR.host_counters(label.cpu().numpy(), conf.cpu().numpy(), gt, C, nbins)
        sums[t, :, 0] = s
    return bins, cls, sums[:, :, 0]


@pytest.fixture(scope="module")
def wanted(dev):
    """the composed counters, once per case, shared and left unchanged"""
    cache = {}

    def get(case, is_prob=False):
        key = (case, is_prob)
        if key not in cache:
            s, n, temps, nbins = case
            a, b, gt = CR.case_inputs(s, n, is_prob)
            ins = [a] if b is None else [a, b]
            cache[key] = (ins, gt, composed(ins, s[3:], gt, dev, temps, nbins, is_prob))
        return cache[key]
    return get


def _check(got, want, where):
    bins, cls, sums = want
    assert got.status == 0, where
    assert np.array_equal(got.out("bins"), bins), where
    assert np.array_equal(got.out("cls"), cls), where
    s = got.out("sums")
    assert np.array_equal(s[:, :2], sums), where
    assert (s[:, 2] >= 0).all() and (bins[:, :, 0].sum(1) == sums[:, 0]).all() and (cls[:, :, 1].sum(1) == sums[:, 1]).all(), where


@pytest.mark.parametrize("case", EXACT, ids=_id)
def test_counters_are_the_composition_exactly(dev, wanted, case):
    s, n, temps, nbins = case
    ins, gt, want = wanted(case)
    if s[3] * s[4] >= 1000:
        assert (gt == 255).any() and (gt == -1).any() and (gt == s[0]).any() and 0 < want[2][0, 0] < s[3] * s[4]
    _check(Calib(ins, s[3:], gt, dev, temps, nbins), want, _id(case))
    if len(temps) > 1 and s[0] > 1:
        assert not np.array_equal(want[0][0], want[0][1])                       # the temperatures do not answer the same question


@pytest.mark.parametrize("nbins", (1, 15, 64))
@pytest.mark.parametrize("n", (1, 2), ids=("one", "two"))
def test_probabilities_are_binned_as_they_are(dev, wanted, n, nbins):
    case = ((21,) + IDENT, n, T1, nbins)
    ins, gt, want = wanted(case, True)
    _check(Calib(ins, IDENT[2:], gt, dev, T1, nbins, is_prob=True), want, _id(case))


SUBSET = [((21,) + IDENT, 2, T2, 15), ((81, 7, 9, 37, 53), 2, T2, 15), ((93,) + IDENT, 1, T16, 15), ((21, 40, 40, 17, 23), 1, T2, 15)]


@pytest.mark.parametrize("case", SUBSET, ids=_id)
def test_outputs_alone_accumulation_reproducibility_and_an_ignored_gt(dev, wanted, case):
    s, n, temps, nbins = case
    ins, gt, want = wanted(case)
    full = Calib(ins, s[3:], gt, dev, temps, nbins)
    _check(full, want, _id(case))
    ref = {k: full.out(k).copy() for k in ("bins", "cls", "sums")}
    for k in ("bins", "cls", "sums"):                                           # each output alone: the bits of the full call, the others untouched
        alone = Calib(ins, s[3:], gt, dev, temps, nbins, want=(k,), fill=3)
        assert alone.status == 0 and np.array_equal(alone.out(k) - 3, ref[k]), k
        assert all((alone.out(o) == 3).all() for o in ref if o != k), k
    again = Calib(ins, s[3:], gt, dev, temps, nbins, into=full)                 # ADDED to: a second call doubles every counter
    assert again.status == 0 and all(np.array_equal(full.out(k), 2 * ref[k]) for k in ref)
    second = Calib(ins, s[3:], gt, dev, temps, nbins)                           # two runs: bit-equal, the fixed-point sums included
    assert all(np.array_equal(second.out(k), ref[k]) for k in ref)
    for ignored in (255, -1, s[0]):
        none = Calib(ins, s[3:], np.full_like(gt, ignored), dev, temps, nbins, fill=7)
        assert none.status == 0 and all((none.out(k) == 7).all() for k in ref), ignored


def test_refused_descriptors_touch_nothing(dev, wanted):
    from dupl_amd import _lib, ops
    case = SUBSET[0]
    s, n, temps, nbins = case
    ins, gt, _ = wanted(case)
    good = Calib(ins, s[3:], gt, dev, temps, nbins, fill=5)
    assert good.status == 0 and not (good.out("sums") == 5).all()
    for over in (dict(T=0), dict(T=17), dict(nbins=0), dict(nbins=65), dict(struct_size=8), dict(is_prob=1), dict(C=0), dict(gt=None)):
        out = {k: KG.Guard(shp, dev, torch.int64) for k, shp in good.shapes.items()}
        inv = (ctypes.c_float * 32)(*([1.0] * 32))
        d = _lib.SegCalibDesc(C=s[0], h=s[1], w=s[2], H=s[3], W=s[4], T=2, nbins=nbins, a=good.ins[0].data_ptr(), b=good.ins[1].data_ptr(),
                              gt=good.gt.data_ptr(), inv_temp=ctypes.cast(inv, ctypes.c_void_p).value, **{k: g.ptr for k, g in out.items()})
        for k, v in over.items():
            setattr(d, k, v)
        assert _lib.lib().dupl_seg_calib.raw(ctypes.byref(d), ops._stream()) == -1, over
        torch.cuda.synchronize()
        assert all(g.untouched() for g in out.values()), over


def test_packed_halves_of_the_privatised_cells_do_not_wrap(dev):
    """1024 x 2048 pixels of constant logits: every pixel of a temperature lands in one bin and one class, 8192 tiles on 2048
    workgroups.  The privatised cells count pixels and correct pixels in the 32-bit halves of one 64-bit word."""
    from dupl_amd import ops
    H, W, C, nbins = 1024, 2048, 3, 15
    px = torch.tensor([1.5, -0.25, -2.0])
    a = px.view(3, 1, 1).expand(3, H, W).contiguous().to(dev)
    gt = torch.zeros((H, W), dtype=torch.int64, device=dev)
    bins, cls, sums = ops.seg_calibration(a, gt=gt, temperatures=T2, nbins=nbins)
    N = H * W
    for t, temp in enumerate(T2):
        small = ops.scale_(px.view(3, 1, 1).expand(3, 4, 64).contiguous().to(dev), ops.inv_temperature(temp))
        label, conf = ops.seg_decide(small)
        assert bool((label == 0).all()) and bool((conf == conf[0, 0]).all())
        c = conf[0, 0].cpu().numpy()
        k = int(CR.bin_conf32(c.reshape(1), nbins)[0])
        q = int(np.rint(c * np.float32(16777216.0)))
        want_b, want_c = np.zeros((nbins, 3), dtype=np.int64), np.zeros((C, 3), dtype=np.int64)
        want_b[k], want_c[0] = (N, N, N * q), (N, N, N * q)
        assert np.array_equal(bins[t].cpu().numpy(), want_b) and np.array_equal(cls[t].cpu().numpy(), want_c)
        assert sums[t, :2].tolist() == [N, N]
    # and with every pixel wrong: the correct half stays 0
    _, cls2, sums2 = ops.seg_calibration(a, gt=gt + 2, temperatures=T1, nbins=nbins)
    assert cls2[0, 0].tolist()[:2] == [N, 0] and sums2[0, :2].tolist() == [N, 0]


def test_ops_wrapper_checks_its_arguments(dev):
    from dupl_amd import ops
    a = torch.zeros((1, 5, 6, 7), device=dev)
    gt = torch.zeros((12, 14), dtype=torch.int64, device=dev)
    bins, cls, sums = ops.seg_calibration(a, None, (12, 14), gt=gt, temperatures=(1.0, 2.0), nbins=4)
    assert bins.shape == (2, 4, 3) and cls.shape == (2, 5, 3) and sums.shape == (2, 4) and sums[:, 0].tolist() == [168, 168]
    assert bins[0, 0].tolist()[:2] == [168, 168] and cls[1, 0, 0].item() == 168                      # 5 equal logits: conf 0.2, class 0
    only = torch.zeros((2, 4), dtype=torch.int64, device=dev)
    assert ops.seg_calibration(a, None, (12, 14), gt=gt, temperatures=(1.0, 2.0), sums=only) == (None, None, only)
    for kw in (dict(temperatures=()), dict(temperatures=(1.0,) * 17), dict(nbins=0), dict(nbins=65), dict(temperatures=(0.0,)),
               dict(is_prob=True), dict(temperatures=(2.0,), is_prob=True, size=None)):
        with pytest.raises(ValueError):
            ops.seg_calibration(a, None, kw.pop("size", (12, 14)), gt=gt, **kw)
    with pytest.raises(ValueError):
        ops.seg_calibration(torch.zeros((256, 2, 2), device=dev), gt=gt[:2, :2].contiguous())


F64 = [(s, n, p, nbins) for (s, n, p) in CR.F64_CASES for nbins in (15, 64)]
WORST = {"nll": 0.0, "brier": 0.0, "conf": 0.0, "aside": 0.0}


@pytest.mark.parametrize("case", F64, ids=lambda c: f"{c[0][0]}c-{c[0][1]}x{c[0][2]}-{c[0][3]}x{c[0][4]}-{c[1]}s-{'prob' if c[2] else 'logit'}-b{c[3]}")
def test_against_float64(dev, case):
    """Bars: the pixel counters exact once the reference's own ambiguous pixels (<= 0.5 % of the case) are set aside; mean NLL and
    mean Brier within 5e-6 max(1, |ref|) of float64 (the partition sum is good to ~1e-7 relative, so is its log; the fixed-point
    rounding adds at most 2^-21 per pixel; the bar is about four times their sum); mean confidence within calib_ref.EPS.
    Worst measured on an MI355X over these 36 cases: mean NLL 4.9e-8, mean Brier 5.6e-9, mean confidence 7.3e-9 off float64 (a
    hundredth of the bar: the per-pixel errors are rounding noise of either sign and average out over 2 000 - 9 000 pixels);
    0.31 % of the pixels set aside at most."""
    shape, n, is_prob, nbins = case
    a, b, gt, ref, share = CR.f64_case(shape, n, is_prob, nbins)
    assert share <= CR.AMBIGUOUS_CAP
    temps = T1 if is_prob else CR.F64_TEMPS
    got = Calib([a] if b is None else [a, b], shape[3:], gt, dev, temps, nbins, is_prob=is_prob)
    assert got.status == 0
    bins, cls, sums = got.out("bins"), got.out("cls"), got.out("sums")
    nvalid = ref["sums"][:, 0]
    mean = {"nll": (sums[:, 2] / float(1 << 20) / nvalid, ref["sums"][:, 2] / nvalid),
            "brier": (sums[:, 3] / float(1 << 24) / nvalid, ref["sums"][:, 3] / nvalid),
            "conf": (bins[:, :, 2].sum(1) / float(1 << 24) / nvalid, ref["bins"][:, :, 2].sum(1) / nvalid)}
    err = {k: float(np.max(np.abs(g - r) / (np.maximum(1.0, np.abs(r)) if k != "conf" else 1.0))) for k, (g, r) in mean.items()}
    for k, v in err.items():
        WORST[k] = max(WORST[k], v)
    WORST["aside"] = max(WORST["aside"], share)
    print(f"set aside {100 * share:.3f} %; mean NLL err {err['nll']:.2e}, mean Brier err {err['brier']:.2e}, mean conf err {err['conf']:.2e}; "
          f"worst so far: NLL {WORST['nll']:.2e} Brier {WORST['brier']:.2e} conf {WORST['conf']:.2e} aside {100 * WORST['aside']:.3f} %")
    assert np.array_equal(bins[:, :, :2], ref["bins"][:, :, :2].astype(np.int64))
    assert np.array_equal(cls[:, :, :2], ref["cls"][:, :, :2].astype(np.int64))
    assert np.array_equal(sums[:, :2], ref["sums"][:, :2].astype(np.int64))
    assert err["nll"] <= 5e-6 and err["brier"] <= 5e-6 and err["conf"] <= CR.EPS


@pytest.mark.parametrize("students", (1, 2), ids=("one", "two"))
def test_a_planted_temperature_is_found(dev, students):
    """21 classes on 96 x 128, z ~ N(0, 3^2), gt drawn from softmax(z / 2), the sweep 0.5:4:13 in ONE pass per image."""
    from dupl_amd.tools import eval_seg
    from dupl_amd.utils import evaluate
    temps = eval_seg.parse_temp_sweep("0.5:4:13")
    zs, gt = CR.planted(students)
    cm = evaluate.CalibrationMatrix(21, dev, temperatures=temps, nbins=15)
    cm.update(torch.from_numpy(gt).to(dev)[None], *[torch.from_numpy(z).to(dev)[None] for z in zs])
    sc, best = cm.scores(), cm.best_temperature()
    ref = CR.reference(zs[0], zs[1] if students == 2 else None, CR.PLANTED[1:], gt, temps, 15)
    ref_nll = ref["sums"][:, 2] / ref["sums"][:, 0]
    Tg, Tf, edge = CR.best_temperature(temps, ref_nll)
    print(f"{students} student(s): T_grid {best['T_grid']} T_fit {best['T_fit']:.4f} (float64 {Tf:.4f}); ECE {sc[0]['ece']:.4f} at T=1, "
          f"{sc[best['index']]['ece']:.4f} at T_grid; acc {sc[0]['acc']:.4f} conf {sc[0]['mean_conf']:.4f}")
    assert best["T_grid"] == Tg and best["at_edge"] is edge is False
    # the NLL bar of 5e-6 moves the vertex of a parabola whose neighbours lie ~2e-2 above it by well under 1e-3 of the 0.17 step in log T
    assert best["T_fit"] == pytest.approx(Tf, rel=1e-3)
    assert max(abs(s["nll"] - r) / max(1.0, r) for s, r in zip(sc, ref_nll)) <= 5e-6
    if students == 1:
        assert best["T_grid"] == 2.0 and 1.68 <= best["T_fit"] <= 2.38
        assert sc[0]["ece"] > 0.2 and sc[best["index"]]["ece"] < 0.05
    assert all(s["n"] == 96 * 128 for s in sc)
    # the curve a user sets --min_conf by: coverage falls with the threshold, and at the fitted temperature accuracy rises with it
    cov = [r["coverage"] for r in sc[best["index"]]["risk_coverage"]]
    assert cov[0] == 1.0 and all(b <= a for a, b in zip(cov, cov[1:]))
