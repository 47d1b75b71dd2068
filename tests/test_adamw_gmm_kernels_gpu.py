"""csrc/optim.hip (the four instantiations of adamw_kernel) and csrc/gmm.hip (the label-noise filter) at their edges.

AdamW: bit-exact against tests/optim_ref.py, the operation-by-operation fp32 emulation of adamw_one that tests/test_par_ref_host.py
checks (its fused multiply-adds round once), for planes on / off x grad_scale 1 / 0.125 / 1/3 -- first update, 0 / eps, |g| from
1e-6 to 1e3, one inf and one NaN gradient that must stay inside their own element of a float4 -- with sentinels past n in every
buffer, the second trip of the capped grid's stride loop, and the launcher's refusals.  A NaN matches any NaN (the payload of a
generated NaN is the processor's choice); everything else is compared bit for bit.  No case has a subnormal intermediate
(optim_ref refuses them): flush-versus-gradual underflow is out of scope.

GMM filter: the checks of test_kernels_gpu.test_gmm_noise_filter_vs_sklearn (seeds equal, EM iteration count equal, parameters to
its tolerances, labels up to the same mismatch cap, against sklearn called as the reference calls it) at HW < 1024, HW not a
multiple of 64, n < 1024, the min_count boundary, images with nothing selected, CE == min_ce exactly, both seedings (the 1.0.2
rejection loop at n just above a power of two) and both ignore values, in ONE launch of a mixed batch so that images leaving at
different exits share it.  Out of scope: degenerate data (all selected values identical, zero variance), which is a warning path of
sklearn's own; and a single selected value (min_count = 0, n = 1), which sklearn refuses (fewer samples than components) -- there
only the count, the fact that a fit ran and the kind of relabelling are checked."""
import warnings

import numpy as np
import pytest
import torch

import optim_ref as R
from kernel_guard import Guard, same_bits, stream

pytestmark = pytest.mark.gpu
ERR_ARG = -1


# =========================================================================================== AdamW
class _Seg:
    """p, g, m, v inside sentinel-guarded buffers (16-byte aligned, more than 8 floats of slack) and, optionally, the two fp16
    planes with 8 halves of slack each, padded as in test_adamw_writes_the_operand_planes_of_the_next_forward"""

    def __init__(self, dev, p, g, m, v, planes):
        self.n = p.size
        self.bufs = [Guard((self.n,), dev, init=torch.from_numpy(np.ascontiguousarray(t))) for t in (p, g, m, v)]
        assert all(b.ptr % 16 == 0 for b in self.bufs)
        self.planes = None
        if planes:
            self.row = (self.n + 3) // 4 * 4 + 8
            self.planes = torch.full((2, self.row), 7.0, device=dev, dtype=torch.float16)
            assert self.planes.data_ptr() % 8 == 0 and (2 * self.row) % 8 == 0

    def plane_ptrs(self):
        return (self.planes.data_ptr(), self.planes.data_ptr() + 2 * self.row) if self.planes is not None else (None, None)

    def step(self, step, scale, plane_exp):
        from dupl_amd.utils.optimizer import adamw_segment
        hi, lo = self.plane_ptrs()
        adamw_segment(*(b.view for b in self.bufs), step, R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"], R.HYPER["wd"],
                      planes=(hi, lo, plane_exp) if self.planes is not None else None, grad_scale=scale)
        return self.result()

    def result(self):
        out = [b.cpu().numpy() for b in self.bufs]                                     # Guard.cpu asserts the sentinels
        if self.planes is not None:
            assert bool((self.planes[:, self.n:] == 7.0).all()), "a plane was written past n"
        return out


def _check_case(dev, p, g, m, v, step, plane_exp):
    for scale in R.ADAMW_SCALES:
        ref = R.adamw_ref(p, g, m, v, step, grad_scale=scale, **R.HYPER)
        gs = (torch.from_numpy(g) * torch.tensor(scale, dtype=torch.float32)).numpy() if scale != 1.0 else g   # one rounding, torch's
        keep = None
        for planes in (False, True):
            seg = _Seg(dev, p, g, m, v, planes)
            p2, g2, m2, v2 = seg.step(step, scale, plane_exp)
            for name, got, want in (("p", p2, ref[0]), ("m", m2, ref[2]), ("v", v2, ref[3])):
                assert R.same_bits_or_both_nan(got, want), f"{name}: planes {planes} scale {scale}: differs from the emulation"
            if scale == 1.0:
                assert same_bits(torch.from_numpy(g2), torch.from_numpy(g)), "the unscaled call must not write g"
            else:
                assert R.same_bits_or_both_nan(g2, gs), "g must leave as exactly g * grad_scale"
                # the unscaled instantiation fed g * scale: bit-equal p, m, v, and g untouched
                seg1 = _Seg(dev, p, gs, m, v, planes)
                p1, g1, m1, v1 = seg1.step(step, 1.0, plane_exp)
                assert same_bits(torch.from_numpy(g1), torch.from_numpy(gs))
                for a, b in ((p1, p2), (m1, m2), (v1, v2)):
                    assert R.same_bits_or_both_nan(a, b), f"scaled and unscaled instantiations differ (planes {planes}, scale {scale})"
                if planes:                   # (a NaN parameter's planes are NaN: compared where p is finite)
                    fin = torch.from_numpy(np.isfinite(p2)).to(dev)
                    assert torch.equal(seg1.planes[:, :seg.n][:, fin], seg.planes[:, :seg.n][:, fin])
            keep = (p2, m2, v2) if keep is None else keep
            for a, b in zip(keep, (p2, m2, v2)):
                assert R.same_bits_or_both_nan(a, b), "planes on and off differ"


@pytest.mark.parametrize("first", [True, False], ids=["first-step", "running"])
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_is_the_emulation_bit_for_bit(dev, n, first):
    """all four instantiations against optim_ref.adamw_ref, against one another, g written / untouched, sentinels intact; the tiny
    segments rotate the special gradients (0, 1e-6 .. 1e3, inf, NaN) through every element"""
    for shift in (range(len(R.G_SPECIALS)) if n <= 5 else (0,)):
        p, g, m, v, step = R.adamw_case(n, first, shift)
        _check_case(dev, p, g, m, v, step, plane_exp=9 if (n + shift) % 2 else 0)


@pytest.mark.parametrize("scale", R.ADAMW_SCALES)
def test_adamw_stride_loop(dev, scale):
    """n = 8192 * 1024 + 1024 + 3: the grid is capped at 8192 blocks, so the last 1024 + 3 elements are the second trip of the
    float4 loop and the scalar tail; one step, planes on and off, against the vectorised emulation"""
    p, g, m, v, step = R.adamw_case(R.ADAMW_STRIDE_N, False)
    ref = R.adamw_ref(p, g, m, v, step, grad_scale=scale, **R.HYPER)
    for planes in (False, True):
        seg = _Seg(dev, p, g, m, v, planes)
        p2, g2, m2, v2 = seg.step(step, scale, 9)
        for name, got, want in (("p", p2, ref[0]), ("g", g2, ref[1]), ("m", m2, ref[2]), ("v", v2, ref[3])):
            assert R.same_bits_or_both_nan(got, want), f"{name}: planes {planes}: differs from the emulation"


def test_adamw_refusals(dev):
    """each returns DUPL_ERR_ARG and leaves every buffer unchanged"""
    from dupl_amd import ops
    raw = ops.L().dupl_adamw.raw
    p, g, m, v, step = R.adamw_case(64, False)
    seg = _Seg(dev, p, g, m, v, True)
    P_, G_, M_, V_ = (b.ptr for b in seg.bufs)
    hi, lo = seg.plane_ptrs()
    h = R.HYPER
    bc1, bc2s = 1.0 - h["beta1"] ** step, float(np.sqrt(1.0 - h["beta2"] ** step))

    def call(p_=P_, n=64, gs=1.0, hi_=None, lo_=None, pe=0):
        return raw(p_, G_, M_, V_, n, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], bc1, bc2s, hi_, lo_, pe, gs, stream())

    assert call(n=0) == ERR_ARG
    for gs in (0.0, -1.0, float("nan")):
        assert call(gs=gs) == ERR_ARG, gs
    assert call(p_=P_ + 4, n=60) == ERR_ARG, "p offset by 4 bytes"
    assert call(hi_=hi) == ERR_ARG, "p_hi without p_lo"
    for pe in (-1, 16):
        assert call(hi_=hi, lo_=lo, pe=pe) == ERR_ARG, pe
    assert call(hi_=hi + 2, lo_=lo + 2, n=60) == ERR_ARG, "planes offset by 2 bytes"
    torch.cuda.synchronize()
    for b, t in zip(seg.bufs, (p, g, m, v)):
        assert same_bits(b.cpu(), torch.from_numpy(t))
    assert bool((seg.planes == 7.0).all())


# =========================================================================================== GMM filter
MIN_CE, VALID, GAMMA = 0.1, 1.0, 0.95


def _gmm_image(H, W, n_sel, kind, ignore, seed):
    """(ce, label) float32 (H, W) with EXACTLY n_sel selected pixels (foreground, not ignore, CE > min_ce).  The others are deselected
    four ways in turn: background; ignore (CE 0 there, as the loss leaves it); CE == min_ce exactly (the strict >); CE below."""
    rng = np.random.RandomState(seed)
    HW = H * W
    assert 0 <= n_sel <= HW
    if kind == "unimodal":
        ce = np.abs(rng.normal(0.8, 0.3, size=HW))
    else:
        ce = np.where(rng.rand(HW) < 0.3, rng.normal(3.2, 0.7, size=HW), np.abs(rng.normal(0.35, 0.15, size=HW)))
    ce = np.maximum(ce, 0.11).astype(np.float32)
    label = rng.randint(1, 21, size=HW).astype(np.float32)
    off = rng.permutation(HW)[n_sel:]
    label[off[0::4]] = 0.0
    label[off[1::4]] = float(ignore)
    ce[off[1::4]] = 0.0
    ce[off[2::4]] = np.float32(MIN_CE)
    ce[off[3::4]] = np.float32(MIN_CE) * np.float32(0.5)
    return ce.reshape(H, W), label.reshape(H, W)


def _nothing_selected(H, W, how, ignore, seed):
    ce, label = _gmm_image(H, W, H * W, "bimodal", ignore, seed)
    if how == "background":
        label[:] = 0.0
    elif how == "ignore":
        label[:] = float(ignore)
    else:
        ce[:] = np.where(np.arange(H * W).reshape(H, W) % 2 == 0, np.float32(MIN_CE), np.float32(0.03))
    return ce, label


def _run_and_check(dev, images, ignore, min_count, skver):
    """ONE launch over the batch; every image against sklearn driven as the reference drives it"""
    from sklearn.mixture import GaussianMixture
    from sklearn.cluster import kmeans_plusplus
    from oracle import dupl_oracle as O
    from dupl_amd.model import losses as LS
    ce = torch.from_numpy(np.stack([c for _, c, _ in images]))
    lab = torch.from_numpy(np.stack([l for _, _, l in images]))
    got = lab.clone().to(dev)
    stats = LS.gmm_noise_filter_(ce.to(dev), got, ignore, VALID, GAMMA, min_ce=MIN_CE, min_count=min_count, sklearn_version=skver)
    torch.cuda.synchronize()
    stats, got = stats.cpu().numpy(), got.cpu()
    rs_of = (lambda: O.sklearn_102_random_state(0)) if skver == "1.0.2" else (lambda: np.random.RandomState(0))
    ref_labels, exits = [], []
    for i, (name, c, l) in enumerate(images):
        sel = (l != 0) & (l != ignore) & (c > np.float32(MIN_CE))
        x = c[sel].reshape(-1, 1)
        n = x.shape[0]
        assert int(stats[i, 0]) == n, f"{name}: counted {int(stats[i, 0])} selected pixels, there are {n}"
        want = lab[i].clone()
        if n <= min_count:
            assert bool((stats[i, 1:] == 0).all()) and torch.equal(got[i], lab[i]), f"{name}: n = {n} <= min_count must not fit"
            exits.append("no fit")
            ref_labels.append(want)
            continue
        assert stats[i, 8] >= 1, f"{name}: n = {n} > min_count must fit"
        changed = got[i] != lab[i]
        assert bool((got[i][changed] == ignore).all()) and bool((lab[i][changed] != 0).all()), f"{name}: relabelling other than to ignore"
        if n < 2:                    # sklearn refuses fewer samples than components: no reference
            exits.append("fit, no reference")
            ref_labels.append(None)
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm = GaussianMixture(n_components=2, max_iter=10, tol=1e-2, reg_covar=5e-4, random_state=rs_of()).fit(x)
            _, idx = kmeans_plusplus(x - x.mean(axis=0), 2, random_state=rs_of())
        if skver == "1.0.2":         # the first seed IS numpy's randint(n)
            assert int(stats[i, 14]) == int(np.random.RandomState(0).randint(n)), name
        assert [int(stats[i, 14]), int(stats[i, 15])] == [int(idx[0]), int(idx[1])], f"{name}: k-means++ seeds"
        assert int(stats[i, 8]) == gm.n_iter_, f"{name}: EM iteration count"
        np.testing.assert_allclose(stats[i, 2:4], gm.means_[:, 0], rtol=1e-3, atol=1e-4, err_msg=name)
        np.testing.assert_allclose(stats[i, 4:6], gm.covariances_[:, 0, 0], rtol=2e-3, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(stats[i, 6:8], gm.weights_, rtol=1e-3, atol=1e-4, err_msg=name)
        gap = abs(gm.means_[0, 0] - gm.means_[1, 0])
        valid = gap > VALID
        if abs(gap - VALID) > 1e-2:
            assert (stats[i, 1] == 1) == valid, name
        if valid:
            prob = gm.predict_proba(c.reshape(-1, 1).astype(np.float64))
            noise = torch.from_numpy(prob[:, gm.means_.argmax()] > GAMMA).reshape(l.shape) & (lab[i] != 0)
            want[noise] = float(ignore)
        mism = int((got[i] != want).sum())
        print(f"{name}: n {n}, EM {gm.n_iter_} iterations, valid {bool(valid)}, relabelled {int(stats[i, 13])}, mismatching px {mism}")
        assert mism <= max(2, n // 20000), name
        exits.append("filtered" if valid else "fit, means too close")
        ref_labels.append(want)
    if min_count == 1000 and ignore == 255:          # the restatement above is the oracle's, image for image
        o = lab.clone()
        O.gmm_noise_filter_(ce, o, VALID, GAMMA, sklearn_version=skver)
        for i, w in enumerate(ref_labels):
            assert w is None or torch.equal(o[i], w), images[i][0]
    return exits


@pytest.mark.parametrize("ignore", [255, -1])
@pytest.mark.parametrize("skver", ["1.2+", "1.0.2"])
@pytest.mark.parametrize("min_count", [0, 1, 1000])
@pytest.mark.parametrize("H,W", [(33, 37), (1, 1500), (40, 25), (64, 64)])
def test_gmm_filter_edges_in_one_mixed_batch(dev, H, W, min_count, skver, ignore):
    pytest.importorskip("sklearn")
    HW = H * W
    s = 7 * H + W + min_count
    images = [(f"n = min_count = {min_count}",) + _gmm_image(H, W, min_count, "bimodal", ignore, s)]
    if min_count + 1 <= HW:
        images.append((f"n = min_count + 1 = {min_count + 1}",) + _gmm_image(H, W, min_count + 1, "bimodal", ignore, s + 1))
    images += [(f"nothing selected: all {how}",) + _nothing_selected(H, W, how, ignore, s + 2) for how in ("background", "ignore", "low CE")]
    images.append(("bimodal, 60 % selected",) + _gmm_image(H, W, (6 * HW) // 10, "bimodal", ignore, s + 3))
    images.append(("unimodal, half selected",) + _gmm_image(H, W, HW // 2, "unimodal", ignore, s + 4))
    images.append(("bimodal, 300 selected",) + _gmm_image(H, W, 300, "bimodal", ignore, s + 5))
    images.append(("bimodal, all selected",) + _gmm_image(H, W, HW, "bimodal", ignore, s + 6))
    exits = _run_and_check(dev, images, ignore, min_count, skver)
    print("exits:", exits)
    assert exits[0] == "no fit" and exits.count("no fit") >= 4
    if min_count < 300:
        assert "filtered" in exits and "fit, means too close" in exits, "the batch must leave at every exit"


@pytest.mark.parametrize("skver", ["1.0.2", "1.2+"])
def test_gmm_seeding_sweep_just_above_powers_of_two(dev, skver):
    """n in {1025, 2049, 4097} (mask 2^k+1 - 1: about half of the MT19937 words are rejected), 1537 and 3000, as images of one
    batch: stats[14] is numpy's RandomState(0).randint(n) itself for the 1.0.2 seeding, the second seed kmeans_plusplus's"""
    pytest.importorskip("sklearn")
    H, W = 60, 70
    images = [(f"n = {n}",) + _gmm_image(H, W, n, "bimodal", 255, 900 + n) for n in (1025, 2049, 4097, 1537, 3000)]
    exits = _run_and_check(dev, images, 255, 1000, skver)
    assert exits == ["filtered"] * 5
