"""CPU checks of tests/input_ref.py, the yardstick of tests/test_input_kernels_gpu.py: (a) on every case of every list the plain
reference equals Pillow called the way the reference project calls it (ImageOps / ImageEnhance / convert / ImageFilter /
Image.resize + numpy flip, pad, crop + torch's ToTensor / Normalize arithmetic), bit for bit; (b) the case lists reach every branch
they are meant to reach, asserted from the references' own branch reports; (c) each classic mistake, swapped in for one primitive of
the reference, differs from Pillow on at least one case of the list the GPU suite runs."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

import input_ref as R
from oracle import dupl_oracle as O

ENH = {0: ImageEnhance.Color, 1: ImageEnhance.Contrast, 2: ImageEnhance.Brightness}


def _pil(img):
    return Image.fromarray(img)


def _np(pil):
    return np.asarray(pil)


def _small_images():
    for H, W, c in R.SMALL_PLANES:
        yield (H, W, c), R.plane(H, W, c)


def _enhance_images(mode):
    yield from _small_images()
    if mode == 1:
        for k in R.TIE_LUMAS:
            yield ("tie", k), R.tie_plane(k)
        yield R.CONTRAST_EXTRA_SHAPE, R.plane(*R.CONTRAST_EXTRA_SHAPE, "random")


# ============================================================================================== (a) + (b): LUT ops
def _lut_vs_pillow():
    """-> {mode: [(case, report)]}; asserts equality with Pillow on the way"""
    out = {0: [], 1: []}
    for mode, fn in ((0, ImageOps.autocontrast), (1, ImageOps.equalize)):
        cases = [((H, W, c), R.plane(H, W, c)) for H, W, c in R.LUT_PLANES] + [(R.TRIP_LUT, R.plane(*R.TRIP_LUT, "random"))]
        for name, img in cases:
            rep = set()
            assert np.array_equal(R.lut_op(img, mode, rep), _np(fn(_pil(img)))), (mode, name)
            out[mode].append((name, rep))
    return out


@pytest.fixture(scope="module")
def lut_reports():
    return _lut_vs_pillow()


def test_lut_ops_equal_pillow_and_reach_every_branch(lut_reports):
    auto, eq = lut_reports[0], lut_reports[1]
    assert any("hi==lo" in r for _, r in auto) and any("hi==lo" not in r for _, r in auto)
    for b in ("nnz<=1", "step==0", "lut_clip", "lut_clip_present"):
        hit = [n for n, r in eq if b in r]
        print(f"equalize {b}: {len(hit)} of {len(eq)} cases, e.g. {hit[:3]}")
        assert hit, b
    small = eq[:len(R.LUT_PLANES)]
    present = sum("lut_clip_present" in r for _, r in small)
    print(f"equalize: a LUT entry above 255 is used by a value of the plane in {present} of {len(small)} small-plane cases")
    assert 4 * present >= len(small)
    assert any(not r for _, r in eq), "no case takes the plain path (step > 0, nothing clipped)"


def test_equalize_lut_wrapped_to_8_bits_is_caught(monkeypatch):
    monkeypatch.setattr(R, "lut_fit", lambda t: t & 255)
    caught = [(H, W, c) for H, W, c in R.LUT_PLANES
              if not np.array_equal(R.lut_op(R.plane(H, W, c), 1), _np(ImageOps.equalize(_pil(R.plane(H, W, c)))))]
    print(f"wrapped LUT differs from Pillow on {len(caught)} small planes")
    assert caught


def test_posterize_equals_pillow():
    for bits in R.POSTERIZE_BITS:
        for name, img in _small_images():
            assert np.array_equal(R.posterize(img, bits), _np(ImageOps.posterize(_pil(img), bits))), (bits, name)
    x = np.random.RandomState(2).randint(0, 256, size=R.TRIP_N, dtype=np.uint8)
    pad = np.concatenate([x, np.zeros((-x.size) % 3, np.uint8)]).reshape(1, -1, 3)
    assert np.array_equal(R.posterize(pad, 5), _np(ImageOps.posterize(_pil(pad), 5)))


# ============================================================================================== (a) + (b): blends
def _enhance_reports():
    out = {}
    for mode in (0, 1, 2):
        for f in R.FACTORS:
            rep = set()
            for name, img in _enhance_images(mode):
                assert np.array_equal(R.enhance(img, mode, f, rep), _np(ENH[mode](_pil(img)).enhance(f))), (mode, f, name)
            out[(mode, f)] = rep
    for f in R.FACTORS:
        rep = set()
        for name, img in _small_images():
            assert np.array_equal(R.sharpness(img, f, rep), _np(ImageEnhance.Sharpness(_pil(img)).enhance(f))), (f, name)
        out[("sharp", f)] = rep
    return out


def test_enhance_and_sharpness_equal_pillow_and_clip_at_both_ends():
    reps = _enhance_reports()
    for op in (0, 1, 2, "sharp"):
        took = set().union(*(reps[(op, f)] for f in R.FACTORS if not 0.0 <= f <= 1.0))
        print(f"op {op}: factors outside [0, 1] took {sorted(took)}")
        assert {"blend_low", "blend_high"} <= took, op
        assert not any(reps[(op, f)] & {"blend_low", "blend_high"} for f in R.FACTORS if 0.0 <= f <= 1.0)
    sharp = set().union(*(reps[("sharp", f)] for f in R.FACTORS))
    assert "interior_empty" in sharp
    # the second trips' images
    for mode in (0, 1, 2):
        for shape in (R.TRIP_LUT, R.TRIP_PHOTO):
            if mode == 2 and shape == R.TRIP_LUT:
                continue
            img = R.plane(*shape, "random")
            assert np.array_equal(R.enhance(img, mode, 1.3), _np(ENH[mode](_pil(img)).enhance(1.3))), (mode, shape)
    img = R.plane(*R.TRIP_SHARP, "random")
    assert np.array_equal(R.sharpness(img, 1.3), _np(ImageEnhance.Sharpness(_pil(img)).enhance(1.3)))
    img = R.plane(*R.TRIP_PHOTO, "random")
    l = _np(_pil(img).convert("L"))
    assert np.array_equal(R.grayscale(img), np.dstack([l, l, l]))


def test_luma_and_contrast_mean_equal_pillow():
    from PIL import ImageStat
    ties = 0
    for name, img in _enhance_images(1):
        l = _pil(img).convert("L")
        assert np.array_equal(R.luma(img), _np(l)), name
        assert R.contrast_mean(img) == int(ImageStat.Stat(l).mean[0] + 0.5), name
        s = int(R.luma(img).sum(dtype=np.int64))
        ties += int(2 * s % (2 * img.shape[0] * img.shape[1]) == img.shape[0] * img.shape[1])
    assert ties >= len(R.TIE_LUMAS)
    assert R.contrast_mean(R.plane(1, 1, "full")) == 255 and R.contrast_mean(R.plane(129, 128, "full")) == 255


def _differs_somewhere(fn_ref, fn_pil, cases):
    return [name for name, img in cases if not np.array_equal(fn_ref(img), fn_pil(img))]


def test_blend_mistakes_are_caught(monkeypatch):
    cases = list(_small_images())
    with monkeypatch.context() as m:
        m.setattr(R, "blend_inside", lambda t: np.rint(t).astype(np.int32).astype(np.uint8))
        for mode in (0, 1, 2):
            assert _differs_somewhere(lambda i: R.enhance(i, mode, 0.7), lambda i: _np(ENH[mode](_pil(i)).enhance(0.7)), cases), mode
        assert _differs_somewhere(lambda i: R.sharpness(i, 0.7), lambda i: _np(ImageEnhance.Sharpness(_pil(i)).enhance(0.7)), cases)
    with monkeypatch.context() as m:
        m.setattr(R, "blend_outside", lambda t: t.astype(np.int32).astype(np.uint8))          # truncated and wrapped, not clipped
        for mode in (0, 1, 2):
            assert _differs_somewhere(lambda i: R.enhance(i, mode, 1.3), lambda i: _np(ENH[mode](_pil(i)).enhance(1.3)), cases), mode
        assert _differs_somewhere(lambda i: R.sharpness(i, 1.3), lambda i: _np(ImageEnhance.Sharpness(_pil(i)).enhance(1.3)), cases)
    with monkeypatch.context() as m:
        m.setattr(R, "mean_round", lambda v: int(v))
        caught = _differs_somewhere(lambda i: R.enhance(i, 1, 0.7), lambda i: _np(ImageEnhance.Contrast(_pil(i)).enhance(0.7)),
                                    list(_enhance_images(1)))
        assert any(n[0] == "tie" for n in caught), caught
    with monkeypatch.context() as m:
        m.setattr(R, "interior_mask", lambda H, W: np.ones((H, W), bool))
        for f in (0.7, 1.3):
            assert _differs_somewhere(lambda i: R.sharpness(i, f), lambda i: _np(ImageEnhance.Sharpness(_pil(i)).enhance(f)), cases)


# ============================================================================================== (a): to_u8, finish, normalise
def _tv_normalize(chw_u8):
    mean = torch.tensor((0.485, 0.456, 0.406), dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor((0.229, 0.224, 0.225), dtype=torch.float32).view(3, 1, 1)
    return (torch.from_numpy(chw_u8.copy()).to(torch.float32).div(255) - mean) / std


def test_to_u8_finish_and_normalise_equal_torch_and_numpy(monkeypatch):
    x = R.to_u8_inputs()
    assert x.size > 700 and x.min() == 0.0 and x.max() == 1.0
    want = torch.from_numpy(x).mul(255).byte().numpy()
    assert np.array_equal(R.to_u8(x), want)
    assert sorted(set(want.tolist())) == list(range(256)) and (np.diff(want[:256].astype(int)) == 1).all()
    big = np.random.RandomState(1).random_sample(R.TRIP_N).astype(np.float32)
    assert np.array_equal(R.to_u8(big), torch.from_numpy(big).mul(255).byte().numpy())
    for W in R.FINISH_WIDTHS:
        img = R.finish_plane(W)
        assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
        exp = torch.flip(_tv_normalize(img.transpose(2, 0, 1)), dims=[2]).numpy()
        assert np.array_equal(R.finish(img).view(np.int32), exp.view(np.int32)), W
    img = R.plane(*R.TRIP_SHARP, "random")
    assert np.array_equal(R.finish(img), torch.flip(_tv_normalize(img.transpose(2, 0, 1)), dims=[2]).numpy())
    with monkeypatch.context() as m:
        m.setattr(R, "flip_w", lambda a: a)
        odd = R.finish_plane(7)
        assert not np.array_equal(R.finish(odd), torch.flip(_tv_normalize(odd.transpose(2, 0, 1)), dims=[2]).numpy())
    for H, W in R.NORMALIZE_SHAPES:
        img = R.normalize_plane(H, W)
        assert np.array_equal(R.normalize_train(img).view(np.int32), _tv_normalize(img.transpose(2, 0, 1)).numpy().view(np.int32))
        val = O.normalize_img(img).transpose(2, 0, 1)
        assert np.array_equal(R.normalize_val(img).view(np.int32), np.ascontiguousarray(val).view(np.int32))
    img = R.normalize_plane(16, 16)
    in32 = np.stack([(img[..., c].astype(np.float32) - np.float32(R.MEAN64[c])) / np.float32(R.STD64[c]) for c in range(3)])
    assert not np.array_equal(in32, R.normalize_val(img)), "val normalisation done in float32 is not noticed"


# ============================================================================================== (a) + (c): hue, blur
def test_hue_and_grayscale_equal_pillow():
    for n, shift in R.HUE_CASES:
        img = R.plane(1, n, "random", seed=shift)
        h, s, v = _pil(img).convert("HSV").split()
        nh = ((np.asarray(h).astype(np.int32) + shift) & 255).astype(np.uint8)
        ref = _np(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
        assert np.array_equal(R.hue_shift(img, shift), ref), (n, shift)
    for name, img in _small_images():
        l = _np(_pil(img).convert("L"))
        assert np.array_equal(R.grayscale(img), np.dstack([l, l, l])), name


def _box_pass_variant(img, fr, clamp=True, far=True):
    """oracle.pil_box_pass_np with two switches: clamp=False wraps the window at the line ends instead of clamping it, far=False
    drops the two fractional far pixels.  With both on it is checked equal to the oracle's below."""
    fr32 = np.float32(fr)
    radius = int(fr32)
    ww = int(np.uint32(np.float32(1 << 24) / (fr32 * np.float32(2) + np.float32(1))))
    fw = (((1 << 24) - (radius * 2 + 1) * ww) & 0xFFFFFFFF) // 2 if far else 0
    W = img.shape[1]
    x = np.arange(W)
    at = (lambda i: np.clip(i, 0, W - 1)) if clamp else (lambda i: i % W)
    acc = np.zeros(img.shape, np.int64)
    for d in range(-radius, radius + 1):
        acc += img[:, at(x + d)]
    farpx = img[:, at(x - radius - 1)].astype(np.int64) + img[:, at(x + radius + 1)]
    return ((((acc * ww + farpx * fw) & 0xFFFFFFFF) + (1 << 23) & 0xFFFFFFFF) >> 24).astype(np.uint8)


def test_blur_equals_pillow_and_box_mistakes_are_caught(monkeypatch):
    reps, imgs = set(), {}
    for H, W, r in R.BLUR_CASES + (R.TRIP_BLUR,):
        img = imgs.setdefault((H, W), R.plane(H, W, "random", seed=3))
        rep = set()
        ref = _np(_pil(img).filter(ImageFilter.GaussianBlur(radius=r)))
        assert np.array_equal(R.gaussian_blur(img, r, rep), ref), (H, W, r)
        reps |= rep
        if (H, W) in ((2, 300), (7, 5)):
            fr = O.pil_gaussian_box_radius(r, 3)
            assert np.array_equal(_box_pass_variant(img, fr), O.pil_box_pass_np(img, fr))
    assert "radius>=len" in reps
    img = imgs[(7, 5)]
    assert np.array_equal(R.gaussian_blur(img, 0.0), img) and np.array_equal(_np(_pil(img).filter(ImageFilter.GaussianBlur(0))), img)
    for kw in (dict(clamp=False), dict(far=False)):
        with monkeypatch.context() as m:
            m.setattr(O, "pil_box_pass_np", lambda i, fr: _box_pass_variant(i, fr, **kw))
            caught = [(H, W, r) for H, W, r in R.BLUR_CASES
                      if not np.array_equal(R.gaussian_blur(imgs[(H, W)], r), _np(_pil(imgs[(H, W)]).filter(ImageFilter.GaussianBlur(r))))]
            print(f"box pass with {kw}: differs from Pillow on {len(caught)} of {len(R.BLUR_CASES)} cases")
            assert caught, kw


# ============================================================================================== (a) + (b) + (c): resample, crop
def _pil_resize(img, w2, h2):
    return _np(_pil(img).resize([w2, h2], resample=Image.BILINEAR))


def test_resample_h_equals_pillow():
    for h, w, w2 in R.RESAMPLE_H_CASES:
        img = R.byte_image(h, w)
        assert np.array_equal(R.resample_h(img, w2), _pil_resize(img, w2, h)), (h, w, w2)
    # both passes, each rounded to uint8; a single rounding at the end differs
    once = 0
    for (h, w, w2), h2 in zip(R.RESAMPLE_H_CASES, (1, 3, 2, 9, 7, 100, 15, 3, 67, 16)):
        img = R.byte_image(h, w)
        ref = _pil_resize(img, w2, h2)
        assert np.array_equal(R.resample_v(R.resample_h(img, w2), h2), ref), (h, w, w2, h2)
        cx, bx, _ = R.resample_coeffs(w, w2)
        cy, by, _ = R.resample_coeffs(h, h2)
        A = np.zeros((w2, w))
        B = np.zeros((h2, h))
        for x in range(w2):
            A[x, bx[x, 0]:bx[x, 0] + bx[x, 1]] = cx[x, :bx[x, 1]] / 2.0 ** 22
        for y in range(h2):
            B[y, by[y, 0]:by[y, 0] + by[y, 1]] = cy[y, :by[y, 1]] / 2.0 ** 22
        one = np.clip(np.floor(np.einsum("yh,hwc,xw->yxc", B, img.astype(np.float64), A) + 0.5), 0, 255).astype(np.uint8)
        once += int(not np.array_equal(one, ref))
    assert once > 0, "rounding once instead of per pass is not noticed"


def _pil_geometry(tmp, h2, flip, hp, wp, hs, ws, S):
    """the reference project's chain: PIL resize -> np.fliplr -> zero pad at (hp, wp) -> crop at (hs, ws)"""
    img = _pil_resize(tmp, tmp.shape[1], h2)
    if flip:
        img = np.fliplr(img)
    h, w = img.shape[:2]
    pad = np.zeros((max(S, h), max(S, w), 3), np.uint8)
    pad[hp:hp + h, wp:wp + w] = img
    return pad[hs:hs + S, ws:ws + S]


def _flip_after_pad(img, flip, hp, wp, hs, ws, S):
    h, w = img.shape[:2]
    pad = np.zeros((max(S, h), max(S, w), 3), np.uint8)
    pad[hp:hp + h, wp:wp + w] = img
    if flip:
        pad = np.fliplr(pad)
    return pad[hs:hs + S, ws:ws + S]


def _offsets_swapped(img, flip, hp, wp, hs, ws, S):
    """output (y, x) = image (y + hp - hs, x + wp - ws) instead of (y + hs - hp, x + ws - wp)"""
    if flip:
        img = np.fliplr(img)
    h, w = img.shape[:2]
    out = np.zeros((S, S, 3), np.uint8)
    for y in range(S):
        for x in range(S):
            Y, X = y + hp - hs, x + wp - ws
            if 0 <= Y < h and 0 <= X < w:
                out[y, x] = img[Y, X]
    return out


def test_vcrop_equals_pillow_covers_the_geometry_and_mistakes_are_caught():
    sides, mixed, n, late_flip, swapped, no_flip = set(), set(), 0, 0, 0, 0
    for h, w2 in R.VCROP_TMP_SHAPES:
        tmp = R.byte_image(h, w2)
        for h2, S, flip, hp, wp, hs, ws in R.vcrop_cases(h, w2):
            rep = set()
            ref = _pil_geometry(tmp, h2, flip, hp, wp, hs, ws, S)
            assert np.array_equal(R.v_crop(tmp, h2, flip, hp, wp, hs, ws, S, rep), ref), (h, w2, h2, S, flip, hp, wp, hs, ws)
            assert ("flip" in rep) == bool(flip)
            sides |= rep
            if flip:                                         # the column remap left out altogether
                no_flip += int(not np.array_equal(R.v_crop(tmp, h2, 0, hp, wp, hs, ws, S), ref))
            if hp > 0 and ws > 0:
                mixed.add(("pad_h+crop_w", flip))
            if wp > 0 and hs > 0:
                mixed.add(("pad_w+crop_h", flip))
            if S < 17 or (h, w2) == (9, 17):             # the double loop of the swapped variant is slow on big crops
                scaled = R.resample_v(tmp, h2)
                late_flip += int(not np.array_equal(_flip_after_pad(scaled, flip, hp, wp, hs, ws, S), ref))
                swapped += int(not np.array_equal(_offsets_swapped(scaled, flip, hp, wp, hs, ws, S), ref))
            n += 1
    print(f"{n} crop cases; flip after the pad differs on {late_flip}, swapped offsets on {swapped}, flip ignored on {no_flip}")
    assert {"outside_top", "outside_bottom", "outside_left", "outside_right", "flip"} <= sides
    assert mixed == {("pad_h+crop_w", 0), ("pad_h+crop_w", 1), ("pad_w+crop_h", 0), ("pad_w+crop_h", 1)}
    assert late_flip > 0 and swapped > 0 and no_flip > 0
    odd_flip = [c for h, w2 in R.VCROP_TMP_SHAPES for c in R.vcrop_cases(h, w2) if c[2] and w2 % 2 == 1]
    assert odd_flip and any(w2 == 1 for _, w2 in R.VCROP_TMP_SHAPES)
    assert any((S * S) % 256 for S in R.VCROP_S)


# ============================================================================================== (a): chains
def test_chains_equal_the_oracle_at_the_untested_magnitudes():
    assert R.AUGMENT_LIST == O.AUGMENT_LIST
    for b, H, W in R.CHAIN_BATCHES:
        x = R.chain_input(b, H, W)
        for m in R.CHAIN_MAGNITUDES:
            seqs = [R.magnitude_ops(m)] * b
            exp = O.augment_data_strong(torch.from_numpy(x), ops_per_image=seqs).numpy()
            assert np.array_equal(R.augment_chain(x, seqs).view(np.int32), exp.view(np.int32)), (b, H, W, m)
