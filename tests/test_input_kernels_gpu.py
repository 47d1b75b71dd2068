"""The input pipeline's kernels (csrc/augment.hip, csrc/photometric.hip, csrc/loader.hip) at their edges, entry point by entry
point, bit for bit against tests/input_ref.py -- the plain numpy restatement of Pillow's arithmetic that
tests/test_input_ref_host.py proves equal to Pillow itself on these same case lists (this file never imports PIL): planes with no
interior, one row / one column / one pixel, factors on both sides of [0, 1], LUTs that are the identity or saturate, exact mean
ties, blur radii beyond the line length, every crop geometry flush with a border, pixel counts that end inside a 256-lane block and
the second trip of every capped grid-stride loop.

Technique (tests/kernel_guard.py): every buffer a kernel writes -- outputs, in-place images, LUT / histogram / sum scratch, the blur's
tmp -- is a view inside a sentinel-guarded allocation (256 bytes of 0xA5 on either side of a uint8 view) that must come back intact,
and the views sit at byte offsets 0 .. 3 off alignment, as the batch path hands kernels u8[i].  The refusal tests only pass
arguments a launcher rejects before launching."""
import numpy as np
import pytest
import torch

import input_ref as R
from kernel_guard import _ALIVE, PAD_U8, Guard, stream

pytestmark = pytest.mark.gpu
ERR_ARG = -1
U8, I32, I64 = torch.uint8, torch.int32, torch.int64


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _ALIVE.clear()


def L():
    from dupl_amd._lib import lib
    return lib()


def planar(img):
    return np.ascontiguousarray(img.transpose(2, 0, 1))


def hwc(chw):
    return np.ascontiguousarray(chw.transpose(1, 2, 0))


def u8_guard(dev, arr=None, shape=None, off=0):
    """a guarded uint8 view `off` bytes off the allocation's alignment, holding arr (or the sentinel)"""
    init = None if arr is None else torch.from_numpy(np.ascontiguousarray(arr))
    return Guard(tuple(arr.shape) if arr is not None else tuple(shape), dev, U8, init=init, front=PAD_U8 + off)


def u8_in(dev, arr, off=0):
    g = u8_guard(dev, arr, off=off)
    _ALIVE.append(g.buf)
    return g.view


def dirty(shape, dev, dtype):
    """guarded scratch left full of 0xFF bytes"""
    g = Guard(shape, dev, dtype)
    g.view.view(U8).fill_(0xFF)
    return g


def eq(got, want, what):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} elements differ"


def small_images():
    for k, (H, W, c) in enumerate(R.SMALL_PLANES):
        yield k, (H, W, c), R.plane(H, W, c)


# ================================================================================================ to_u8, posterize, finish
def _to_u8(dev, x, off):
    xin = torch.from_numpy(x).to(dev)
    out = u8_guard(dev, shape=x.shape, off=off)
    L().dupl_aug_to_u8(xin.data_ptr(), out.ptr, x.size, stream())
    return out.cpu()


def test_to_u8_on_the_lattice_its_neighbours_and_the_second_trip(dev):
    x = R.to_u8_inputs()
    for off in (0, 1, 3):
        eq(_to_u8(dev, x, off), R.to_u8(x), f"to_u8 lattice, offset {off}")
    one = np.asarray([1.0], np.float32)
    eq(_to_u8(dev, one, 2), R.to_u8(one), "to_u8 n = 1")
    big = np.random.RandomState(1).random_sample(R.TRIP_N).astype(np.float32)
    eq(_to_u8(dev, big, 1), R.to_u8(big), "to_u8 second trip")


@pytest.mark.parametrize("bits", R.POSTERIZE_BITS)
def test_posterize(dev, bits):
    for k, name, img in small_images():
        g = u8_guard(dev, planar(img), off=k % 4)
        L().dupl_aug_posterize(g.ptr, img.size, bits, stream())
        eq(hwc(g.cpu().numpy()), R.posterize(img, bits), f"posterize {bits} {name}")
    if bits == 5:
        x = np.random.RandomState(2).randint(0, 256, size=R.TRIP_N, dtype=np.uint8)
        g = u8_guard(dev, x, off=3)
        L().dupl_aug_posterize(g.ptr, x.size, bits, stream())
        eq(g.cpu(), R.posterize(x, bits), "posterize second trip")


def _finish(dev, img, off):
    out = Guard((3,) + img.shape[:2], dev)
    L().dupl_aug_finish(u8_in(dev, planar(img), off).data_ptr(), out.ptr, img.shape[0], img.shape[1], stream())
    return out.cpu()


def test_finish_every_byte_value_odd_and_even_widths_and_the_second_trip(dev):
    for W in R.FINISH_WIDTHS:
        img = R.finish_plane(W)
        eq(_finish(dev, img, W % 4), R.finish(img), f"finish W = {W}")
    for k, name, img in small_images():
        if name[2] == "random":
            eq(_finish(dev, img, k % 4), R.finish(img), f"finish {name}")
    img = R.plane(*R.TRIP_SHARP, "random")
    eq(_finish(dev, img, 1), R.finish(img), "finish second trip")


# ================================================================================================ LUT ops
def _lut_op(dev, img, mode, hist, lut, off):
    g = u8_guard(dev, planar(img), off=off)
    L().dupl_aug_lut_op(g.ptr, img.shape[0], img.shape[1], mode, hist.ptr, lut.ptr, stream())
    got = hwc(g.cpu().numpy())
    assert hist.intact() and lut.intact()
    return got


@pytest.mark.parametrize("mode", (0, 1))
def test_lut_ops_degenerate_saturating_and_plain_on_one_dirty_scratch(dev, mode):
    """Every plane of R.LUT_PLANES through ONE histogram / LUT scratch that starts full of 0xFF bytes and is never cleaned by the test:
    identity LUTs (hi == lo; at most one bin; step == 0), LUT entries above 255 that Pillow clips, each image after a different
    one (the plain path as a whole plane is test_lut_apply_second_trip's).  The histogram the call leaves behind is the image's."""
    hist, lut = dirty((768,), dev, I32), dirty((768,), dev, U8)
    for k, (H, W, c) in enumerate(R.LUT_PLANES):
        img = R.plane(H, W, c)
        eq(_lut_op(dev, img, mode, hist, lut, k % 4), R.lut_op(img, mode), f"lut_op mode {mode} {(H, W, c)}")
        want = np.concatenate([R.hist256(img[..., ch]) for ch in range(3)]).astype(np.int32)
        eq(hist.view.cpu(), want, f"histogram {(H, W, c)}")


@pytest.mark.parametrize("mode", (0, 1))
def test_lut_apply_second_trip(dev, mode):
    img = R.plane(*R.TRIP_LUT, "random")
    if mode == 0:
        img = (img // 2 + 17).astype(np.uint8)               # lo = 17, hi = 144: a LUT that is not the identity
    hist, lut = dirty((768,), dev, I32), dirty((768,), dev, U8)
    eq(_lut_op(dev, img, mode, hist, lut, 1), R.lut_op(img, mode), f"lut_op second trip mode {mode}")


# ================================================================================================ blends
def _enhance_images(mode):
    for k, name, img in small_images():
        yield k, name, img
    if mode == 1:
        for k in R.TIE_LUMAS:
            yield k, ("tie", k), R.tie_plane(k)
        yield 1, R.CONTRAST_EXTRA_SHAPE, R.plane(*R.CONTRAST_EXTRA_SHAPE, "random")


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_aug_enhance_factors_on_both_sides_and_mean_ties(dev, mode):
    """Color / Contrast / Brightness of augment.hip (planar) at 0, 0.1, 0.7, 1, 1.3, 1.9 and an off-grid factor on every small plane;
    for Contrast also lumas k, k + 1 (the mean is k + 0.5 exactly), one pixel, all 255, and 181 x 182 (17 blocks of the luma-sum grid, the last part full).
    The sum scratch starts as 0xFF bytes and is shared by all calls."""
    lsum = dirty((1,), dev, I64)
    for f in R.FACTORS:
        for k, name, img in _enhance_images(mode):
            g = u8_guard(dev, planar(img), off=k % 4)
            L().dupl_aug_enhance(g.ptr, img.shape[0], img.shape[1], mode, f, lsum.ptr, stream())
            eq(hwc(g.cpu().numpy()), R.enhance(img, mode, f), f"aug_enhance mode {mode} f {f} {name}")
            assert lsum.intact()
            if mode == 1:
                assert int(lsum.view.cpu()) == int(R.luma(img).sum(dtype=np.int64)), name


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_photo_enhance_factors_on_both_sides_and_mean_ties(dev, mode):
    """the same for photometric.hip's interleaved twin"""
    lsum = dirty((1,), dev, I64)
    for f in R.FACTORS:
        for k, name, img in _enhance_images(mode):
            g = u8_guard(dev, img, off=k % 4)
            L().dupl_photo_enhance(g.ptr, img.shape[0], img.shape[1], mode, f, lsum.ptr if mode == 1 else None, stream())
            eq(g.cpu(), R.enhance(img, mode, f), f"photo_enhance mode {mode} f {f} {name}")
            assert lsum.intact()


@pytest.mark.parametrize("which,mode", [("aug", 0), ("aug", 1), ("photo", 0), ("photo", 1), ("photo", 2)])
def test_enhance_second_trips(dev, which, mode):
    lsum = dirty((1,), dev, I64)
    if which == "aug":
        img = R.plane(*R.TRIP_LUT, "random")
        g = u8_guard(dev, planar(img), off=3)
        L().dupl_aug_enhance(g.ptr, img.shape[0], img.shape[1], mode, 1.3, lsum.ptr, stream())
        got = hwc(g.cpu().numpy())
    else:
        img = R.plane(*R.TRIP_PHOTO, "random")
        g = u8_guard(dev, img, off=1)
        L().dupl_photo_enhance(g.ptr, img.shape[0], img.shape[1], mode, 1.3, lsum.ptr, stream())
        got = g.cpu().numpy()
    eq(got, R.enhance(img, mode, 1.3), f"{which} enhance second trip, mode {mode}")
    assert lsum.intact()


def _sharpness(dev, img, f, off):
    out = u8_guard(dev, shape=(3,) + img.shape[:2], off=off)
    L().dupl_aug_sharpness(u8_in(dev, planar(img), (off + 1) % 4).data_ptr(), out.ptr, img.shape[0], img.shape[1], f, stream())
    return hwc(out.cpu().numpy())


@pytest.mark.parametrize("f", R.FACTORS)
def test_sharpness_planes_without_interior_and_both_clips(dev, f):
    for k, name, img in small_images():
        eq(_sharpness(dev, img, f, k % 4), R.sharpness(img, f), f"sharpness f {f} {name}")


def test_sharpness_second_trip(dev):
    img = R.plane(*R.TRIP_SHARP, "random")
    eq(_sharpness(dev, img, 1.3, 1), R.sharpness(img, 1.3), "sharpness second trip")


# ================================================================================================ grayscale, hue, blur
def test_grayscale_small_planes_and_second_trip(dev):
    for k, name, img in list(small_images()) + [(1, R.TRIP_PHOTO, R.plane(*R.TRIP_PHOTO, "random"))]:
        g = u8_guard(dev, img, off=k % 4)
        L().dupl_photo_grayscale(g.ptr, img.shape[0] * img.shape[1], stream())
        eq(g.cpu(), R.grayscale(img), f"grayscale {name}")


def test_hue_pixel_counts_around_a_wave(dev):
    for k, (n, shift) in enumerate(R.HUE_CASES):
        img = R.plane(1, n, "random", seed=shift)
        g = u8_guard(dev, img, off=k % 4)
        L().dupl_photo_hue(g.ptr, n, shift, stream())
        eq(g.cpu(), R.hue_shift(img, shift), f"hue n {n} shift {shift}")


def _blur(dev, img, r, off):
    g = u8_guard(dev, img, off=off)
    tmp = u8_guard(dev, shape=img.shape, off=(off + 2) % 4)
    L().dupl_photo_gaussian_blur(g.ptr, tmp.ptr, img.shape[0], img.shape[1], r, stream())
    got = g.cpu().numpy()
    assert tmp.intact()
    return got, tmp


@pytest.mark.parametrize("H,W", R.BLUR_SHAPES)
def test_blur_radii_up_to_far_beyond_the_line(dev, H, W):
    img = R.plane(H, W, "random", seed=3)
    for k, r in enumerate(R.BLUR_RADII):
        got, _ = _blur(dev, img, r, k % 4)
        eq(got, R.gaussian_blur(img, r), f"blur {H}x{W} radius {r}")
    got, tmp = _blur(dev, img, 0.0, 1)
    eq(got, img, "radius 0 returns the image")
    assert tmp.untouched()


def test_blur_second_trip(dev):
    H, W, r = R.TRIP_BLUR
    img = R.plane(H, W, "random", seed=3)
    got, _ = _blur(dev, img, r, 3)
    eq(got, R.gaussian_blur(img, r), "blur second trip")


# ================================================================================================ loader
@pytest.mark.parametrize("mode", (0, 1))
def test_normalize_every_byte_value_and_counts_around_a_block(dev, mode):
    for k, (H, W) in enumerate(R.NORMALIZE_SHAPES):
        img = R.normalize_plane(H, W)
        out = Guard((3, H, W), dev)
        L().dupl_loader_normalize(u8_in(dev, img, (k + 1) % 4).data_ptr(), out.ptr, H, W, mode, stream())
        eq(out.cpu(), (R.normalize_train if mode == 0 else R.normalize_val)(img), f"normalize mode {mode} {H}x{W}")


def _tables(dev, n_in, n_out):
    coef, bounds, ksize = R.resample_coeffs(n_in, n_out)
    c = torch.from_numpy(np.ascontiguousarray(coef, np.int32)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(bounds, np.int32)).to(dev)
    _ALIVE.extend([c, b])
    return c, b, ksize


@pytest.mark.parametrize("h,w,w2", R.RESAMPLE_H_CASES)
def test_resample_h_alone(dev, h, w, w2):
    img = R.byte_image(h, w)
    c, b, k = _tables(dev, w, w2)
    out = u8_guard(dev, shape=(h, w2, 3), off=(h + w2) % 4)
    L().dupl_loader_resample_h(u8_in(dev, img, w % 4).data_ptr(), out.ptr, c.data_ptr(), b.data_ptr(), k, h, w, w2, stream())
    eq(out.cpu(), R.resample_h(img, w2), f"resample_h {h}x{w} -> {w2}")


@pytest.mark.parametrize("h,w2", R.VCROP_TMP_SHAPES)
def test_resample_v_crop_every_geometry(dev, h, w2):
    """every (h2, crop, flip, pad / start offsets) of R.vcrop_cases: image smaller than the crop at either end of the canvas, larger
    with the window at either end, padded on one axis and cropped on the other, crop sizes whose square ends inside a block"""
    tmp = R.byte_image(h, w2)
    tin = u8_in(dev, tmp, 1)
    tables, n = {}, 0
    for h2, S, flip, hp, wp, hs, ws in R.vcrop_cases(h, w2):
        if h2 not in tables:
            tables[h2] = _tables(dev, h, h2)
        c, b, k = tables[h2]
        out = u8_guard(dev, shape=(S, S, 3), off=n % 4)
        L().dupl_loader_resample_v_crop(tin.data_ptr(), out.ptr, c.data_ptr(), b.data_ptr(), k, w2, h2, flip, hp, wp, hs, ws, S, stream())
        eq(out.cpu(), R.v_crop(tmp, h2, flip, hp, wp, hs, ws, S), f"v_crop {(h, w2)} -> {(h2, S, flip, hp, wp, hs, ws)}")
        n += 1
    print(f"{n} geometries from a {h} x {w2} plane")


# ================================================================================================ scratch reuse, chains
def test_contrast_twice_through_one_transform(dev):
    """DeviceTransform keeps its sum scratch across items: two different crops, contrast on in both, one after the other"""
    from dupl_amd.datasets.device_loader import DeviceTransform
    from dupl_amd.datasets.transforms import Photometric
    tf = DeviceTransform(dev)
    for seed, f in ((1, 1.3), (2, 0.7)):
        img = R.plane(23, 23, "dark_band", seed=seed)
        crop = torch.from_numpy(img).to(dev)
        tf.photometric_view(crop, Photometric(True, (1,), 1.0, f, 1.0, 0.0, False, None))
        eq(crop.cpu(), R.enhance(img, 1, f), f"photometric_view contrast {f}")
    assert tf._sum is not None


@pytest.mark.parametrize("b,H,W", R.CHAIN_BATCHES)
def test_augment_data_strong_all_seven_ops_at_the_untested_magnitudes(dev, b, H, W):
    """RandAugment magnitudes 0 (factor 0.1, one posterize bit), 20 (imutils' own default: factor 1.3) and 30 (1.9, 6 bits)"""
    from dupl_amd.utils import imutils
    x = R.chain_input(b, H, W)
    for m in R.CHAIN_MAGNITUDES:
        seqs = [R.magnitude_ops(m)] * b
        out = imutils.augment_data_strong(torch.from_numpy(x).to(dev), ops_per_image=seqs)
        eq(out.cpu(), R.augment_chain(x, seqs), f"chain magnitude {m} batch {b} x {H} x {W}")


# ================================================================================================ refusals
def _refused(raw, good, bad_sets):
    """raw(*good with one argument replaced) == -1 for every (index, value) of bad_sets"""
    for i, v in bad_sets:
        a = list(good)
        a[i] = v
        assert raw(*a) == ERR_ARG, (i, v)


def test_augment_refusals(dev):
    lib, st = L(), stream()
    img = R.plane(4, 5, "random")
    x = torch.rand(60, device=dev)
    g = u8_guard(dev, planar(img), off=1)
    out = u8_guard(dev, shape=(3, 4, 5), off=2)
    fout = Guard((3, 4, 5), dev)
    hist, lut, lsum = Guard((768,), dev, I32), Guard((768,), dev, U8), Guard((1,), dev, I64)
    _refused(lib.dupl_aug_to_u8.raw, (x.data_ptr(), out.ptr, 60, st), [(0, None), (1, None), (2, 0), (2, -1)])
    _refused(lib.dupl_aug_lut_op.raw, (g.ptr, 4, 5, 0, hist.ptr, lut.ptr, st),
             [(0, None), (4, None), (5, None), (1, 0), (1, -3), (2, 0), (2, -1), (3, -1), (3, 2)])
    _refused(lib.dupl_aug_posterize.raw, (g.ptr, 60, 4, st), [(0, None), (1, 0), (1, -60), (2, 0), (2, 9), (2, -1)])
    _refused(lib.dupl_aug_enhance.raw, (g.ptr, 4, 5, 1, 0.5, lsum.ptr, st),
             [(0, None), (1, 0), (2, 0), (1, -4), (2, -5), (3, -1), (3, 3), (5, None)])
    _refused(lib.dupl_aug_sharpness.raw, (g.ptr, out.ptr, 4, 5, 0.5, st), [(0, None), (1, None), (1, g.ptr), (2, 0), (3, 0), (2, -4)])
    _refused(lib.dupl_aug_finish.raw, (g.ptr, fout.ptr, 4, 5, st), [(0, None), (1, None), (2, 0), (3, 0), (3, -5)])
    torch.cuda.synchronize()
    assert out.untouched() and fout.untouched() and hist.untouched() and lut.untouched() and lsum.untouched()
    assert g.intact() and np.array_equal(hwc(g.view.cpu().numpy()), img)


def test_photometric_refusals(dev):
    lib, st = L(), stream()
    img = R.plane(4, 5, "random")
    g = u8_guard(dev, img, off=3)
    tmp = u8_guard(dev, shape=(4, 5, 3), off=1)
    lsum = Guard((1,), dev, I64)
    _refused(lib.dupl_photo_enhance.raw, (g.ptr, 4, 5, 1, 0.5, lsum.ptr, st),
             [(0, None), (1, 0), (2, 0), (1, -4), (3, -1), (3, 3), (5, None)])
    _refused(lib.dupl_photo_hue.raw, (g.ptr, 20, 7, st), [(0, None), (1, 0), (1, -20), (2, -1), (2, 256)])
    _refused(lib.dupl_photo_grayscale.raw, (g.ptr, 20, st), [(0, None), (1, 0), (1, -1)])
    _refused(lib.dupl_photo_gaussian_blur.raw, (g.ptr, tmp.ptr, 4, 5, 1.0, st),
             [(0, None), (1, None), (1, g.ptr), (2, 0), (3, 0), (2, -4), (4, -0.5), (4, float("nan")), (4, 4096.5), (4, float("inf"))])
    torch.cuda.synchronize()
    assert tmp.untouched() and lsum.untouched()
    assert g.intact() and np.array_equal(g.view.cpu().numpy(), img)


def test_loader_refusals(dev):
    lib, st = L(), stream()
    img = R.byte_image(7, 9)
    src = u8_in(dev, img, 1)
    cx, bx, kx = _tables(dev, 9, 18)
    cy, by, ky = _tables(dev, 7, 15)
    out = u8_guard(dev, shape=(16, 18, 3), off=1)
    fout = Guard((3, 7, 9), dev)
    _refused(lib.dupl_loader_resample_h.raw, (src.data_ptr(), out.ptr, cx.data_ptr(), bx.data_ptr(), kx, 7, 9, 18, st),
             [(0, None), (1, None), (2, None), (3, None), (4, 0), (4, -3), (5, 0), (6, 0), (7, 0), (7, -18)])
    _refused(lib.dupl_loader_resample_v_crop.raw,
             (src.data_ptr(), out.ptr, cy.data_ptr(), by.data_ptr(), ky, 9, 15, 0, 1, 7, 0, 0, 16, st),
             [(0, None), (1, None), (2, None), (3, None), (4, 0), (4, -3), (5, 0), (6, 0), (12, 0), (12, -16), (8, -1), (9, -1),
              (10, -1), (11, -1)])
    _refused(lib.dupl_loader_normalize.raw, (src.data_ptr(), fout.ptr, 7, 9, 0, st),
             [(0, None), (1, None), (2, 0), (3, 0), (2, -7), (4, -1), (4, 2)])
    torch.cuda.synchronize()
    assert out.untouched() and fout.untouched()
