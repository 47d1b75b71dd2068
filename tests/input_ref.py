"""Plain numpy restatements of the input pipeline's pixel arithmetic (csrc/augment.hip, csrc/photometric.hip, csrc/loader.hip) and
the case lists of its two edge suites.  Every function is written from Pillow's / torchvision's / numpy's documented arithmetic, not
from the kernels; tests/test_input_ref_host.py proves each of them equal to Pillow itself, bit for bit, on every case listed here,
and tests/test_input_kernels_gpu.py then compares the kernels with them (it never imports PIL).

Images are (H, W, 3) uint8 arrays like the ones PIL hands to numpy; the GPU suite transposes for the planar kernels.  A function
that has branches takes `report`, a set it adds the names of the branches it took to:
    hi==lo, nnz<=1, step==0, lut_clip (a LUT entry above 255), lut_clip_present (... for a value the plane holds),
    blend_low / blend_high (factor outside [0, 1] and the result clipped at 0 / 255), interior_empty,
    radius>=len, outside_top / _bottom / _left / _right (crop pixels outside the image), flip.
The rounding primitives (lut_fit, blend_inside, blend_outside, mean_round, interior_mask, flip_w) are module-level functions so the
host suite can swap one for a classic mistake and show that the case lists notice."""
import itertools

import numpy as np

from dupl_amd.datasets.transforms import resample_coeffs

f32, f64 = np.float32, np.float64
MEAN32 = np.asarray((0.485, 0.456, 0.406), f32)
STD32 = np.asarray((0.229, 0.224, 0.225), f32)
MEAN64 = (123.675, 116.28, 103.53)
STD64 = (58.395, 57.12, 57.375)
AUGMENT_LIST = (("AutoContrast", 0, 1), ("Equalize", 0, 1), ("Posterize", 0, 6), ("Color", 0.1, 1.9), ("Contrast", 0.1, 1.9),
                ("Brightness", 0.1, 1.9), ("Sharpness", 0.1, 1.9))


def _mark(report, name, cond=True):
    if report is not None and bool(cond):
        report.add(name)


# ================================================================================================ primitives (mutation points)
def lut_fit(t):
    """ImageOps.equalize hands its list to Image.point, which stores it in 8 bits by clipping"""
    return min(t, 255)


def blend_inside(t):
    """ImagingBlend, 0 <= alpha <= 1: (UINT8) of the float, i.e. truncation (the value is inside [0, 255])"""
    return t.astype(np.int32).astype(np.uint8)


def blend_outside(t):
    """ImagingBlend, alpha outside [0, 1]: <= 0 -> 0, >= 255 -> 255, else (UINT8)"""
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def mean_round(m):
    """ImageEnhance.Contrast: int(mean + 0.5)"""
    return int(m + 0.5)


def interior_mask(H, W):
    """ImagingFilter 3x3 copies the first / last row and column: only pixels with all eight neighbours are filtered"""
    m = np.zeros((H, W), bool)
    m[1:H - 1, 1:W - 1] = True
    return m


def flip_w(a):
    """augment_data_strong's torch.flip(dims=[2]) of a (3, H, W) tensor"""
    return a[:, :, ::-1]


# ================================================================================================ augment.hip
def to_u8(x):
    """transforms.ToPILImage of a float tensor: pic.mul(255).byte() -- float32 product, truncation.  Finite x in [0, 1]."""
    return (np.asarray(x, f32) * f32(255)).astype(np.int32).astype(np.uint8)


def hist256(plane):
    return np.bincount(np.asarray(plane).ravel(), minlength=256)


def autocontrast_lut(h, report=None):
    """ImageOps.autocontrast(cutoff=0) of one channel: lo / hi = first / last non-empty bin; identity when hi <= lo; else
    scale = 255.0 / (hi - lo), offset = -lo * scale, lut[i] = clip(int(i * scale + offset)) in Python floats (doubles)."""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        _mark(report, "hi==lo")
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.asarray([min(max(int(i * scale + offset), 0), 255) for i in range(256)], np.uint8)


def equalize_lut(h, report=None):
    """ImageOps.equalize of one channel: histo = the non-zero bins; identity when there is at most one; step = (sum(histo) -
    histo[-1]) // 255; identity when 0; else n = step // 2, lut[i] = n // step, n += h[i]; stored in 8 bits (lut_fit)."""
    h = [int(v) for v in h]
    histo = [v for v in h if v]
    if len(histo) <= 1:
        _mark(report, "nnz<=1")
        return np.arange(256, dtype=np.uint8)
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        _mark(report, "step==0")
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        t = n // step
        _mark(report, "lut_clip", t > 255)
        _mark(report, "lut_clip_present", t > 255 and h[i])
        lut.append(lut_fit(t))
        n += h[i]
    return np.asarray(lut, np.int64).astype(np.uint8)


def lut_op(img, mode, report=None):
    """mode 0: ImageOps.autocontrast, 1: ImageOps.equalize -- per channel a LUT from that channel's histogram"""
    out = np.empty_like(img)
    for c in range(3):
        lut = (autocontrast_lut if mode == 0 else equalize_lut)(hist256(img[..., c]), report)
        out[..., c] = lut[img[..., c]]
    return out


def posterize(img, bits):
    """ImageOps.posterize: keep the top `bits` bits"""
    return img & np.uint8(~(2 ** (8 - bits) - 1) & 0xFF)


def blend(d, p, f, report=None):
    """Image.blend(degenerate, image, f): (int)d + alpha * ((int)p - (int)d) with a float alpha, i.e. float32 arithmetic;
    truncated for alpha in [0, 1], clipped outside"""
    a = f32(f)
    t = np.asarray(d, np.int32).astype(f32) + a * (np.asarray(p, np.int32) - np.asarray(d, np.int32)).astype(f32)
    t = np.broadcast_to(t, np.broadcast_shapes(np.shape(d), np.shape(p)))
    if 0.0 <= a <= 1.0:
        return blend_inside(t)
    _mark(report, "blend_low", (t <= 0).any())
    _mark(report, "blend_high", (t >= 255).any())
    return blend_outside(t)


def luma(img):
    """convert("L"), ITU-R 601-2 in 16-bit fixed point: (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    v = img.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def contrast_mean(img):
    """ImageEnhance.Contrast: int(ImageStat.Stat(image.convert("L")).mean[0] + 0.5), the mean a Python float sum / count"""
    l = luma(img)
    return mean_round(float(int(l.sum(dtype=np.int64))) / float(l.size))


def enhance(img, mode, f, report=None):
    """mode 0: ImageEnhance.Color (degenerate = L), 1: Contrast (the rounded mean of L), 2: Brightness (black)"""
    if mode == 0:
        d = luma(img)[..., None]
    elif mode == 1:
        d = np.full(img.shape[:2] + (1,), contrast_mean(img), np.int32)
    else:
        d = np.zeros(img.shape[:2] + (1,), np.int32)
    return blend(d, img, f, report)


def smooth(img, report=None):
    """ImageFilter.SMOOTH: 3x3 (1,1,1, 1,5,1, 1,1,1) / 13, the kernel stored as float32, the sum started at the rounding offset 0.5
    and accumulated in float32 row by row from the row below, clipped and truncated; the 1-pixel border is copied"""
    H, W = img.shape[:2]
    inside = interior_mask(H, W)
    _mark(report, "interior_empty", not inside.any())
    k = [f32(v / 13) for v in (1, 1, 1, 1, 5, 1, 1, 1, 1)]
    p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge").astype(f32)

    def row(dy, k0):
        r = p[1 + dy:1 + dy + H]
        return (r[:, 0:W] * k[k0] + r[:, 1:W + 1] * k[k0 + 1]) + r[:, 2:W + 2] * k[k0 + 2]

    ss = row(1, 0) + f32(0.5)
    ss = ss + row(0, 3)
    ss = ss + row(-1, 6)
    s = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss.astype(np.int32))).astype(np.uint8)
    return np.where(inside[..., None], s, img)


def sharpness(img, f, report=None):
    """ImageEnhance.Sharpness: blend(SMOOTH(image), image, f)"""
    return blend(smooth(img, report), img, f, report)


def finish(img):
    """ToTensor (u8 / 255 in float32) -> Normalize ((t - mean) / std in float32) -> flip along W; (H, W, 3) -> (3, H, W)"""
    t = img.transpose(2, 0, 1).astype(f32) / f32(255)
    return np.ascontiguousarray(flip_w((t - MEAN32[:, None, None]) / STD32[:, None, None]))


def apply_op(img, name, val, report=None):
    """one op of RandAugment's list at value `val`, the way utils/randomaug.py calls Pillow"""
    if name in ("AutoContrast", "Equalize"):
        return lut_op(img, ("AutoContrast", "Equalize").index(name), report)
    if name == "Posterize":
        return posterize(img, max(1, int(val)))
    if name == "Sharpness":
        return sharpness(img, val, report)
    return enhance(img, ("Color", "Contrast", "Brightness").index(name), val, report)


def augment_chain(x, ops_per_image):
    """augment_data_strong: x (b, 3, H, W) float32 in [0, 1] -> ToPILImage, the ops, ToTensor, Normalize, flip"""
    out = np.empty(x.shape, f32)
    for i in range(x.shape[0]):
        img = np.ascontiguousarray(to_u8(x[i]).transpose(1, 2, 0))
        for name, val in ops_per_image[i]:
            img = apply_op(img, name, val)
        out[i] = finish(img)
    return out


def magnitude_ops(m):
    """all seven ops once at RandAugment magnitude m: val = m / 30 * (max - min) + min"""
    return [(name, (float(m) / 30) * float(hi - lo) + lo) for name, lo, hi in AUGMENT_LIST]


# ================================================================================================ photometric.hip
def hue_shift(img, shift):
    from oracle import dupl_oracle as O
    return O.pil_hue_shift_np(img, shift)


def gaussian_blur(img, radius, report=None):
    from oracle import dupl_oracle as O
    if radius > 0:
        r = int(f32(O.pil_gaussian_box_radius(radius, 3)))
        _mark(report, "radius>=len", r >= min(img.shape[:2]))
    return O.pil_gaussian_blur_np(img, radius)


def grayscale(img):
    l = luma(img)
    return np.stack([l, l, l], -1)


# ================================================================================================ loader.hip
def _resample_axis1(img, out_size):
    """one pass of ImagingResample over axis 1 of (h, w, 3): 22-bit coefficients, (2^21 + sum) >> 22, clipped to uint8"""
    coef, bounds, _ = resample_coeffs(img.shape[1], out_size)
    out = np.empty((img.shape[0], out_size, 3), np.uint8)
    v = img.astype(np.int64)
    for x in range(out_size):
        x0, n = int(bounds[x, 0]), int(bounds[x, 1])
        acc = (v[:, x0:x0 + n] * coef[x, :n].astype(np.int64)[None, :, None]).sum(1) + (1 << 21)
        out[:, x] = np.clip(acc >> 22, 0, 255)
    return out


def resample_h(img, w2):
    return _resample_axis1(img, w2)


def resample_v(tmp, h2):
    return np.ascontiguousarray(_resample_axis1(tmp.transpose(1, 0, 2), h2).transpose(1, 0, 2))


def flip_pad_crop(img, flip, hp, wp, hs, ws, S, report=None):
    """transforms.random_fliplr -> random_crop(mean_rgb = 0): flip the image, put it at (hp, wp) of a zero canvas of
    max(S, h) x max(S, w), cut the S x S window that starts at (hs, ws)"""
    h, w = img.shape[:2]
    if flip:
        _mark(report, "flip")
        img = np.fliplr(img)
    H, W = max(S, h), max(S, w)
    assert 0 <= hp <= H - h and 0 <= wp <= W - w and 0 <= hs <= H - S and 0 <= ws <= W - S
    pad = np.zeros((H, W, 3), np.uint8)
    pad[hp:hp + h, wp:wp + w] = img
    _mark(report, "outside_top", hp - hs > 0)
    _mark(report, "outside_bottom", h + hp - hs < S)
    _mark(report, "outside_left", wp - ws > 0)
    _mark(report, "outside_right", w + wp - ws < S)
    return np.ascontiguousarray(pad[hs:hs + S, ws:ws + S])


def v_crop(tmp, h2, flip, hp, wp, hs, ws, S, report=None):
    return flip_pad_crop(resample_v(tmp, h2), flip, hp, wp, hs, ws, S, report)


def normalize_train(img):
    """T.ToTensor + T.Normalize: float32 ((v / 255) - mean) / std; (H, W, 3) -> (3, H, W)"""
    t = img.transpose(2, 0, 1).astype(f32) / f32(255)
    return np.ascontiguousarray((t - MEAN32[:, None, None]) / STD32[:, None, None])


def normalize_val(img):
    """transforms.normalize_img: (uint8 - python float) / python float in float64, rounded once into the float32 array"""
    out = np.empty((3,) + img.shape[:2], f32)
    for c in range(3):
        out[c] = (img[..., c].astype(f64) - MEAN64[c]) / STD64[c]
    return out


# ================================================================================================ contents and case lists
SMALL_SHAPES = ((1, 1), (1, 2), (2, 1), (1, 9), (9, 1), (2, 2), (3, 3), (3, 4), (16, 17), (23, 25), (40, 52), (129, 128))
CONTRAST_EXTRA_SHAPE = (181, 182)             # 32,942 pixels: 17 blocks of the luma-sum grid, the last one part full
CONTENTS = ("random", "quant4", "const_channel", "two_value", "zeros", "full", "dark_band")
FACTORS = (0.0, 0.1, 0.7, 1.0, 1.3, 1.9, float(np.float32(0.73219)))
POSTERIZE_BITS = (1, 4, 5, 8)
TIE_LUMAS = (0, 100, 127, 254)                # 1 x 2 planes with lumas k, k + 1: the mean is k + 0.5 exactly


def plane(H, W, content, seed=0):
    """(H, W, 3) uint8 test image"""
    rng = np.random.RandomState(1000 * H + 10 * W + seed)
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    if content == "random":
        pass
    elif content == "quant4":
        img = (img // 64 * 85).astype(np.uint8)
    elif content == "const_channel":
        img[..., 1] = 77
    elif content == "two_value":
        img[..., 0] = np.where(img[..., 0] < 128, 3, 250)
        img[..., 2] = np.where(img[..., 2] < 200, 254, 255)
    elif content == "zeros":
        img[:] = 0
    elif content == "full":
        img[:] = 255
    elif content == "dark_band":
        img[:max(1, H // 3)] //= 8
    else:
        raise ValueError(content)
    return img


def tie_plane(k):
    """1 x 2 grey plane with lumas k and k + 1 (a grey pixel's luma is its value)"""
    return np.asarray([[[k, k, k], [k + 1, k + 1, k + 1]]], np.uint8)


SMALL_PLANES = tuple((H, W, c) for (H, W) in SMALL_SHAPES for c in CONTENTS)
# equalize needs H * W - h[hi] >= 255 before its LUT can pass 255: four more planes just above that, so that a quarter of its cases clip
LUT_EXTRA_SHAPES = ((16, 16), (15, 18), (31, 33), (64, 5))
LUT_PLANES = SMALL_PLANES + tuple((H, W, c) for (H, W) in LUT_EXTRA_SHAPES for c in CONTENTS)

# second trips of the grid-stride loops: (name, H, W) with random content
TRIP_LUT = (1025, 1024)
TRIP_SHARP = (592, 591)
TRIP_PHOTO = (725, 724)
TRIP_BLUR = (419, 418, 1.0)
TRIP_N = 1048576 + 257

BLUR_RADII = (0.1, 0.5, 1.0, 2.0, 3.7, 9.3, 40.0, 300.0)
BLUR_SHAPES = ((1, 1), (1, 2), (2, 1), (1, 64), (64, 1), (3, 3), (2, 300), (7, 5))
BLUR_CASES = tuple((H, W, r) for (H, W) in BLUR_SHAPES for r in BLUR_RADII)

HUE_CASES = tuple((n, s) for n in (1, 63, 64, 65, 257) for s in (0, 1, 128, 255))

FINISH_WIDTHS = (1, 2, 7, 8)
NORMALIZE_SHAPES = ((16, 16), (1, 255), (257, 1), (1, 1))

RESAMPLE_H_CASES = ((1, 1, 1), (1, 1, 2), (1, 5, 9), (5, 1, 1), (3, 500, 250), (257, 3, 1), (7, 9, 18), (7, 9, 9), (33, 47, 94),
                    (33, 47, 23))

VCROP_TMP_SHAPES = ((1, 1), (5, 1), (9, 17), (33, 47), (17, 9))     # (17, 9): the only one with w2 < S < h2 for an S of the list
VCROP_S = (1, 15, 16, 17, 33)


def all_bytes_plane(H, W):
    """(H, W, 3) holding every byte value in every channel (H * W >= 256), in a different order per channel"""
    n = H * W
    assert n >= 256
    base = np.arange(n) % 256
    return np.stack([base, (base * 7 + 3) % 256, 255 - base], -1).astype(np.uint8).reshape(H, W, 3)


def finish_plane(W):
    return all_bytes_plane(-(-256 // W), W)


def normalize_plane(H, W):
    return all_bytes_plane(H, W) if H * W >= 256 else plane(H, W, "random", seed=5)


def to_u8_inputs():
    """the 256 lattice values k / 255 as float32, their float32 neighbours inside [0, 1], 0.0 and 1.0"""
    lat = (np.arange(256, dtype=f32) / f32(255)).astype(f32)
    x = np.concatenate([lat, np.nextafter(lat, f32(-1)), np.nextafter(lat, f32(2)), np.asarray([0.0, 1.0], f32)]).astype(f32)
    return x[(x >= 0) & (x <= 1)]


def _axis_offsets(size, S):
    """(pad, start) pairs an axis can take: random_crop pads when the image is smaller than the crop and cuts when it is larger"""
    if size < S:
        return [(0, 0), (S - size, 0)]
    if size > S:
        return [(0, 0), (0, size - S)]
    return [(0, 0)]


def vcrop_cases(h, w2):
    """(h2, S, flip, hp, wp, hs, ws) for a tmp plane (h, w2, 3): every h2 of {1, h // 2, h, 2 h + 1}, every S, both flips, each axis
    flush with either border"""
    out = []
    for h2 in sorted({v for v in (1, h // 2, h, 2 * h + 1) if v >= 1}):
        for S in VCROP_S:
            for (hp, hs), (wp, ws) in itertools.product(_axis_offsets(h2, S), _axis_offsets(w2, S)):
                for flip in (0, 1):
                    out.append((h2, S, flip, hp, wp, hs, ws))
    return out


def byte_image(h, w):
    """uniform random (h, w, 3) uint8: the resample passes' input"""
    return np.random.RandomState(31 * h + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


CHAIN_MAGNITUDES = (0, 20, 30)
CHAIN_BATCHES = ((2, 23, 25), (1, 40, 52))


def chain_input(b, H, W):
    """(b, 3, H, W) float32 in [0, 1], off the k / 255 lattice so that ToPILImage's truncation matters"""
    return np.random.RandomState(b * 100 + H).random_sample((b, 3, H, W)).astype(f32)


assert TRIP_N > 4096 * 256 and 3 * TRIP_SHARP[0] * TRIP_SHARP[1] > 4096 * 256 and TRIP_LUT[0] * TRIP_LUT[1] > 4096 * 256
assert TRIP_PHOTO[0] * TRIP_PHOTO[1] > 2048 * 256 and 3 * TRIP_BLUR[0] * TRIP_BLUR[1] > 2048 * 256
assert TRIP_LUT[0] * TRIP_LUT[1] > 64 * 256 * 16 and TRIP_PHOTO[0] * TRIP_PHOTO[1] > 128 * 256 * 8     # histogram / luma-sum grids capped
