"""numpy / float64 references of the label-less inference kernels (a helper, not a test), written from the definitions in
include/dupl_hip.h: dupl_seg_decide, dupl_seg_paint, dupl_window_gather / dupl_window_merge; and the uint8 guarded buffer the GPU
suite needs (kernel_guard.Guard has no uint8 sentinel).  Shared by tests/test_predict_host.py and tests/test_predict_gpu.py."""
import functools

import numpy as np
import torch

import kernel_guard as KG
import seg_ensemble_ref as ER

SHAPES = ER.SHAPES
Q24 = float(1 << 24)

PAINT_SHAPES = ((1, 1), (5, 3), (37, 53), (64, 257))
PAINT_ALPHAS = (0, 128, 154, 256)
# (C, canvas (hs, ws), window tokens, stride tokens)
MERGE_CASES = tuple((C, hw, win, st) for C in (5, 21) for hw in ((4, 6), (7, 9)) for win in (2, 3) for st in (1, 2))
PLAN_CASES = ((1, 28, 20), (28, 28, 20), (29, 28, 20), (64, 28, 20), (57, 28, 28), (100, 28, 16))


class U8Guard:
    """A uint8 tensor of `shape` inside a larger device allocation whose slack holds 0xA5; `front` bytes in front (an odd number
    puts the tensor on an odd address: the packed stores' unaligned head)."""
    PAT = 0xA5

    def __init__(self, shape, dev, init=None, front=67, back=61):
        self.n = int(np.prod(shape))
        self.front, self.back = front, back
        self.buf = torch.full((self.n + front + back,), self.PAT, dtype=torch.uint8, device=dev)
        self.view = self.buf[front:front + self.n].view(shape)
        if init is not None:
            self.view.copy_(torch.as_tensor(init))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:self.front] == self.PAT).all()) and bool((b[self.front + self.n:] == self.PAT).all())

    def untouched(self):
        return bool((self.buf.cpu() == self.PAT).all())

    def cpu(self):
        torch.cuda.synchronize()
        assert self.intact(), "the kernel wrote outside its uint8 output"
        return self.view.cpu()


# ------------------------------------------------------------------------------------------------------------------ seg_decide
def decide64(a, b, H, W, is_prob=False):
    """a, b (C,h,w) (b may be None) -> (winner (H,W) int64, conf (H,W) float64, margin (H,W) = top-1 - top-2 of what the winner is
    taken from): one student the argmax of the up-sampled logits and its softmax value, two students the argmax of the mean
    probability vector and its value, is_prob the values (their mean) themselves."""
    if is_prob:
        v = np.asarray(a, dtype=np.float64) if b is None else 0.5 * (np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64))
        rank, prob = v, v
    elif b is None:
        u = ER.upsample64(a, H, W)
        rank, prob = u, ER.softmax64(u)
    else:
        e = 0.5 * (ER.softmax64(ER.upsample64(a, H, W)) + ER.softmax64(ER.upsample64(b, H, W)))
        rank, prob = e, e
    win = rank.argmax(0)
    conf = np.take_along_axis(prob, win[None], 0)[0]
    if rank.shape[0] > 1:
        top = np.sort(rank, axis=0)[-2:]
        margin = top[1] - top[0]
    else:
        margin = np.full(win.shape, np.inf)
    return win, conf, margin


@functools.lru_cache(maxsize=None)
def decide_case(shape, two):
    """float64 winner / conf of one of SHAPES on seg_ensemble_ref's inputs, computed once and shared; read-only."""
    C, h, w, H, W = shape
    a, b, _, _ = ER.case(shape)
    return decide64(a[0].numpy(), b[0].numpy() if two else None, H, W)


def labels_of(winner, conf32, min_conf, ignore_index):
    """label = ignore_index where the fp32 conf < min_conf (compared in fp32), else the winner."""
    rej = np.asarray(conf32, dtype=np.float32) < np.float32(min_conf)
    return np.where(rej, ignore_index, winner).astype(np.uint8), rej


def stats_ref(winner, conf32, rej, C):
    """(2, C+1) int64: pixels per output label with slot C for the rejected, and the sums of rint(conf * 2^24) (fp32 product: exact;
    np.rint rounds halves to even like rintf)."""
    slot = np.where(rej, C, winner).astype(np.int64).ravel()
    q = np.rint(np.asarray(conf32, dtype=np.float32) * np.float32(Q24)).astype(np.int64).ravel()
    out = np.zeros((2, C + 1), dtype=np.int64)
    np.add.at(out[0], slot, 1)
    np.add.at(out[1], slot, q)
    return out


# ------------------------------------------------------------------------------------------------------------------- seg_paint
def paint_inputs(H, W, seed=0):
    """label (H,W) uint8 with regions, single pixels and the values 0 and 255; image (H,W,3) uint8."""
    g = np.random.RandomState(100 + seed + 7 * H + W)
    label = g.randint(0, 4, size=((H + 3) // 4, (W + 5) // 6)).astype(np.uint8).repeat(4, 0).repeat(6, 1)[:H, :W].copy()
    speck = g.rand(H, W)
    label[speck < 0.05] = 255
    label[(speck >= 0.05) & (speck < 0.1)] = 20
    label[(speck >= 0.1) & (speck < 0.12)] = 254
    image = g.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    return label, image


def contour_mask(label):
    lab = np.asarray(label)
    m = np.zeros(lab.shape, dtype=bool)
    m[:, :-1] |= lab[:, :-1] != lab[:, 1:]
    m[:-1, :] |= lab[:-1, :] != lab[1:, :]
    return m


def paint_ref(label, palette, image=None, alpha256=154, tint_background=False, contour=False, contour_rgb=(255, 255, 255)):
    """(H,W,3) uint8, integers only: the definition of dupl_seg_paint."""
    lab = np.asarray(label)
    pal = np.asarray(palette, dtype=np.int64)[lab]
    if image is None:
        out = pal
    else:
        img = np.asarray(image, dtype=np.int64)
        out = (img * (256 - alpha256) + pal * alpha256 + 128) >> 8
        if not tint_background:
            out = np.where((lab == 0)[..., None], img, out)
    if contour:
        out = np.where(contour_mask(lab)[..., None], np.asarray(contour_rgb, dtype=np.int64)[None, None], out)
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- sliding windows
def grid_origins(hs, ws, win, stride):
    """the windows tools/predict plans on a (hs,ws) token grid, row-major"""
    from dupl_amd.tools.predict import plan_windows
    return [(r, c) for r in plan_windows(hs, win, stride) for c in plan_windows(ws, win, stride)]


def merge_ref(logits, origins, hs, ws):
    """logits (2 nW, C, wth, wtw) fp32 -> canvas (2, C, hs, ws) fp32: the windows added in ascending index in fp32 starting from 0,
    one fp32 division by the count; uncovered elements are 0."""
    lg = np.asarray(logits, dtype=np.float32)
    nW = len(origins)
    assert lg.shape[0] == 2 * nW
    _, C, wth, wtw = lg.shape
    acc = np.zeros((2, C, hs, ws), dtype=np.float32)
    cnt = np.zeros((hs, ws), dtype=np.int32)
    for k, (r0, c0) in enumerate(origins):
        for f in range(2):
            acc[f, :, r0:r0 + wth, c0:c0 + wtw] = acc[f, :, r0:r0 + wth, c0:c0 + wtw] + lg[f * nW + k]
        cnt[r0:r0 + wth, c0:c0 + wtw] += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        out = acc / cnt.astype(np.float32)[None, None]
    out[:, :, cnt == 0] = 0.0
    return out.astype(np.float32)


def merge_inputs(C, hs, ws, win, stride, seed=3):
    org = grid_origins(hs, ws, win, stride)
    wth, wtw = min(hs, win), min(ws, win)
    return KG.rnd(2 * len(org), C, wth, wtw, seed=seed + C + hs, scale=3.0), org
