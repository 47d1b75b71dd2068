"""numpy / scipy reference of csrc/regions.hip: connected regions of a label map in canonical numbering, their table and per-label
statistics, and the single-pass absorption of small regions -- plus the cases the host and GPU suites share.

  label_ref      scipy.ndimage.label per class present, the components sorted by their first raster index;
  flood_ref      the same labelling by a plain flood fill, without scipy (the cross-check of label_ref, and the fallback where
                 scipy is missing);
  clean_ref      the cleaning pass of include/dupl_hip.h (dupl_seg_regions_clean), in plain numpy.
Everything is integer: every comparison against these is exact equality."""
import functools

import numpy as np

try:
    from scipy import ndimage
except ImportError:                      # the flood fill below is the reference then
    ndimage = None

IGNORE = 255
COLS = 8                                 # class, area, y0, x0, y1, x1, conf_sum, first_index

SHAPES = ((1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (97, 131), (375, 500))
ODD_ADDRESS = (97, 131)                  # this shape's label sits on an odd byte address in the GPU suite
PATTERNS = ("uniform", "all_ignore", "random3", "random21_ignore", "checker", "serpentine", "comb", "rings", "diag", "blobs")
CLASSES = {"uniform": 2, "all_ignore": 2, "random3": 3, "random21_ignore": 21, "checker": 2, "serpentine": 2, "comb": 4, "rings": 3,
           "diag": 2, "blobs": 21}
CASES = [(s, p, CLASSES[p]) for s in SHAPES for p in PATTERNS]


def case_id(case):
    return f"{case[0][0]}x{case[0][1]}-{case[1]}"


def smooth_labels(rng, classes, H, W, cell=24):
    """argmax over `classes` bilinearly interpolated coarse random fields: blobs of about `cell` pixels"""
    gh, gw = H // cell + 2, W // cell + 2
    g = rng.standard_normal((classes, gh, gw)).astype(np.float32)
    ys, xs = np.arange(H, dtype=np.float32) / cell, np.arange(W, dtype=np.float32) / cell
    y0, x0 = ys.astype(np.int64), xs.astype(np.int64)
    fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
    top = g[:, y0][:, :, x0] * (1 - fx) + g[:, y0][:, :, x0 + 1] * fx
    bot = g[:, y0 + 1][:, :, x0] * (1 - fx) + g[:, y0 + 1][:, :, x0 + 1] * fx
    return (top * (1 - fy) + bot * fy).argmax(0).astype(np.uint8)


def pattern(name, H, W, classes):
    """the (H,W) uint8 label map of one pattern; seeded, the same on every machine"""
    rng = np.random.RandomState(1000 + 7 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "uniform":
        return np.full((H, W), 1, np.uint8)
    if name == "all_ignore":
        return np.full((H, W), IGNORE, np.uint8)
    if name == "random3":
        return rng.randint(0, 3, size=(H, W)).astype(np.uint8)
    if name == "random21_ignore":
        lab = rng.randint(0, 21, size=(H, W)).astype(np.uint8)
        lab[rng.random_sample((H, W)) < 0.05] = IGNORE
        return lab
    if name == "checker":
        return ((yy + xx) & 1).astype(np.uint8)
    if name == "serpentine":                       # full rows every other line, joined at alternating ends: one winding path
        lab = np.zeros((H, W), np.uint8)
        lab[0::2] = 1
        odd = np.arange(1, H, 2)
        lab[odd, np.where((odd // 2) % 2 == 0, W - 1, 0)] = 1
        return lab
    if name == "comb":                             # teeth that meet only at the far end: vertical ones on the left, horizontal on the right
        lab = np.zeros((H, W), np.uint8)
        half = W // 2
        left = (xx < half) & (((xx % 4 == 0) & (yy < H - 1)) | (yy == H - 1))
        right = (xx > half) & (((yy % 4 == 2) & (xx < W - 1)) | (xx == W - 1))
        lab[left] = 2
        lab[right] = 3
        return lab
    if name == "rings":
        return (np.minimum(np.minimum(yy, xx), np.minimum(H - 1 - yy, W - 1 - xx)) % 2 + 1).astype(np.uint8)
    if name == "diag":
        return (yy == xx).astype(np.uint8)
    if name == "blobs":
        lab = smooth_labels(rng, classes, H, W)
        speck = rng.random_sample((H, W)) < 0.005
        lab[speck] = rng.randint(0, classes, size=(H, W)).astype(np.uint8)[speck]
        return lab
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(shape, name, classes):
    """(label (H,W) uint8, conf (H,W) fp32 in (0, 1]) of one of CASES, computed once per session and shared; treat as read-only."""
    H, W = shape
    lab = pattern(name, H, W, classes)
    conf = (1.0 - np.random.RandomState(77 + H + 3 * W).random_sample((H, W))).astype(np.float32)
    lab.setflags(write=False)
    conf.setflags(write=False)
    return lab, conf


def _canonical(prov, lab, conf, classes):
    """prov (H,W) int64: 0 on ignored pixels, otherwise any positive component id -> (region, n, table, stats)"""
    H, W = lab.shape
    flat = prov.ravel()
    idx = np.nonzero(flat)[0]
    region = np.full(H * W, -1, np.int64)
    if len(idx):
        ids, first = np.unique(flat[idx], return_index=True)        # first occurrence = first pixel in raster order
        first = idx[first]
        order = np.argsort(first, kind="stable")
        remap = np.zeros(int(flat.max()) + 1, np.int64)
        remap[ids[order]] = np.arange(len(ids))
        region[idx] = remap[flat[idx]]
        first = first[order]
    else:
        first = np.zeros(0, np.int64)
    n = len(first)
    q = np.zeros(H * W, np.int64) if conf is None else np.rint(conf.astype(np.float32).ravel() * np.float32(1 << 24)).astype(np.int64)
    table = np.zeros((n, COLS), np.int64)
    r, ys, xs = region[idx], idx // W, idx % W
    table[:, 0] = lab.ravel()[first]
    table[:, 1] = np.bincount(r, minlength=n)
    table[:, 2], table[:, 3] = H, W
    np.minimum.at(table[:, 2], r, ys)
    np.minimum.at(table[:, 3], r, xs)
    np.maximum.at(table[:, 4], r, ys)
    np.maximum.at(table[:, 5], r, xs)
    np.add.at(table[:, 6], r, q[idx])
    table[:, 7] = first
    stats = np.zeros((2, classes + 1), np.int64)
    slot = np.where(region >= 0, lab.ravel().astype(np.int64), classes)
    stats[0] = np.bincount(slot, minlength=classes + 1)
    np.add.at(stats[1], slot, q)
    return region.reshape(H, W), n, table, stats


def _valid(lab, classes, ignore_index):
    return (lab != ignore_index) & (lab < classes)


def label_ref(lab, connectivity, classes, conf=None, ignore_index=IGNORE):
    """scipy.ndimage.label per class present -> (region (H,W) int64 with -1 on ignored pixels, n, table (n, 8), stats (2, classes+1))"""
    if ndimage is None:
        return flood_ref(lab, connectivity, classes, conf, ignore_index)
    structure = np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    prov = np.zeros(lab.shape, np.int64)
    offset = 0
    for c in np.unique(lab[_valid(lab, classes, ignore_index)]):
        m, k = ndimage.label(lab == c, structure)
        prov[m > 0] = m[m > 0] + offset
        offset += k
    return _canonical(prov, lab, conf, classes)


def flood_ref(lab, connectivity, classes, conf=None, ignore_index=IGNORE):
    """label_ref without scipy: a flood fill from every unlabelled pixel in raster order"""
    H, W = lab.shape
    steps = [(-1, 0), (0, -1), (0, 1), (1, 0)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    valid = _valid(lab, classes, ignore_index)
    prov = np.zeros((H, W), np.int64)
    n = 0
    for y in range(H):
        for x in range(W):
            if not valid[y, x] or prov[y, x]:
                continue
            n += 1
            prov[y, x] = n
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for dy, dx in steps:
                    qy, qx = cy + dy, cx + dx
                    if 0 <= qy < H and 0 <= qx < W and not prov[qy, qx] and valid[qy, qx] and lab[qy, qx] == lab[y, x]:
                        prov[qy, qx] = n
                        stack.append((qy, qx))
    return _canonical(prov, lab, conf, classes)


def clean_ref(lab, min_area, connectivity, classes, ignore_index=IGNORE, max_regions=None):
    """The cleaning pass: (label_out, changed = [regions relabelled, pixels relabelled]).  A region is kept when area >= min_area;
    a small region takes the class most of its (pixel, 4-neighbour in a kept region) pairs vote for, first maximum wins, no vote:
    unchanged; decided entirely on the input map.  Small regions with id >= max_regions stay."""
    region, n, table, _ = label_ref(lab, connectivity, classes, None, ignore_index)
    H, W = lab.shape
    kept = table[:, 1] >= min_area
    votes = np.zeros((n, classes), np.int64)
    for p, q in (((slice(1, H), slice(0, W)), (slice(0, H - 1), slice(0, W))), ((slice(0, H - 1), slice(0, W)), (slice(1, H), slice(0, W))),
                 ((slice(0, H), slice(1, W)), (slice(0, H), slice(0, W - 1))), ((slice(0, H), slice(0, W - 1)), (slice(0, H), slice(1, W)))):
        rp, rq, lq = region[p].ravel(), region[q].ravel(), lab[q].ravel()
        both = (rp >= 0) & (rq >= 0)
        rp, rq, lq = rp[both], rq[both], lq[both]
        m = ~kept[rp] & kept[rq]
        np.add.at(votes, (rp[m], lq[m].astype(np.int64)), 1)
    small = ~kept
    if max_regions is not None:
        small[max_regions:] = False
    moved = small & (votes.max(1) > 0) if n else np.zeros(0, bool)
    newcls = np.where(moved, votes.argmax(1) if n else 0, table[:, 0])
    out = lab.copy()
    inside = region >= 0
    out[inside] = newcls[region[inside]].astype(np.uint8)
    return out, np.array([int(moved.sum()), int(table[moved, 1].sum())], np.int64)
