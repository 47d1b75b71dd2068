"""Brute-force reference of the DenseCRF mean-field update (a helper, not a test): the formulas of the Krähenbühl & Koltun
update exactly as pydensecrf.DenseCRF2D sets it up for utils/dcrf.py (Potts compatibility, DIAG_KERNEL, NORMALIZE_SYMMETRIC),
evaluated in torch on the host with the N x N kernel materialised -- in float64 as the reference, in float32 as the yardstick
of what "fp32-equivalent" means for the device code.

    k(i,j)   = exp(-|f_i - f_j|^2 / 2) over ALL j (j = i included); Gaussian f = (x, y) / sxy,
               bilateral f = (x/sxy, y/sxy, r/srgb, g/srgb, b/srgb); pixels row-major, i = y W + x
    n_i      = 1 / sqrt(sum_j k(i,j) + 1e-20)
    M(Q)[c,i] = n_i sum_j k(i,j) n_j Q[c,j]
    Q^0 = softmax_c(-U);  Q <- softmax_c(-U + w_g M_g(Q) + w_b M_b(Q)),  T times
"""
import math

import torch

# (w_g, sxy_g, w_b, sxy_b, srgb_b): `eval` = DenseCRF(10, 1, 1, 4, 121, 5) of tools/eval_seg_voc.py:104-111, `helper` =
# crf_inference of utils/dcrf.py:20-21
PARAMS = {"eval": dict(w_g=1.0, sxy_g=1.0, w_b=4.0, sxy_b=121.0, srgb_b=5.0),
          "helper": dict(w_g=3.0, sxy_g=3.0, w_b=10.0, sxy_b=80.0, srgb_b=13.0)}
CASES = ((48, 64, 21), (61, 83, 21), (40, 56, 81))          # (H, W, C) of the dense_crf checks
EPS32 = 2.0 ** -24                                          # half an ulp: what rounding the exact result to fp32 costs
MARGIN = 1e-4                                               # fp64 top-2 margin under which an argmax may differ
TIE_SHARE = 2e-3                                            # cap on the share of such pixels per case (device result)
REF_TIE_SHARE = 9e-4                                        # what the fp64 reference alone stays under (tests/test_crf_host.py)


def case_seed(H, W):
    return H * 1000 + W + 1


def features(H, W, img, sxy, srgb, dtype):
    """(N, 2) or (N, 5) feature vectors; img (H,W,3) uint8 or None."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    f = [xs.reshape(-1).to(dtype) / sxy, ys.reshape(-1).to(dtype) / sxy]
    if img is not None:
        f += [img[..., k].reshape(-1).to(dtype) / srgb for k in range(3)]
    return torch.stack(f, 1)


def kernel_rows(f, rows=None):
    """k(i, j) for i in rows (all rows when None) and every j: (R, N)."""
    fi = f if rows is None else f[rows]
    d2 = torch.zeros((fi.shape[0], f.shape[0]), dtype=f.dtype)
    for d in range(f.shape[1]):
        d2 += (fi[:, d, None] - f[None, :, d]) ** 2
    return torch.exp(-0.5 * d2)


def norm_of(K):
    return 1.0 / torch.sqrt(K.sum(1) + 1e-20)


def message(K, Q, n=None):
    """M(Q) (C,N) for the full kernel matrix K (N,N) and Q (C,N); n None = no normalisation."""
    if n is None:
        return Q @ K.T
    return ((Q * n[None, :]) @ K.T) * n[None, :]


def message_rows(f, Q, rows, n=None, chunk=64):
    """M(Q)[:, rows] without materialising K: (C, R).  n (N,) = the normaliser of every pixel, or None."""
    out = []
    Qn = Q if n is None else Q * n[None, :]
    for r0 in range(0, len(rows), chunk):
        r = rows[r0:r0 + chunk]
        m = Qn @ kernel_rows(f, r).T
        out.append(m if n is None else m * n[r][None, :])
    return torch.cat(out, 1)


def rowsum_rows(f, rows, chunk=64):
    return torch.cat([kernel_rows(f, rows[r0:r0 + chunk]).sum(1) for r0 in range(0, len(rows), chunk)])


def mean_field(img, U, T, w_g, sxy_g, w_b, sxy_b, srgb_b, dtype=torch.float64):
    """Q (C,H,W) after T iterations; U (C,H,W), img (H,W,3) uint8."""
    C, H, W = U.shape
    U = U.reshape(C, -1).to(dtype)
    Kg = kernel_rows(features(H, W, None, sxy_g, 1.0, dtype))
    Kb = kernel_rows(features(H, W, img, sxy_b, srgb_b, dtype))
    ng, nb = norm_of(Kg), norm_of(Kb)
    Q = torch.softmax(-U, 0)
    for _ in range(T):
        Q = torch.softmax(-U + w_g * message(Kg, Q, ng) + w_b * message(Kb, Q, nb), 0)
    return Q.reshape(C, H, W)


def unary_from_softmax(p):
    return -torch.log(p.clamp(1e-5, 1.0)).float()


def unary_from_labels(labels, n, gt_prob):
    H, W = labels.shape
    U = torch.full((n, H * W), -math.log((1.0 - gt_prob) / (n - 1)), dtype=torch.float32)
    U[labels.reshape(-1), torch.arange(H * W)] = -math.log(gt_prob)
    return U.reshape(n, H, W)


def make_case(H, W, C, seed, n_sites=7):
    """Seeded input: a Voronoi-region colour image plus noise (H,W,3) uint8, the region labels (H,W), and logits (C,H,W) equal to
    2.5 x the one-hot of the labels shifted by 2 px plus unit Gaussian noise (so the raw argmax is wrong along every region
    border and at scattered pixels, and the CRF has something to repair)."""
    g = torch.Generator().manual_seed(seed)
    sy, sx = torch.rand(n_sites, generator=g) * H, torch.rand(n_sites, generator=g) * W
    site_label = torch.randint(0, C, (n_sites,), generator=g)
    site_colour = torch.randint(20, 236, (n_sites, 3), generator=g).double()
    ys, xs = torch.meshgrid(torch.arange(H).double(), torch.arange(W).double(), indexing="ij")
    region = ((ys[..., None] - sy.double()) ** 2 + (xs[..., None] - sx.double()) ** 2).argmin(-1)
    img = (site_colour[region] + 3.0 * torch.randn((H, W, 3), generator=g).double()).round().clamp(0, 255).to(torch.uint8)
    labels = site_label[region]
    shifted = torch.roll(labels, (2, 2), (0, 1))
    logits = 2.5 * torch.nn.functional.one_hot(shifted, C).permute(2, 0, 1).float() + torch.randn((C, H, W), generator=g)
    return img, labels, logits


def row_rel_err(a, ref):
    """Largest error of a pixel's row of C values relative to that row's fp64 value (its largest entry): a, ref (C, R)."""
    a, ref = a.double().reshape(ref.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    return float(((a - ref).abs().amax(0) / ref.abs().amax(0)).max())


def rel_err(a, ref):
    return float(((a.double() - ref.double()).abs() / ref.double().abs()).max())


def top2_margin(Q):
    t = Q.topk(2, dim=0).values
    return t[0] - t[1]


# ---------------------------------------------------------------------------- helpers of tests/test_crf_edges_gpu.py
# (H, W) whose pixel counts sit on, one short of and one past the sizes of the device tiling: 32 (an MFMA tile), 64 (a wave's
# queries), 128 (a key tile, a row-sum half block), 256 (a query block), 512
SEAM_SHAPES = ((31, 1), (4, 8), (3, 11), (7, 9), (5, 13), (1, 127), (128, 1), (3, 43), (15, 17), (16, 16), (1, 257), (7, 73), (19, 27))
SEAM_N = (31, 32, 33, 63, 65, 127, 128, 129, 255, 256, 257, 511, 513)
CHUNK_C = (1, 31, 32, 33, 64, 65)                           # around the 32-channel chunk of the dense kernel
# dense_crf with a zero weight: (H, W, C) x (w_g, w_b), the other parameters those of PARAMS["eval"].  The seed is chosen so
# that NO pixel of the fp64 result has a top-2 margin under MARGIN (600 pixels: REF_TIE_SHARE admits none).
BRANCH_CASES = ((20, 30, 21), (20, 30, 33))
BRANCH_WEIGHTS = ((0.0, 4.0), (1.0, 0.0), (0.0, 0.0))
BRANCH_T = 10
EXTREME_STD = (1e-25, 1e-19, 1e-3, 1e6, 3e38)


def branch_seed(H, W, C):
    return case_seed(H, W) + C + 500


def gauss_radius(sxy):
    """The radius of the truncated Gaussian window as csrc/crf.hip documents it (crf_gauss_radius): the mass outside a disc of
    radius R, 2 pi s^2 exp(-R^2 / 2 s^2), is below 2^-32, i.e. R = ceil(s sqrt(2 (ln(2 pi s^2 + 1) + 32 ln 2))), capped at 10^6."""
    s = float(sxy)
    r = s * math.sqrt(2.0 * (math.log(2.0 * math.pi * s * s + 1.0) + 32.0 * math.log(2.0)))
    return 1000000 if r > 1.0e6 else int(math.ceil(r))


def gauss_takes_stencil(H, W, sxy):
    """Whether the Gaussian kernel runs as the truncated stencil: only when its square window is smaller than the image."""
    win = 2 * gauss_radius(sxy) + 1
    return win * win < H * W


def wide_range_q(C, H, W, seed, scale=25.0):
    """Q (C, H*W) fp32 = softmax over the channels of `scale` x unit Gaussian logits, evaluated in fp64 and rounded: the entries
    span from 1 down to the fp32 denormals (and to 0 below them); channel 1 is exactly 0 everywhere."""
    g = torch.Generator().manual_seed(seed)
    z = scale * torch.randn((C, H * W), generator=g, dtype=torch.float64)
    z[1] = -math.inf
    return torch.softmax(z, 0).float()


def decades(Q):
    """log10 of the ratio of the largest to the smallest positive entry."""
    pos = Q[Q > 0].double()
    return float(torch.log10(pos.max() / pos.min()))


def ulp_distance(a, b):
    """Number of fp32 values between a and b, elementwise (+0 and -0 are the same value); a, b finite fp32."""
    def order(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (order(a.float()) - order(b.float())).abs()


def unary_exact(p):
    """-log(clip(p, 1e-5f, 1)) of fp32 p: the clip in fp32 as the device does it (exact), the logarithm in fp64, rounded once."""
    return (-torch.log(p.float().clamp(1e-5, 1.0).double())).float()


def unary_from_logits(z, dtype=torch.float64):
    """-log(clip(softmax_c(z), 1e-5, 1)) with everything in `dtype`; z (C, N)."""
    return -torch.log(torch.softmax(z.to(dtype), 0).clamp(1e-5, 1.0))


def unary_from_any_labels(labels, n, gt_prob):
    """unary_from_labels for labels that may lie outside [0, n): such a pixel gets the "other" energy in every channel."""
    e_gt, e_other = -math.log(gt_prob), -math.log((1.0 - gt_prob) / (n - 1))
    hit = labels.reshape(1, -1) == torch.arange(n).reshape(-1, 1)
    return torch.where(hit, torch.tensor(e_gt, dtype=torch.float32), torch.tensor(e_other, dtype=torch.float32))
