"""Micro-timings of the small (non-GEMM) kernels of the step at their step shapes, through dupl_amd.ops (torch events on the
current stream, 200 launches each).  Usage: python tools/op_bench.py [ln_bwd] [ln_fwd] [split] [attn_bwd] [crf] [cam_eval] [seg_ensemble] | backbone | nograd | seg_render | predict | crf_lattice | regions | boundary | calibration
`crf` (only when named: it runs for seconds) times DenseCRF(10, 1, 1, 4, 121, 5) and its launches at 375x500x21 and 480x640x81.
`cam_eval` (only when named) times the fused tail of tools/infer_cam (ops.cam_eval) against the composed path it replaces.
`seg_ensemble` (only when named) times the fused ensemble tail of tools/eval_seg --ensemble 1 (ops.seg_ensemble) against the composition
of existing ops that yields the same matrices, at the VOC and the COCO form.
`crf_lattice` (only when named; then nothing else runs) times DenseCRF(10, 1, 1, 4, 121, 5) exact and on the permutohedral lattice,
alternating in one process, at 375x500x21 and 480x640x81 (construction and iterations apart; a uniform-colour and a noise image too).
`seg_render` (only when named; then nothing else runs) times ops.seg_decide against the composition of existing ops that yields the
same label and confidence (VOC and COCO form, one and two students) and ops.seg_paint against the host palette-and-blend.
`regions` (only when named; then nothing else runs) times ops.seg_regions and ops.seg_regions_clean (min_area 64) against the host path
(label.cpu() -> scipy.ndimage.label per class -> find_objects -> bincount) on a VOC-sized and a 1024 x 2048 prediction-like map and on
a 1024 x 2048 single-label map, after asserting that ids, areas and boxes agree.
`boundary` (only when named; then nothing else runs) times ops.seg_boundary (band histogram + Boundary IoU counters, R = 32) at 375x500x21
and 480x640x81 against ops.confusion_accum on the same maps (what eval_seg --boundary 1 adds per image and column), against the host
path (.cpu() -> the scipy filters and erosions of tests/boundary_ref.py, equality asserted first) and against the 16 B/px of reading the
two int64 maps once; its three kernels are timed apart through a second call that stops after each of them.
`calibration` (only when named; then nothing else runs) times ops.seg_calibration (all three counter tables, 15 bins) at the VOC form
(375x500x21, identity) and the COCO form (480x640x81 from 28x28), one and two students, at T = 1 and at 14 temperatures, against the
composition that yields the same counters -- scale_ -> seg_decide -> read-back -> numpy bincount, once per temperature, equality asserted
first -- and against its two floors: the bytes read once, and the v_exp_f32 instructions of the soft-max.
`predict` (only when named; then nothing else runs) times tools/predict on one synthetic 1024 x 2048 image, ViT-B, whole image against
sliding windows, with the peak device memory of each.
`backbone` (only when named; then nothing else runs) times one phase-B training step at VOC 448^2, 4 images, two student streams
for every registered --backbone, or for the names that follow it: bench.py's own workload and timed region (bench.Workload.measure:
warm-up steps, then K steps between synchronisations), so the deit_base_patch16_224 row is bench.py's figure.
    python tools/op_bench.py backbone [name ...] [steps=20] [warmup=5]
`nograd` (only when named; then nothing else runs) times the merged no-grad ms-CAM pass of one ViT-B student at the bench shape
(engine.cam_logits_multi on 8 x 224^2 + 8 x 672^2: the 0.5x and 1.5x scales of 4 images at 448^2, flipped copies included) in both
modes of engine.set_nograd_gemm_mode, interleaved in one process, and prints what the single-product mode changes in the result:
the max-abs difference of the normalised multi-scale CAMs and the number of cam_to_label pixels that differ, 448^2, 4 images,
seeded synthetic batch and seeded random weights (no pretrained checkpoint: the accuracy on trained weights is not measured)."""
import gc
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from dupl_amd import ops  # noqa: E402


def timeit(fn, n=200, warm=20):
    gc.collect()            # a generation-2 collection inside the timed loop shows up as a 40 ms outlier
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def crf_bench(dev, g):
    """The full 10-iteration CRF of eval_seg --crf 1, one bilateral message launch, one Gaussian (stencil) launch, the two
    normaliser launches and the fused softmax, per image size.  pairs/s = N^2 / (time of one bilateral launch)."""
    for H, W, C in ((375, 500, 21), (480, 640, 81)):
        N = H * W
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        Q = torch.softmax(torch.randn(C, H, W, generator=g) * 2, 0).to(dev)
        U = ops.crf_unary(Q)
        nb, ng = ops.crf_norm(img, H, W, 121.0, 5.0), ops.crf_norm(None, H, W, 1.0, device=dev)
        t_b = timeit(lambda: ops.crf_message(img, Q, 121.0, 5.0, normalize=nb), n=5, warm=1)
        t_g = timeit(lambda: ops.crf_message(None, Q, 1.0, normalize=ng), n=20, warm=2)
        t_nb = timeit(lambda: ops.crf_norm(img, H, W, 121.0, 5.0), n=5, warm=1)
        t_u = timeit(lambda: ops.crf_unary(Q, from_logits=True), n=20, warm=2)
        t_all = timeit(lambda: ops.dense_crf(U, img, 10, 1.0, 1.0, 4.0, 121.0, 5.0), n=2, warm=1)
        chunks = (C + 31) // 32
        print(f"crf {H}x{W}x{C}: dense_crf T=10 {t_all / 1e3:.1f} ms/image; bilateral message {t_b / 1e3:.2f} ms = "
              f"{N * N / t_b / 1e6:.2f} Tpairs/s ({chunks} channel chunk(s): {chunks * N * N / t_b / 1e6:.2f} T kernel evaluations/s, "
              f"{2 * 32 * chunks * N * N / t_b / 1e6:.1f} TFLOP/s of MFMA, 32 channel rows per chunk); bilateral normaliser {t_nb / 1e3:.2f} ms; Gaussian stencil message "
              f"{t_g:.0f} us; unary from logits {t_u:.0f} us")


def crf_lattice_bench(dev, g):
    """DenseCRF(10, 1, 1, 4, 121, 5), exact (ops.dense_crf) and on the permutohedral lattice (ops.lattice_crf), alternating in one
    process, at 375x500x21 and 480x640x81.  The lattice's cost depends on the image (the number of vertices M): `smooth` is a
    low-frequency colour field plus sigma-3 noise (what the seeded test cases look like), `uniform` one colour (a handful of
    bilateral vertices with entry ranges of ~1e5: the splat's worst case), `noise` independent uniform pixels (M at its largest:
    the blur's worst case).  Construction (embed, sort, index, link, n: both lattices) and the iterations are timed apart."""
    def smooth(H, W):
        low = torch.rand(1, 3, 6, 8, generator=g) * 255
        up = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        return (up + 3.0 * torch.randn(H, W, 3, generator=g)).round().clamp(0, 255).to(torch.uint8)

    cases = [("smooth", 375, 500, 21, smooth), ("smooth", 480, 640, 81, smooth),
             ("uniform", 375, 500, 21, lambda H, W: torch.full((H, W, 3), 117, dtype=torch.uint8)),
             ("noise", 375, 500, 21, lambda H, W: torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))]
    par = (1.0, 1.0, 4.0, 121.0, 5.0)
    for name, H, W, C, make in cases:
        img = make(H, W).contiguous().to(dev)
        Q = torch.softmax(torch.randn(C, H, W, generator=g) * 2, 0).to(dev)
        U = ops.crf_unary(Q)
        build = lambda: (ops.crf_lattice_build(None, H, W, 1.0, device=dev), ops.crf_lattice_build(img, H, W, 121.0, 5.0))
        lg, lb = build()
        t_exact, t_lat = [], []
        for r in range(3):                      # alternating; the first round warms both up
            t_exact.append(timeit(lambda: ops.dense_crf(U, img, 10, *par), n=1, warm=0))
            t_lat.append(timeit(lambda: ops.lattice_crf(U, img, 10, *par), n=3, warm=0))
        t_build = timeit(build, n=5, warm=1)
        t0 = timeit(lambda: ops.crf_lattice_infer(U, lg, lb, 0, 1.0, 4.0), n=20, warm=2)
        t10 = timeit(lambda: ops.crf_lattice_infer(U, lg, lb, 10, 1.0, 4.0), n=10, warm=2)
        t_mg = timeit(lambda: ops.crf_lattice_message(lg, Q), n=20, warm=2)
        t_mb = timeit(lambda: ops.crf_lattice_message(lb, Q), n=20, warm=2)
        agree = float((ops.dense_crf(U, img, 10, *par).argmax(0) == ops.lattice_crf(U, img, 10, *par).argmax(0)).float().mean())
        te, tl = min(t_exact[1:]) / 1e3, min(t_lat[1:]) / 1e3
        print(f"crf_lattice {name} {H}x{W}x{C}: exact {te:.1f} ms/image, lattice {tl:.2f} ms/image ({te / tl:.1f}x); lattice = "
              f"construction {t_build / 1e3:.2f} ms + 10 iterations x {(t10 - t0) / 1e4:.3f} ms; one message: Gaussian "
              f"{t_mg:.0f} us (M {lg.M}, P {lg.P}), bilateral {t_mb:.0f} us (M {lb.M}, P {lb.P}, {lb.multi.numel()} multi-piece "
              f"vertices); labels equal to the exact path's at {100 * agree:.2f} % of the pixels (random logits)")


def cam_eval_bench(dev, g):
    """ops.cam_eval (histograms of T thresholds + label map + value, one launch) against the composed path of the ops it fuses:
    resize_bilinear, then per threshold cam_to_label and ConfusionMatrix.update; 448^2 CAMs, batch 1.  Bytes of the fused pass:
    8 (gt) + 4 (value) + 1 (label) per pixel plus the 448^2 floats of every class present, read once."""
    from dupl_amd.utils import cam_helper, evaluate
    for H, W, C, K in ((375, 500, 20, 2), (480, 640, 80, 6), (480, 640, 80, 20)):       # K = 20 at T = 19: two threshold chunks
        nc = C + 1
        low = torch.rand((1, C, 28, 28), generator=g)
        cam = torch.nn.functional.interpolate(low, size=(448, 448), mode="bilinear", align_corners=False).to(dev).contiguous()
        cls = torch.zeros((1, C))
        cls[0, torch.randperm(C, generator=g)[:K]] = 1.0
        # ground truth as in a data set: blobs of background and the classes present, some 255
        ids = torch.cat([torch.zeros(1), torch.nonzero(cls[0])[:, 0] + 1, torch.tensor([255.0])])
        gt = ids[torch.randint(0, ids.numel(), (1, 1, 6, 8), generator=g)]
        gt = torch.nn.functional.interpolate(gt, size=(H, W), mode="nearest")[0].long().to(dev)
        cls = cls.to(dev)
        for thr in ([0.5], [0.05 + 0.05 * i for i in range(19)]):
            T = len(thr)
            hist = torch.zeros((T, nc, nc), device=dev, dtype=torch.int64)
            cms = [evaluate.ConfusionMatrix(nc, dev) for _ in thr]

            def composed():
                rc = ops.resize_bilinear(cam, H, W)
                for t, cm in zip(thr, cms):
                    cm.update(gt, cam_helper.cam_to_label(rc, cls, bkg_thre=t))

            t_c = timeit(composed, n=50, warm=5)
            t_f = timeit(lambda: ops.cam_eval(cam, cls, (H, W), thr, gt=gt, hist=hist, label_at=T // 2, want_value=True), n=200)
            t_g = timeit(lambda: ops.cam_eval(cam, cls, (H, W), thr, gt=gt, hist=hist, label_at=T // 2, want_value=True, impl=1), n=50,
                         warm=5)
            # the launch alone: descriptor and outputs built once, so the host adds one ctypes call per launch
            import ctypes
            import numpy as np
            from dupl_amd import _lib
            label = torch.empty((1, H, W), device=dev, dtype=torch.uint8)
            value = torch.empty((1, H, W), device=dev, dtype=torch.float32)
            arr = np.asarray(thr, dtype=np.float32)
            d = _lib.CamEvalDesc(B=1, C=C, h=448, w=448, H=H, W=W, T=T, num_classes=nc, label_at=T // 2, cam=cam.data_ptr(),
                                 cls_label=cls.data_ptr(), thr=arr.ctypes.data, gt=gt.data_ptr(), hist=hist.data_ptr(),
                                 label_out=label.data_ptr(), value_out=value.data_ptr())
            fn, ref, st = ops.L().dupl_cam_eval.raw, ctypes.byref(d), ops._stream()
            t_k = timeit(lambda: fn(ref, st), n=500)
            nbytes = H * W * 13 + K * 448 * 448 * 4
            print(f"cam_eval {H}x{W} C={C} K={K} T={T}: ops.cam_eval {t_f:.1f} us, launch alone {t_k:.1f} us ({nbytes / t_k / 1e6:.3f} TB/s); "
                  f"composed {t_c:.1f} us ({t_c / t_f:.1f}x ops.cam_eval); with the global-atomics histogram {t_g:.1f} us")


def seg_ensemble_bench(dev, g):
    """ops.seg_ensemble (three confusion matrices + the agreement counters, one launch; with and without the (C,H,W) probabilities)
    against the composition of existing ops that yields the same matrices and counters: resize_bilinear x 2 -> softmax x 2 -> mean ->
    argmax_channels x 3 -> confusion_accum x 3 (+ the two masked sums of the counters), per call at batch 1.  VOC form: 375 x 500,
    C = 21, logits at label size (smooth, as accumulated from up-sampled maps); COCO form: 480 x 640, C = 81, logits 28 x 28.  Floor bytes of the fused pass: both students' logits
    once + 8 B/px of gt (+ 4 C B/px of prob); the rate printed is those bytes over the time of the call, wrapper included."""
    from dupl_amd.utils import evaluate
    for name, C, h, w, H, W in (("VOC", 21, 375, 500, 375, 500), ("COCO", 81, 28, 28, 480, 640)):
        # logits as a network gives them: smooth at label size (the VOC form accumulates up-sampled 1/16-resolution maps), so that
        # predictions come in regions and a workgroup's pixels fall into a few histogram bins; i.i.d. noise per pixel would make
        # every workgroup flush hundreds of counters and time the atomics instead
        def logits():
            if h <= 32:
                return (torch.randn((1, C, h, w), generator=g) * 3).to(dev)
            up = torch.nn.functional.interpolate(torch.randn((1, C, 24, 32), generator=g) * 3, size=(h, w), mode="bilinear", align_corners=False)
            return (up + 0.05 * torch.randn((1, C, h, w), generator=g)).contiguous().to(dev)

        a, b = logits(), logits()
        gt = torch.randint(0, C, (1, 1, 6, 8), generator=g).float()
        gt[0, 0, 0, :2] = 255.0
        gt = torch.nn.functional.interpolate(gt, size=(H, W), mode="nearest")[0, 0].long().to(dev)
        em = evaluate.EnsembleMatrix(C, dev)
        cms = [evaluate.ConfusionMatrix(C, dev) for _ in range(3)]
        cnt = torch.zeros(2, device=dev, dtype=torch.int64)

        def composed():
            ua, ub = ops.resize_bilinear(a, H, W), ops.resize_bilinear(b, H, W)
            e = (torch.softmax(ua, 1) + torch.softmax(ub, 1)) * 0.5
            pa, pb, pe = ops.argmax_channels(ua)[0], ops.argmax_channels(ub)[0], ops.argmax_channels(e)[0]
            for cm, p in zip(cms, (pa, pb, pe)):
                cm.update(gt, p)
            ok = (gt >= 0) & (gt < C)
            cnt[0] += ok.sum()
            cnt[1] += (ok & (pa == pb)).sum()
            return e

        def composed_hist_only():        # without the counters' two masked sums (five more launches the fused pass has no use for)
            ua, ub = ops.resize_bilinear(a, H, W), ops.resize_bilinear(b, H, W)
            e = (torch.softmax(ua, 1) + torch.softmax(ub, 1)) * 0.5
            for cm, p in zip(cms, (ua, ub, e)):
                cm.update(gt, ops.argmax_channels(p)[0])

        fused = lambda: ops.seg_ensemble(a, b, (H, W), gt=gt, hist=em.hist, counts=em.counts)
        fused_prob = lambda: ops.seg_ensemble(a, b, (H, W), gt=gt, hist=em.hist, counts=em.counts, want_prob=True)
        # alternate the two sides twice: the spread between the two rounds is the noise of one lease
        rounds = [(timeit(fused, n=200), timeit(fused_prob, n=200), timeit(composed, n=50, warm=5), timeit(composed_hist_only, n=50, warm=5))
                  for _ in range(2)]
        floor = 2 * C * h * w * 4 + H * W * 8
        floor_p = floor + C * H * W * 4
        for i, (t_f, t_p, t_c, t_h) in enumerate(rounds):
            print(f"seg_ensemble {name} {H}x{W} C={C} from {h}x{w}, round {i}: fused {t_f:.1f} us ({floor / t_f / 1e6:.3f} TB/s of its "
                  f"{floor / 1e6:.1f} MB floor), fused + prob {t_p:.1f} us ({floor_p / t_p / 1e6:.3f} TB/s of {floor_p / 1e6:.1f} MB); composed "
                  f"{t_c:.1f} us ({t_c / t_f:.1f}x fused, {t_c / t_p:.1f}x fused + prob), composed without the counters {t_h:.1f} us "
                  f"({t_h / t_f:.1f}x fused)")


def seg_render_bench(dev, g):
    """ops.seg_decide (label + conf + stats, one launch) against the composition of existing ops that yields the same label and conf
    -- resize_bilinear -> softmax (x 2 and the mean with two students) -> max -> argmax_channels -> uint8 --, per call at batch 1, at
    the VOC form (375 x 500, C = 21, logits at label size) and the COCO form (480 x 640, C = 81, from 28 x 28), one and two students;
    and ops.seg_paint against the host palette lookup and blend it replaces (label and image already on the host, the result left
    there: the device -> host copies the host path needs on top are not counted)."""
    import numpy as np
    from dupl_amd.utils import imutils
    for name, C, h, w, H, W in (("VOC", 21, 375, 500, 375, 500), ("COCO", 81, 28, 28, 480, 640)):
        def logits():            # smooth at label size, as seg_ensemble_bench's: predictions come in regions
            if h <= 32:
                return (torch.randn((1, C, h, w), generator=g) * 3).to(dev)
            up = torch.nn.functional.interpolate(torch.randn((1, C, 24, 32), generator=g) * 3, size=(h, w), mode="bilinear", align_corners=False)
            return (up + 0.05 * torch.randn((1, C, h, w), generator=g)).contiguous().to(dev)

        a, b = logits(), logits()
        stats = torch.zeros((2, C + 1), device=dev, dtype=torch.int64)

        def composed(two):
            p = torch.softmax(ops.resize_bilinear(a, H, W), 1)
            if two:
                p = (p + torch.softmax(ops.resize_bilinear(b, H, W), 1)) * 0.5
                label = ops.argmax_channels(p)[0]
            else:
                label = ops.upsample_argmax(a, H, W)[0] if (h, w) != (H, W) else ops.argmax_channels(a)[0]
            return label.to(torch.uint8), p[0].max(0).values

        for two in (False, True):
            fused = lambda: ops.seg_decide(a, b if two else None, (H, W), min_conf=0.5, stats=stats)
            rounds = [(timeit(fused, n=200), timeit(lambda: composed(two), n=50, warm=5)) for _ in range(2)]
            floor = (2 if two else 1) * C * h * w * 4 + H * W * 5
            for i, (t_f, t_c) in enumerate(rounds):
                print(f"seg_decide {name} {H}x{W} C={C} from {h}x{w}, {'two students' if two else 'one student'}, round {i}: fused {t_f:.1f} us "
                      f"({floor / t_f / 1e6:.3f} TB/s of its {floor / 1e6:.2f} MB floor); composed (no stats) {t_c:.1f} us ({t_c / t_f:.1f}x fused)")
    pal_np = imutils.colormap()
    pal = torch.from_numpy(pal_np).to(dev)
    for H, W in ((375, 500), (1024, 2048)):
        lab_np = np.repeat(np.repeat(torch.randint(0, 21, (H // 25 + 1, W // 25 + 1), generator=g).numpy().astype(np.uint8), 25, 0), 25, 1)[:H, :W].copy()
        img_np = torch.randint(0, 256, (H, W, 3), generator=g).numpy().astype(np.uint8)
        lab, img = torch.from_numpy(lab_np).to(dev), torch.from_numpy(img_np).to(dev)

        def host():
            out = (img_np.astype(np.int32) * 102 + pal_np[lab_np].astype(np.int32) * 154 + 128) >> 8
            return np.where((lab_np == 0)[..., None], img_np, out).astype(np.uint8)

        import time
        host()
        t0 = time.perf_counter()
        for _ in range(5):
            host()
        t_h = (time.perf_counter() - t0) / 5 * 1e6
        assert np.array_equal(ops.seg_paint(lab, pal, img, alpha256=154).cpu().numpy(), host())
        for i in range(2):
            t_o = timeit(lambda: ops.seg_paint(lab, pal, img, alpha256=154), n=200)
            t_c = timeit(lambda: ops.seg_paint(lab, pal, img, alpha256=154, contour=True), n=200)
            t_p = timeit(lambda: ops.seg_paint(lab, pal), n=200)
            print(f"seg_paint {H}x{W}, round {i}: overlay {t_o:.1f} us ({H * W * 7 / t_o / 1e6:.3f} TB/s of 7 B/px), with contours {t_c:.1f} us, "
                  f"palette only {t_p:.1f} us; host numpy palette + blend {t_h:.0f} us ({t_h / t_o:.0f}x)")


def regions_bench(dev, g):
    """ops.seg_regions (region map + count + table with conf sums + stats: every launch, the count's read-back included) and
    ops.seg_regions_clean (min_area 64: label, clean, label again) against what users do today: label.cpu(), scipy.ndimage.label per
    class present (8-connectivity), find_objects, np.bincount.  (a), (b): a smooth seeded field plus 0.5 % seeded speckle, C = 21;
    (c) one label everywhere -- every pixel lands on one table row.  Floor: 5 B/px (label in, region map out).  The launches of
    one call, timed apart on (b), say what sets the time."""
    import time
    import numpy as np
    from scipy import ndimage

    def blobs(H, W):
        up = torch.nn.functional.interpolate(torch.randn((1, 21, H // 24 + 2, W // 24 + 2), generator=g), size=(H, W), mode="bilinear",
                                             align_corners=False)
        lab = up[0].argmax(0).to(torch.uint8)
        speck = torch.rand((H, W), generator=g) < 0.005
        lab[speck] = torch.randint(0, 21, (H, W), generator=g, dtype=torch.uint8)[speck]
        return lab

    def host(label_dev):
        lab = label_dev.cpu().numpy()
        found = []
        for c in np.unique(lab):
            m, k = ndimage.label(lab == c, np.ones((3, 3), int))
            area = np.bincount(m.ravel(), minlength=k + 1)[1:]
            ids, at = np.unique(m.ravel(), return_index=True)       # the first pixel of every component, in raster order
            first = np.zeros(k + 1, np.int64)
            first[ids] = at
            for j, sl in enumerate(ndimage.find_objects(m)):
                found.append((int(first[j + 1]), int(c), int(area[j]), sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1))
        return sorted(found)

    def host_timed(label_dev):        # the same without the first-pixel bookkeeping that only the comparison needs
        lab = label_dev.cpu().numpy()
        n = 0
        for c in np.unique(lab):
            m, k = ndimage.label(lab == c, np.ones((3, 3), int))
            ndimage.find_objects(m)
            np.bincount(m.ravel(), minlength=k + 1)
            n += k
        return n

    for name, label in (("(a) 375x500 blobs + speckle", blobs(375, 500)), ("(b) 1024x2048 blobs + speckle", blobs(1024, 2048)),
                        ("(c) 1024x2048 one label", torch.full((1024, 2048), 7, dtype=torch.uint8))):
        label = label.to(dev)
        H, W = label.shape
        conf = torch.rand((H, W), generator=g).to(dev)
        stats = torch.zeros((2, 22), device=dev, dtype=torch.int64)
        region, n, table = ops.seg_regions(label, conf, stats=stats)
        want = host(label)
        t = table.cpu().numpy()
        assert n == len(want) == t.shape[0], (n, len(want))
        assert [(int(r[7]), int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5])) for r in t] == want
        reg = region.cpu().numpy()
        assert np.array_equal(reg.ravel()[t[:, 7]], np.arange(n)) and np.array_equal(np.bincount(reg.ravel(), minlength=n), t[:, 1])
        t0 = time.perf_counter()
        for _ in range(3):
            host_timed(label)
        t_h = (time.perf_counter() - t0) / 3 * 1e6
        floor = 5 * H * W
        for i in range(2):
            t_r = timeit(lambda: ops.seg_regions(label, conf, stats=stats), n=100, warm=10)
            t_m = timeit(lambda: ops.seg_regions(label), n=100, warm=10)
            t_c = timeit(lambda: ops.seg_regions_clean(label, min_area=64, conf=conf, stats=stats), n=50, warm=5)
            print(f"regions {name}, {n} regions, round {i}: seg_regions {t_r:.1f} us ({t_r * 1e3 / (H * W):.3f} ns/px; floor {floor / 1e6:.2f} MB = "
                  f"{floor / 5.0e6:.1f} us at 5 TB/s, {floor / t_r / 1e6:.3f} TB/s of it), without conf and stats {t_m:.1f} us; "
                  f"seg_regions_clean(64) {t_c:.1f} us; host scipy path {t_h:.0f} us ({t_h / t_r:.0f}x seg_regions)")
    # where the time of one call on (b) and (c) goes: the launches between two events each, 50 calls
    for name, label in (("(b)", blobs(1024, 2048).to(dev)), ("(c)", torch.full((1024, 2048), 7, dtype=torch.uint8, device=dev))):
        H, W = label.shape
        conf = torch.rand((H, W), generator=g).to(dev)
        stats = torch.zeros((2, 22), device=dev, dtype=torch.int64)
        t_all = timeit(lambda: ops._seg_regions(label, conf, 8, 255, 65536, stats, 21), n=100, warm=10)
        t_n = timeit(lambda: _count_only(label), n=100, warm=10)
        print(f"regions {name} without the read-back: all six launches {t_all:.1f} us; local + seam + flatten + scan alone (n_regions only) "
              f"{t_n:.1f} us; number + stats {t_all - t_n:.1f} us")


def boundary_bench(dev, g):
    """ops.seg_boundary into resident counters (what evaluate.BoundaryMatrix.update enqueues) on prediction-like maps: gt = the argmax
    of a smooth seeded field with a 255 contour, pred = the argmax of the same field plus noise (it agrees inside the objects and
    strays at their edges).  Floor: 16 B/px, the two int64 maps read once.  The kernels apart: rocprofv3 --kernel-trace --stats on
    this mode (bd_pack_kernel, bd_row_kernel, bd_col_kernel)."""
    import os
    import time
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import boundary_ref as BR
    from dupl_amd.utils import evaluate

    def maps(H, W, nc):
        f = torch.randn((1, nc, H // 24 + 2, W // 24 + 2), generator=g)
        up = lambda t: torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)[0]
        gt = up(f).argmax(0)
        pred = up(f + 0.3 * torch.randn(f.shape, generator=g)).argmax(0)
        edge = torch.zeros((H, W), dtype=torch.bool)
        edge[:, 1:] |= gt[:, 1:] != gt[:, :-1]
        edge[1:, :] |= gt[1:, :] != gt[:-1, :]
        return torch.where(edge, torch.full_like(gt, 255), gt), pred

    R = 32
    for H, W, nc in ((375, 500, 21), (480, 640, 81)):
        d = evaluate.biou_dist(H, W)
        gt_h, pred_h = maps(H, W, nc)
        gt, pred = gt_h.to(dev), pred_h.to(dev)
        hist = torch.zeros((R + 1, nc, nc), device=dev, dtype=torch.int64)
        biou = torch.zeros((3, nc), device=dev, dtype=torch.int64)
        conf = torch.zeros((nc, nc), device=dev, dtype=torch.int64)
        ops.seg_boundary(gt, pred, num_classes=nc, max_dist=R, biou_dist=d, band_hist=hist, biou=biou)

        def host():
            a, b = gt.cpu().numpy(), pred.cpu().numpy()
            return BR.band_hist(a, b, nc, R), BR.biou_counts(a, b, nc, d)
        t0 = time.perf_counter()
        want = host()
        t_h = (time.perf_counter() - t0) * 1e6
        assert np.array_equal(hist.cpu().numpy(), want[0]) and np.array_equal(biou.cpu().numpy(), want[1])
        near = int(want[0][:R].sum()) / max(int(want[0].sum()), 1)
        floor = 16 * H * W
        for i in range(3):
            t_b = timeit(lambda: ops.seg_boundary(gt, pred, num_classes=nc, max_dist=R, biou_dist=d, band_hist=hist, biou=biou), n=300, warm=30)
            t_t = timeit(lambda: ops.seg_boundary(gt, pred, num_classes=nc, max_dist=R, band_hist=hist), n=300, warm=30)
            t_c = timeit(lambda: ops.confusion_accum(gt, pred, conf), n=300, warm=30)
            print(f"boundary {H}x{W}x{nc} R={R} d={d} ({100 * near:.0f} % of the valid pixels within R), round {i}: seg_boundary {t_b:.1f} us "
                  f"({t_b * 1e3 / (H * W):.3f} ns/px; floor {floor / 1e6:.2f} MB = {floor / 6.3e6:.1f} us at 6.3 TB/s, {floor / t_b / 1e6:.3f} TB/s "
                  f"of it), without the Boundary IoU counters {t_t:.1f} us; confusion_accum alone {t_c:.1f} us (+{t_b - t_c:.1f} us per image and "
                  f"column); host scipy path {t_h:.0f} us ({t_h / t_b:.0f}x)")


def calibration_bench(dev, g):
    """ops.seg_calibration into resident counters (what evaluate.CalibrationMatrix.update enqueues per image and column) on seeded
    N(0, 2^2) logits and a seeded ground truth with 5 % ignored pixels.  Floors: the logits and the int64 gt read once at 6.3 TB/s;
    the v_exp_f32 the definition needs -- per pixel, temperature and student C for one student (the partition sum), 2 C for two
    (partition sum, then the mean; where the values stay in registers the second sweep reuses the first's) -- at 8 cycles per
    wave instruction on 1024 SIMDs at 2.4 GHz."""
    import os
    import time
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import calib_ref as CR
    import ctypes
    from dupl_amd import _lib
    nbins = 15
    sweep = (1.0,) + tuple(float(f"{0.45 * (4.2 / 0.45) ** (i / 12):.12g}") for i in range(13))
    for name, C, (h, w), (H, W) in (("VOC", 21, (375, 500), (375, 500)), ("COCO", 81, (28, 28), (480, 640))):
        z = [(torch.randn((C, h, w), generator=g) * 2).to(dev) for _ in range(2)]
        gt_h = torch.randint(0, C, (H, W), generator=g)
        gt_h[torch.rand((H, W), generator=g) < 0.05] = 255
        gt, gt_np = gt_h.to(dev), gt_h.numpy()
        for students in (1, 2):
            ins = z[:students]
            for temps in ((1.0,), sweep):
                T = len(temps)
                bins = torch.zeros((T, nbins, 3), device=dev, dtype=torch.int64)
                cls = torch.zeros((T, C, 3), device=dev, dtype=torch.int64)
                sums = torch.zeros((T, 4), device=dev, dtype=torch.int64)
                call = lambda: ops.seg_calibration(*ins, size=(H, W), gt=gt, temperatures=temps, nbins=nbins, bins=bins, cls=cls, sums=sums)

                def composed():
                    out = []
                    for t in temps:
                        label, conf = ops.seg_decide(*[ops.scale_(v.clone(), ops.inv_temperature(t)) for v in ins], size=(H, W))
                        out.append(CR.host_counters(label.cpu().numpy(), conf.cpu().numpy(), gt_np, C, nbins))
                    return out
                # the launch alone: a descriptor built once (the wrapper's checks, inverse temperatures and ctypes struct are host time)
                inv = (ctypes.c_float * T)(*[ops.inv_temperature(t) for t in temps])
                desc = _lib.SegCalibDesc(C=C, h=h, w=w, H=H, W=W, T=T, nbins=nbins, a=ins[0].data_ptr(), b=ins[1].data_ptr() if students == 2
                                         else None, gt=gt.data_ptr(), inv_temp=ctypes.cast(inv, ctypes.c_void_p).value, bins=bins.data_ptr(),
                                         cls=cls.data_ptr(), sums=sums.data_ptr())
                fn, ref, stream = ops.L().dupl_seg_calib, ctypes.byref(desc), ops._stream()
                only = _lib.SegCalibDesc.from_buffer_copy(desc)                  # sums alone: the same pixels, 4 T counters to flush
                only.bins = only.cls = None
                ref_only = ctypes.byref(only)
                call()
                want = composed()
                for t in range(T):
                    assert np.array_equal(bins[t].cpu().numpy(), want[t][0]) and np.array_equal(cls[t].cpu().numpy(), want[t][1])
                    assert sums[t, :2].tolist() == want[t][2].tolist()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    composed()
                t_c = (time.perf_counter() - t0) * 1e6 / 3
                nbytes = 4 * C * h * w * students + 8 * H * W
                n_exp = T * H * W * C * (1 if students == 1 else 2) * students
                f_mem, f_exp = nbytes / 6.3e6, n_exp / 64 * 8 / (1024 * 2.4e3)
                for i in range(3):
                    t_w = timeit(call, n=100, warm=10)
                    t_k = timeit(lambda: fn(ref, stream), n=100, warm=10)
                    t_s = timeit(lambda: fn(ref_only, stream), n=100, warm=10)
                    print(f"calibration {name} {H}x{W}x{C} from {h}x{w}, {students} student(s), T={T}, round {i}: seg_calibration {t_w:.1f} us "
                          f"through ops, {t_k:.1f} us the launch alone, {t_s:.1f} us with sums alone ({t_k * 1e3 / (H * W * T):.3f} ns per pixel and temperature; floors: {nbytes / 1e6:.2f} MB = {f_mem:.1f} us at 6.3 TB/s, "
                          f"{n_exp / 1e6:.1f} M v_exp_f32 = {f_exp:.1f} us: {max(f_mem, f_exp) / t_k:.2f} of the larger); composed "
                          f"scale_ -> seg_decide -> read-back -> bincount x {T}: {t_c:.0f} us ({t_c / t_k:.0f}x)")


def _count_only(label):
    """dupl_seg_regions asked for n_regions alone: the labelling launches without number and stats"""
    import ctypes
    from dupl_amd import _lib
    H, W = label.shape
    n = torch.empty((1,), device=label.device, dtype=torch.int32)
    d = _lib.SegRegionsDesc(H=H, W=W, C=21, connectivity=8, ignore_index=255, max_regions=0, label=label.data_ptr(), n_regions=n.data_ptr())
    nbytes = ops.L().dupl_seg_regions_workspace(ctypes.byref(d))
    ws = torch.empty((nbytes // 8 + 1,), device=label.device, dtype=torch.int64)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    ops.L().dupl_seg_regions(ctypes.byref(d), ops._stream())
    return n


def predict_bench(argv):
    """tools/predict on one synthetic 1024 x 2048 image, ViT-B (seeded random weights), scales 1.0 / 1.5 / 1.25: the whole image per
    scale against sliding windows (window=448 stride=320 window_batch=8), ms per image and peak device memory.
        python tools/op_bench.py predict [H=1024] [W=2048] [window=448] [stride=320] [window_batch=8] [n=3] [backbone=vit_base_patch16_224]"""
    import numpy as np
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.tools import predict
    opts = dict(a.split("=", 1) for a in argv if "=" in a)
    H, W, n = int(opts.get("H", 1024)), int(opts.get("W", 2048)), int(opts.get("n", 3))
    window, stride, wb = int(opts.get("window", 448)), int(opts.get("stride", 320)), int(opts.get("window_batch", 8))
    backbone = opts.get("backbone", "vit_base_patch16_224")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = siamese_network(backbone=backbone, num_classes=21, pretrained=False, aux_layer=-3).to(dev).eval()
    image = np.random.RandomState(0).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    arms = [("windows", dict(window=window, stride=stride, window_batch=wb))]
    if opts.get("whole", "1") == "1":
        arms.append(("whole image", dict(window=0)))
    for name, kw in arms:
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        try:
            r = predict.predict_image(model, image, branch="ens", **kw)          # warm-up: allocations, the pos-embed grids
            torch.cuda.synchronize()
            ms = timeit(lambda: predict.predict_image(model, image, branch="ens", **kw), n=n, warm=0) / 1e3
        except (RuntimeError, torch.OutOfMemoryError) as e:
            print(f"predict {backbone} {H}x{W} {name}: could not run: {type(e).__name__}: {str(e).splitlines()[0][:200]}")
            continue
        print(f"predict {backbone} {H}x{W} {name} {kw}: {ms:.1f} ms / image, windows per scale {r['windows']}, "
              f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def backbone_bench(argv):
    """ms / step and img / s of one phase-B step (VOC, 448^2, 4 images on one GPU, two streams) per backbone."""
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from dupl_amd.model.backbone import FAMILY
    opts = dict(a.split("=", 1) for a in argv if "=" in a)
    names = [a for a in argv if a in FAMILY] or list(FAMILY)
    unknown = [a for a in argv if a != "backbone" and "=" not in a and a not in FAMILY]
    assert not unknown, f"not a registered backbone: {unknown}; registered: {FAMILY}"
    steps, warmup = int(opts.get("steps", 20)), int(opts.get("warmup", 5))
    sys.argv = [sys.argv[0], "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    import bench
    args = bench.parse()
    rows = []
    for name in names:
        wl = bench.Workload(args, 1, 0, 0, "voc", 4, name, bench.DEFAULT_N_ITER["voc"])
        assert wl.phase == "B", wl.phase
        res = wl.measure(name)
        cfg = wl.model.branch1._cfg
        g = wl.model.flat_storage.guard.summary()
        rows.append((name, cfg, res["ms"], res["value"], g))
        print(f"backbone {name}: D {cfg.embed_dim} depth {cfg.depth} heads {cfg.num_heads} grid {cfg.grid}: {res['ms']:.2f} ms / step, "
              f"{res['value']:.2f} img / s (loss {res['loss']:.4f}; sites on f32 {g['sites_on_f32']}, on format 0 {g['sites_on_fmt0']})", flush=True)
        del wl, res
        gc.collect()
        torch.cuda.empty_cache()
    print(f"\n| backbone | embed dim | depth | heads | pos-embed grid | ms / step | img / s |\n|---|---|---|---|---|---|---|")
    for name, cfg, ms, v, _ in rows:
        print(f"| `{name}` | {cfg.embed_dim} | {cfg.depth} | {cfg.num_heads} | {cfg.grid} x {cfg.grid} | {ms:.2f} | {v:.2f} |")


def nograd_bench(argv):
    from dupl_amd import engine
    from dupl_amd.model.model_dupl import network
    from dupl_amd.synthetic import synthetic_batch
    from dupl_amd.utils import cam_helper
    opts = dict(a.split("=", 1) for a in argv if "=" in a)
    n, rounds = int(opts.get("n", 10)), int(opts.get("rounds", 3))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = network("deit_base_patch16_224", num_classes=21, pretrained=False, aux_layer=-3).to(dev).eval()
    inputs, cls_label, _ = synthetic_batch(4, 20, 448, seed=0)
    inputs, cls_label = inputs.to(dev), cls_label.to(dev).float()
    xs = [ops.resize_bilinear(inputs, s, s, flip_cat=True) for s in (224, 672)]
    rows = sum(x.shape[0] * ((x.shape[2] // 16) ** 2 + 1) for x in xs)
    times = {"f16x3": [], "f16": []}
    with torch.no_grad():
        for r in range(rounds):           # the two modes interleaved: both see the same clocks and temperature
            for mode in ("f16x3", "f16"):
                engine.set_nograd_gemm_mode(mode)
                times[mode].append(timeit(lambda: engine.cam_logits_multi(net._P, xs), n=n, warm=3 if r == 0 else 1) / 1e3)
        for mode in ("f16x3", "f16"):
            t = sorted(times[mode])
            print(f"nograd {mode}: cam_logits_multi, {rows} token rows (8 x 224^2 + 8 x 672^2), ViT-B: median {t[len(t) // 2]:.2f} ms "
                  f"(rounds of {n}: {', '.join(f'{v:.2f}' for v in times[mode])})")
        m3, m1 = sorted(times["f16x3"])[rounds // 2], sorted(times["f16"])[rounds // 2]
        print(f"nograd f16 / f16x3 = {m1 / m3:.3f}")
        res = {}
        for mode in ("f16x3", "f16"):
            engine.set_nograd_gemm_mode(mode)
            cam, cam_aux = cam_helper.multi_scale_cam2(net, inputs, (1.0, 0.5, 1.5))
            res[mode] = (cam, cam_aux, cam_helper.cam_to_label(cam, cls_label, bkg_thre=0.45),
                         cam_helper.cam_to_label(cam_aux, cls_label, bkg_thre=0.45))
        engine.set_nograd_gemm_mode("f16x3")
    a, b = res["f16x3"], res["f16"]
    npx = a[2].numel()
    print(f"nograd CAM (448^2, 4 images, scales 1.0 / 0.5 / 1.5, normalised to [0, 1)): max-abs-diff cam {float((a[0] - b[0]).abs().max()):.3e}, "
          f"cam_aux {float((a[1] - b[1]).abs().max()):.3e}; cam_to_label (bkg_thre 0.45) pixels that differ: cam {int((a[2] != b[2]).sum())}, "
          f"cam_aux {int((a[3] != b[3]).sum())} of {npx}")
    print("guard:", net._store.guard.summary())


def main():
    if "backbone" in sys.argv[1:]:
        return backbone_bench(sys.argv[1:])
    if "nograd" in sys.argv[1:]:
        return nograd_bench(sys.argv[1:])
    if "predict" in sys.argv[1:]:
        return predict_bench(sys.argv[1:])
    if "seg_render" in sys.argv[1:]:
        return seg_render_bench(torch.device("cuda:0"), torch.Generator().manual_seed(0))
    if "regions" in sys.argv[1:]:
        return regions_bench(torch.device("cuda:0"), torch.Generator().manual_seed(0))
    if "boundary" in sys.argv[1:]:
        return boundary_bench(torch.device("cuda:0"), torch.Generator().manual_seed(0))
    if "calibration" in sys.argv[1:]:
        return calibration_bench(torch.device("cuda:0"), torch.Generator().manual_seed(0))
    if "crf_lattice" in sys.argv[1:]:
        return crf_lattice_bench(torch.device("cuda:0"), torch.Generator().manual_seed(0))
    which = set(sys.argv[1:]) or {"ln_bwd", "ln_fwd", "split", "attn_bwd", "multi", "cam"}
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if "seg_ensemble" in which:
        seg_ensemble_bench(dev, g)
        which = which - {"seg_ensemble"}
        if not which:
            return
    if "cam_eval" in which:
        cam_eval_bench(dev, g)
        if which <= {"cam_eval", "crf"} and "crf" not in which:
            return
    if "crf" in which:
        crf_bench(dev, g)
        if which == {"crf"}:
            return
    rows, D = 3140, 768
    x = torch.randn(rows, D, generator=g).to(dev)
    dy = (torch.randn(rows, D, generator=g) * 1e-5).to(dev)
    dres = (torch.randn(rows, D, generator=g) * 1e-5).to(dev)
    gamma = torch.ones(D, device=dev)
    beta = torch.zeros(D, device=dev)
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-6).rsqrt()
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    if "ln_bwd" in which:
        for rpw in (8, 4, 2, 1):
            ops.LNB_ROWS_PER_WAVE = rpw
            t = timeit(lambda: ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, dres=dres, two_stage=False))
            t2 = timeit(lambda: ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, dres=dres, two_stage=True))
            print(f"layernorm_bwd {rows}x{D} rows/wave {rpw}: atomics {t:.1f} us ({4 * rows * D * 4 / t / 1e6:.2f} TB/s), "
                  f"two-stage {t2:.1f} us ({4 * rows * D * 4 / t2 / 1e6:.2f} TB/s)")
        ops.LNB_ROWS_PER_WAVE = 0
    if "ln_fwd" in which:
        for r in (3140, 6280, 15696):
            xx = torch.randn(r, D, generator=g).to(dev)
            t = timeit(lambda: ops.layernorm_fwd16(xx, gamma, beta, 1e-6))
            print(f"layernorm_fwd16 {r}x{D}: {t:.1f} us")
    if "split" in which:
        for (r, c) in ((3140, 768), (3140, 3072), (3140, 2304)):
            xx = (torch.randn(r, c, generator=g) * 1e-5).to(dev)
            t = timeit(lambda: ops.split_prepare(xx, scaled=True, want_rm=True, want_T=True, rows_pad=3168))
            t2 = timeit(lambda: ops.split_prepare(xx, scaled=False, want_rm=False, want_T=True, rows_pad=3168))
            print(f"split_prepare {r}x{c}: scaled rm+T {t:.1f} us (amax + split), T only {t2:.1f} us")
    if "multi" in which:
        xs = [torch.randn(3140, c, generator=g).to(dev) for c in (3072, 768, 768, 768)]
        ws = [torch.randn(r, c, generator=g).to(dev) for r, c in ((768, 3072), (3072, 768), (768, 768), (2304, 768))]
        items = [(x, False, True, 3168) for x in xs] + [(w, False, True, w.shape[0]) for w in ws]

        def singles():
            for x, rm, T, rp in items:
                ops.split_prepare(x, scaled=False, want_rm=rm, want_T=T, rows_pad=rp)
        t1 = timeit(singles, n=100)
        t2 = timeit(lambda: ops.split_prepare_multi(items), n=100)
        t3 = timeit(lambda: ops.split_prepare_multi(items[:4]), n=100)
        print(f"block operands (4 x^T + 4 W^T): 8 launches {t1:.1f} us, one multi launch {t2:.1f} us; x^T only, one launch {t3:.1f} us")
        t4 = timeit(lambda: ops.split_prepare_multi(items[4:]), n=100)
        print(f"  W^T only, one launch {t4:.1f} us")
        for k in range(8):
            tk = timeit(lambda: ops.split_prepare_multi(items[k:k + 1]), n=100)
            ts = timeit(lambda: ops.split_prepare(items[k][0], scaled=False, want_rm=False, want_T=True, rows_pad=items[k][3]), n=100)
            print(f"  item {k} {tuple(items[k][0].shape)}: multi(1) {tk:.1f} us, single {ts:.1f} us")
        for m in (5, 6, 7):
            tm = timeit(lambda: ops.split_prepare_multi(items[:m]), n=100)
            print(f"  first {m} items: {tm:.1f} us")
    if "cam" in which:
        for C in (20, 80):
            B, H, W = 4, 448, 448
            sizes = [(28, 28), (14, 14), (42, 42)]
            lows = [torch.randn(2 * B * (1 + h * w), C, generator=g).to(dev) for h, w in sizes]
            for nb in (384, 512, 768, 1024, 1536, 2048, 4096):
                t = timeit(lambda: ops.cam_fuse(lows, sizes, B, C, H, W, 1, C, band_blocks=nb), n=100)
                print(f"cam_fuse C={C} band kernel, {nb} blocks aimed at: {t:.1f} us = {B * C * H * W * 4 / t / 1e6:.2f} TB/s of output (incl. the min/max init launch)")
    if "attn_bwd" in which:
        B, N, H, hd = 4, 785, 12, 64
        qkv = torch.randn(B * N, 3 * H * hd, generator=g).to(dev)
        dout = (torch.randn(B * N, H * hd, generator=g) * 1e-5).to(dev)
        qkv16 = ops.split16(qkv)
        out = torch.empty(B * N, H * hd, device=dev)
        lse = ops.attention_fwd16(qkv16, B, N, H, hd, hd ** -0.5, need_lse=True, out=out)
        t = timeit(lambda: ops.attention_bwd16(qkv16, out, dout, lse, B, N, H, hd, hd ** -0.5), n=100)
        print(f"attention_bwd16 B{B} N{N}: {t:.1f} us (delta + dq + dv + dk + the dout split)")


if __name__ == "__main__":
    main()
