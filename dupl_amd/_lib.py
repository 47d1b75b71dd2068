"""ctypes binding of libdupl_hip.so -- the reference-side stub INTEGRATION.md describes.

The prototypes are read from include/dupl_hip.h (single source of truth) and turned into ctypes
signatures; every exported function is wrapped so that a non-zero status raises.  There is NO
fallback: if the shared library is missing or a symbol is absent, importing the product path fails.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "dupl_hip.h")
LIB_PATH = os.path.join(HERE, "libdupl_hip.so")


class GemmDesc(ctypes.Structure):
    """Mirror of `dupl_gemm_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("tile_rows", ctypes.c_int32), ("tile_cols", ctypes.c_int32), ("group", ctypes.c_int32),
        ("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p),
        ("bias", ctypes.c_void_p), ("res", ctypes.c_void_p), ("aux", ctypes.c_void_p),
        ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
        ("lda", ctypes.c_int32), ("ldb", ctypes.c_int32), ("ldc", ctypes.c_int32),
        ("ldr", ctypes.c_int32), ("ldaux", ctypes.c_int32),
        ("batch", ctypes.c_int32), ("zdiv", ctypes.c_int32),
        ("sA0", ctypes.c_int64), ("sA1", ctypes.c_int64), ("sB0", ctypes.c_int64), ("sB1", ctypes.c_int64),
        ("sC0", ctypes.c_int64), ("sC1", ctypes.c_int64), ("sR0", ctypes.c_int64), ("sR1", ctypes.c_int64),
        ("sX0", ctypes.c_int64), ("sX1", ctypes.c_int64), ("sBias0", ctypes.c_int64), ("sBias1", ctypes.c_int64),
        ("alpha", ctypes.c_float), ("flags", ctypes.c_int32), ("deterministic", ctypes.c_int32), ("reserved0", ctypes.c_int32),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(GemmDesc)


class Gemm16Desc(ctypes.Structure):
    """Mirror of `dupl_gemm16_desc` (include/dupl_hip.h): operands as fp16 hi / lo planes."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("deterministic", ctypes.c_int32),
        ("A_hi", ctypes.c_void_p), ("A_lo", ctypes.c_void_p), ("B_hi", ctypes.c_void_p), ("B_lo", ctypes.c_void_p),
        ("C", ctypes.c_void_p), ("C_hi", ctypes.c_void_p), ("C_lo", ctypes.c_void_p),
        ("bias", ctypes.c_void_p), ("res", ctypes.c_void_p), ("aux", ctypes.c_void_p),
        ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
        ("lda", ctypes.c_int32), ("ldb", ctypes.c_int32), ("ldc", ctypes.c_int32), ("ldo", ctypes.c_int32),
        ("ldr", ctypes.c_int32), ("ldaux", ctypes.c_int32),
        ("flags", ctypes.c_int32), ("c_rows", ctypes.c_int32),
        ("alpha_dev", ctypes.c_void_p), ("fmt", ctypes.c_int32), ("out_exp", ctypes.c_int32), ("post_scale", ctypes.c_float),
        ("amax_out", ctypes.c_void_p),
        ("a_layout", ctypes.c_int32), ("b_layout", ctypes.c_int32), ("ka_valid", ctypes.c_int32), ("kb_valid", ctypes.c_int32),
        ("tile", ctypes.c_int32), ("concurrency", ctypes.c_int32), ("persist_blocks", ctypes.c_int32), ("group", ctypes.c_int32),
        ("sk_slices", ctypes.c_int32), ("products", ctypes.c_int32),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(Gemm16Desc)


class SplitDesc(ctypes.Structure):
    """Mirror of `dupl_split_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("ld", ctypes.c_int32), ("R", ctypes.c_int32), ("C", ctypes.c_int32),
        ("x", ctypes.c_void_p), ("slot", ctypes.c_void_p), ("next_bits", ctypes.c_void_p),
        ("hi", ctypes.c_void_p), ("lo", ctypes.c_void_p), ("hiT", ctypes.c_void_p), ("loT", ctypes.c_void_p),
        ("Rp", ctypes.c_int32), ("target_exp", ctypes.c_int32), ("colsum_accum", ctypes.c_void_p),
        ("amax_mode", ctypes.c_int32), ("fmt", ctypes.c_int32), ("rows_zero_to", ctypes.c_int32), ("deterministic", ctypes.c_int32),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SplitDesc)


class CrfDesc(ctypes.Structure):
    """Mirror of `dupl_crf_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("T", ctypes.c_int32), ("reserved0", ctypes.c_int32),
        ("img", ctypes.c_void_p), ("Q", ctypes.c_void_p), ("norm", ctypes.c_void_p), ("unary", ctypes.c_void_p),
        ("out", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("sxy", ctypes.c_float), ("srgb", ctypes.c_float), ("w_g", ctypes.c_float), ("sxy_g", ctypes.c_float),
        ("w_b", ctypes.c_float), ("sxy_b", ctypes.c_float), ("srgb_b", ctypes.c_float), ("reserved1", ctypes.c_int32),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(CrfDesc)


class CrfLattice(ctypes.Structure):
    """Mirror of `dupl_crf_lattice` (include/dupl_hip.h): one built lattice."""
    _fields_ = [
        ("D", ctypes.c_int32), ("M", ctypes.c_int32), ("P", ctypes.c_int32), ("n_multi", ctypes.c_int32),
        ("keys", ctypes.c_void_p), ("weights", ctypes.c_void_p), ("vkeys", ctypes.c_void_p), ("entry", ctypes.c_void_p),
        ("vertex", ctypes.c_void_p), ("piece_begin", ctypes.c_void_p), ("piece_vertex", ctypes.c_void_p),
        ("vpiece", ctypes.c_void_p), ("multi", ctypes.c_void_p), ("nbr", ctypes.c_void_p), ("norm", ctypes.c_void_p),
    ]


class CrfLatticeDesc(ctypes.Structure):
    """Mirror of `dupl_crf_lattice_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("T", ctypes.c_int32), ("reserved0", ctypes.c_int32),
        ("lat", CrfLattice * 2),
        ("img", ctypes.c_void_p), ("Q", ctypes.c_void_p), ("unary", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("sxy", ctypes.c_float), ("srgb", ctypes.c_float), ("w_g", ctypes.c_float), ("w_b", ctypes.c_float),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(CrfLatticeDesc)


class CamEvalDesc(ctypes.Structure):
    """Mirror of `dupl_cam_eval_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
        ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("T", ctypes.c_int32), ("num_classes", ctypes.c_int32),
        ("label_at", ctypes.c_int32), ("impl", ctypes.c_int32), ("reserved0", ctypes.c_int32),
        ("cam", ctypes.c_void_p), ("cls_label", ctypes.c_void_p), ("thr", ctypes.c_void_p), ("gt", ctypes.c_void_p),
        ("hist", ctypes.c_void_p), ("label_out", ctypes.c_void_p), ("value_out", ctypes.c_void_p),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(CamEvalDesc)


class SegEnsembleDesc(ctypes.Structure):
    """Mirror of `dupl_seg_ensemble_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("C", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
        ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("gt", ctypes.c_void_p),
        ("hist", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("pred", ctypes.c_void_p), ("prob", ctypes.c_void_p),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SegEnsembleDesc)


class SegDecideDesc(ctypes.Structure):
    """Mirror of `dupl_seg_decide_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("C", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
        ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("is_prob", ctypes.c_int32), ("ignore_index", ctypes.c_int32),
        ("min_conf", ctypes.c_float), ("reserved0", ctypes.c_int32),
        ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("conf", ctypes.c_void_p), ("label", ctypes.c_void_p),
        ("stats", ctypes.c_void_p),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SegDecideDesc)


class SegPaintDesc(ctypes.Structure):
    """Mirror of `dupl_seg_paint_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("alpha256", ctypes.c_int32),
        ("tint_background", ctypes.c_int32), ("contour", ctypes.c_int32),
        ("contour_rgb", ctypes.c_uint8 * 3), ("reserved0", ctypes.c_uint8),
        ("label", ctypes.c_void_p), ("image", ctypes.c_void_p), ("palette", ctypes.c_void_p), ("out", ctypes.c_void_p),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SegPaintDesc)


class WindowGatherDesc(ctypes.Structure):
    """Mirror of `dupl_window_gather_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("Hs", ctypes.c_int32),
        ("Ws", ctypes.c_int32), ("nW", ctypes.c_int32), ("wh", ctypes.c_int32), ("ww", ctypes.c_int32),
        ("x", ctypes.c_void_p), ("origins", ctypes.c_void_p), ("out", ctypes.c_void_p),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(WindowGatherDesc)


class WindowMergeDesc(ctypes.Structure):
    """Mirror of `dupl_window_merge_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("C", ctypes.c_int32), ("hs", ctypes.c_int32), ("ws", ctypes.c_int32),
        ("nW", ctypes.c_int32), ("wth", ctypes.c_int32), ("wtw", ctypes.c_int32),
        ("logits", ctypes.c_void_p), ("origins", ctypes.c_void_p), ("canvas", ctypes.c_void_p),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(WindowMergeDesc)


class SegRegionsDesc(ctypes.Structure):
    """Mirror of `dupl_seg_regions_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("C", ctypes.c_int32),
        ("connectivity", ctypes.c_int32), ("ignore_index", ctypes.c_int32), ("max_regions", ctypes.c_int32), ("reserved0", ctypes.c_int32),
        ("label", ctypes.c_void_p), ("conf", ctypes.c_void_p), ("region", ctypes.c_void_p), ("n_regions", ctypes.c_void_p),
        ("table", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SegRegionsDesc)


class SegRegionsCleanDesc(ctypes.Structure):
    """Mirror of `dupl_seg_regions_clean_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("C", ctypes.c_int32),
        ("max_regions", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("min_area", ctypes.c_int64),
        ("label", ctypes.c_void_p), ("region", ctypes.c_void_p), ("n_regions", ctypes.c_void_p), ("table", ctypes.c_void_p),
        ("label_out", ctypes.c_void_p), ("changed", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SegRegionsCleanDesc)


class SegBoundaryDesc(ctypes.Structure):
    """Mirror of `dupl_seg_boundary_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("num_classes", ctypes.c_int32),
        ("max_dist", ctypes.c_int32), ("biou_dist", ctypes.c_int32),
        ("gt", ctypes.c_void_p), ("pred", ctypes.c_void_p), ("band_hist", ctypes.c_void_p), ("biou", ctypes.c_void_p),
        ("dist_gt", ctypes.c_void_p), ("dist_pred", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SegBoundaryDesc)


class SegCalibDesc(ctypes.Structure):
    """Mirror of `dupl_seg_calib_desc` (include/dupl_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("C", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
        ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("is_prob", ctypes.c_int32), ("T", ctypes.c_int32),
        ("nbins", ctypes.c_int32), ("reserved0", ctypes.c_int32),
        ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("inv_temp", ctypes.c_void_p),
        ("bins", ctypes.c_void_p), ("cls", ctypes.c_void_p), ("sums", ctypes.c_void_p),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(SegCalibDesc)


GEMM_A_MCONTIG, GEMM_B_NCONTIG, GEMM_GELU, GEMM_ACCUM = 1, 2, 4, 8
GEMM_MUL_DGELU, GEMM_RELU, GEMM_MUL_RELUMASK, GEMM_ABS, GEMM_STORE_PRE = 16, 32, 64, 128, 256
GEMM_C_FRESH = 512            # DUPL_GEMM_C_FRESH (dupl_gemm_f16x3_group)

class SplitItem(ctypes.Structure):
    """dupl_split_item (include/dupl_hip.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("hi", ctypes.c_void_p), ("lo", ctypes.c_void_p), ("hiT", ctypes.c_void_p),
                ("loT", ctypes.c_void_p), ("ld", ctypes.c_int32), ("R", ctypes.c_int32), ("C", ctypes.c_int32),
                ("Rp", ctypes.c_int32)]


class AttnSeg(ctypes.Structure):
    """dupl_attn_seg (include/dupl_hip.h): one batch of a segmented attention-forward launch."""
    _fields_ = [("row0", ctypes.c_int64), ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("B_f32", ctypes.c_int32),
                ("reserved0", ctypes.c_int32), ("out", ctypes.c_void_p), ("lse", ctypes.c_void_p)]


ATTN_SEGS_MAX = 4             # DUPL_ATTN_SEGS_MAX
SPLIT_MULTI_MAX = 16
GEMM16_GROUP_MAX = 8          # DUPL_GEMM16_GROUP_MAX
CAM_EVAL_MAX_T, CAM_EVAL_MAX_C = 64, 255      # DUPL_CAM_EVAL_MAX_T, DUPL_CAM_EVAL_MAX_C
SEG_ENSEMBLE_MAX_C = 255      # DUPL_SEG_ENSEMBLE_MAX_C
SEG_DECIDE_MAX_C = 255        # DUPL_SEG_DECIDE_MAX_C
WINDOW_MAX = 256              # DUPL_WINDOW_MAX
CRF_LATTICE_PIECE = 128       # DUPL_CRF_LATTICE_PIECE
SEG_REGIONS_MAX_C, SEG_REGIONS_COLS = 256, 8  # DUPL_SEG_REGIONS_MAX_C, DUPL_SEG_REGIONS_COLS
SEG_BOUNDARY_MAX_C, SEG_BOUNDARY_MAX_DIST = 255, 64   # DUPL_SEG_BOUNDARY_MAX_C, DUPL_SEG_BOUNDARY_MAX_DIST
SEG_CALIB_MAX_C, SEG_CALIB_MAX_T, SEG_CALIB_MAX_BINS = 255, 16, 64    # DUPL_SEG_CALIB_MAX_C, DUPL_SEG_CALIB_MAX_T, DUPL_SEG_CALIB_MAX_BINS

_PROTO = re.compile(r"^\s*int\s+(dupl_\w+)\s*\(([^;{]*)\)\s*;", re.M | re.S)


def _ctype(decl: str):
    d = decl.strip()
    if d == "void" or not d:
        return None
    if "dupl_gemm16_desc" in d:
        return ctypes.POINTER(Gemm16Desc)
    if "dupl_split_desc" in d:
        return ctypes.POINTER(SplitDesc)
    if "dupl_gemm_desc" in d:
        return ctypes.POINTER(GemmDesc)
    if "dupl_crf_desc" in d:
        return ctypes.POINTER(CrfDesc)
    if "dupl_crf_lattice_desc" in d:
        return ctypes.POINTER(CrfLatticeDesc)
    if "dupl_cam_eval_desc" in d:
        return ctypes.POINTER(CamEvalDesc)
    if "dupl_seg_ensemble_desc" in d:
        return ctypes.POINTER(SegEnsembleDesc)
    if "dupl_seg_decide_desc" in d:
        return ctypes.POINTER(SegDecideDesc)
    if "dupl_seg_paint_desc" in d:
        return ctypes.POINTER(SegPaintDesc)
    if "dupl_window_gather_desc" in d:
        return ctypes.POINTER(WindowGatherDesc)
    if "dupl_window_merge_desc" in d:
        return ctypes.POINTER(WindowMergeDesc)
    if "dupl_seg_regions_desc" in d:
        return ctypes.POINTER(SegRegionsDesc)
    if "dupl_seg_regions_clean_desc" in d:
        return ctypes.POINTER(SegRegionsCleanDesc)
    if "dupl_seg_boundary_desc" in d:
        return ctypes.POINTER(SegBoundaryDesc)
    if "dupl_seg_calib_desc" in d:
        return ctypes.POINTER(SegCalibDesc)
    if "*" in d or d.startswith("dupl_stream_t"):
        return ctypes.c_void_p
    base = d.replace("const", "").split()
    ty = base[0]
    return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint8_t": ctypes.c_uint8,
            "int": ctypes.c_int, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[ty]


def parse_header(path: str = HEADER) -> Dict[str, List]:
    """{function name: [ctypes argtypes]} for every `int dupl_*(...)` prototype in the header."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out: Dict[str, List] = {}
    for m in _PROTO.finditer(src):
        name, args = m.group(1), m.group(2)
        tys = [_ctype(a) for a in args.split(",")]
        out[name] = [t for t in tys if t is not None]
    return out


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  dupl_amd has no CPU / eager fallback by design.")
        # The process must hold ONE HIP runtime.  torch ships its own libamdhip64 (SONAME libamdhip64.so.7, found by
        # libtorch_hip under the file name libamdhip64.so): when torch is loaded first our NEEDED libamdhip64.so.7
        # binds to that copy; loaded the other way round the dynamic linker maps /opt/rocm's runtime for us and torch's
        # for torch, and torch stream handles passed across the C ABI are then foreign (launches fail with -2).
        import torch  # noqa: F401  (device memory + streams come from torch: load its runtime first)
        self.cdll = ctypes.CDLL(LIB_PATH)
        runtimes = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
        if len(runtimes) > 1:
            raise ImportError(f"two HIP runtimes mapped in one process ({sorted(runtimes)}): stream handles and "
                              "device pointers would not be interchangeable")
        self.protos = parse_header()
        for name, argtypes in self.protos.items():
            fn = getattr(self.cdll, name)  # AttributeError if the .so does not export a declared symbol
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
            # getters return a value, everything else a status (0 = ok) that is checked on every call
            setattr(self, name, fn if name in ("dupl_abi_version", "dupl_layernorm_bwd_blocks") else self._checked(name, fn))
        # Build identity (ABI 4): the digest of the kernel sources is baked into the library at build time.  The GPU box runs a
        # PREBUILT, git-ignored .so that travels with the tree: if the sources next to it are not the ones it was built from, refuse
        # it here rather than measure (or test) one set of kernels under the name of another.
        buf = ctypes.create_string_buffer(80)
        if self.cdll.dupl_build_digest(buf, 80) != 0:
            raise ImportError(f"{LIB_PATH}: dupl_build_digest failed")
        self.build_digest = buf.value.decode()
        # the one size getter with a 64-bit result (the prototype scan above covers the `int` entry points only)
        self.dupl_crf_lattice_workspace = self.cdll.dupl_crf_lattice_workspace
        self.dupl_crf_lattice_workspace.argtypes = [ctypes.POINTER(CrfLatticeDesc), ctypes.c_int32]
        self.dupl_crf_lattice_workspace.restype = ctypes.c_int64
        for name, desc in (("dupl_seg_regions_workspace", SegRegionsDesc), ("dupl_seg_regions_clean_workspace", SegRegionsCleanDesc),
                           ("dupl_seg_boundary_workspace", SegBoundaryDesc)):
            fn = getattr(self.cdll, name)
            fn.argtypes, fn.restype = [ctypes.POINTER(desc)], ctypes.c_int64
            setattr(self, name, fn)
        from .build import source_digest, _sources
        if _sources() and os.environ.get("DUPL_SKIP_DIGEST_CHECK", "0") != "1":
            have = source_digest()
            if have != self.build_digest:
                raise ImportError(
                    f"{LIB_PATH} was built from kernel sources with digest {self.build_digest[:16]}, the sources in this tree have "
                    f"{have[:16]}: rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")

    @staticmethod
    def _checked(name, fn):
        def call(*a):
            rc = fn(*a)
            if rc != 0:
                raise RuntimeError(f"{name} failed with status {rc} (-1 bad argument, -2 launch failure)")
            return rc
        call.__name__ = name
        call.raw = fn
        return call


_LIB = None


def lib() -> _Lib:
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB
