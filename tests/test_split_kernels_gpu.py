"""The operand-preparation kernels -- dupl_split_f16x2 / f16x2b (csrc/gemm_split.hip), dupl_split_prepare / _multi
(csrc/split_prep.hip), the result planes that linear16, attention_fwd16 and layernorm_fwd16 write, and dupl_param_bounds
(csrc/range.hip) -- against tests/split_ref.py, the plane formats written from their definition in numpy, whose own exactness
tests/test_split_ref_host.py checks first.  Planes are compared bit for bit (a NaN of the reference asks for any NaN).

Technique (tests/kernel_guard.py): every output lives inside sentinel slack that must be bit-unchanged, every input inside NaN
slack (the gap of ld > C included), kernels are called through ops.L() on the current stream.  Refusal tests only exercise
host-side DUPL_ERR_ARG returns: nothing is launched by them, and their outputs must still be all sentinel.  The two tolerance
tests (column sums, row norms) derive their bound in the docstring and print the worst err / bound."""
import ctypes
import math

import numpy as np
import pytest
import torch

import split_ref as S
from kernel_guard import NAN, EPS24, PAD, _ALIVE, Guard, Tally, nan_in, stream

pytestmark = pytest.mark.gpu

ERR_ARG = -1
U = EPS24                    # unit roundoff of fp32


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _ALIVE.clear()


def L():
    from dupl_amd import ops
    return ops.L()


class HGuard(Guard):
    """fp16 planes of `shape` (an even number of elements) inside int32 sentinel slack"""

    def __init__(self, shape, dev, front=None):
        self.hshape = tuple(shape)
        n = int(np.prod(shape))
        assert n % 2 == 0
        super().__init__((n // 2,), dev, torch.int32, front=front)

    def h(self):
        return self.cpu().numpy().view(np.float16).reshape(self.hshape)

    def tensor(self):
        return self.view.view(torch.float16).view(self.hshape)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def word(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def assert_planes(got, ref, what, x=None):
    assert S.same_f16(got, ref), f"{what}: {S.first_diff(got, ref, x)}"


# ================================================================================= dupl_split_f16x2 / dupl_split_f16x2b
def _split(dev, x, exp, fmt1):
    xin = nan_in(f32(x), dev)
    hi, lo = HGuard((x.size,), dev), HGuard((x.size,), dev)
    if fmt1:
        L().dupl_split_f16x2b(xin.data_ptr(), hi.ptr, lo.ptr, x.size, exp, stream())
    else:
        L().dupl_split_f16x2(xin.data_ptr(), hi.ptr, lo.ptr, x.size, stream())
    return hi.h(), lo.h()


def _special():
    x = S.special_values()
    return np.concatenate([x, np.zeros((-x.size) % 4, dtype=np.float32)])


@pytest.mark.parametrize("exp", [0, 3, 9, 15])
def test_split_special_values(dev, exp):
    """every fp16 pattern, its float32 neighbours, every tie, the subnormal ranges, the top of the range up to FLT_MAX (finite
    values saturate, the ones past the old 3.0e38 guard included), Inf and NaN: the bits of the definition"""
    x = _special()
    assert x.size % 4 == 0
    if exp == 0:
        hi, lo = _split(dev, x, 0, False)
        rh, rl = S.split0(x)
        assert_planes(hi, rh, "format 0 hi", x)
        assert_planes(lo, rl, "format 0 lo", x)
    hi, lo = _split(dev, x, exp, True)
    rh, rl = S.split1(x, exp)
    assert_planes(hi, rh, f"format 1 (exp {exp}) hi", x)
    assert_planes(lo, rl, f"format 1 (exp {exp}) lo", x)


@pytest.mark.parametrize("n", [4, 4 * (256 + 3), 8192 * 256 * 4 + 4 * 301])
def test_split_sizes(dev, n):
    """one float4; a float4 count that is no multiple of the block; more float4 than 8192 blocks hold (the grid-stride loop
    takes a second trip)"""
    g = np.random.default_rng(n)
    x = (g.standard_normal(n) * 10.0 ** g.integers(-6, 4, n)).astype(np.float32)
    hi, lo = _split(dev, x, 0, False)
    rh, rl = S.split0(x)
    assert_planes(hi, rh, "format 0 hi", x)
    assert_planes(lo, rl, "format 0 lo", x)
    hi, lo = _split(dev, x, 3, True)
    rh, rl = S.split1(x, 3)
    assert_planes(hi, rh, "format 1 hi", x)
    assert_planes(lo, rl, "format 1 lo", x)


def test_split_refusals(dev):
    x = nan_in(torch.ones(16), dev)
    hi, lo = HGuard((16,), dev), HGuard((16,), dev)
    a, b = L().dupl_split_f16x2.raw, L().dupl_split_f16x2b.raw
    xp, st = x.data_ptr(), stream()
    for args in [(xp, hi.ptr, lo.ptr, 6), (xp, hi.ptr, lo.ptr, 0), (xp, hi.ptr, lo.ptr, -4), (xp + 4, hi.ptr, lo.ptr, 8),
                 (xp + 8, hi.ptr, lo.ptr, 8), (xp, hi.ptr + 4, lo.ptr, 8), (xp, hi.ptr, lo.ptr + 4, 8), (xp, hi.ptr + 2, lo.ptr, 8),
                 (None, hi.ptr, lo.ptr, 8), (xp, None, lo.ptr, 8), (xp, hi.ptr, None, 8)]:
        assert a(*args, st) == ERR_ARG, args
        assert b(*args, 3, st) == ERR_ARG, args
    for exp in (-1, 16):
        assert b(xp, hi.ptr, lo.ptr, 8, exp, st) == ERR_ARG
    torch.cuda.synchronize()
    assert hi.untouched() and lo.untouched()


# ========================================================================================================= dupl_split_prepare
def _desc(x, ld, R, C, slot=None, nxt=None, hi=None, lo=None, hiT=None, loT=None, Rp=0, target=15, colsum=None, amax_mode=0,
          fmt=0, rz=0, det=0):
    from dupl_amd import _lib
    d = _lib.SplitDesc()
    d.x, d.ld, d.R, d.C, d.slot, d.next_bits = x, ld, R, C, slot, nxt
    d.hi, d.lo, d.hiT, d.loT, d.Rp, d.target_exp = hi, lo, hiT, loT, Rp, target
    d.colsum_accum, d.amax_mode, d.fmt, d.rows_zero_to, d.deterministic = colsum, amax_mode, fmt, rz, det
    return d


def _matrix(x, R, C, ld):
    """x [R, C] as [R, ld] with NaN in the gap columns"""
    m = np.full((R, ld), np.nan, dtype=np.float32)
    m[:, :C] = x
    return m


SLOT_FILL, NEXT_FILL = 7.0, 5.0


def _prepare(dev, x, ld=None, want_rm=True, want_T=True, Rp=None, rz=0, fmt=0, scaled=False, target=15, amax_mode=0, prev=None,
             what=""):
    """One dupl_split_prepare call on x [R, C] with every output guarded, compared with split_prepare_ref.  Returns the column
    sums (device result, float64 reference, float64 sum of |x|) when prev (the accumulator's previous content) is given."""
    R, C = x.shape
    ld = ld or C
    Rp = Rp if Rp is not None else (R + 7) // 8 * 8
    xin = nan_in(f32(_matrix(x, R, C, ld)), dev)
    Rz = max(R, rz)
    rm = (HGuard((Rz, C), dev), HGuard((Rz, C), dev)) if want_rm else None
    T = (HGuard((C, Rp), dev), HGuard((C, Rp), dev)) if want_T else None
    slot = nxt = cs = None
    if scaled:
        stale = 0 if amax_mode == 0 else (S.amax_bits(x) if amax_mode == 1 else word(3.0e9))
        slot = Guard((4,), dev, torch.int32, init=torch.tensor([word(SLOT_FILL), word(SLOT_FILL), stale - (1 << 32) * (stale >> 31),
                                                               word(SLOT_FILL)], dtype=torch.int32))
        nxt = Guard((4,), dev, torch.int32, init=torch.tensor([word(NEXT_FILL)] * 4, dtype=torch.int32))
    if prev is not None:
        cs = Guard((C,), dev, init=f32(prev))
    d = _desc(xin.data_ptr(), ld, R, C, slot.ptr if slot else None, nxt.ptr + 8 if nxt else None,
              rm[0].ptr if rm else None, rm[1].ptr if rm else None, T[0].ptr if T else None, T[1].ptr if T else None,
              Rp, target, cs.ptr if cs else None, amax_mode, fmt, rz)
    L().dupl_split_prepare(ctypes.byref(d), stream())
    (rh, rl), (rhT, rlT), (s, inv), colsum = S.split_prepare_ref(_matrix(x, R, C, ld), R, C, ld, scaled, target, bool(fmt), Rp, rz)
    what = f"{what} R {R} C {C} ld {ld} rm {want_rm} T {want_T} Rp {Rp} rz {rz} fmt {fmt} target {target} amax_mode {amax_mode}"
    if scaled:
        sl, nx = slot.cpu().numpy().view(np.uint32), nxt.cpu().numpy().view(np.uint32)
        assert int(sl[2]) == S.amax_bits(x), f"{what}: amax word {int(sl[2]):#x}, max-abs bits {S.amax_bits(x):#x}"
        got = sl[:2].view(np.float32)
        assert (int(sl[0]), int(sl[1])) == (word(s), word(inv)), \
            f"{what}: slot holds scale {float(got[0])!r}, 1 / scale {float(got[1])!r}; scale_rule gives {float(s)!r}, {float(inv)!r}"
        assert int(sl[3]) == word(SLOT_FILL), f"{what}: the slot's fourth word was written"
        assert int(nx[2]) == 0, f"{what}: the successor's amax word is {int(nx[2]):#x}, not zero"
        assert [int(v) for v in nx[[0, 1, 3]]] == [word(NEXT_FILL)] * 3, f"{what}: the successor's other words were written"
    xs = np.zeros((Rz, C), dtype=np.float32)
    xs[:R] = x
    if rm:
        assert_planes(rm[0].h(), rh, what + ": row-major hi", xs)
        assert_planes(rm[1].h(), rl, what + ": row-major lo", xs)
    if T:
        xt = np.zeros((C, Rp), dtype=np.float32)
        xt[:, :R] = x.T
        assert_planes(T[0].h(), rhT, what + ": transposed hi", xt)
        assert_planes(T[1].h(), rlT, what + ": transposed lo", xt)
    if cs is not None:
        return cs.cpu().double().numpy(), colsum, np.abs(x.astype(np.float64)).sum(axis=0)


SHAPES = [(1, 4), (5, 12), (63, 68), (64, 64), (65, 132), (130, 200)]


def _data(R, C, seed=0, scale=1.0):
    g = np.random.default_rng(1000 * R + C + seed)
    return (g.standard_normal((R, C)) * 10.0 ** g.integers(-4, 3, (R, C)) * scale).astype(np.float32)


@pytest.mark.parametrize("R,C", SHAPES)
def test_split_prepare_unscaled_layouts(dev, R, C):
    """row-major only / transposed only / both; Rp = R rounded up to 8, + 64 (one padding tile row), + 136 (two, ragged):
    padding tiles beyond the last data tile are zeros and nothing beyond Rp is written (the guards); rows_zero_to; both
    formats; ld > C"""
    x = _data(R, C)
    R8 = (R + 7) // 8 * 8
    for fmt in (0, 1):
        for want_rm, want_T in ((True, False), (False, True), (True, True)):
            for Rp in ((R8, R8 + 64, R8 + 136) if want_T else (0,)):
                for rz in ((0, R + 3, R + 70) if want_rm else (0,)):
                    _prepare(dev, x, want_rm=want_rm, want_T=want_T, Rp=Rp, rz=rz, fmt=fmt)
        _prepare(dev, x, ld=C + 8, Rp=R8 + 64, rz=R + 3, fmt=fmt, what="ld > C")


def _amax_case(name, R, C):
    """x [R, C] whose max-abs is the case's value at the case's position; every other element is at most half of it"""
    g = np.random.default_rng(len(name) * 131 + R)
    A, pos, sign, odd = {"pow2": (2.0 ** -7, R * C // 2, 1, None), "below_pow2": (float(np.nextafter(np.float32(2.0 ** -7), np.float32(0))), 3, 1, None),
                         "first": (0.37, 0, 1, None), "last": (0.37, R * C - 1, 1, None), "negative": (0.37, R * C // 3, -1, None),
                         "3e-6": (3e-6, 17, 1, None), "1e-30": (1e-30, 17, -1, None), "1e-36": (1e-36, 17, 1, None),
                         "min_subnormal": (2.0 ** -149, 17, -1, None), "1e30": (1e30, 17, 1, None),
                         "inf": (0.01, 17, 1, np.inf), "nan": (0.01, 17, 1, np.nan)}[name]
    x = (g.uniform(-0.5, 0.5, R * C) * A).astype(np.float32)
    x[pos] = np.float32(sign * A)
    if name == "min_subnormal":
        x[pos + 5] = np.float32(2.0 ** -149)
    if odd is not None:
        x[R * C // 2] = odd
    return x.reshape(R, C)


AMAX_CASES = ["pow2", "below_pow2", "first", "last", "negative", "3e-6", "1e-30", "1e-36", "min_subnormal", "1e30", "inf", "nan"]


@pytest.mark.parametrize("name", AMAX_CASES)
def test_split_prepare_scaled(dev, name):
    """planes, {scale, 1 / scale}, the amax word and the successor's cleared word for a tensor whose max-abs is: a power of two,
    just below one, the first / the last element, negative, the workload's 3e-6, 1e-30, 1e-36 and the smallest subnormal (where
    2^(target - e) is no float32: scale_rule's clamp), 1e30, and next to one Inf (scale 1: the amax is not finite) or one NaN
    (the amax pass skips it: the scale of the finite rest); the Inf / NaN element itself stays (Inf, NaN) / (NaN, NaN)"""
    R, C = 65, 132
    x = _amax_case(name, R, C)
    for fmt in (0, 1):
        for target in (4, 15):
            for amax_mode in (0, 2):
                _prepare(dev, x, Rp=72 + 64, fmt=fmt, scaled=True, target=target, amax_mode=amax_mode, what=name)
    # the producer's word (amax_mode 1: no amax pass, so ld > C is allowed)
    _prepare(dev, x, ld=C + 4, Rp=72, fmt=1, scaled=True, target=15, amax_mode=1, what=name + " ld > C")


@pytest.mark.parametrize("R,C", [(5, 12), (63, 68), (65, 132), (130, 200)])
def test_split_prepare_colsum(dev, R, C):
    """colsum_accum[c] += sum_r x[r][c] onto non-zero previous content, unscaled values of a scaled split.

    Bound: in a 64-row tile a thread adds its 4 rows into a zero (the first add is exact: 3 roundings), two shuffle adds fold
    the four lanes that hold the same columns (2), the four waves' partials are added as (a + b) + (c + d) (2), and one atomic
    per tile adds the result onto the accumulator (1 rounding per row tile, T = ceil(R / 64) of them, in any order).  So every
    term -- the previous content included -- passes through at most 7 + T fp32 roundings, and by the standard bound for a sum
    of rounded additions  |got - exact| <= ((1 + u)^(7 + T) - 1) * (|prev| + sum_r |x[r][c]|),  u = 2^-24."""
    T = Tally(f"colsum {R}x{C}")
    x = _data(R, C, seed=5, scale=1e-3)
    prev = (np.random.default_rng(C).standard_normal(C) * 0.1).astype(np.float32)
    tiles = (R + 63) // 64
    for scaled, ld in ((True, C), (False, C + 4)):
        got, colsum, sabs = _prepare(dev, x, ld=ld, scaled=scaled, prev=prev, what="colsum")
        exact = colsum + prev.astype(np.float64)
        bound = ((1.0 + U) ** (7 + tiles) - 1.0) * (np.abs(prev.astype(np.float64)) + sabs)
        T.add(f"scaled {scaled}", torch.from_numpy(np.abs(got - exact)), torch.from_numpy(bound))
    T.done()


def test_split_prepare_ring_wraps(dev):
    """130 consecutive scaled splits on one stream (the ring has 128 slots), alternating a tensor with a 2^-20 times smaller
    one: every scale is scale_rule of that tensor's own amax (a slot's stale amax word would give the larger tensor's)"""
    from dupl_amd import ops
    big = _data(65, 132, seed=9)
    small = big * np.float32(2.0 ** -20)
    xs = [f32(big).to(dev), f32(small).to(dev)]
    want = [S.scale_rule(S.amax_bits(big), 15), S.scale_rule(S.amax_bits(small), 15)]
    assert want[0] != want[1]
    recs = []
    for i in range(130):
        rm, _, _ = ops.split_prepare(xs[i & 1], scaled=True, want_rm=True, want_T=False, fmt1=True)
        recs.append(rm.planes._dupl_scale.clone())
    got = torch.stack(recs).cpu().numpy().view(np.uint32)
    for i in range(130):
        s, inv = want[i & 1]
        assert (int(got[i, 0]), int(got[i, 1])) == (word(s), word(inv)), f"split {i}: scale {got[i, :2].view(np.float32)}, want {s}, {inv}"
        assert int(got[i, 2]) == S.amax_bits(big if not i & 1 else small), f"split {i}: amax word"
    rh, rl = S.split1(small * want[1][0], 0)
    assert_planes(rm.planes[0].cpu().numpy(), rh, "the last split's hi")
    assert_planes(rm.planes[1].cpu().numpy(), rl, "the last split's lo")


def test_split_prepare_refusals(dev):
    from dupl_amd import _lib
    R, C, Rp = 5, 12, 8
    x = nan_in(torch.ones(R + 8, 16), dev)
    outs = [HGuard((R + 8, 16), dev) for _ in range(2)] + [HGuard((16, 16), dev) for _ in range(2)]
    slot, cs = Guard((8,), dev), Guard((16,), dev)
    hi, lo, hiT, loT = (o.ptr for o in outs)
    xp = x.data_ptr()

    def mk(**kw):
        a = dict(x=xp, ld=C, R=R, C=C, slot=None, nxt=None, hi=hi, lo=lo, hiT=hiT, loT=loT, Rp=Rp, target=15, colsum=None,
                 amax_mode=0, fmt=0, rz=0, det=0)
        a.update(kw)
        return _desc(**a)

    good = mk()
    bad_size = mk()
    bad_size.struct_size = ctypes.sizeof(_lib.SplitDesc) - 4
    cases = {"struct_size": bad_size, "C % 4": mk(C=10), "ld % 4": mk(ld=14), "ld < C": mk(ld=8), "no output": mk(hi=None, lo=None, hiT=None, loT=None),
             "hi without lo": mk(lo=None), "lo without hi": mk(hi=None), "hiT without loT": mk(loT=None), "loT without hiT": mk(hiT=None),
             "Rp < R": mk(Rp=0), "Rp % 8": mk(Rp=12), "target 0": mk(target=0), "target 16": mk(target=16),
             "amax_mode 3": mk(amax_mode=3, slot=slot.ptr), "amax_mode -1": mk(amax_mode=-1, slot=slot.ptr),
             "amax_mode 1 without slot": mk(amax_mode=1), "amax_mode 2 without slot": mk(amax_mode=2), "fmt 2": mk(fmt=2), "fmt -1": mk(fmt=-1),
             "rows_zero_to < R": mk(rz=R - 1), "rows_zero_to < 0": mk(rz=-1), "rows_zero_to without row-major planes": mk(rz=R + 3, hi=None, lo=None),
             "x off 16 bytes": mk(x=xp + 4), "x null": mk(x=None), "R 0": mk(R=0), "C 0": mk(C=0),
             "colsum deterministic": mk(colsum=cs.ptr, det=1),
             "ld > C with slot, amax_mode 0": mk(ld=16, slot=slot.ptr), "ld > C with slot, amax_mode 2": mk(ld=16, slot=slot.ptr, amax_mode=2)}
    raw = L().dupl_split_prepare.raw
    for name, d in cases.items():
        assert raw(ctypes.byref(d), stream()) == ERR_ARG, name
    assert raw(None, stream()) == ERR_ARG
    torch.cuda.synchronize()
    for g in outs + [slot, cs]:
        assert g.untouched()
    assert raw(ctypes.byref(good), stream()) == 0, "the descriptor the refusals were derived from is accepted"
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs)


# =================================================================================================== dupl_split_prepare_multi
def _multi(dev, specs):
    """specs: [(R, C, ld, want_rm, want_T, Rp)] launched 16 items at a time; every item against the reference"""
    from dupl_amd import _lib
    items, keep = [], []
    for i, (R, C, ld, want_rm, want_T, Rp) in enumerate(specs):
        x = _data(R, C, seed=i)
        xin = nan_in(f32(_matrix(x, R, C, ld)), dev)
        rm = (HGuard((R, C), dev), HGuard((R, C), dev)) if want_rm else None
        T = (HGuard((C, Rp), dev), HGuard((C, Rp), dev)) if want_T else None
        d = _lib.SplitItem()
        d.x, d.ld, d.R, d.C, d.Rp = xin.data_ptr(), ld, R, C, Rp
        d.hi, d.lo = (rm[0].ptr, rm[1].ptr) if rm else (None, None)
        d.hiT, d.loT = (T[0].ptr, T[1].ptr) if T else (None, None)
        items.append(d)
        keep.append((x, rm, T))
    for i in range(0, len(items), 16):
        chunk = items[i:i + 16]
        arr = (_lib.SplitItem * len(chunk))(*chunk)
        L().dupl_split_prepare_multi(ctypes.cast(arr, ctypes.c_void_p), len(chunk), stream())
    for i, ((R, C, ld, want_rm, want_T, Rp), (x, rm, T)) in enumerate(zip(specs, keep)):
        (rh, rl), (rhT, rlT), _, _ = S.split_prepare_ref(_matrix(x, R, C, ld), R, C, ld, False, 15, False, Rp, 0)
        what = f"item {i} of {len(specs)} R {R} C {C} ld {ld} Rp {Rp}"
        if rm:
            assert_planes(rm[0].h(), rh, what + ": row-major hi")
            assert_planes(rm[1].h(), rl, what + ": row-major lo")
        if T:
            assert_planes(T[0].h(), rhT, what + ": transposed hi")
            assert_planes(T[1].h(), rlT, what + ": transposed lo")


@pytest.mark.parametrize("n", [1, 16, 17])
def test_split_prepare_multi(dev, n):
    """a one-tile item first and last, ragged multi-tile items and ld > C between them, every output form"""
    pool = [(130, 200, 200, True, True, 136), (65, 132, 140, False, True, 72 + 64), (63, 68, 68, True, False, 0),
            (64, 64, 72, True, True, 64), (5, 12, 12, False, True, 8 + 136)]
    specs = [(1, 4, 4, True, True, 8)] + [pool[i % len(pool)] for i in range(max(n - 2, 0))] + ([(5, 12, 16, True, True, 8)] if n > 1 else [])
    assert len(specs) == n
    _multi(dev, specs)


def test_split_prepare_multi_refusals(dev):
    from dupl_amd import _lib
    x = nan_in(torch.ones(8, 8), dev)
    hi, lo = HGuard((8, 8), dev), HGuard((8, 8), dev)
    arr = (_lib.SplitItem * 17)()
    for d in arr:
        d.x, d.ld, d.R, d.C, d.Rp, d.hi, d.lo = x.data_ptr(), 8, 8, 8, 8, hi.ptr, lo.ptr
    raw = L().dupl_split_prepare_multi.raw
    p = ctypes.cast(arr, ctypes.c_void_p)
    assert raw(p, 0, stream()) == ERR_ARG and raw(p, 17, stream()) == ERR_ARG and raw(None, 1, stream()) == ERR_ARG
    arr[1].C = 6
    assert raw(p, 2, stream()) == ERR_ARG, "a bad second item refuses the whole launch"
    torch.cuda.synchronize()
    assert hi.untouched() and lo.untouched()


# ===================================================================================== result planes that other kernels write
def _split16_of(dev, x, exp):
    from dupl_amd import ops
    return ops.split16(f32(x).to(dev), exp=exp)


@pytest.mark.parametrize("tile", [0, 28])
@pytest.mark.parametrize("out_exp", [0, 3])
def test_linear16_planes_are_the_split_of_its_fp32_output(dev, tile, out_exp):
    """linear16 with fp32 and plane outputs, 65 x 72 x 32, bias + GELU + residual, format 1 operands, on the default tile and on
    the generic-walk code 28, format 0 and format 1 planes.  Every epilogue of csrc/gemm_split.hip stores v[c] to C and hands the
    same v[c] (times the power-of-two out_scale for format 1) to split_f32 / split_f32_u, so the planes must be the split of
    the fp32 output, bit for bit -- the reconstruction bar of 2^-21 of the maximum would hide a one-ulp disagreement between
    hi and the residual behind lo on every element that is not near the maximum."""
    from dupl_amd import ops
    M, N, K = 65, 72, 32
    g = np.random.default_rng(tile + out_exp)
    x, W = g.standard_normal((M, K)).astype(np.float32), (g.standard_normal((N, K)) * 0.05).astype(np.float32)
    b, res = nan_in(f32(g.standard_normal(N) * 0.1), dev), nan_in(f32(g.standard_normal((M, N))), dev)
    xs, Ws = _split16_of(dev, x, ops.EXP_ACT), _split16_of(dev, W, ops.EXP_W)
    y, planes = Guard((M, N), dev), HGuard((2, M, N), dev)
    y16 = ops.Split16(planes.tensor(), out_exp)
    ops.linear16(xs, Ws, b, gelu=True, res=res, out=y.view, out16=y16, tuning=dict(ops.GEMM16_TUNING, tile=tile))
    yv = y.cpu().numpy()
    assert np.isfinite(yv).all()
    rh, rl = S.split1(yv, out_exp) if out_exp else S.split0(yv)
    got = planes.h()
    assert_planes(got[0], rh, f"tile {tile} out_exp {out_exp} hi", yv)
    assert_planes(got[1], rl, f"tile {tile} out_exp {out_exp} lo", yv)
    want = torch.nn.functional.gelu(f32(x).double() @ f32(W).double().t() + b.cpu().double()) + res.cpu().double()
    # a sanity bar only (half an fp16 ulp of the maximum: y is this GEMM's output, not zeros); the accuracy is test_gemm_*'s subject
    assert float((torch.from_numpy(yv).double() - want).abs().max()) <= 2.0 ** -11 * float(want.abs().max()), "not this GEMM's output"


def test_linear16_format0_operands_planes(dev):
    """the format 0 GEMM (two accumulator sets), bias only: the same property"""
    from dupl_amd import ops
    M, N, K = 65, 72, 32
    g = np.random.default_rng(11)
    x, W = g.standard_normal((M, K)).astype(np.float32), (g.standard_normal((N, K)) * 0.05).astype(np.float32)
    b = nan_in(f32(g.standard_normal(N) * 0.1), dev)
    y, planes = Guard((M, N), dev), HGuard((2, M, N), dev)
    ops.linear16(_split16_of(dev, x, 0), _split16_of(dev, W, 0), b, out=y.view, out16=ops.Split16(planes.tensor(), 0))
    yv = y.cpu().numpy()
    rh, rl = S.split0(yv)
    assert np.isfinite(yv).all()
    assert_planes(planes.h()[0], rh, "format 0 GEMM hi", yv)
    assert_planes(planes.h()[1], rl, "format 0 GEMM lo", yv)


@pytest.mark.parametrize("mfma", [0, 32])
@pytest.mark.parametrize("out_exp", [0, 3])
def test_attention_fwd16_planes_are_the_split_of_its_fp32_output(dev, mfma, out_exp, monkeypatch):
    """attention_fwd16 with out and out16, B 1, N 50, H 2, hd 64, on both MFMA shapes: both kernels of csrc/attn_split.hip compute
    v[j] once, store it to out and split the same v[j] (times out_scale for format 1), so bit-equality is asserted"""
    from dupl_amd import ops
    monkeypatch.setitem(ops.ATTN16_TUNING, "mfma", mfma)
    B, N, H, hd = 1, 50, 2, 64
    g = np.random.default_rng(mfma + out_exp)
    qkv16 = _split16_of(dev, g.standard_normal((B * N, 3 * H * hd)).astype(np.float32), 0)
    out, planes = Guard((B * N, H * hd), dev), HGuard((2, B * N, H * hd), dev)
    ops.attention_fwd16(qkv16, B, N, H, hd, hd ** -0.5, out=out.view, out16=ops.Split16(planes.tensor(), out_exp))
    ov = out.cpu().numpy()
    assert np.isfinite(ov).all() and float(np.abs(ov).max()) > 0.1
    rh, rl = S.split1(ov, out_exp) if out_exp else S.split0(ov)
    assert_planes(planes.h()[0], rh, f"mfma {mfma} out_exp {out_exp} hi", ov)
    assert_planes(planes.h()[1], rl, f"mfma {mfma} out_exp {out_exp} lo", ov)


@pytest.mark.parametrize("exp", [0, 3])
def test_layernorm_fwd16_planes_are_the_split_of_its_fp32_output(dev, exp):
    """layernorm_fwd16 with the fp32 copy, 37 x 192: csrc/norm.hip stores o and splits the same o (times plane_scale)"""
    rows, D = 37, 192
    g = np.random.default_rng(exp)
    x = nan_in(f32(g.standard_normal((rows, D)) * 3.0 + 0.5), dev)
    gamma, beta = nan_in(f32(1.0 + 0.2 * g.standard_normal(D)), dev), nan_in(f32(0.1 * g.standard_normal(D)), dev)
    y, hi, lo = Guard((rows, D), dev), HGuard((rows, D), dev), HGuard((rows, D), dev)
    L().dupl_layernorm_fwd16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.ptr, hi.ptr, lo.ptr, None, None, rows, D, 1e-6, 0, exp,
                             stream())
    yv = y.cpu().numpy()
    assert np.isfinite(yv).all() and 0.5 < float(yv.std()) < 2.0
    rh, rl = S.split1(yv, exp) if exp else S.split0(yv)
    assert_planes(hi.h(), rh, f"exp {exp} hi", yv)
    assert_planes(lo.h(), rl, f"exp {exp} lo", yv)


# =========================================================================================================== dupl_param_bounds
# (rows, cols, offset of the tensor in floats modulo 4, decimal exponent of its scale)
BOUND_TENSORS = [(1, 7, 1, 0), (3, 100, 0, -2), (1, 768, 0, 1), (5, 768, 2, 0), (300, 64, 0, -3), (130, 260, 0, 2), (2, 8, 0, None)]


def _bounds_layout():
    g = np.random.default_rng(21)
    offs, parts, o = [], [], 0
    for rows, cols, mod, dec in BOUND_TENSORS:
        gap = 8 + (mod - o - 8) % 4                          # NaN between the tensors
        parts.append(np.full(gap, np.nan, dtype=np.float32))
        o += gap
        offs.append(o)
        t = np.zeros(rows * cols, dtype=np.float32) if dec is None else (g.standard_normal(rows * cols) * 10.0 ** dec).astype(np.float32)
        parts.append(t)
        o += t.size
    return offs, np.concatenate(parts)


def _run_bounds(dev, flat, offs):
    n = len(BOUND_TENSORS)
    base = nan_in(f32(flat), dev)
    assert base.data_ptr() % 16 == 0
    tab = np.zeros((n, 2), dtype=np.int64)
    for i, (rows, cols, _, _) in enumerate(BOUND_TENSORS):
        tab[i] = (offs[i], rows | (cols << 32))
    tabd = torch.from_numpy(tab).to(dev)
    out = Guard((2 * n,), dev)
    L().dupl_param_bounds(base.data_ptr(), tabd.data_ptr(), n, out.ptr, stream())
    return out.cpu().numpy().reshape(n, 2)


def test_param_bounds(dev):
    """max-abs bit-exact, the row norm within split_ref.row_norm_bound: a 7-element vector at an odd offset (scalar path), ragged and
    aligned matrices, rows that are a multiple of 4 long but misaligned, more than 128 rows (a second trip of the row loop),
    an all-zero tensor"""
    offs, flat = _bounds_layout()
    assert offs[0] % 2 == 1 and offs[3] % 4 == 2
    got = _run_bounds(dev, flat, offs)
    T = Tally("param_bounds row norm")
    for i, (rows, cols, _, _) in enumerate(BOUND_TENSORS):
        t = flat[offs[i]:offs[i] + rows * cols].reshape(rows, cols)
        amax, rnorm = S.param_bounds_ref(t)
        assert word(got[i, 0]) == word(amax), f"tensor {i}: max-abs {got[i, 0]!r}, exact {amax!r}"
        T.add(f"tensor {i} {rows}x{cols}", abs(float(got[i, 1]) - rnorm), S.row_norm_bound(rows, cols, offs[i]) * rnorm)
    assert tuple(got[6]) == (0.0, 0.0)
    T.done()


@pytest.mark.parametrize("which,pos,val", [(1, 5, NAN), (5, 130 * 260 - 3, NAN), (0, 6, NAN), (4, 150 * 64 + 1, float("inf")),
                                           (4, 299 * 64 + 63, float("-inf"))],
                         ids=["nan_first_row", "nan_last_row_of_largest", "nan_scalar_path", "inf", "neg_inf_last_element"])
def test_param_bounds_nonfinite(dev, which, pos, val):
    """a NaN or an Inf gives (+inf, +inf) for its tensor and leaves every other tensor's pair as it was"""
    offs, flat = _bounds_layout()
    clean = _run_bounds(dev, flat, offs)
    flat = flat.copy()
    flat[offs[which] + pos] = val
    got = _run_bounds(dev, flat, offs)
    assert np.isposinf(got[which]).all(), got[which]
    others = [i for i in range(len(BOUND_TENSORS)) if i != which]
    assert (got[others].view(np.uint32) == clean[others].view(np.uint32)).all() and np.isfinite(got[others]).all()


def test_param_bounds_refusals(dev):
    base, tab, out = nan_in(torch.ones(8), dev), torch.zeros(2, dtype=torch.int64, device=dev), Guard((2,), dev)
    raw = L().dupl_param_bounds.raw
    for args in [(base.data_ptr(), tab.data_ptr(), 0, out.ptr), (base.data_ptr(), tab.data_ptr(), -1, out.ptr),
                 (None, tab.data_ptr(), 1, out.ptr), (base.data_ptr(), None, 1, out.ptr), (base.data_ptr(), tab.data_ptr(), 1, None)]:
        assert raw(*args, stream()) == ERR_ARG, args
    torch.cuda.synchronize()
    assert out.untouched()
