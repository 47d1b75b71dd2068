"""Sentinel / NaN-slack helpers shared by the kernel edge suites (tests/test_glue_kernels_gpu.py, tests/test_loss_norm_kernels_gpu.py):
every output lives inside a larger buffer whose slack holds a sentinel that must be bit-unchanged afterwards; every input lives
inside a buffer whose slack is NaN, so a finite result proves nothing else was read."""
import math

import numpy as np
import torch

NAN = float("nan")
EPS24 = 2.0 ** -24
PAD = 64                     # floats of slack on either side: keeps the 256-byte alignment of the allocation
PAD_U8 = 256                 # bytes of slack on either side of a uint8 view; front = PAD_U8 + k puts the view k bytes off alignment
SENT = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.int32: (torch.int32, -0x5A5A5A5B),
        torch.int64: (torch.int64, -0x5A5A5A5A5A5A5A5B), torch.uint8: (torch.uint8, 0xA5)}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def rndint(lo, hi, *shape, seed=0):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed))


class Guard:
    """A tensor of `shape` inside a larger device allocation; the slack holds a sentinel (a NaN payload for floats)."""

    def __init__(self, shape, dev, dtype=torch.float32, init=None, front=None, back=None):
        self.n = int(np.prod(shape)) if len(shape) else 1
        slack = PAD_U8 if dtype == torch.uint8 else PAD     # byte-granular kernels: an off-by-one write lands one byte past the view
        front, back = slack if front is None else front, slack if back is None else back
        self.front, self.back = front, back
        self.buf = torch.empty(self.n + front + back, dtype=dtype, device=dev)
        self.itype, self.pat = SENT[dtype]
        self.buf.view(self.itype).fill_(self.pat)
        self.view = self.buf[front:front + self.n].view(shape)
        if init is not None:
            self.view.copy_(init)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        i = self.buf.view(self.itype).cpu()
        return bool((i[:self.front] == self.pat).all()) and bool((i[self.front + self.n:] == self.pat).all())

    def untouched(self):
        return bool((self.buf.view(self.itype).cpu() == self.pat).all())

    def cpu(self):
        torch.cuda.synchronize()
        assert self.intact(), "the kernel wrote outside its output"
        return self.view.cpu()


_ALIVE = []                  # inputs handed to a kernel as bare pointers stay allocated until the test is over


def nan_in(t, dev, front=PAD, back=PAD):
    """t on the device inside a buffer whose slack is NaN; returns the view."""
    t = t.contiguous()
    buf = torch.full((t.numel() + front + back,), NAN, dtype=torch.float32, device=dev)
    view = buf[front:front + t.numel()].view(t.shape)
    view.copy_(t)
    _ALIVE.append(buf)
    return view


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def stream():
    from dupl_amd import ops
    return ops._stream()


def ratio_report(tag, err, bound, quiet=False):
    """worst err / bound, printed (unless quiet) and returned; a zero bound admits only a zero error"""
    err, bound = err.double(), bound.double().expand_as(err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(r.max()) if r.numel() else 0.0
    if not quiet:
        print(f"{tag}: worst err / bound {worst:.3f}")
    return worst


class Tally:
    """the worst err / bound over the comparisons of one test: every one must stay below 1; one line is printed at the end"""

    def __init__(self, tag):
        self.tag, self.worst, self.where, self.n = tag, 0.0, "", 0

    def add(self, name, err, bound):
        r = ratio_report(name, torch.as_tensor(err), torch.as_tensor(bound), quiet=True)
        self.n += 1
        if r >= self.worst:
            self.worst, self.where = r, name
        assert r < 1.0, f"{self.tag} {name}: err / bound {r:.3f}"
        return r

    def done(self):
        print(f"{self.tag}: worst err / bound {self.worst:.3f} ({self.where}; {self.n} comparisons)")
