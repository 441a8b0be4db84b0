"""Guard bands for buffers handed to the C ABI: did a call write outside the bytes it was given?

``Guarded(nbytes, device, fill)`` is ONE uint8 allocation ``[front pad | interior | back pad]``.  Both pads hold the byte 0xA5 (not zero,
not a NaN pattern, not -1, nothing a kernel writes as padding); the interior holds ``fill`` (0xFF for outputs: NaN as fp32 / fp16 / bf16 and
-1 as an integer, so an element the kernel never wrote still shows in the value check).  The interior starts on a 256-byte boundary.
``.strided`` gives a row view with ld > cols whose inter-row gaps carry the guard byte too.  ``check()`` synchronises and asserts that every
guard byte is unchanged, reporting the first and last changed byte RELATIVE TO THE INTERIOR'S END (an overrun of `n` rows of pitch `p`
reads as an offset below n * p; a negative offset lies in a row gap or, below -nbytes, in the front pad).

What this sees and what it does not:
  * the pad is DERIVED, not measured: one full 256-row tile (the largest row tile in the tree) at the tested row pitch, at least 64 KiB.
    A stray write that lands further away than the pad is NOT detected;
  * a read past a buffer is not detected at all -- only, by running a case with two different pad contents (``guard=0x00`` and
    ``guard=0xFF``), whether a RESULT depends on it.  Every byte a test may see overwritten is memory the test itself owns.

``exact_workspaces(monkeypatch)`` replaces ``rap_amd``'s grow-only scratch buffer with a fresh ``Guarded`` of exactly the requested bytes
per request, so every wrapper runs with what its ``rap_*_workspace_bytes()`` query returned and not one byte more.
"""
import math

import torch

GUARD = 0xA5
ROW_TILE = 256                  # the largest row tile of any kernel in the tree (256 x 256 GEMM tiles, 256-query attention items)
PAD_FLOOR = 64 * 1024
ALIGN = 256
WORKSPACE_MODULES = ("procrustes", "selection", "metrics", "data", "spinnet", "modeling", "flow_model")


def pad_bytes(pitch: int = 0) -> int:
    """bytes of each pad for rows of `pitch` bytes: one full ROW_TILE-row tile, at least PAD_FLOOR, a multiple of ALIGN"""
    return -(-max(PAD_FLOOR, ROW_TILE * int(pitch)) // ALIGN) * ALIGN


class GuardError(AssertionError):
    pass


class Guarded:
    def __init__(self, nbytes: int, device, fill: int = 0xFF, pitch: int = 0, guard: int = GUARD, name: str = ""):
        self.nbytes, self.fill, self.guard, self.name = int(nbytes), int(fill), int(guard), name
        pad = pad_bytes(pitch)
        self.buf = torch.empty(pad + self.nbytes + pad + ALIGN, dtype=torch.uint8, device=device)
        self.start = pad + (-(self.buf.data_ptr() + pad)) % ALIGN       # >= pad bytes in front, interior on a 256-byte boundary
        self.end = self.start + self.nbytes                               # >= pad bytes behind
        self.buf.fill_(self.guard)
        self.interior = self.buf[self.start:self.end]
        self.interior.fill_(self.fill)
        self.is_guard = torch.ones_like(self.buf, dtype=torch.bool)
        self.is_guard[self.start:self.end] = False
        assert (self.buf.data_ptr() + self.start) % ALIGN == 0 and self.start >= pad and self.buf.numel() - self.end >= pad

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.start

    def view(self, dtype, shape) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        assert n <= self.nbytes, (n, self.nbytes)
        return self.interior[:n].view(dtype).view(shape)

    def strided(self, dtype, rows: int, cols: int, ld: int) -> torch.Tensor:
        """(rows, cols) view with row pitch ld >= cols elements; the ld - cols elements after every row become guard bytes"""
        isz = torch.empty((), dtype=dtype).element_size()
        assert ld >= cols and ((rows - 1) * ld + cols) * isz <= self.nbytes, (rows, cols, ld, self.nbytes)
        full = min(rows, self.nbytes // (ld * isz))                       # rows whose whole pitch lies inside the interior
        if ld > cols and full:
            for t, val in ((self.buf, self.guard), (self.is_guard, True)):
                t[self.start:self.start + full * ld * isz].view(full, ld * isz)[:, cols * isz:] = val
        for r in range(full, rows):                                       # (a last row that ends before its pitch does)
            a, b = self.start + (r * ld + cols) * isz, min(self.start + (r + 1) * ld * isz, self.end)
            self.buf[a:b] = self.guard
            self.is_guard[a:b] = True
        span = min(rows * ld * isz, self.nbytes) // isz
        return torch.as_strided(self.interior[:span * isz].view(dtype), (rows, cols), (ld, 1))

    def put(self, t: torch.Tensor) -> torch.Tensor:
        """copy a contiguous tensor into the front of the interior; returns the view that holds it"""
        t = t.contiguous()
        v = self.view(t.dtype, t.shape)
        v.copy_(t)
        return v

    def check(self) -> None:
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        bad = ((self.buf != self.guard) & self.is_guard).nonzero().flatten()
        if bad.numel():
            first, last = int(bad[0]) - self.end, int(bad[-1]) - self.end
            where = "front pad" if int(bad[0]) < self.start else ("row gap" if int(bad[0]) < self.end else "back pad")
            raise GuardError(f"guard {self.name!r}: {bad.numel()} guard bytes changed around an interior of {self.nbytes} bytes; first at offset "
                             f"{first}, last at offset {last} relative to the interior's end (first one in the {where}; "
                             f"{int(bad[0]) - self.start} from the interior's start)")

    def untouched(self) -> bool:
        """the interior still holds `fill` everywhere (row gaps aside): a refused call wrote nothing"""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        return bool(((self.buf == self.fill) | self.is_guard)[self.start:self.end].all())


def guarded_like(t: torch.Tensor, device, guard: int = GUARD, name: str = ""):
    """-> (Guarded, view): the contiguous tensor `t` on `device` with `guard` bytes either side of it (an INPUT placed in a guard)"""
    t = t.contiguous()
    g = Guarded(t.numel() * t.element_size(), device, fill=0, pitch=(t.shape[-1] * t.element_size() if t.dim() > 1 else 0), guard=guard, name=name)
    return g, g.put(t)


class ExactWorkspaces:
    def __init__(self, pitch: int):
        self.pitch, self.handed = pitch, []

    def workspace(self, device, nbytes: int) -> torch.Tensor:
        g = Guarded(int(nbytes), device, fill=0xFF, pitch=self.pitch, name=f"workspace #{len(self.handed)} ({int(nbytes)} bytes)")
        self.handed.append(g)
        return g.view(torch.uint8, (int(nbytes),))

    def check_all(self) -> None:
        assert self.handed, "no workspace was requested: the call under test did not go through rap_amd's workspace()"
        for g in self.handed:
            g.check()


def exact_workspaces(monkeypatch, pitch: int = 8192) -> ExactWorkspaces:
    """Every ``workspace(device, nbytes)`` request of a rap_amd module is answered with the interior of a fresh Guarded of exactly nbytes
    (pads: one 256-row tile of `pitch` bytes; the default 8 KiB is the widest scratch row of the models these tests run, 2 * 4 * 256
    fp32).  Undone by pytest's monkeypatch at the end of the test."""
    import importlib
    ex = ExactWorkspaces(pitch)
    for name in WORKSPACE_MODULES:
        mod = importlib.import_module(f"rap_amd.{name}")
        assert hasattr(mod, "workspace"), name
        monkeypatch.setattr(mod, "workspace", ex.workspace)
    return ex
