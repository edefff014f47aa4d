"""Guard-band allocator for the memory-contract tests (tests/test_gpu_memory_contract.py, tests/test_guard_host.py).

The package allocates every caller-visible buffer through ``torch.empty / zeros / empty_like / zeros_like`` looked up on
the module-level name ``torch``, and the library never allocates such a buffer itself.  ``Guard`` replaces that name in
the listed package modules, for the length of a ``with`` block, by a proxy that forwards everything except those four
functions.  Each of them returns a contiguous view into one larger ``uint8`` allocation

    [ front band | interior | back band ]

whose bands and (for ``empty`` / ``empty_like``) interior are filled with one byte value.  The interior starts on a
512-byte boundary (the library asks 256 for arenas, 16 for operands); the back band starts at the byte after the
interior's last one, so a one-element overrun is seen.  ``zeros`` / ``zeros_like`` interiors are zero: the
accumulate-into gradients rely on it.

Band size is not a knob.  It is the largest unconditional store unit include/gww.h documents -- two 256-row panels =
512 rows -- of the buffer's own row pitch (its last dimension), and for a byte arena or any other 1-D buffer, which has
no pitch of its own, 512 rows of the widest row the library carves from it, given by the caller as ``arena_row_bytes``
(``4 * max(3 * d_model, ffn)`` for the encoder arenas).  Never less than 1 MiB.

Fill bytes: 0xFF (NaN as fp32 / bf16 / fp64, -1 as an integer), 0x7F (3.39e38: finite, so a masked ``0 * garbage`` stays
clean but a sum over it does not) and 0x00, the benign value ordinary allocations tend to hold, kept as the third.

What this sees: a stray WRITE outside a buffer (``check``), a MISSING write (``unwritten``: interior elements that still
hold the fill pattern) and a RESULT THAT DEPENDS on bytes outside the contract (run under two fills, compare bits).  What
it cannot see: a stray READ whose value is discarded.  A stray access it catches lands, by construction, inside memory
the test owns.
"""

from __future__ import annotations

import contextlib
import importlib
import os
import traceback

import torch as _torch

FILLS = (0xFF, 0x7F, 0x00)
ALIGN = 512
PANEL_ROWS = 512            # two 256-row panels: the slack csrc/encoder_impl.h (padded_rows) itself reasons in
MIN_BAND = 1 << 20

PACKAGE_MODULES = tuple("gw_whisper_amd." + m for m in
                        ("ops", "encoder", "training", "whiten", "qscan", "inference", "glitch", "mlgwsc_train"))

_ALLOC_KWARGS = {"dtype", "device", "requires_grad", "layout", "pin_memory", "memory_format"}


def encoder_arena_row_bytes(d_model: int, ffn: int) -> int:
    """Widest row the library carves from the encoder / training arenas: fp32 [., max(3 d, ffn)]."""
    return 4 * max(3 * d_model, ffn)


class GuardError(AssertionError):
    pass


class _Record:
    __slots__ = ("raw", "off", "nbytes", "band", "shape", "dtype", "site", "kind")

    def __init__(self, raw, off, nbytes, band, shape, dtype, site, kind):
        self.raw, self.off, self.nbytes, self.band = raw, off, nbytes, band
        self.shape, self.dtype, self.site, self.kind = tuple(shape), dtype, site, kind

    def describe(self) -> str:
        return f"{self.kind} {self.shape} {self.dtype} ({self.nbytes} bytes, bands {self.band}) allocated at {self.site}"


def _site() -> str:
    here = os.path.abspath(__file__)
    for fr in reversed(traceback.extract_stack()):
        if os.path.abspath(fr.filename) != here and "contextlib" not in fr.filename:
            return f"{os.path.basename(fr.filename)}:{fr.lineno} in {fr.name}"
    return "?"


class _TorchProxy:
    """Stands in for the module ``torch``: forwards every attribute except the four allocation functions."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    @staticmethod
    def _shape(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
            return tuple(int(s) for s in args[0])
        return tuple(int(s) for s in args)

    def _new(self, real, kind, zero, args, kw):
        unknown = set(kw) - _ALLOC_KWARGS
        assert not unknown, f"guard: torch.{kind} called with keyword(s) {sorted(unknown)} the proxy does not know"
        device = _torch.device(kw.get("device") or "cpu")
        if not self._guard._wants(device):
            return real(*args, **kw)
        dtype = kw.get("dtype") or _torch.get_default_dtype()
        t = self._guard._alloc(self._shape(args), dtype, device, kind, zero)
        return t.requires_grad_() if kw.get("requires_grad") else t

    def _like(self, real, kind, zero, x, kw):
        unknown = set(kw) - _ALLOC_KWARGS
        assert not unknown, f"guard: torch.{kind} called with keyword(s) {sorted(unknown)} the proxy does not know"
        device = _torch.device(kw.get("device") or x.device)
        if not self._guard._wants(device):
            return real(x, **kw)
        return self._guard._alloc(tuple(x.shape), kw.get("dtype") or x.dtype, device, kind, zero)

    def empty(self, *args, **kw):
        return self._new(_torch.empty, "empty", False, args, kw)

    def zeros(self, *args, **kw):
        return self._new(_torch.zeros, "zeros", True, args, kw)

    def empty_like(self, x, **kw):
        return self._like(_torch.empty_like, "empty_like", False, x, kw)

    def zeros_like(self, x, **kw):
        return self._like(_torch.zeros_like, "zeros_like", True, x, kw)


class Guard:
    """One guarded run: ``with Guard(0xFF, arena_row_bytes=...) as g: out = op(g.place(x)); g.check()``.

    ``modules``: the modules whose name ``torch`` is replaced (names or module objects; default: the package modules
    that allocate).  ``cpu=True`` guards CPU allocations too (the host self-tests); GPU allocations always are."""

    def __init__(self, fill: int, arena_row_bytes: int = 0, modules=None, cpu: bool = False):
        assert fill in FILLS, f"fill byte must be one of {[hex(f) for f in FILLS]}"
        self.fill = int(fill)
        self.arena_row_bytes = int(arena_row_bytes)
        self.cpu = bool(cpu)
        self.records: list[_Record] = []
        self.n_alloc = 0            # allocations through the proxy (placed inputs do not count)
        self._modules = PACKAGE_MODULES if modules is None else tuple(modules)
        self._stack = None

    # ---- scope
    def __enter__(self):
        self._stack = contextlib.ExitStack()
        proxy = _TorchProxy(self)
        for m in self._modules:
            mod = importlib.import_module(m) if isinstance(m, str) else m
            assert getattr(mod, "torch", None) is _torch, f"guard: {mod.__name__} has no module-level name 'torch'"
            setattr(mod, "torch", proxy)
            self._stack.callback(setattr, mod, "torch", _torch)
        return self

    def __exit__(self, *exc):
        self._stack.close()
        self._stack = None
        return False

    # ---- allocation
    def _wants(self, device) -> bool:
        return device.type == "cuda" or (self.cpu and device.type == "cpu")

    def band_bytes(self, shape, itemsize: int, pitch_elems: int | None = None) -> int:
        if pitch_elems is not None:
            row = pitch_elems * itemsize
        elif len(shape) >= 2:
            row = int(shape[-1]) * itemsize
        else:
            row = self.arena_row_bytes
        return max(MIN_BAND, PANEL_ROWS * row)

    def _block(self, nbytes: int, band: int, device, shape, dtype, kind) -> _Record:
        raw = _torch.empty((band + ALIGN + nbytes + band,), dtype=_torch.uint8, device=device)
        off = band + (-(raw.data_ptr() + band)) % ALIGN
        raw.fill_(self.fill)
        rec = _Record(raw, off, nbytes, band, shape, dtype, _site(), kind)
        self.records.append(rec)
        return rec

    def _alloc(self, shape, dtype, device, kind, zero):
        itemsize = _torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        rec = self._block(numel * itemsize, self.band_bytes(shape, itemsize), device, shape, dtype, kind)
        self.n_alloc += 1
        interior = rec.raw[rec.off:rec.off + rec.nbytes]
        if zero:
            interior.zero_()
        return interior.view(dtype).view(shape)

    def empty(self, shape, dtype, device="cuda"):
        """A guarded buffer for a test that calls the C entry point itself (interior = fill)."""
        return self._alloc(tuple(int(s) for s in shape), dtype, _torch.device(device), "empty", False)

    def zeros(self, shape, dtype, device="cuda"):
        return self._alloc(tuple(int(s) for s in shape), dtype, _torch.device(device), "zeros", True)

    def allocations(self, site: str = "", shape=None, kind: str = ""):
        """The recorded allocations whose call site contains ``site`` (and of that shape / kind): how a test shows
        that a buffer it cannot reach -- one autograd took over -- was allocated under the guard."""
        return [r for r in self.records if site in r.site and kind in r.kind
                and (shape is None or tuple(shape) == r.shape)]

    def interior(self, rec):
        """The typed view of a recorded allocation's interior (what the proxy returned for it)."""
        return rec.raw[rec.off:rec.off + rec.nbytes].view(rec.dtype).view(rec.shape)

    def place(self, tensor, pitch: int | None = None, device=None):
        """Copy a test input into a guarded block.  ``pitch`` (elements, >= the row length): the rows of a 2-D input are
        laid out with that stride -- the gap between row end and stride, also behind the last row, holds the fill -- and
        the strided [rows, n] view is returned."""
        t = tensor.detach()
        device = _torch.device(device) if device is not None else t.device
        itemsize = t.element_size()
        if pitch is None:
            t = t.contiguous()
            rec = self._block(t.numel() * itemsize, self.band_bytes(t.shape, itemsize), device, t.shape, t.dtype, "place")
            view = rec.raw[rec.off:rec.off + rec.nbytes].view(t.dtype).view(t.shape)
            view.copy_(t)
            return view
        assert t.dim() == 2 and pitch >= t.shape[1], "place(pitch=): a 2-D input and a pitch >= its row length"
        rows, n = t.shape
        rec = self._block(rows * pitch * itemsize, self.band_bytes(t.shape, itemsize, pitch), device, (rows, pitch), t.dtype,
                          f"place(pitch={pitch})")
        view = rec.raw[rec.off:rec.off + rec.nbytes].view(t.dtype).view(rows, pitch)[:, :n]
        view.copy_(t)
        return view

    # ---- queries
    def _record_of(self, tensor):
        if tensor is None or not _torch.is_tensor(tensor):
            return None
        p = tensor.data_ptr()
        store = tensor.untyped_storage().data_ptr()
        for rec in self.records:
            lo = rec.raw.data_ptr() + rec.off
            if rec.raw.untyped_storage().data_ptr() == store and lo <= p and (p < lo + rec.nbytes or rec.nbytes == 0):
                return rec
        return None

    def owns(self, tensor) -> bool:
        """True when ``tensor`` is (a view into) the interior of a block this guard made."""
        return self._record_of(tensor) is not None

    def repoison(self, tensor, fill: int | None = None):
        """Refill the whole interior of the block ``tensor`` lives in (scratch between two library calls)."""
        rec = self._record_of(tensor)
        assert rec is not None, "repoison: not a guarded tensor"
        rec.raw[rec.off:rec.off + rec.nbytes].fill_(self.fill if fill is None else int(fill))

    def unwritten_mask(self, tensor):
        """Flat bool mask of the elements of ``tensor`` whose bytes all still hold the fill byte (a missing write).
        Meaningless for fill 0x00, where a legitimate zero looks the same: asserted only under 0xFF and 0x7F."""
        t = tensor.detach().contiguous()
        b = t.view(-1).view(_torch.uint8).view(t.numel(), t.element_size())
        return (b == self.fill).all(dim=1)

    def unwritten(self, tensor) -> int:
        """Number of elements of ``tensor`` that still hold the fill pattern."""
        return int(self.unwritten_mask(tensor).sum().item()) if tensor.numel() else 0

    def check(self):
        """Synchronise, then assert that at least one allocation went through the guard and that every band still
        holds its fill byte.  Offsets in the report are bytes relative to the interior's first byte (negative: in front
        of it; >= the interior's size: behind it)."""
        if _torch.cuda.is_available() and any(r.raw.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        if self.n_alloc == 0:
            raise GuardError("guard: no allocation went through the proxy -- this case tests nothing")
        problems = []
        for rec in self.records:
            for name, lo, hi in (("front", 0, rec.off), ("back", rec.off + rec.nbytes, rec.raw.numel())):
                bad = (rec.raw[lo:hi] != self.fill).nonzero()
                if bad.numel():
                    first, last = int(bad[0]) + lo - rec.off, int(bad[-1]) + lo - rec.off
                    problems.append(f"{name} band damaged: offsets {first} .. {last} relative to the interior "
                                    f"({rec.nbytes} bytes), extent {last - first + 1} bytes, {int(bad.numel())} bytes changed; "
                                    f"{rec.describe()}")
        if problems:
            raise GuardError("guard (fill 0x%02X): " % self.fill + "\n  ".join(problems))


class NoGuard:
    """The unguarded run of a case: plain tensors from the ordinary allocator, the same call surface."""
    fill = None

    def place(self, tensor, pitch: int | None = None, device=None):
        t = tensor.detach()
        device = _torch.device(device) if device is not None else t.device
        if pitch is None:
            return t.to(device, copy=True).contiguous()
        buf = _torch.zeros((t.shape[0], pitch), dtype=t.dtype, device=device)
        buf[:, :t.shape[1]].copy_(t)
        return buf[:, :t.shape[1]]

    def empty(self, shape, dtype, device="cuda"):
        return _torch.empty(tuple(shape), dtype=dtype, device=device)

    def zeros(self, shape, dtype, device="cuda"):
        return _torch.zeros(tuple(shape), dtype=dtype, device=device)

    def owns(self, tensor) -> bool:
        return True

    def repoison(self, tensor, fill=None):
        pass


def run_contract(fn, arena_row_bytes: int = 0, modules=None, cpu: bool = False, may_hold_fill=(), fills=FILLS,
                 atomic=None):
    """The contract check of one case.  ``fn(g)`` runs the op with its inputs ``g.place``d and returns a dict
    name -> tensor restricted to the DOCUMENTED extent of every output it inspects.  It is run once per fill byte under a ``Guard``
    and then unguarded (``NoGuard``); after each guarded run the bands are checked, every returned tensor must
    come from the guard (``owns``) and -- except the names in ``may_hold_fill``, outputs the contract leaves partly
    unwritten -- must hold no element that still carries a non-zero fill pattern.  Then every result must be
    bit-identical to the unguarded one and to each other, and finite.  ``atomic`` = {name: rel}: outputs of the few
    kernels that sum with float atomics, whose bits differ from run to run by design; they are compared to within
    ``rel`` of their largest entry -- the run-to-run bound the existing test of that op asserts -- which a NaN or a
    3.39e38 that leaked in still fails.  Returns the 0xFF run's tensors (clones)."""
    atomic = dict(atomic or {})
    runs = {}
    for fill in fills:
        with Guard(fill, arena_row_bytes, modules, cpu) as g:
            out = fn(g)
            g.check()
            assert out, "run_contract: the case returned no output"
            for name, t in out.items():
                assert g.owns(t), f"output {name!r} did not come from the guard (fill 0x{fill:02X})"
                if fill != 0 and name not in may_hold_fill:
                    n = g.unwritten(t)
                    assert n == 0, (f"output {name!r}: {n} element(s) the contract says are written still hold the fill "
                                    f"0x{fill:02X}, first at flat index {int(g.unwritten_mask(t).nonzero()[0])}")
            runs[fill] = {k: v.detach().clone() for k, v in out.items()}
    # (the unguarded run comes last: a stray store has been caught inside owned memory by then)
    r0 = {k: v.detach().clone() for k, v in fn(NoGuard()).items()}
    assert set(r0) == set(runs[fills[0]])
    for fill, r in runs.items():
        for name, t in r.items():
            if t.is_floating_point() and name not in may_hold_fill:
                assert bool(_torch.isfinite(t).all()), f"output {name!r} is not finite under fill 0x{fill:02X}"
            if name in atomic:
                diff = float((t.double() - r0[name].double()).abs().max())
                assert diff <= atomic[name] * float(r0[name].double().abs().max()), \
                    f"output {name!r} under fill 0x{fill:02X} differs from the unguarded run by {diff}"
                continue
            assert _torch.equal(t, r0[name]), (f"output {name!r} under fill 0x{fill:02X} differs from the unguarded run: it "
                                               f"depends on bytes outside the contract")
    return runs[fills[0]]
