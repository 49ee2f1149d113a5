"""Poisoned, guarded allocations for the buffers the library allocates itself.

Every device buffer of ``flooder_amd`` is a ``torch.empty`` / ``empty_like`` / ``zeros`` / ``full`` ... of its Python
drivers.  ``poisoned(pattern, device_type)`` replaces those constructors for the duration of a ``with`` block:

* ``torch.empty``, ``torch.empty_like``: ``nbytes + 2 * GUARD`` bytes of uint8 from the real constructor, the WHOLE block
  filled with the byte ``pattern`` (on the current stream, like the library's own launches), and the payload returned as
  ``raw[GUARD:GUARD + nbytes].view(dtype).view(shape)``.  A kernel that reads a word of such a buffer before any launch
  of the call has written it reads the pattern, and its result changes with the pattern.
* ``torch.zeros``, ``torch.zeros_like``, ``torch.full``, ``torch.full_like``, ``Tensor.new_zeros``: the same guards, the
  payload initialised as asked (guarded, not poisoned).
* passed through to the real constructor: tensors of another device type, zero-element tensors, ``out=``,
  ``pin_memory=True``, a non-contiguous ``memory_format`` (and ``*_like`` of a non-contiguous tensor, whose strides the
  default ``preserve_format`` copies), other layouts, named tensors.

GUARD = 512 bytes is the caching allocator's own rounding: the payload keeps the address alignment it has in an
unpatched run, and the upper guard starts at the first byte behind the payload - where an overrun of a few elements
lands in the allocator's slack and nothing notices.

The recorder ``rec`` keeps every raw block alive until the block ends (no guard is handed out again as somebody's
payload) and ``rec.broken()`` - to be called INSIDE the block - synchronises and lists every allocation with a guard
byte that no longer equals ``pattern``: shape, dtype, side, and the allocating line in ``flooder_amd``.

The three patterns (``PATTERNS``), and why one is not enough:

* ``0xFF``: floats are NaN, ints are -1.  As unsigned bits it is the maximum, so an atomic-min buffer that was never
  filled looks correctly initialised;
* ``0x7F``: floats are 3.39e38 - finite, and below the +inf word 0x7F800000 - ints are large and positive;
* ``0x01``: floats are tiny, ints are small positive counters and indices: it wins every such minimum and makes every
  counter non-zero.

Plain Python; needs no GPU to import (tests/test_poison_helper_cpu.py runs it on CPU tensors).
"""
import contextlib
import os
import sys

import torch

GUARD = 512
PATTERNS = (0xFF, 0x7F, 0x01)
PACKAGE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flooder_amd")

# what the helper replaces, as the coverage check of tests/test_poison_helper_cpu.py spells an attribute reference:
# "torch.<name>" for a function of the module, "<obj>.<name>" for a method of a tensor
POISONED = ("torch.empty", "torch.empty_like")
GUARDED_ONLY = ("torch.zeros", "torch.zeros_like", "torch.full", "torch.full_like", "<obj>.new_zeros")
WRAPPED = POISONED + GUARDED_ONLY


class Allocation:
    """One guarded block: ``raw`` (uint8, guard | payload | guard), what was asked for, and who asked."""
    __slots__ = ("raw", "nbytes", "shape", "dtype", "kind", "where")

    def __init__(self, raw, nbytes, shape, dtype, kind, where):
        self.raw, self.nbytes, self.shape, self.dtype, self.kind, self.where = raw, nbytes, shape, dtype, kind, where


class Recorder:
    def __init__(self, pattern, device_type):
        self.pattern, self.device_type = int(pattern), device_type
        self.allocations = []
        self.passed_through = 0
        self.open = True

    def __len__(self):
        return len(self.allocations)

    def broken(self):
        """[{shape, dtype, side, where, kind}] for every allocation with a changed guard byte ("below": the 512 bytes in
        front of the payload, "above": those behind it).  Synchronises the device first."""
        if not self.open:
            raise RuntimeError("Recorder.broken() after the block has ended: the raw blocks are released")
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        out = []
        by_device = {}
        for a in self.allocations:
            by_device.setdefault(a.raw.device, []).append(a)
        for allocs in by_device.values():
            for first in range(0, len(allocs), 1024):
                part = allocs[first:first + 1024]
                guards = torch.stack([g for a in part for g in (a.raw[:GUARD], a.raw[GUARD + a.nbytes:])])
                bad = (guards != self.pattern).any(dim=1).cpu().tolist()
                for i, a in enumerate(part):
                    for side, hit in (("below", bad[2 * i]), ("above", bad[2 * i + 1])):
                        if hit:
                            out.append(dict(shape=a.shape, dtype=a.dtype, side=side, where=a.where, kind=a.kind))
        return out


def _caller_in_package():
    """"flooder_amd/file.py:line" of the innermost frame of the call stack that lies in flooder_amd/ and " <- file.py:line"
    of the package frame that called it (the innermost one may be a small helper of the driver, as ``empty`` of
    ``FusedWorkspace``); outside the package: the caller's "file.py:line"."""
    f = sys._getframe(1)
    first, inside = None, []
    while f is not None and len(inside) < 2:
        name = f.f_code.co_filename
        if name != __file__:
            if first is None:
                first = f"{os.path.basename(name)}:{f.f_lineno}"
            if os.path.dirname(os.path.abspath(name)) == PACKAGE_DIR:
                inside.append(f"{os.path.basename(name)}:{f.f_lineno}")
        f = f.f_back
    return "flooder_amd/" + " <- ".join(inside) if inside else first


def _shape_of(args, kw):
    """The size of ``torch.empty(*size)`` / ``torch.empty(size)`` / ``torch.empty(size=...)`` as a tuple of ints."""
    if "size" in kw:
        size = kw.pop("size")
    elif len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        size = args[0]
    else:
        size = args
    if isinstance(size, int):
        size = (size,)
    return tuple(int(s) for s in size)


def _default_device():
    return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")


@contextlib.contextmanager
def poisoned(pattern, device_type="cuda"):
    """Replace the constructors of ``WRAPPED`` until the block ends (always restored) -> the ``Recorder``."""
    if not 0 <= int(pattern) <= 0xFF:
        raise ValueError("pattern is one byte")
    rec = Recorder(pattern, device_type)
    real = {name: getattr(torch, name) for name in ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like")}
    real_new_zeros, own_new_zeros = torch.Tensor.new_zeros, "new_zeros" in torch.Tensor.__dict__
    contiguous = (None, torch.contiguous_format)

    def plain(kw):
        """None of the keywords that ask for something a guarded view cannot be."""
        return (kw.get("out") is None and not kw.get("pin_memory", False) and kw.get("names") is None
                and kw.get("layout", torch.strided) is torch.strided)

    def guarded(shape, dtype, device, requires_grad, kind, init):
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * real["empty"](0, dtype=dtype).element_size()
        raw = real["empty"](nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
        raw.fill_(rec.pattern)
        payload = raw[GUARD:GUARD + nbytes].view(dtype).view(shape)
        init(payload)
        rec.allocations.append(Allocation(raw, nbytes, shape, dtype, kind, _caller_in_package()))
        return payload.requires_grad_(True) if requires_grad else payload

    def factory(kind, args, kw, init, default_dtype=None, more=()):
        """``torch.<kind>(*size, *more, ...)``: guarded where it is a plain dense tensor of ``device_type`` with elements."""
        keep_args, keep_kw = args, dict(kw)
        kw = dict(kw)
        try:
            shape = _shape_of(args, kw)
        except (TypeError, ValueError):
            shape = None
        device = torch.device(kw["device"]) if kw.get("device") is not None else _default_device()
        if (shape is None or not plain(kw) or kw.get("memory_format") not in contiguous or device.type != rec.device_type
                or 0 in shape or any(s < 0 for s in shape)):
            rec.passed_through += 1
            return real[kind](*keep_args, *more, **keep_kw)
        dtype = kw.get("dtype") or default_dtype or torch.get_default_dtype()
        return guarded(shape, dtype, device, bool(kw.get("requires_grad", False)), kind, init)

    def like(kind, t, kw, init):
        """``torch.<kind>_like(t, ...)``."""
        fmt = kw.get("memory_format", torch.preserve_format)
        device = torch.device(kw["device"]) if kw.get("device") is not None else t.device
        dense = t.layout is torch.strided and (fmt is torch.contiguous_format
                                               or (fmt in (None, torch.preserve_format) and t.is_contiguous()))
        if not dense or not plain(kw) or device.type != rec.device_type or t.numel() == 0:
            return None
        return guarded(tuple(t.shape), kw.get("dtype") or t.dtype, device, bool(kw.get("requires_grad", False)),
                       kind, init)

    def nothing(payload):
        pass

    def empty(*args, **kw):
        return factory("empty", args, kw, nothing)

    def zeros(*args, **kw):
        return factory("zeros", args, kw, lambda p: p.zero_())

    def full(size, fill_value, **kw):
        inferred = None if kw.get("dtype") is not None else real["full"]((1,), fill_value).dtype
        return factory("full", (size,), kw, lambda p: p.fill_(fill_value), inferred, (fill_value,))

    def empty_like(t, **kw):
        got = like("empty_like", t, kw, nothing)
        if got is None:
            rec.passed_through += 1
            return real["empty_like"](t, **kw)
        return got

    def zeros_like(t, **kw):
        got = like("zeros_like", t, kw, lambda p: p.zero_())
        if got is None:
            rec.passed_through += 1
            return real["zeros_like"](t, **kw)
        return got

    def full_like(t, fill_value, **kw):
        got = like("full_like", t, kw, lambda p: p.fill_(fill_value))
        if got is None:
            rec.passed_through += 1
            return real["full_like"](t, fill_value, **kw)
        return got

    def new_zeros(self, *args, **kw):
        keep = dict(kw)
        try:
            shape = _shape_of(args, kw)
        except (TypeError, ValueError):
            shape = None
        device = torch.device(kw["device"]) if kw.get("device") is not None else self.device
        if (shape is None or not plain(kw) or self.layout is not torch.strided or device.type != rec.device_type
                or 0 in shape or any(s < 0 for s in shape)):
            rec.passed_through += 1
            return real_new_zeros(self, *args, **keep)
        return guarded(shape, kw.get("dtype") or self.dtype, device, bool(kw.get("requires_grad", False)), "new_zeros",
                       lambda p: p.zero_())

    patched = dict(empty=empty, empty_like=empty_like, zeros=zeros, zeros_like=zeros_like, full=full, full_like=full_like)
    try:
        for name, f in patched.items():
            setattr(torch, name, f)
        torch.Tensor.new_zeros = new_zeros
        yield rec
    finally:
        for name, f in real.items():
            setattr(torch, name, f)
        if own_new_zeros:
            torch.Tensor.new_zeros = real_new_zeros
        elif "new_zeros" in torch.Tensor.__dict__:
            del torch.Tensor.new_zeros     # (inherited from the base class again)
        rec.open = False
        rec.allocations.clear()
