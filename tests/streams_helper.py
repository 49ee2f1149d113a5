"""Helpers of tests/test_gpu_streams.py: the hold of the default stream and the held call.

The hold: ONE small kernel on the default stream that runs for a chosen wall time (``torch.cuda._sleep``, calibrated once
with two events; a fixed chain of large matmuls where the sleep kernel does not scale) and an event ``held`` recorded
behind it.  PyTorch's pool streams are non-blocking: work on a side stream does not wait for the default stream, so as
long as ``held.query()`` is False everything a side stream has finished was finished without the default stream and
without a device-wide wait.

The held call of ``f`` (``held_call``):
  1. reference: ``f(real)`` on the default stream, twice; the second run is timed (t_w)
  2. decoy: ``f(decoy)`` on the side stream - same shapes and options, other values, another result
  3. hold the default stream for max(20 t_w, 0.2 s), at most 3 s
  4. ``f(real)`` under ``torch.cuda.stream(side)``, every output brought to the host inside the context
  5. ``held.query()`` must still be False, and
  6. the outputs must equal the reference bit for bit.
"""
import time

import numpy as np
import torch

HOLD_FACTOR, HOLD_MIN_S, HOLD_CAP_S = 20, 0.2, 3.0
_CALIBRATION = {}


def _calibrate(dev):
    """("sleep", cycles per ms) or ("matmul", (operand, ms per product)) for the default stream of ``dev``."""
    if dev not in _CALIBRATION:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        how = None
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)   # (first use: the code object)
            cycles = 20_000_000
            a.record(); torch.cuda._sleep(cycles); b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            if ms > 0.5:
                rate = cycles / ms
                a.record(); torch.cuda._sleep(int(rate * 40)); b.record()   # does 40 ms asked give 40 ms?
                torch.cuda.synchronize()
                if 20.0 <= a.elapsed_time(b) <= 80.0:
                    how = ("sleep", rate)
        if how is None:
            x = torch.randn(4096, 4096, device=dev)
            torch.mm(x, x)
            torch.cuda.synchronize()
            a.record()
            for _ in range(8):
                torch.mm(x, x)
            b.record()
            torch.cuda.synchronize()
            how = ("matmul", (x, a.elapsed_time(b) / 8))
        _CALIBRATION[dev] = how
    return _CALIBRATION[dev]


def hold_kind(dev):
    return _calibrate(dev)[0]


def hold(dev, seconds):
    """Occupy the DEFAULT stream of ``dev`` for ``seconds`` -> the event ``held`` recorded behind the work."""
    kind, cal = _calibrate(dev)
    main = torch.cuda.default_stream(dev)
    with torch.cuda.stream(main):
        if kind == "sleep":
            torch.cuda._sleep(int(cal * seconds * 1e3))
        else:
            x, ms = cal
            for _ in range(max(1, int(seconds * 1e3 / ms) + 1)):
                torch.mm(x, x)
        held = torch.cuda.Event()
        held.record(main)
    return held


def to_host(x):
    """The outputs of a call as host data (tensors through ``.cpu()``: the wait is for the current stream only)."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    if isinstance(x, dict):
        keys = sorted(x)
        return (keys, np.array([x[k] for k in keys], dtype=np.float64))
    if isinstance(x, (list, tuple)):
        return [to_host(v) for v in x]
    return x


def same_bits(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype
                and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes())
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(u, v) for u, v in zip(a, b))
    return a == b


def differing(a, b):
    """Positions of the top-level outputs that differ (for the failure message)."""
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b):
        return [i for i, (u, v) in enumerate(zip(a, b)) if not same_bits(u, v)]
    return [0]


def hold_seconds(t_w):
    return min(max(HOLD_FACTOR * t_w, HOLD_MIN_S), HOLD_CAP_S)


def held_call(label, f, real, decoy, side, check_hold=True):
    """The protocol of the module docstring for ``f(*real)`` (``decoy``: arguments of the same shapes, dtypes and options
    with other values).  ``f`` returns tensors, dicts, numpy arrays or lists of them.  ``check_hold=False`` leaves step 5
    out (the caller says why).  Returns the reference outputs on the host."""
    dev = side.device
    try:
        ref = to_host(f(*real))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = to_host(f(*real))
        torch.cuda.synchronize()
        t_w = time.perf_counter() - t0
        assert same_bits(ref, again), f"{label}: two runs on the default stream differ (not identical run to run)"
        with torch.cuda.stream(side):
            other = to_host(f(*decoy))
        assert not same_bits(other, ref), f"{label}: the decoy gives the reference's result - it would hide a late launch"
        torch.cuda.synchronize()
        seconds = hold_seconds(t_w)
        assert t_w < HOLD_CAP_S / 2, f"{label}: the call takes {t_w:.2f} s - shrink its shape (the hold is capped at {HOLD_CAP_S} s)"
        held = hold(dev, seconds)
        with torch.cuda.stream(side):
            got = to_host(f(*real))
            still_held = not held.query()
        print(f"[streams] {label}: t_w {t_w * 1e3:.1f} ms, hold {seconds * 1e3:.0f} ms ({hold_kind(dev)})"
              f"{'' if check_hold else ', step 5 not checked'}")
        if check_hold:
            assert still_held, (f"{label}: the call outlasted its hold or waited for the default stream "
                                f"(t_w {t_w * 1e3:.1f} ms, hold {seconds * 1e3:.0f} ms)")
        assert same_bits(got, ref), (f"{label}: the run on the side stream differs from the default-stream reference "
                                     f"(outputs {differing(got, ref)})")
        return ref
    finally:
        torch.cuda.synchronize()
