"""The poisoned-allocation harness (poison_helper.py) tested on CPU tensors, and the check that it wraps every
constructor idiom the package uses: a harness that silently hands out ordinary memory checks nothing."""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import poison_helper as ph
from poison_helper import GUARD, PATTERNS, poisoned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw_bytes(t):
    """The payload of a contiguous tensor as numpy uint8, through its address (not through torch)."""
    n = t.numel() * t.element_size()
    return np.frombuffer((ctypes.c_uint8 * n).from_address(t.data_ptr()), dtype=np.uint8)


# ----------------------------------------------------------------------------------------------- payloads
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8])
def test_empty_holds_the_pattern(pattern, dtype):
    with poisoned(pattern, "cpu") as rec:
        for t, shape in ((torch.empty(5, dtype=dtype), (5,)), (torch.empty((3, 4), dtype=dtype), (3, 4)),
                         (torch.empty(3, 4, dtype=dtype), (3, 4)), (torch.empty(size=(2, 7), dtype=dtype), (2, 7)),
                         (torch.empty_like(torch.ones(6, dtype=dtype)), (6,)),
                         (torch.empty_like(torch.ones(2, 3), dtype=dtype), (2, 3))):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
            assert t.storage_offset() * t.element_size() == GUARD and t.data_ptr() % 64 == 0
            assert (raw_bytes(t) == pattern).all()
        assert len(rec) == 6 and rec.broken() == []
    word = int.from_bytes(bytes([pattern]) * 4, "little")
    assert {0xFF: word == 0xFFFFFFFF, 0x7F: word < 0x7F800000, 0x01: 0 < word < 1 << 25}[pattern]


def test_what_the_patterns_are_as_numbers():
    vals = {}
    for pattern in PATTERNS:
        with poisoned(pattern, "cpu"):
            vals[pattern] = (torch.empty(3), torch.empty(3, dtype=torch.int32))     # (default dtype: float32)
    assert vals[0xFF][0].dtype == torch.float32 and torch.isnan(vals[0xFF][0]).all() and (vals[0xFF][1] == -1).all()
    assert torch.isfinite(vals[0x7F][0]).all() and (vals[0x7F][0] > 3e38).all() and (vals[0x7F][1] > 2 ** 30).all()
    assert (vals[0x01][0] > 0).all() and (vals[0x01][0] < 1e-37).all() and (vals[0x01][1] == 0x01010101).all()


def test_initialised_constructors_are_guarded_and_hold_what_was_asked():
    with poisoned(0x7F, "cpu") as rec:
        like = torch.ones(4, 2, dtype=torch.float64)
        made = [torch.zeros(5, dtype=torch.int32), torch.zeros((2, 3)), torch.zeros_like(like),
                torch.full((3,), 7, dtype=torch.int64), torch.full((2, 2), float("inf")), torch.full((3,), 5),
                torch.full_like(like, -1.0), like.new_zeros((3, 1)), like.new_zeros(2, 2), like.new_zeros(4, dtype=torch.int32),
                torch.zeros((), dtype=torch.float64)]
        want = [np.zeros(5, np.int32), np.zeros((2, 3), np.float32), np.zeros((4, 2)),
                np.full(3, 7, np.int64), np.full((2, 2), np.inf, np.float32), np.full(3, 5, np.int64),
                np.full((4, 2), -1.0), np.zeros((3, 1)), np.zeros((2, 2)), np.zeros(4, np.int32), np.zeros(())]
        for t, w in zip(made, want):
            assert t.storage_offset() * t.element_size() == GUARD and t.is_contiguous()
            got = t.numpy()
            assert got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got, w)
        assert len(rec) == len(made) and rec.broken() == []
        assert {a.kind for a in rec.allocations} == {"zeros", "zeros_like", "full", "full_like", "new_zeros"}


def test_requires_grad_is_honoured():
    with poisoned(0x01, "cpu"):
        x = torch.empty(4, dtype=torch.float64, requires_grad=True)
        z = torch.zeros(3, requires_grad=True)
        assert x.requires_grad and x.is_leaf and z.requires_grad and z.is_leaf
        (g,) = torch.autograd.grad((z * torch.arange(3.0)).sum(), z)
    assert g.tolist() == [0.0, 1.0, 2.0]


def test_pass_through_cases_are_the_real_constructor():
    with poisoned(0xFF, "cpu") as rec:
        out = torch.ones(4)
        plain = [torch.empty(0), torch.empty((3, 0), dtype=torch.int32), torch.zeros(0), torch.full((0,), 1.0),
                 torch.empty(4, device="meta"), torch.zeros(4, device="meta"),
                 torch.empty((1, 2, 4, 4), memory_format=torch.channels_last),
                 torch.empty_like(torch.ones(4, 6).t()), torch.zeros_like(torch.ones(4, 6).t()),
                 torch.empty_like(torch.ones(0)), torch.ones(3).new_zeros(0)]
        for t in plain:
            assert t.storage_offset() == 0
        assert torch.empty(4, out=out) is out and torch.zeros(4, out=out) is out and out.storage_offset() == 0
        assert torch.equal(torch.full((4,), 2.0, out=out), torch.full((4,), 2.0)) and out.storage_offset() == 0
        assert torch.empty_like(torch.ones(4, 6).t()).stride() == (1, 6)     # (preserve_format: the strides are kept)
        if torch.cuda.is_available():
            pinned = torch.empty(8, pin_memory=True)
            assert pinned.is_pinned() and pinned.storage_offset() == 0
            assert torch.empty(4, device="cuda").storage_offset() == 0       # (another device type than the patched one)
        assert len(rec) == 1          # (the torch.full((4,), 2.0) of the comparison)
        assert rec.passed_through >= len(plain) + 3


def test_a_device_type_that_is_not_the_patched_one_passes_through():
    with poisoned(0xFF, "cuda") as rec:
        t = torch.empty(5)
        z = torch.zeros(5, dtype=torch.int32)
    assert t.storage_offset() == 0 and z.storage_offset() == 0 and (z == 0).all() and len(rec) == 0


# ----------------------------------------------------------------------------------------------- what it detects
def test_a_read_of_unwritten_scratch_changes_with_the_pattern():
    def sums_its_scratch(x):
        scratch = torch.empty(8, dtype=torch.int32)
        scratch[:4] = x            # (half of it is written ...)
        return int(scratch.sum())  # (... and all of it is read)

    def writes_all_of_it(x):
        scratch = torch.empty(4, dtype=torch.int32)
        scratch[:] = x
        return int(scratch.sum())

    x = torch.arange(4, dtype=torch.int32)
    got, clean = [], []
    for pattern in PATTERNS:
        with poisoned(pattern, "cpu"):
            got.append(sums_its_scratch(x))
            clean.append(writes_all_of_it(x))
    assert len(set(got)) == 3 and clean == [6, 6, 6]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_one_byte_past_either_end_is_reported(pattern):
    with poisoned(pattern, "cpu") as rec:
        a = torch.empty(5, dtype=torch.int32)
        b = torch.empty((3, 4), dtype=torch.float64)
        c = torch.zeros(7, dtype=torch.int64)
        assert rec.broken() == []
        other = 0x00 if pattern != 0x00 else 0xAA
        ctypes.memset(a.data_ptr() + a.numel() * 4, other, 1)       # the first byte behind a
        ctypes.memset(b.data_ptr() - 1, other, 1)                   # the last byte in front of b
        found = rec.broken()
        assert [(f["shape"], f["dtype"], f["side"], f["kind"]) for f in found] == \
            [((5,), torch.int32, "above", "empty"), ((3, 4), torch.float64, "below", "empty")]
        assert all("test_poison_helper_cpu.py" in f["where"] for f in found)
        ctypes.memset(c.data_ptr() + 7 * 8 + GUARD - 1, other, 1)   # the last byte of c's upper guard
        assert [(f["shape"], f["side"], f["kind"]) for f in rec.broken()][-1] == ((7,), "above", "zeros")
        ctypes.memset(a.data_ptr(), other, 20)                      # (the payload is the owner's to write)
        assert len(rec.broken()) == 3
    with pytest.raises(RuntimeError, match="after the block has ended"):
        rec.broken()


def test_the_allocating_line_in_the_package_is_named():
    from flooder_amd import core

    with poisoned(0x01, "cpu") as rec:
        core._no_simplices(core._FaceTable(None, 4, "cpu"), 4, "cpu", True)     # (zero elements: passed through)
        ws = core.FusedWorkspace(3, 100, 4, None, "cpu", wit=False, owner=False)
        assert (raw_bytes(ws.d2) == 0x01).all() and ws.d2.shape == (3, 100)
        where = {a.where.split(":")[0] for a in rec.allocations}
        assert where == {"flooder_amd/core.py"}, where
        # (the workspace's local helper ``empty`` and the line of the workspace that called it: the buffer by name)
        assert all(" <- core.py:" in a.where for a in rec.allocations if a.kind == "empty" and a.shape != (ws.n_words,))
        assert len({a.where for a in rec.allocations}) >= 5
        assert rec.broken() == []


# ----------------------------------------------------------------------------------------------- restoring
def test_constructors_are_restored_after_an_exception():
    names = ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like")
    before = {n: getattr(torch, n) for n in names}
    new_zeros_before = torch.Tensor.new_zeros
    own_before = "new_zeros" in torch.Tensor.__dict__
    with pytest.raises(KeyError):
        with poisoned(0xFF, "cpu"):
            assert all(getattr(torch, n) is not before[n] for n in names)
            assert torch.Tensor.new_zeros is not new_zeros_before
            raise KeyError("inside the block")
    assert all(getattr(torch, n) is before[n] for n in names)
    assert torch.Tensor.new_zeros is new_zeros_before and ("new_zeros" in torch.Tensor.__dict__) == own_before
    assert torch.empty(5).storage_offset() == 0 and torch.ones(2).new_zeros(3).storage_offset() == 0
    with pytest.raises(ValueError):
        with poisoned(0x1FF, "cpu"):
            pass


def test_nested_blocks_restore_in_order():
    real = torch.empty
    with poisoned(0xFF, "cpu") as outer:
        with poisoned(0x01, "cpu") as inner:
            t = torch.empty(4, dtype=torch.uint8)
            assert (raw_bytes(t) == 0x01).all() and len(inner) == 1
        u = torch.empty(4, dtype=torch.uint8)
        assert (raw_bytes(u) == 0xFF).all()
        assert len(outer) >= 1 and outer.broken() == []
    assert torch.empty is real


# ----------------------------------------------------------------------------------------------- coverage
WORDS = ("empty", "zeros", "full", "resize_", "set_")

# every other attribute of that kind the package refers to, and why it is none of the harness's business
NOT_DEVICE_MEMORY = {
    "np.empty": "numpy array on the host", "np.zeros": "numpy array on the host", "np.full": "numpy array on the host",
    "np.empty_like": "numpy array on the host",
    "torch.cuda.set_device": "selects the current device; allocates nothing",
    "torch.cuda.empty_cache": "releases the allocator's cache; allocates nothing",
    "torch.cuda.reset_peak_memory_stats": "a counter of the allocator (the CLI's report)",
    "torch.set_rng_state": "the CPU generator's state (distributed: the ranks draw the same weights)",
    "re.fullmatch": "a regular expression of the CLI",
}


def constructor_idioms():
    """{"torch.empty" | "np.zeros" | "<obj>.new_zeros" | "name empty" ...: ["file.py:line", ...]} over flooder_amd/*.py:
    every attribute REFERENCE (a call, or ``(torch.empty if fused else torch.zeros)(...)``) whose name contains one of
    ``WORDS``, spelled with its dotted receiver where that is a module path and ``<obj>`` where it is a value; plus every
    such name imported from torch (``from torch import empty`` would slip past a patched ``torch.empty``)."""
    found = {}

    def dotted(node):
        parts = []
        while isinstance(node, ast.Attribute):
            parts.append(node.attr)
            node = node.value
        if isinstance(node, ast.Name) and node.id in ("torch", "np", "numpy", "re"):
            return ".".join(["np" if node.id == "numpy" else node.id] + parts[::-1])
        return None

    files = sorted(glob.glob(os.path.join(ROOT, "flooder_amd", "*.py")))
    assert len(files) >= 10, files
    for path in files:
        with open(path) as fh:
            tree = ast.parse(fh.read(), path)
        for node in ast.walk(tree):
            where = f"{os.path.basename(path)}:{getattr(node, 'lineno', 0)}"
            if isinstance(node, ast.Attribute) and any(w in node.attr for w in WORDS):
                found.setdefault(dotted(node) or f"<obj>.{node.attr}", []).append(where)
            elif isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[0] == "torch":
                for alias in node.names:
                    if any(w in alias.name for w in WORDS):
                        found.setdefault(f"from torch import {alias.name}", []).append(where)
    return found


def test_the_harness_wraps_every_constructor_idiom_of_the_package():
    found = constructor_idioms()
    for name in sorted(found):
        kind = "wrapped" if name in ph.WRAPPED else "not device memory" if name in NOT_DEVICE_MEMORY else "UNKNOWN"
        print(f"[poison] {name}: {len(found[name])} references, {kind}")
    unknown = {n: w[:3] for n, w in found.items() if n not in ph.WRAPPED and n not in NOT_DEVICE_MEMORY}
    assert not unknown, (f"constructor idioms that poison_helper neither wraps nor lists in NOT_DEVICE_MEMORY: {unknown} "
                         "- wrap them (a new_empty, empty_strided, resize_ or set_ hands out unpoisoned memory)")
    # the table of this file names what is there, nothing stale: every wrapped constructor is used, every exemption too
    assert set(ph.WRAPPED) <= set(found), sorted(set(ph.WRAPPED) - set(found))
    assert set(NOT_DEVICE_MEMORY) <= set(found), sorted(set(NOT_DEVICE_MEMORY) - set(found))
    assert len(found["torch.empty"]) > 80       # (53 in core.py and 28 in neighbors.py alone)


def test_the_coverage_check_sees_an_idiom_it_does_not_know():
    tree = ast.parse("import torch\nx = torch.empty_strided((2,), (1,))\ny = x.new_empty(3)\nz = x.resize_(4)\n")
    names = sorted(n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and any(w in n.attr for w in WORDS))
    assert names == ["empty_strided", "new_empty", "resize_"]
    assert not any(f"torch.{n}" in ph.WRAPPED or f"<obj>.{n}" in ph.WRAPPED for n in names)
