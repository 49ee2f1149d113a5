"""The face table of csrc/cell_faces.cpp where its lock-free set has to grow, and the host-parallel entries above their
single-thread thresholds (CPU only; no test here needs a GPU).

flooder_cell_faces collects the distinct faces in an open-addressing set that starts with ``initial_capacity(n_cells)``
slots and is rebuilt twice as large when more than half of it is taken.  Before this file no test made it grow; a
table that filled completely (one thread, or at most 256 cells: one chunk, whose insert count was published only at
its end) left every thread with a new key probing forever.  The cases below are the ones that did; each asserts from
the references alone that it is such a case before any native call is made.

References: the brute-force set of ``itertools.combinations`` rows, and the numpy path of
``simplex_tree.faces_of_cells`` (``NATIVE_FACES_MIN`` patched out of reach) - neither calls native code.

Every flooder_cell_faces call runs in a fresh child process (ctypes and numpy only) under a time limit of 30 s plus
ten times the wall time of the numpy path for the same input: a call that never returns fails its test instead of
hanging the suite.  FLOODER_TEST_HOST_LIB points the file at another build of libflooder_host.so (the parent commit's,
to see the cases fail there)."""
import ctypes
import functools
import itertools
import json
import math
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

from flooder_amd import build, simplex_tree as stm
from test_delaunay_nd import qhull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_LIMIT = 30.0       # seconds; the limit tells "returns" from "never returns", so it is generous
NUMPY_FACTOR = 10.0


def host_lib_path():
    return os.environ.get("FLOODER_TEST_HOST_LIB") or build.build_host()


def initial_capacity(n_cells):
    """Slots of the first table of flooder_cell_faces: the smallest power of two >= max(4 n_cells, 1024).  It is
    rebuilt twice as large once more than half of the slots are taken."""
    cap = 1024
    while cap < max(4 * n_cells, 1024):
        cap *= 2
    return cap


# ---------------------------------------------------------------------------------------------------- the references
def brute_force(cells, k):
    """Sorted distinct k-vertex faces of the cells: a Python set of itertools.combinations rows."""
    faces = set()
    for row in cells.tolist():
        faces.update(itertools.combinations(row, k))
    return np.array(sorted(faces), dtype=np.int64).reshape(-1, k)


def numpy_path(cells, k, n_points):
    """(table, seconds) of simplex_tree.faces_of_cells with the native routine out of reach."""
    old = stm.NATIVE_FACES_MIN
    stm.NATIVE_FACES_MIN = 10 ** 15
    try:
        t0 = time.perf_counter()
        table, _ = stm.faces_of_cells(cells, k - 1, n_points, want_index=False)
        return table, time.perf_counter() - t0
    finally:
        stm.NATIVE_FACES_MIN = old


@functools.lru_cache(maxsize=None)
def gauss_cells(n, dim, seed):
    """Delaunay cells (Qhull) of default_rng(seed).normal(size=(n, dim)); computed once per module."""
    cells = qhull(np.random.default_rng(seed).normal(size=(n, dim)))
    cells.setflags(write=False)
    return cells


def disjoint_cells(count, width):
    return np.arange(count * width, dtype=np.int64).reshape(count, width)


# name -> (cells, k, n_points, thread counts, reference, (n_cells, distinct faces) expected or None)
CASES = {
    # 1. vertex-disjoint 8-simplices on one thread: 126 faces per cell, below / above the 1024 slots
    "disjoint-8": (lambda: disjoint_cells(8, 9), 5, 72, (1,), "brute", (8, 1008)),
    "disjoint-9": (lambda: disjoint_cells(9, 9), 5, 81, (1,), "brute", (9, 1134)),
    # 2. many growths from 1024 slots: 4 x C(16, 8) faces, 48-bit keys (the narrow path)
    "wide-cells": (lambda: disjoint_cells(4, 16), 8, 64, (1, 3), "brute", (4, 51480)),
    # 3. one chunk at any thread count (n = 14: at most 256 cells), two chunks (n = 16), five (n = 20)
    "gauss8d-14": (lambda: gauss_cells(14, 8, 1), 5, 14, (1, 2, 8, 24), "brute", (127, 1778)),
    "gauss8d-16": (lambda: gauss_cells(16, 8, 1), 5, 16, (1, 2, 8, 24), "brute", (310, 3431)),
    "gauss8d-20": (lambda: gauss_cells(20, 8, 1), 5, 20, (1, 2, 3), "brute", (1222, 9461)),
    # 4. what Python reaches (cells x faces above NATIVE_FACES_MIN for n = 45); 128 threads: oversubscribed
    "gauss8d-30": (lambda: gauss_cells(30, 8, 1), 5, 30, (1, 3, 8, 128), "numpy", (7505, 45313)),
    "gauss8d-45": (lambda: gauss_cells(45, 8, 1), 5, 45, (1, 8), "numpy", (30007, 158207)),
    # 5. growth without saturation: above half of the first table, below its capacity
    "gauss8d-26-k4": (lambda: gauss_cells(26, 8, 1), 4, 26, (1, 8), "brute", (3994, 9985)),
}
SATURATES = {"disjoint-9", "wide-cells", "gauss8d-14", "gauss8d-16", "gauss8d-20", "gauss8d-30", "gauss8d-45"}


@functools.lru_cache(maxsize=None)
def case(name):
    """(cells, k, n_points, reference table, seconds of the numpy path); premises asserted from the references."""
    make, k, n_points, _, ref, expect = CASES[name]
    cells = make()
    want_np, seconds = numpy_path(cells, k, n_points)
    want = want_np
    if ref == "brute":      # (n = 30 and n = 45: a million and four million tuples - the numpy path alone there)
        want = brute_force(cells, k)
        assert np.array_equal(want, want_np), "the two references disagree"
    want.setflags(write=False)
    n_cells, distinct, cap = cells.shape[0], want.shape[0], initial_capacity(cells.shape[0])
    assert k * math.log2(n_points) < 62, "narrow keys"
    if expect is not None:
        assert (n_cells, distinct) == expect
    if name in SATURATES:
        assert distinct > cap, "the first table must fill completely"
    if name == "disjoint-8":
        assert distinct == 126 * 8 < cap == 1024
    if name == "disjoint-9":
        assert distinct == 126 * 9 and cap == 1024
    if name == "wide-cells":
        assert distinct == 4 * math.comb(16, 8) and cap == 1024 and 8 * math.log2(64) == 48
    if name == "gauss8d-14":
        assert n_cells <= 256, "one chunk whatever the thread count"
    if name == "gauss8d-16":      # (two chunks, 256 and 54 cells: the first alone holds more faces than there are slots)
        assert 256 < n_cells <= 512 and brute_force(cells[:256], k).shape[0] > cap == 2048
    if name == "gauss8d-20":
        assert n_cells > 256 and cap == 8192
    if name == "gauss8d-45":
        assert n_cells * math.comb(9, k) >= stm.NATIVE_FACES_MIN, "faces_of_cells takes the native routine here"
    if name == "gauss8d-26-k4":
        assert cap // 2 < distinct < cap == 16384, "grows once, never full"
    return cells, k, n_points, want, seconds


# ------------------------------------------------------------------------------------------- the native call, confined
CHILD = r"""
import ctypes, json, sys
import numpy as np
lib_path, cells_path, out_path, jobs = sys.argv[1], sys.argv[2], sys.argv[3], json.loads(sys.argv[4])
lib = ctypes.CDLL(lib_path)
lib.flooder_cell_faces.restype = ctypes.c_int64
lib.flooder_cell_faces.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                   ctypes.c_int, ctypes.POINTER(ctypes.POINTER(ctypes.c_int32))]
lib.flooder_host_free.restype = None
lib.flooder_host_free.argtypes = [ctypes.c_void_p]
cells = np.ascontiguousarray(np.load(cells_path), dtype=np.int32)
res = {}
for i, (k, n_points, threads) in enumerate(jobs):
    out = ctypes.POINTER(ctypes.c_int32)()
    rc = int(lib.flooder_cell_faces(cells.ctypes.data, cells.shape[0], cells.shape[1], k, n_points, threads,
                                    ctypes.byref(out)))
    res["count%d" % i] = np.int64(rc)
    res["rows%d" % i] = np.ctypeslib.as_array(out, shape=(rc, k)).copy() if rc > 0 else np.zeros((0, k), np.int32)
    if out:
        lib.flooder_host_free(out)
np.savez(out_path, **res)
"""


def run_child(args, limit, what):
    """A fresh interpreter under a time limit; killed, and the test failed, when it runs out."""
    try:
        done = subprocess.run([sys.executable, *args], capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:      # (subprocess.run kills the child before it raises)
        pytest.fail(f"{what}: no return within {limit:.0f} s")
    assert done.returncode == 0, f"{what}: exit {done.returncode}\n{done.stderr[-2000:]}"
    return done.stdout


def native_faces(tmp_path, cells, jobs, numpy_seconds, what):
    """[(count, rows)] of flooder_cell_faces for each (k, n_points, threads) of ``jobs``, from one child process."""
    cells_path, out_path = str(tmp_path / "cells.npy"), str(tmp_path / "faces.npz")
    np.save(cells_path, np.ascontiguousarray(cells, dtype=np.int32))
    limit = BASE_LIMIT + NUMPY_FACTOR * numpy_seconds
    run_child(["-c", CHILD, host_lib_path(), cells_path, out_path, json.dumps([list(map(int, j)) for j in jobs])],
              limit, what)
    with np.load(out_path) as z:
        return [(int(z[f"count{i}"]), z[f"rows{i}"]) for i in range(len(jobs))]


def check_table(count, rows, want):
    """Shape of the result (count = rows; ascending ids per row; rows strictly ascending, so distinct), then the
    reference's rows in the reference's order."""
    k = want.shape[1]
    assert count == rows.shape[0] and rows.shape[1] == k and rows.dtype == np.int32
    if k > 1:
        assert (np.diff(rows, axis=1) > 0).all(), "a row is not strictly ascending"
    if rows.shape[0] > 1:
        differ = rows[1:] != rows[:-1]
        assert differ.any(axis=1).all(), "duplicate rows"
        first = differ.argmax(axis=1)
        at = np.arange(rows.shape[0] - 1)
        assert (rows[1:][at, first] > rows[:-1][at, first]).all(), "rows not in lexicographic order"
    assert count == want.shape[0]
    assert np.array_equal(rows.astype(np.int64), want)


@pytest.mark.parametrize("name,threads", [(n, t) for n, c in CASES.items() for t in c[3]])
def test_face_table_that_has_to_grow(name, threads, tmp_path):
    """Cases 1 - 5 of the module docstring's table: the count and the rows of the reference, in order, at every thread
    count that used to spin (and, for gauss8d-26-k4 and disjoint-8, at the ones that did not)."""
    cells, k, n_points, want, seconds = case(name)
    (count, rows), = native_faces(tmp_path, cells, [(k, n_points, threads)], seconds, f"{name}, {threads} thread(s)")
    check_table(count, rows, want)


@pytest.mark.parametrize("name", list(CASES))
def test_two_runs_on_eight_threads_give_identical_bytes(name, tmp_path):
    """Which thread inserts a key first differs from run to run; the sorted table does not."""
    cells, k, n_points, want, seconds = case(name)
    (c0, r0), (c1, r1) = native_faces(tmp_path, cells, [(k, n_points, 8)] * 2, 2 * seconds, f"{name}, 8 threads twice")
    check_table(c0, r0, want)
    assert c0 == c1 and r0.tobytes() == r1.tobytes()


# ------------------------------------------------------------------------------------------ through the public functions
PUBLIC_CHILD = r"""
import sys
import numpy as np
lib_path, threads, out_path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
from flooder_amd import build, simplex_tree as stm
if lib_path:
    build.build_host = lambda *a, **k: lib_path
stm.DELAUNAY_THREADS = threads
points = np.random.default_rng(1).normal(size=(45, 8))
res = {}
for d, rows in enumerate(stm.delaunay_simplices(points, max_dimension=4)):
    res["delaunay%d" % d] = rows
cells = stm.delaunay_cells(points)
res["cells"] = cells
st = stm.SimplexTree.from_cells(cells, 45)
for d in range(9):
    res["tree%d" % d] = st.simplices_of_dimension(d)
# the routes on which simplex_tree asks flooder_cell_faces for this complex: a table without cell -> face rows, and a
# table enumerated after the monotone pass has run
res["noindex4"] = stm.faces_of_cells(cells, 4, 45, want_index=False)[0]
late = stm.SimplexTree.from_cells(cells, 45, eager=0)
late.make_filtration_non_decreasing()
res["late4"] = late.simplices_of_dimension(4)
res["late3"] = late.simplices_of_dimension(3)
np.savez(out_path, **res)
"""


@pytest.mark.parametrize("threads", [1, 8])
def test_public_functions_on_the_45_point_cloud(threads, tmp_path):
    """delaunay_simplices(max_dimension=4) and SimplexTree.from_cells on the 8-D cloud of 45 points, DELAUNAY_THREADS 1
    and 8: every dimension's table is the numpy path's.  With the default settings these two keep the cell -> face
    rows of a complex of this size and enumerate with numpy; flooder_cell_faces is asked where no such rows are wanted
    (want_index=False, and any table first touched after make_filtration_non_decreasing), so those routes are run
    too - with one thread they are the calls that never returned."""
    cells, _, _, want5, seconds = case("gauss8d-45")
    wants = {4: want5}
    for d in (1, 2, 3, 5, 6, 7):
        wants[d], s = numpy_path(cells, d + 1, 45)
        seconds += s
    out_path = str(tmp_path / "public.npz")
    override = os.environ.get("FLOODER_TEST_HOST_LIB", "")
    run_child(["-c", PUBLIC_CHILD, override, str(threads), out_path], BASE_LIMIT + NUMPY_FACTOR * 4 * seconds,
              f"public functions, {threads} thread(s)")
    with np.load(out_path) as z:
        assert np.array_equal(z["cells"], cells)
        assert np.array_equal(z["delaunay0"], np.arange(45)[:, None]) and np.array_equal(z["tree0"], z["delaunay0"])
        for d in range(1, 5):
            assert np.array_equal(z[f"delaunay{d}"], wants[d]), d
        for d in range(1, 8):
            assert np.array_equal(z[f"tree{d}"], wants[d]), d
        assert np.array_equal(z["tree8"], cells)
        assert np.array_equal(z["noindex4"], wants[4])
        assert np.array_equal(z["late4"], wants[4]) and np.array_equal(z["late3"], wants[3])


# ------------------------------------------------------------------------- the other entries above their thresholds
THREADS = (1, 2, 3, 8, 24)


@functools.lru_cache(maxsize=None)
def big_complex():
    """The 6-D Delaunay complex of 150 Gaussian points of test_parallel_face_table_equals_numpy (about 41 000 cells, 289 000
    entries): above the single-thread threshold of every entry."""
    n, dim = 150, 6
    cells = gauss_cells(n, dim, dim + n + 3)
    assert cells.shape[1] == 7 and cells.shape[0] > 38000
    return cells, n


def host():
    """The library under test through ctypes (these calls never spun: they run in this process)."""
    if not os.environ.get("FLOODER_TEST_HOST_LIB"):
        lib = stm._load_host()
        assert lib is not None
        return lib
    lib = ctypes.CDLL(host_lib_path())
    c_int, i64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.flooder_widen_i32.restype = None
    lib.flooder_widen_i32.argtypes = [ptr, i64, ptr, c_int]
    lib.flooder_locate_rows.restype = i64
    lib.flooder_locate_rows.argtypes = [ptr, i64, c_int, ptr, i64, i64, ptr, c_int]
    lib.flooder_raise_dimension.restype = i64
    lib.flooder_raise_dimension.argtypes = [ptr, i64, c_int, ptr, i64, ptr, ptr, i64, c_int]
    return lib


def pack(rows, base):
    """Rows as numbers to the base ``base``, first column most significant (exact: below 2^62 here)."""
    k = rows.shape[1]
    assert base ** k < 2 ** 62
    return rows @ (base ** np.arange(k - 1, -1, -1, dtype=np.int64))


@pytest.mark.parametrize("threads", THREADS)
def test_locate_rows_above_its_threshold(threads):
    """flooder_locate_rows with (n + m) k >= 2^17: present rows, absent rows and rows with ids outside [0, n_points),
    against np.searchsorted on the packed keys."""
    cells, n = big_complex()
    rng = np.random.default_rng(21)
    k = 7
    absent = np.sort(rng.integers(0, n, size=(3000, k)), axis=1)
    outside = np.sort(rng.integers(n - 10, n + 20, size=(500, k)), axis=1)
    outside[::2, 0] = -1 - outside[::2, 0]                       # (negative ids too)
    outside = outside[((outside < 0) | (outside >= n)).any(axis=1)]
    query = np.ascontiguousarray(np.concatenate([cells[rng.permutation(len(cells))], absent, outside]))
    assert (len(query) + len(cells)) * k >= 1 << 17, "below the entry's single-thread threshold"
    in_range = ((query >= 0) & (query < n)).all(axis=1)
    tkey, qkey = pack(cells, n), pack(np.where(in_range[:, None], query, 0), n)
    pos = np.minimum(np.searchsorted(tkey, qkey), len(tkey) - 1)
    want = np.where(in_range & (tkey[pos] == qkey), pos, -1)
    assert (want[: len(cells)] >= 0).all() and (want[len(cells):] < 0).sum() > 3000 and len(outside) > 100
    table = np.ascontiguousarray(cells)
    got = np.full(len(query), -7, dtype=np.int64)
    assert host().flooder_locate_rows(query.ctypes.data, len(query), k, table.ctypes.data, len(table), n,
                                      got.ctypes.data, threads) == 0
    assert np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def monotone_reference():
    """Rows, facets and values (NaN among the rows' own values and among the facets') and what the numpy monotone
    pass of SimplexTree._raise_dimension makes of them."""
    cells, n = big_complex()
    lower, _ = numpy_path(cells, 6, n)
    rng = np.random.default_rng(22)
    vals = rng.random(len(cells))
    vals[rng.random(len(vals)) < 0.3] = np.nan
    lower_vals = rng.random(len(lower))
    lower_vals[rng.random(len(lower_vals)) < 0.6] = np.nan      # (0.6^7: a few hundred rows all of whose facets are NaN)
    tkey = pack(lower, n)
    face_max = np.full(len(cells), -np.inf)
    for j in range(7):
        fkey = pack(np.delete(cells, j, axis=1), n)
        pos = np.minimum(np.searchsorted(tkey, fkey), len(tkey) - 1)
        assert (tkey[pos] == fkey).all()
        fv = lower_vals[pos]
        face_max = np.maximum(face_max, np.where(np.isnan(fv), -np.inf, fv))
    raised = np.where(np.isnan(vals), face_max, np.maximum(vals, face_max))
    raised = np.where(np.isneginf(raised), vals, raised)
    changed = int((~((raised == vals) | (np.isnan(raised) & np.isnan(vals)))).sum())
    assert 0 < changed < len(vals) and np.isnan(raised).any() and np.isnan(vals).sum() > np.isnan(raised).sum()
    return lower, vals, lower_vals, raised, changed


@pytest.mark.parametrize("threads", THREADS)
def test_raise_dimension_above_its_threshold(threads):
    """flooder_raise_dimension with n k >= 2^16 against the numpy monotone pass: the raised values bit for bit (NaN
    where every facet is NaN too) and the same count of changed rows."""
    cells, n = big_complex()
    lower, vals, lower_vals, raised, changed = monotone_reference()
    assert len(cells) * 7 >= 1 << 16, "below the entry's single-thread threshold"
    rows, lo = np.ascontiguousarray(cells), np.ascontiguousarray(lower)
    v = vals.copy()
    rc = host().flooder_raise_dimension(rows.ctypes.data, len(rows), 7, lo.ctypes.data, len(lo), lower_vals.ctypes.data,
                                        v.ctypes.data, n, threads)
    assert rc == changed
    assert np.array_equal(np.isnan(v), np.isnan(raised))
    assert np.array_equal(v[~np.isnan(v)].view(np.uint64), raised[~np.isnan(raised)].view(np.uint64))


@pytest.mark.parametrize("threads", THREADS)
def test_widen_above_its_threshold(threads):
    """flooder_widen_i32 with count >= 2^18 against astype (negative values and the int32 extremes included)."""
    cells, _ = big_complex()
    src = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1).copy()
    src[:4] = [-1, np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0]
    assert src.size >= 1 << 18, "below the entry's single-thread threshold"
    dst = np.full(src.size + 1, -7, dtype=np.int64)
    host().flooder_widen_i32(src.ctypes.data, src.size, dst.ctypes.data, threads)
    assert np.array_equal(dst[:-1], src.astype(np.int64)) and dst[-1] == -7


@pytest.mark.parametrize("threads", THREADS)
def test_face_tables_of_the_big_complex(threads, tmp_path):
    """flooder_cell_faces for every k of the 6-D complex: the key sort runs with more than one bucket (2048 distinct
    faces or more) on every thread count, and the tables with more faces than half of the first table grow."""
    cells, n = big_complex()
    wants, seconds = {}, 0.0
    for k in range(1, 8):
        wants[k], s = numpy_path(cells, k, n) if k > 1 else (np.unique(cells)[:, None], 0.0)
        seconds += s
    assert sum(len(w) >= 2048 for w in wants.values()) >= 5, "several buckets in sort_keys_parallel"
    assert max(len(w) for w in wants.values()) > initial_capacity(len(cells)) // 2, "no table grows"
    got = native_faces(tmp_path, cells, [(k, n, threads) for k in range(1, 8)], seconds, f"6-D complex, {threads} thread(s)")
    for k, (count, rows) in zip(range(1, 8), got):
        check_table(count, rows, wants[k])


# ------------------------------------------------------------------------------------------------- the pool on its own
def test_pool_survives_exceptions_in_parallel_regions(tmp_path):
    """tests/host_pool_main.cpp: a body that throws on a worker, on the calling thread or on all threads, at 1, 2 and 8
    threads - one exception reaches the caller, after every thread has left the region, and the pool works on."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "host_pool_main"
    include = os.environ.get("FLOODER_TEST_POOL_INCLUDE") or os.path.join(ROOT, "flooder_amd", "csrc")
    subprocess.run([cxx, "-O2", "-std=c++17", "-pthread", f"-I{include}", os.path.join(ROOT, "tests", "host_pool_main.cpp"),
                    "-o", str(exe)], check=True)
    try:
        done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired:
        pytest.fail("host_pool_main: no return within 60 s")
    assert done.returncode == 0, f"exit {done.returncode}\n{done.stdout}\n{done.stderr[-2000:]}"
    lines = done.stdout.strip().splitlines()
    assert lines[-1] == "all ok" and len(lines) == 19 and all(line.endswith(": ok") for line in lines[:-1])
