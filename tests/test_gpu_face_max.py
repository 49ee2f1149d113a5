"""The float32 face epilogue on its own: ``flooder_face_max_f32`` (both kernels of ``csrc/flood_kernels.hip``, every
branch of each) and ``flooder_face_values_f32`` through ctypes, bit for bit against numpy - ``np.sqrt`` of the float32
maximum over the rows a face lists, ``+0.0`` for a face without rows, ``np.sqrt`` of every word for ``out_dist``.  The
outputs are prefilled with a NaN pattern no square root of a non-negative float produces, so a word that is never
written is seen, and a guard behind every output shows a write past its end.  Runs on a real MI355X only (-m gpu)."""

import functools

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64                     # words behind every output buffer that no kernel may touch
UNWRITTEN = 0x7FC0DEAD         # a quiet NaN: not the square root of anything
INF, MAX_FINITE, MIN_NORMAL = 0x7F800000, 0x7F7FFFFF, 0x00800000
BIG = 1024                     # face_max_kernel: faces of at least this many rows are reduced by the whole block


def _stream():
    return _native.current_stream_ptr(DEV)


# ------------------------------------------------------------------------------------------------ inputs
def _words(rng, S, R):
    """(S, R) uint32 bit patterns of non-negative float32 numbers, none of them denormal: ordinary values over sixty
    decades, exact zeros, +inf, the largest finite float, perfect squares, and runs of equal values along a row."""
    v = (np.abs(rng.standard_normal((S, R))) * 10.0 ** rng.uniform(-30, 30, size=(S, R))).astype(np.float32)
    w = v.view(np.uint32).copy()
    w[(w > 0) & (w < MIN_NORMAL)] = MIN_NORMAL
    kind = rng.integers(0, 16, size=(S, R))
    w[kind == 0] = 0
    w[kind == 1] = INF
    w[kind == 2] = MAX_FINITE
    squares = (rng.integers(0, 4096, size=(S, R)).astype(np.float32) ** 2).view(np.uint32)      # below 2**24: exact
    w[kind == 3] = squares[kind == 3]
    for s in range(min(S, 64)):                  # runs of equal values (the later rows of the array stay as drawn)
        a = int(rng.integers(0, R))
        w[s, a:a + int(rng.integers(2, 9))] = w[s, a]
    assert ((w == 0) | (w >= MIN_NORMAL)).all() and (w <= INF).all()
    return w


def _csr(lists):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    rows = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    if rows.size == 0:
        rows = np.zeros(1, dtype=np.int32)       # (never read: a buffer to point at)
    return ptr, rows


@functools.lru_cache(maxsize=None)
def _grid_table(ppe, d):
    """The face table ``flood_complex`` builds for the lattice of ``ppe`` points per edge on a d-simplex: (R, ptr, rows)."""
    weights, _, face_idxs = core.generate_grid(ppe, d, "cpu", torch.float32)
    faces = core._FaceTable(face_idxs, weights.shape[0], "cpu")
    return weights.shape[0], faces.ptr.numpy().copy(), faces.rows.numpy().copy()


def _all_rows(R):
    """One face of all rows: the table of a ``num_rand`` call."""
    return _csr([np.arange(R)])


def _handmade(rng, R, F):
    """F faces over R rows: lengths from 1 to R, rows drawn without order, the last face lists every row."""
    lists = [rng.choice(R, size=int(rng.integers(1, R + 1)), replace=False) for _ in range(F - 1)]
    return _csr(lists + [rng.permutation(R)])


# (R, F) -> where its table comes from: (points_per_edge, simplex dimension) of a real lattice, or None (hand-made)
SMALL_SHAPES = {(1, 1): None, (5, 3): (5, 1), (64, 1): None, (36, 7): (8, 2), (56, 15): (6, 3), (35, 31): (4, 4),
                (64, 32): None}
TOP_GRIDS = {(3, 5): (21, 63), (4, 6): (84, 127), (2, 7): (8, 255), (3, 8): (45, 511)}     # (ppe, d) -> (R, F)


def _small_table(rng, R, F):
    grid = SMALL_SHAPES[(R, F)]
    if grid is not None:
        r, ptr, rows = _grid_table(*grid)
        assert (r, len(ptr) - 1) == (R, F)
        return ptr, rows
    return _all_rows(R) if F == 1 else _handmade(rng, R, F)


def _lg(F):
    lg = 1
    while (1 << lg) < F:
        lg += 1
    return lg


# ------------------------------------------------------------------------------------------------ reference and call
def _reference(words, ptr, rows):
    S = words.shape[0]
    F = len(ptr) - 1
    vals = words.view(np.float32)
    want = np.zeros((S, F), dtype=np.float32)
    for f in range(F):
        if ptr[f + 1] > ptr[f]:
            want[:, f] = vals[:, rows[ptr[f]:ptr[f + 1]]].max(axis=1)
    with np.errstate(all="ignore"):
        return np.sqrt(want).view(np.uint32), np.sqrt(vals).view(np.uint32)


def _face_max(words, ptr, rows, want_dist):
    """One call on fresh buffers: (S, F) uint32 face words, (S, R) uint32 distance words or None."""
    S, R = words.shape
    F = len(ptr) - 1
    t_w = torch.as_tensor(words.view(np.int32), device=DEV)
    t_ptr, t_rows = torch.as_tensor(ptr, device=DEV), torch.as_tensor(rows, device=DEV)
    face = torch.full((S * F + GUARD,), UNWRITTEN, dtype=torch.int32, device=DEV)
    dist = torch.full((S * R + GUARD,), UNWRITTEN, dtype=torch.int32, device=DEV) if want_dist else None
    _native.check(_native.load().flooder_face_max_f32(_native.ptr(t_w), S, R, _native.ptr(t_ptr), _native.ptr(t_rows), F,
                                                      _native.ptr(face), _native.ptr(dist), _stream()),
                  "flooder_face_max_f32")
    face = face.cpu().numpy().view(np.uint32)
    assert (face[S * F:] == UNWRITTEN).all(), "face_max wrote behind out_face"
    if want_dist:
        dist = dist.cpu().numpy().view(np.uint32)
        assert (dist[S * R:] == UNWRITTEN).all(), "face_max wrote behind out_dist"
        dist = dist[:S * R].reshape(S, R)
    assert np.array_equal(t_w.cpu().numpy().view(np.uint32), words), "the d2 words were changed"
    return face[:S * F].reshape(S, F), dist


def _check(words, ptr, rows, what):
    """Both forms of the call (``out_dist`` NULL and given) against the reference, word for word."""
    want, want_dist = _reference(words, ptr, rows)
    for with_dist in (False, True):
        face, dist = _face_max(words, ptr, rows, with_dist)
        bad = np.argwhere(face != want)
        assert len(bad) == 0, (what, with_dist, len(bad), [(int(s), int(f), hex(face[s, f]), hex(want[s, f]))
                                                          for s, f in bad[:5]])
        if with_dist:
            bad = np.argwhere(dist != want_dist)
            assert len(bad) == 0, (what, "out_dist", len(bad), [(int(s), int(r), hex(dist[s, r]), hex(want_dist[s, r]))
                                                               for s, r in bad[:5]])


def _peak(words, s, row):
    """Simplex ``s``: every word below 2**125, the largest finite float in ``row`` alone."""
    words[s] = np.minimum(words[s], np.uint32(0x7E000000))
    words[s, row] = MAX_FINITE


# ------------------------------------------------------------------------------------------------ the small kernel
def test_shapes_cover_what_they_must():
    assert {_lg(F) for _, F in SMALL_SHAPES} == {1, 2, 3, 4, 5}
    assert any(F & (F - 1) for _, F in SMALL_SHAPES)                               # F below a power of two
    assert all(R <= 64 and F <= 32 for R, F in SMALL_SHAPES)
    for (ppe, d), (R, F) in TOP_GRIDS.items():
        r, ptr, rows = _grid_table(ppe, d)
        assert (r, len(ptr) - 1) == (R, F) and F == 2 ** (d + 1) - 1 and F > 32
        assert int(np.diff(ptr).max()) == R and int(np.diff(ptr).min()) == 1 and rows.max() == R - 1


@pytest.mark.parametrize("R,F", sorted(SMALL_SHAPES))
def test_small_kernel_bitwise(R, F):
    """R <= 64 rows and <= 32 faces: a wave takes U = 64 >> lgF simplices per step.  One simplex, one short of a step,
    one more than a step, and four steps and a ragged one."""
    rng = np.random.default_rng(1000 * R + F)
    ptr, rows = _small_table(rng, R, F)
    U = 64 >> _lg(F)
    for S in sorted({1, U - 1, U + 1, 4 * U + 3} - {0}):
        _check(_words(rng, S, R), ptr, rows, (R, F, S))


@pytest.mark.parametrize("R,F,S", [(3, 1, 131072 + 77), (64, 32, 2 * 16384 + 5)])
def test_small_kernel_past_the_block_cap(R, F, S):
    """More simplices than the capped grid takes in one turn (1024 blocks x 128 at one face, 2048 x 8 at 32): the
    grid-stride loop runs again and ends on a ragged step."""
    rng = np.random.default_rng(S)
    ptr, rows = _all_rows(R) if F == 1 else _handmade(rng, R, F)
    U = 64 >> _lg(F)
    # (the cap as flooder_face_max_f32 computes it, flood_kernels.hip "resident blocks": if it changes there, change it
    # here - the assertion below only says that S is past one turn of the grid)
    lds = 4 * U * 64 * 4
    cap = (8 if lds <= 8192 else 6 if lds <= 16384 else 4) * 256
    assert cap * 4 * U < S and S % U != 0
    _check(_words(rng, S, R), ptr, rows, (R, F, S))


# ------------------------------------------------------------------------------------------------ the block kernel
@pytest.mark.parametrize("R,F", [(65, 1), (10, 33)])
def test_block_kernel_just_past_the_small_one(R, F):
    """One row, or one face, more than the small kernel takes."""
    rng = np.random.default_rng(R + F)
    ptr, rows = _all_rows(R) if F == 1 else _handmade(rng, R, F)
    for S in (1, 5, 67):
        _check(_words(rng, S, R), ptr, rows, (R, F, S))


@pytest.mark.parametrize("ppe,d", sorted(TOP_GRIDS))
def test_block_kernel_on_the_tables_of_top_simplices(ppe, d):
    """The face tables of 6- to 9-vertex simplices: 63, 127, 255 and 511 faces, a wave per face, round robin."""
    R, ptr, rows = _grid_table(ppe, d)
    rng = np.random.default_rng(10 * ppe + d)
    for S in (1, 4, 131):
        _check(_words(rng, S, R), ptr, rows, (ppe, d, S))


def test_block_kernel_empty_face_and_single_rows():
    """A face without rows between two others gets +0.0; faces of one row give the root of that row."""
    rng = np.random.default_rng(5)
    R = 70
    lists = [[69], rng.permutation(R)[:40], [], [0], rng.permutation(R), [], [33]] + [[int(r)] for r in rng.integers(0, R, 30)]
    ptr, rows = _csr(lists)
    words = _words(rng, 9, R)
    words[words == 0] = MIN_NORMAL             # no zero among the inputs: a zero in the output is the empty face's
    _check(words, ptr, rows, "empty")
    face, _ = _face_max(words, ptr, rows, False)
    assert (face[:, [2, 5]] == 0).all() and (face[:, [0, 1, 3, 4, 6]] != 0).all()


def test_whole_block_face_of_all_rows_vector_loads():
    """R = 1024, one face of all rows: four words per load; the maximum in the last row, in row 0, and in a row that
    only the last wave of the block reads (thread t loads rows 4t .. 4t + 3: row 800 belongs to thread 200)."""
    rng = np.random.default_rng(1024)
    R = 1024
    ptr, rows = _all_rows(R)
    words = _words(rng, 6, R)
    for s, row in enumerate((R - 1, 0, 800)):
        _peak(words, s, row)
    _check(words, ptr, rows, "uint4")
    face, _ = _face_max(words, ptr, rows, False)
    assert (face[:3, 0] == np.sqrt(np.array([MAX_FINITE], dtype=np.uint32).view(np.float32)).view(np.uint32)[0]).all()


def test_whole_block_face_of_all_rows_scalar_loads():
    """R = 1027 (no multiple of four), one face of all rows: one word per load, thread t reads rows t, t + 256, ...;
    rows 1026 and 0, and row 968 = 3 * 256 + 200 for the last wave."""
    rng = np.random.default_rng(1027)
    R = 1027
    ptr, rows = _all_rows(R)
    words = _words(rng, 6, R)
    for s, row in enumerate((R - 1, 0, 968)):
        _peak(words, s, row)
    _check(words, ptr, rows, "scalar")
    face, _ = _face_max(words, ptr, rows, False)
    assert (face[:3, 0] == np.sqrt(np.array([MAX_FINITE], dtype=np.uint32).view(np.float32)).view(np.uint32)[0]).all()


def test_whole_block_indexed_face_then_small_faces():
    """R = 1500: a face of 1100 rows in shuffled order (reduced by the whole block through its index list), then 40
    small faces (a wave each) in the same launch.  The maximum sits at the row listed last, listed first, and listed at
    position 1018 = 3 * 256 + 250, which only the last wave reads."""
    rng = np.random.default_rng(1500)
    R = 1500
    big = rng.permutation(R)[:1100]
    lists = [big] + [rng.choice(R, size=int(rng.integers(1, 200)), replace=False) for _ in range(40)]
    ptr, rows = _csr(lists)
    assert ptr[1] - ptr[0] >= BIG and int(np.diff(ptr)[1:].max()) < BIG
    words = _words(rng, 5, R)
    for s, pos in enumerate((1099, 0, 1018)):
        _peak(words, s, int(big[pos]))
    _check(words, ptr, rows, "indexed")
    face, _ = _face_max(words, ptr, rows, False)
    assert (face[:3, 0] == np.sqrt(np.array([MAX_FINITE], dtype=np.uint32).view(np.float32)).view(np.uint32)[0]).all()
    # the big face in the middle and at the end of the table: the first loop skips the small ones, the second the big
    for at in (20, 40):
        order = list(range(1, at + 1)) + [0] + list(range(at + 1, 41))
        ptr2, rows2 = _csr([lists[i] for i in order])
        _check(words, ptr2, rows2, ("indexed", at))


# ------------------------------------------------------------------------------------------------ permuted rows
def test_permuted_row_lists():
    """``core._sweep_dimension_bvh`` passes the face rows in sweep order (``SamplePlan.rows_perm``): the order of a
    face's list and of the rows must not matter.  A shuffled list per face, and the plan's own table against words
    permuted the same way."""
    R, ptr, rows = _grid_table(4, 6)
    rng = np.random.default_rng(46)
    shuffled = rows.copy()
    for f in range(len(ptr) - 1):
        shuffled[ptr[f]:ptr[f + 1]] = rng.permutation(rows[ptr[f]:ptr[f + 1]])
    assert not np.array_equal(shuffled, rows)
    words = _words(rng, 23, R)
    _check(words, ptr, shuffled, "shuffled")
    weights, _, face_idxs = core.generate_grid(4, 6, DEV, torch.float32)
    plan = core.SamplePlan(weights, core._FaceTable(face_idxs, R, DEV))
    assert plan.memb_all is None                                             # 127 faces: no fused face masks
    rows_perm, inv = plan.rows_perm.cpu().numpy(), plan.inv.cpu().numpy()
    assert not np.array_equal(rows_perm, rows) and np.array_equal(np.sort(inv), np.arange(R))
    permuted = np.empty_like(words)
    permuted[:, inv] = words                                                  # row r of the lattice sits at inv[r]
    want, _ = _reference(words, ptr, rows)
    face, _ = _face_max(permuted, ptr, rows_perm, False)
    assert np.array_equal(face, want)


# ------------------------------------------------------------------------------------------------ face values
def _face_values(bits):
    n = bits.shape[0]
    t_b = torch.as_tensor(bits.view(np.int32), device=DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((n + GUARD,), UNWRITTEN, dtype=torch.int32, device=DEV)
    _native.check(_native.load().flooder_face_values_f32(_native.ptr(t_b), n, _native.ptr(out), _stream()),
                  "flooder_face_values_f32")
    out = out.cpu().numpy().view(np.uint32)
    assert (out[n:] == UNWRITTEN).all(), "face_values wrote behind its output"
    return out[:n]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1_000_003])
def test_face_values_bitwise(n):
    """``np.sqrt`` per word; 1 000 003 words are more than 2048 blocks x 256 take in one turn."""
    bits = _words(np.random.default_rng(n), 1, max(n, 1))[0, :n]
    with np.errstate(all="ignore"):
        want = np.sqrt(bits.view(np.float32)).view(np.uint32)
    got = _face_values(bits)
    bad = np.argwhere(got != want).ravel()
    assert bad.size == 0, (n, bad.size, [(int(i), hex(bits[i]), hex(got[i]), hex(want[i])) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------ denormals
def test_denormal_inputs_bitwise():
    """Words below 0x00800000 (denormal float32 numbers, as a squared distance below 1.2e-38 is): the square root is a
    normal number and must be the correctly rounded one, in both kernels, in ``out_dist`` and in
    ``flooder_face_values_f32``."""
    rng = np.random.default_rng(8)

    def denormals(S, R):
        w = rng.integers(1, MIN_NORMAL, size=(S, R)).astype(np.uint32)
        w[rng.integers(0, 8, size=(S, R)) == 0] >>= np.uint32(12)              # short mantissas, down to one bit
        w[w == 0] = 1
        w[0, 0] = 1
        w[-1, -1] = MIN_NORMAL - 1
        return w

    R, ptr, rows = _grid_table(8, 2)                                            # the small kernel
    _check(denormals(37, R), ptr, rows, "denormal, small kernel")
    R, ptr, rows = _grid_table(3, 8)                                            # a wave per face
    _check(denormals(11, R), ptr, rows, "denormal, block kernel")
    ptr, rows = _all_rows(1027)                                                 # the whole block
    _check(denormals(3, 1027), ptr, rows, "denormal, whole block")
    bits = denormals(1, 5000)[0]
    with np.errstate(all="ignore"):
        want = np.sqrt(bits.view(np.float32)).view(np.uint32)
    got = _face_values(bits)
    bad = np.argwhere(got != want).ravel()
    assert bad.size == 0, (bad.size, [(hex(bits[i]), hex(got[i]), hex(want[i])) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    lib = _native.load()
    rng = np.random.default_rng(2)
    R, ptr, rows = _grid_table(8, 2)
    F = len(ptr) - 1
    S = 9
    words = _words(rng, S, R)
    t_w = torch.as_tensor(words.view(np.int32), device=DEV)
    t_ptr, t_rows = torch.as_tensor(ptr, device=DEV), torch.as_tensor(rows, device=DEV)
    face = torch.full((S * F,), UNWRITTEN, dtype=torch.int32, device=DEV)
    dist = torch.full((S * R,), UNWRITTEN, dtype=torch.int32, device=DEV)
    good = dict(d2=_native.ptr(t_w), S=S, R=R, ptr=_native.ptr(t_ptr), rows=_native.ptr(t_rows), F=F,
                face=_native.ptr(face), dist=_native.ptr(dist))

    def call(**change):
        a = {**good, **change}
        return lib.flooder_face_max_f32(a["d2"], a["S"], a["R"], a["ptr"], a["rows"], a["F"], a["face"], a["dist"], _stream())

    for name in ("d2", "ptr", "rows", "face"):
        assert call(**{name: None}) != 0, name
    assert call(F=0) != 0 and call(R=0) != 0
    assert call(S=0) == 0
    assert lib.flooder_face_values_f32(None, 5, _native.ptr(face), _stream()) != 0
    assert lib.flooder_face_values_f32(_native.ptr(t_w), 5, None, _stream()) != 0
    assert lib.flooder_face_values_f32(_native.ptr(t_w), -1, _native.ptr(face), _stream()) != 0
    assert lib.flooder_face_values_f32(_native.ptr(t_w), 0, _native.ptr(face), _stream()) == 0
    torch.cuda.synchronize()
    assert bool((face == UNWRITTEN).all()) and bool((dist == UNWRITTEN).all()), "a refused or empty call wrote"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((face != UNWRITTEN).all()) and bool((dist != UNWRITTEN).all())
    assert call(dist=None) == 0
