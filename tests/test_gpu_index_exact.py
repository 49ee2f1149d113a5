"""The point index against ``index_reference``: the bounding box, the curve codes word for word, the order of a
curve-built index, the padded rows and every node of the box tree, the density grid cell by cell with its cloud-kind
words, and the sub-cloud selection.  The C entry points are called directly through ``_native``, ``core.PointIndex``
where the whole build is meant.  What makes the inputs exact, and the conditions the comparisons rely on, is checked
on the host in ``test_index_reference_cpu.py``.

NaN and infinite coordinates are out of scope: the library documents no behaviour for them (NaN appears here only in
the gap columns of ``ld > dim`` inputs, which no kernel may read)."""

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import grad_reference as gr
import index_reference as ir
from helpers import get_options, set_options

pytestmark = pytest.mark.gpu

LATTICES, LEVEL_TABLE = ir.LATTICES, ir.LEVEL_TABLE

DEV = torch.device("cuda:0")
GUARD = 64                      # words behind an output buffer that no kernel may touch
SENT64 = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A


def _stream():
    return _native.current_stream_ptr(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. bounding box
BBOX_SIZES = (1, 255, 256, 257, 1025, 1_048_579)


def _bbox_input(n, dim, ld, seed):
    """Normal draws with rows of -0.0, +-FLT_MAX and denormals among them; gap columns NaN."""
    rng = np.random.default_rng(seed)
    a = np.full((n, ld), np.nan, dtype=np.float32)
    a[:, :dim] = rng.standard_normal((n, dim), dtype=np.float32)
    s = ir.special_rows(dim)
    if n == 1:
        a[0, :dim] = s[3]
    else:
        for row, at in zip(s, (0, 63, 64, n // 2, n - 2, n - 1)):
            a[at, :dim] = row
    return a


def _box_call(call):
    box = torch.full((16 + GUARD,), 12345.0, dtype=torch.float32, device=DEV)
    call(box)
    got = _host(box)
    assert (got[16:] == 12345.0).all(), "written behind the 16 floats of the box"
    return got[:16]


def _assert_box(got16, pts, dim, what):
    lo, hi = ir.bbox(pts[:, :dim])
    assert np.array_equal(got16[:dim], lo), (what, got16[:dim], lo)           # by value: -0.0 == 0.0, nothing else
    assert np.array_equal(got16[8:8 + dim], hi), (what, got16[8:8 + dim], hi)


@pytest.mark.parametrize("dim", range(1, 9))
def test_bounding_box(dim):
    """flooder_bbox_f32 and flooder_bbox_chunk_f32 + flooder_bbox_reduce_f32 against np.min / np.max."""
    lib = _native.load()
    partial = torch.empty(1024 * 16, dtype=torch.float32, device=DEV)
    for n in BBOX_SIZES:
        for ld in (dim, dim + 3):
            a = _bbox_input(n, dim, ld, 100 * dim + ld + n % 1000)
            t = _dev(a)
            partial.fill_(float("nan"))
            got = _box_call(lambda box: _native.check(lib.flooder_bbox_f32(
                _native.ptr(t), n, dim, ld, _native.ptr(box), _native.ptr(partial), _stream()), "flooder_bbox_f32"))
            _assert_box(got, a, dim, ("whole", n, ld))
            # three chunks of 64 blocks each, the last one ragged
            per = (n + 2) // 3
            cuts = [(c * per, min(n, (c + 1) * per)) for c in range(3) if c * per < n]
            part = torch.full((len(cuts) * 64 * 16,), float("nan"), dtype=torch.float32, device=DEV)
            for c, (lo, hi) in enumerate(cuts):
                _native.check(lib.flooder_bbox_chunk_f32(t[lo:hi].data_ptr(), hi - lo, dim, ld,
                                                         part[c * 64 * 16:].data_ptr(), 64, _stream()), "bbox_chunk")
            got = _box_call(lambda box: _native.check(lib.flooder_bbox_reduce_f32(
                _native.ptr(part), len(cuts) * 64, dim, _native.ptr(box), _stream()), "flooder_bbox_reduce_f32"))
            _assert_box(got, a, dim, ("chunks", n, ld))


@pytest.mark.parametrize("dim", [1, 3, 8])
def test_bounding_box_of_more_than_256_partials(dim):
    """Five chunks of 64 blocks, the last chunk three rows long: 320 partial rows (the final kernel loops), most blocks
    of the last chunk own no row and their (+inf, -inf) partials must not enter the result; the extremes of the cloud
    sit in those last three rows, behind the first 256 partials."""
    lib = _native.load()
    per, n, ld = 5000, 4 * 5000 + 3, dim + 3
    a = _bbox_input(n, dim, ld, 77 + dim)
    a[63, :dim] = 0.5                                     # (no +-FLT_MAX here: the extremes sit at the end)
    a[64, :dim] = -0.5
    a[n - 3, :dim] = np.float32(5e6)
    a[n - 2, :dim] = np.float32(-7e6)
    a[n - 1, :dim] = np.float32(-0.0)
    assert np.abs(a[:n - 3, :dim]).max() < 100
    t = _dev(a)
    part = torch.full((5 * 64 * 16,), float("nan"), dtype=torch.float32, device=DEV)
    for c in range(5):
        lo, hi = c * per, min(n, (c + 1) * per)
        _native.check(lib.flooder_bbox_chunk_f32(t[lo:hi].data_ptr(), hi - lo, dim, ld, part[c * 64 * 16:].data_ptr(), 64,
                                                 _stream()), "bbox_chunk")
    got = _box_call(lambda box: _native.check(lib.flooder_bbox_reduce_f32(
        _native.ptr(part), 320, dim, _native.ptr(box), _stream()), "flooder_bbox_reduce_f32"))
    _assert_box(got, a, dim, "320 partials")
    p = _host(part).reshape(320, 16)
    assert np.isposinf(p[257:, :dim]).all() and np.isneginf(p[257:, 8:8 + dim]).all()   # blocks without a row


# ---------------------------------------------------------------------------------------------- 2. curve codes
def _codes(lib, pts, dim, box, ld=None, zero=None):
    """Codes of flooder_morton_f32 (``zero``: (buffer, words) for flooder_morton_zero_f32) as uint64, after the storage
    contract of flooder_curve_key_bits is checked: at most 32 key bits give n uint32 words, more give int64 words."""
    n = pts.shape[0]
    ld = pts.shape[1] if ld is None else ld
    key_bits = int(lib.flooder_curve_key_bits(dim))
    buf = torch.full((n + GUARD,), SENT64, dtype=torch.int64, device=DEV)
    t, b = _dev(pts), _dev(box)
    if zero is None:
        _native.check(lib.flooder_morton_f32(_native.ptr(t), n, dim, ld, _native.ptr(b), _native.ptr(buf), _stream()),
                      "flooder_morton_f32")
    else:
        _native.check(lib.flooder_morton_zero_f32(_native.ptr(t), n, dim, ld, _native.ptr(b), _native.ptr(buf),
                                                  _native.ptr(zero[0]), zero[1], _stream()), "flooder_morton_zero_f32")
    raw = _host(buf)
    if key_bits <= 32:
        words = raw.view(np.uint32)
        assert (words[n:] == SENT32).all(), "narrow keys are n uint32 words"
        return words[:n].astype(np.uint64), key_bits
    assert (raw[n:] == SENT64).all()
    return raw[:n].view(np.uint64).copy(), key_bits


def _lattice_case(dim, bits):
    """The full lattice (one axis: it keeps 21 bits, so the lattice is a corner of its range), a few points outside
    the box, and the box (0, 2^b - 1) that makes the scale exactly 1."""
    b = ir.curve_bits(dim, bits)
    cells = ir.full_lattice(dim, bits).astype(np.float32)
    top = float((1 << b) - 1)
    outside = np.array([[-5.0] * dim, [top + 4.0] * dim, [top] * dim, [-0.0] * dim], dtype=np.float32)
    outside[0, dim - 1] = top + 100.0
    return np.concatenate([cells, outside]), np.zeros(dim, np.float32), np.full(dim, top, np.float32), b


@pytest.mark.parametrize("dim,bits", LATTICES)
def test_curve_codes_of_the_full_lattice(dim, bits):
    """Option curve_bits = b, integer points, box (0, 2^b - 1): every operation of the kernel is exact and its codes
    are the reference's word for word, Hilbert and Morton; points outside the box land in the rim cells; an axis of
    no extent gives cell 0 on that axis."""
    lib = _native.load()
    keep = get_options(lib, b"curve_bits", b"curve")
    try:
        set_options(lib, {b"curve_bits": bits})
        pts, lo, hi, b = _lattice_case(dim, bits)
        for curve in (1, 0):
            set_options(lib, {b"curve": curve})
            got, key_bits = _codes(lib, pts, dim, ir.box16(lo, hi))
            assert key_bits == b * dim
            assert np.array_equal(got, ir.point_codes(pts, lo, hi, b, curve)), (dim, bits, curve)
            n_cells = 1 << (bits * dim)
            if dim > 1:
                assert np.array_equal(np.sort(got[:n_cells]), np.arange(n_cells, dtype=np.uint64))
            flat = hi.copy()
            flat[0] = 0.0                                  # no extent on axis 0
            got, _ = _codes(lib, pts, dim, ir.box16(lo, flat))
            assert np.array_equal(got, ir.point_codes(pts, lo, flat, b, curve)), (dim, bits, curve, "flat axis")
            moved = pts.copy()
            moved[:, 0] = 0.0
            assert np.array_equal(got, ir.point_codes(moved, lo, hi, b, curve))    # cell 0 on that axis
    finally:
        set_options(lib, keep)


@pytest.mark.parametrize("dim,bits", [(3, 11), (3, 21), (8, 7)])
def test_wide_curve_codes(dim, bits):
    """More than 32 key bits: int64 words.  Random cells of the lattice (dimension 8 sits at its cap of 7 bits)."""
    lib = _native.load()
    keep = get_options(lib, b"curve_bits", b"curve")
    try:
        set_options(lib, {b"curve_bits": 12 if dim == 8 else bits})
        rng = np.random.default_rng(dim * bits)
        top = (1 << bits) - 1
        pts = rng.integers(0, top + 1, (30_011, dim)).astype(np.float32)
        pts[0], pts[1] = 0.0, float(top)
        lo, hi = np.zeros(dim, np.float32), np.full(dim, top, np.float32)
        for curve in (1, 0):
            set_options(lib, {b"curve": curve})
            got, key_bits = _codes(lib, pts, dim, ir.box16(lo, hi))
            assert key_bits == bits * dim > 32
            assert np.array_equal(got, ir.point_codes(pts, lo, hi, bits, curve)), (dim, bits, curve)
    finally:
        set_options(lib, keep)


@pytest.mark.parametrize("dim", [2, 3, 6])
def test_curve_codes_of_random_floats(dim):
    """Default bits, normal draws, the cloud's own box: the reference quantises in float32 in the kernel's order of
    operations (no fused multiply-add can form in (p - lo) * scale, the division is the correctly rounded one)."""
    lib = _native.load()
    keep = get_options(lib, b"curve")
    try:
        n = 100_003
        a = np.full((n, dim + 3), np.nan, dtype=np.float32)
        a[:, :dim] = ir.gaussian(n, dim, 40 + dim)
        lo, hi = ir.bbox(a[:, :dim])
        for curve in (1, 0):
            set_options(lib, {b"curve": curve})
            for pts, ld in ((np.ascontiguousarray(a[:, :dim]), dim), (a, dim + 3)):
                got, key_bits = _codes(lib, pts, dim, ir.box16(lo, hi), ld=ld)
                assert key_bits == ir.curve_bits(dim) * dim
                want = ir.point_codes(a[:, :dim], lo, hi, ir.curve_bits(dim), curve)
                assert np.array_equal(got, want), (dim, curve, ld, int((got != want).sum()))
    finally:
        set_options(lib, keep)


def test_morton_zero_clears_exactly_its_words():
    lib = _native.load()
    pts, lo, hi, b = _lattice_case(2, 1)                   # eight points: one workgroup strides over the buffer
    for words in (0, 1, 255, 100_003):
        buf = torch.full((words + GUARD,), SENT32, dtype=torch.int32, device=DEV)
        got, _ = _codes(lib, pts, 2, ir.box16(lo, np.full(2, float((1 << ir.curve_bits(2)) - 1), np.float32)),
                        zero=(buf, words))
        z = _host(buf)
        assert (z[:words] == 0).all() and (z[words:] == SENT32).all(), words
        assert np.array_equal(got, ir.point_codes(pts, lo, np.full(2, float((1 << ir.curve_bits(2)) - 1), np.float32),
                                                  ir.curve_bits(2)))


# ---------------------------------------------------------------------------------------------- 3. curve order
def _index_box(idx):
    box = _host(idx.box)
    return box[:idx.dim].copy(), box[8:8 + idx.dim].copy()


@pytest.mark.parametrize("dim,kind", [(2, "normal"), (3, "normal"), (2, "tripled"), (3, "tripled"), (2, "million"),
                                      (3, "million")])
def test_order_of_a_curve_built_index(dim, kind):
    """``order32`` is the stable argsort of the reference codes taken with the index's own box: equal codes stay in
    ascending original index (every point tripled: runs of three at least); a million points take the radix sort's
    size-chosen block shape."""
    n = {"normal": 100_003, "tripled": 20_001, "million": 1_048_579}[kind]
    pts = ir.gaussian(n, dim, 60 + dim)
    if kind == "tripled":
        pts = np.concatenate([pts, pts, pts])
    idx = core.PointIndex(_dev(pts))
    assert not idx.kd
    lo, hi = _index_box(idx)
    _assert_box(_host(idx.box), pts, dim, "index box")
    want = ir.curve_order(pts, lo, hi, ir.curve_bits(dim))
    assert np.array_equal(_host(idx.order32).astype(np.int64), want)


# ---------------------------------------------------------------------------------------------- 4. rows and the tree
def _assert_rows(rows, want, what):
    got = _host(rows)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.int32) == want.view(np.int32)            # bit for bit: pad columns +0.0, pad rows +inf
    assert same.all(), (what, "first differing row", int(np.nonzero(~same.all(axis=1))[0][0]))


def _assert_nodes(nodes, want, n, what):
    got = _host(nodes)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for level, (off, count) in enumerate(ir.make_levels(n)[0]):
        pad = (count + 63) // 64 * 64
        same = (got[off:off + pad] == want[off:off + pad]).all(axis=1)   # by value (no NaN on either side)
        assert same.all(), (what, "level", level, "first differing node", int(np.nonzero(~same)[0][0]), "of", count)
    assert np.array_equal(got, want), what


def _check_index(pts, want_kd=None, curve_order=False):
    """PointIndex of ``pts`` and flooder_gather_rows_f32 + flooder_bvh_build_f32 with its order, both against the
    reference rows and the reference tree of ``pts[order]``."""
    lib = _native.load()
    n, dim = pts.shape
    t = _dev(pts)
    idx = core.PointIndex(t)
    if want_kd is not None:
        assert idx.kd == want_kd
    order = _host(idx.order32).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n)), "the order is no permutation"
    if curve_order:
        lo, hi = _index_box(idx)
        assert np.array_equal(order, ir.curve_order(pts, lo, hi, ir.curve_bits(dim)))
    rows_ref = ir.padded_rows(pts, order)
    nodes_ref = ir.tree_nodes(pts[order])
    assert int(lib.flooder_bvh_node_count(n)) == nodes_ref.shape[0] == idx.nodes.shape[0]
    _assert_rows(idx.pts, rows_ref, ("PointIndex rows", n, dim))
    _assert_nodes(idx.nodes, nodes_ref, n, ("PointIndex nodes", n, dim))
    rows = torch.full_like(idx.pts, float("nan"))
    nodes = torch.full_like(idx.nodes, float("nan"))
    _native.check(lib.flooder_gather_rows_f32(_native.ptr(t), n, dim, dim, _native.ptr(idx.order32), _native.ptr(rows),
                                              rows.shape[0], _stream()), "flooder_gather_rows_f32")
    _native.check(lib.flooder_bvh_build_f32(_native.ptr(rows), n, dim, _native.ptr(nodes), _stream()),
                  "flooder_bvh_build_f32")
    _assert_rows(rows, rows_ref, ("gathered rows", n, dim))
    _assert_nodes(nodes, nodes_ref, n, ("built nodes", n, dim))
    return idx, order


@pytest.mark.parametrize("n", [n for n in sorted(LEVEL_TABLE) if n < 1_000_000])
def test_rows_and_tree_at_the_level_boundaries(n):
    _check_index(ir.gaussian(n, 3, n % 1000), want_kd=False, curve_order=True)


def test_rows_and_tree_of_four_levels():
    """4 194 305 points in the plane: four levels, and the stride loop of the gather beyond its 8192 workgroups."""
    n = 4_194_305
    assert LEVEL_TABLE[n] == 4 and (n + 15) // 16 * 16 > 8192 * 256
    _check_index(ir.gaussian(n, 2, 4))


@pytest.mark.parametrize("n", [1025, 65_537])
@pytest.mark.parametrize("dim", range(1, 9))
def test_rows_and_tree_in_every_dimension(dim, n):
    """Padded widths 2, 4 and 8, each dimension its own template instance; above three dimensions this is the k-d
    order (the default)."""
    _check_index(ir.gaussian(n, dim, 10 * dim + n % 7), want_kd=dim > 3, curve_order=dim <= 3)


@pytest.mark.parametrize("n", [1025, 65_537])
@pytest.mark.parametrize("dim", range(4, 9))
def test_rows_and_tree_in_curve_order_above_three_dimensions(dim, n, monkeypatch):
    monkeypatch.setattr(core, "KD_ORDER_ABOVE_DIM", 8)
    _check_index(ir.gaussian(n, dim, 10 * dim + n % 7), want_kd=False, curve_order=True)


@pytest.mark.parametrize("dim,kd_above", [(2, 3), (3, 3), (5, 3), (5, 8), (8, 3)])
def test_rows_and_tree_of_special_values(dim, kd_above, monkeypatch):
    """-0.0, denormals of both signs and +-3e38: a box must contain its rows exactly (a denormal bound flushed to zero
    would not).  The cloud's extent overflows float32, so nothing is said about the ORDER here - any order is valid."""
    monkeypatch.setattr(core, "KD_ORDER_ABOVE_DIM", kd_above)
    pts = ir.special_cloud(2100, dim, 7)
    idx, order = _check_index(pts)
    nodes, dp = _host(idx.nodes), idx.dp
    rows = pts[order]
    leaf = np.arange(2100) // 16
    assert (nodes[leaf, :dim] <= rows).all() and (rows <= nodes[leaf, dp:dp + dim]).all()


@pytest.mark.parametrize("dim,kd_above", [(3, 3), (5, 3), (5, 8)])
def test_rows_and_tree_of_one_point_repeated(dim, kd_above, monkeypatch):
    monkeypatch.setattr(core, "KD_ORDER_ABOVE_DIM", kd_above)
    pts = np.tile(ir.gaussian(1, dim, 3), (2100, 1))
    idx, order = _check_index(pts)
    if not idx.kd:
        assert np.array_equal(order, np.arange(2100))             # equal codes: the stable order is the identity


@pytest.mark.parametrize("dim", [2, 3, 5])
def test_index_rows_with_a_row_stride(dim):
    """flooder_index_rows_f32 with ld = dim + 3, NaN in the gap, and a random permutation as the order (any order is
    a valid index)."""
    lib = _native.load()
    n = 66_561
    a = np.full((n, dim + 3), np.nan, dtype=np.float32)
    a[:, :dim] = ir.gaussian(n, dim, 90 + dim)
    order = np.random.default_rng(dim).permutation(n)
    rows_ref, nodes_ref = ir.padded_rows(a[:, :dim], order), ir.tree_nodes(a[order, :dim])
    rows = torch.full(rows_ref.shape, float("nan"), dtype=torch.float32, device=DEV)
    nodes = torch.full(nodes_ref.shape, float("nan"), dtype=torch.float32, device=DEV)
    t, o = _dev(a), _dev(order.astype(np.int32))
    _native.check(lib.flooder_index_rows_f32(_native.ptr(t), n, dim, dim + 3, _native.ptr(o), _native.ptr(rows),
                                             rows.shape[0], _native.ptr(nodes), 0, 0, _stream()), "flooder_index_rows_f32")
    _assert_rows(rows, rows_ref, ("strided rows", dim))
    _assert_nodes(nodes, nodes_ref, n, ("strided nodes", dim))


# ---------------------------------------------------------------------------------------------- 5 / 6. density grid
def _grids(pts):
    """(index, fused grid + words, stand-alone grid + words, rows in index order, box) of a cloud."""
    lib = _native.load()
    n, dim = pts.shape
    nf = ir.grid_cells(dim) ** dim
    idx = core.PointIndex(_dev(pts))
    assert int(lib.flooder_density_grid_words(dim)) == nf + 4 == idx.dens.numel()
    alone = torch.zeros(nf + 4, dtype=torch.int32, device=DEV)
    _native.check(lib.flooder_density_grid_f32(_native.ptr(idx.nodes), n, dim, _native.ptr(idx.box), _native.ptr(alone),
                                               _stream()), "flooder_density_grid_f32")
    before = _host(alone).astype(np.int64)
    assert (before[nf:] == 0).all()                                      # the grid alone leaves the words alone
    _native.check(lib.flooder_cloud_kind(_native.ptr(alone), dim, _stream()), "flooder_cloud_kind")
    after = _host(alone).astype(np.int64)
    assert np.array_equal(before[:nf], after[:nf])
    lo, hi = _index_box(idx)
    return idx, _host(idx.dens).astype(np.int64), after, pts[_host(idx.order32).astype(np.int64)], lo, hi


def _assert_kind(words, grid, dim, n, what):
    """Words [2], [3]: points in interior coarse cells, all points; [0], [1]: reserved, nothing writes them."""
    inner, total = ir.cloud_kind(grid, dim)
    assert total == n
    assert words.tolist() == [0, 0, inner, n], (what, words.tolist(), inner, n)


@pytest.mark.parametrize("n", ir.INTEGER_SIZES + (1, 16, 1024))
@pytest.mark.parametrize("dim", [2, 3])
def test_density_grid_of_integer_clouds(dim, n):
    """Integer coordinates in [0, G]^dim: the fused grid of the index build and the grid of flooder_density_grid_f32
    equal the reference in every cell, and the cloud-kind words of both forms equal the reference - also for a tree of
    one level (n <= 1024), where the index build launches the statistic on its own."""
    pts = ir.integer_cloud(n, dim, 100 + dim)
    nf = ir.grid_cells(dim) ** dim
    idx, fused, alone, rows, lo, hi = _grids(pts)
    if n > 1:
        assert (lo == 0).all() and (hi == ir.grid_cells(dim)).all()
    want = ir.density_grid(rows, lo, hi)
    assert want.sum() == n
    assert np.array_equal(fused[:nf], want), ("fused", int((fused[:nf] != want).sum()))
    assert np.array_equal(alone[:nf], want), ("stand-alone", int((alone[:nf] != want).sum()))
    _assert_kind(alone[nf:], want, dim, n, "stand-alone")
    _assert_kind(fused[nf:], want, dim, n, "fused")


@pytest.mark.parametrize("name", sorted(ir.FLOAT_CLOUDS))
def test_density_grid_of_float_clouds(name):
    """Random float clouds: the sum is n, and every leaf sits in the reference's cell - or in the neighbouring one along
    an axis where the float64 centre lies within 2^-12 cell of the boundary (at most 1 % of the leaves: asserted on the
    host for these seeds).  The words are exact integers of the grid they were computed from."""
    dim, make = ir.FLOAT_CLOUDS[name]
    pts = make()
    n, nf = pts.shape[0], ir.grid_cells(dim) ** dim
    idx, fused, alone, rows, lo, hi = _grids(pts)
    _assert_box(_host(idx.box), pts, dim, name)
    assert np.array_equal(rows, pts[ir.curve_order(pts, lo, hi, ir.curve_bits(dim))])    # the order the host test assumed
    for what, grid in (("fused", fused), ("stand-alone", alone)):
        assert grid[:nf].sum() == n
        n_amb = ir.check_density_grid(grid[:nf], rows, lo, hi)
        assert n_amb <= 0.01 * ((n + 15) // 16)
        _assert_kind(grid[nf:], grid[:nf], dim, n, (name, what))


# ---------------------------------------------------------------------------------------------- 7. sub-cloud selection
def _select(pts, dim, box_lo, box_hi, centers=None, radii=None, ld=None):
    """flooder_box_select_f32 called directly; returns the rows written (``count`` of them, checked against what the
    output buffer shows)."""
    lib = _native.load()
    n = pts.shape[0]
    ld = dim if ld is None else ld
    t = _dev(pts)
    out = torch.full((n + GUARD, dim), float("nan"), dtype=torch.float32, device=DEV)
    count = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
    bbox = _dev(np.concatenate([box_lo, box_hi]).astype(np.float32))
    nb = int(lib.flooder_select_grid_bytes(dim))
    assert (nb > 0) == (dim in (2, 3))
    flags = cbox = c = r = None
    if centers is not None and nb > 0:
        flags = torch.zeros(nb + GUARD, dtype=torch.uint8, device=DEV)
        cbox = _dev(ir.box16(*ir.bbox(pts[:, :dim])))
        c, r = _dev(centers.astype(np.float32)), _dev(radii.astype(np.float32))
    _native.check(lib.flooder_box_select_f32(_native.ptr(t), n, dim, ld, _native.ptr(bbox), _native.ptr(cbox),
                                             _native.ptr(c), _native.ptr(r), 0 if c is None else centers.shape[0],
                                             _native.ptr(flags), _native.ptr(out), _native.ptr(count), _stream()),
                  "flooder_box_select_f32")
    cnt = _host(count)
    assert (cnt[1:] == 0).all() and 0 <= cnt[0] <= n
    rows = _host(out)
    written = ~np.isnan(rows).any(axis=1)
    assert written[:cnt[0]].all() and not written[cnt[0]:].any(), "count is not the number of rows written"
    if flags is not None:
        f = _host(flags)
        assert (f[nb:] == 0).all() and set(np.unique(f[:nb]).tolist()) <= {0, 1}
    return rows[:cnt[0]]


def _select_cloud(n, dim, seed):
    pts = ir.gaussian(n, dim, seed)
    if n > 100:                                    # duplicated rows: the selection is a sub-MULTIset
        pts[n // 2:n // 2 + 20] = pts[:20]
    return pts


def _tight_box(pts):
    """A box between the 10 % and 90 % quantiles of every axis whose bounds along axis 0 are the coordinates of two
    rows inside it."""
    n = pts.shape[0]
    s = np.sort(pts, axis=0)
    lo, hi = s[n // 10].copy(), s[n - 1 - n // 10].copy()
    inside = np.nonzero(ir.inside_box(pts, lo, hi))[0]
    j = inside[0]
    i = inside[pts[inside, 0] > pts[j, 0]][0]
    lo[0], hi[0] = pts[j, 0], pts[i, 0]
    assert ir.inside_box(pts[[j, i]], lo, hi).all()
    return lo, hi, (int(j), int(i))


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 300_000])
@pytest.mark.parametrize("dim", [2, 3, 5])
def test_sub_cloud_selection(dim, n):
    """Dimensions 2 and 3 go through the flag grid, 5 through the box alone; one workgroup step takes 2048 rows."""
    pts = _select_cloud(n, dim, 200 + dim)
    lo, hi = ir.bbox(pts)
    rng = np.random.default_rng(n + dim)
    wide = (lo - 1, hi + 1)
    # no ball reaches the cloud: far away, the box is the balls' own
    centers = (np.full((3, dim), 50.0) + rng.standard_normal((3, dim))).astype(np.float32)
    radii = np.array([1.0, 2.0, 0.5], dtype=np.float32)
    far = ((centers - radii[:, None]).min(axis=0), (centers + radii[:, None]).max(axis=0))
    assert _select(pts, dim, *far, centers, radii).shape[0] == 0
    # one ball covering everything, the box wide: every row
    centers, radii = np.zeros((1, dim), np.float32), np.array([float(np.abs(pts).max()) * 3 * dim + 1], np.float32)
    sel = _select(pts, dim, *wide, centers, radii)
    assert ir.check_selection(sel, pts, *wide, centers, radii) == n == sel.shape[0]
    # ... and a box whose bounds ARE coordinates of rows inside it (bounds are inclusive)
    if n > 1:
        tight_lo, tight_hi, on_rim = _tight_box(pts)
        sel = _select(pts, dim, tight_lo, tight_hi, centers, radii)
        assert ir.check_selection(sel, pts, tight_lo, tight_hi, centers, radii) == sel.shape[0]
        have = ir.multiset(sel)
        assert all(ir.row_keys(pts[j:j + 1])[0].tobytes() in have for j in on_rim)
    # balls hanging over the rim of the cloud's box, and some inside; the box is the balls' own (block_subcloud's)
    k = 40
    centers = np.concatenate([np.where(rng.random((k, dim)) < 0.5, lo, hi) + 0.1 * rng.standard_normal((k, dim)),
                              0.5 * rng.standard_normal((k, dim))]).astype(np.float32)
    radii = rng.uniform(0.05, 0.6, 2 * k).astype(np.float32)     # (float32 as the kernel reads them; the reference widens)
    own = ((centers - radii[:, None]).min(axis=0), (centers + radii[:, None]).max(axis=0))
    sel = _select(pts, dim, *own, centers, radii)
    need = ir.check_selection(sel, pts, *own, centers, radii)
    assert need <= sel.shape[0]
    if n >= 2047:
        assert 0 < need
        if dim in (2, 3):
            assert sel.shape[0] < ir.inside_box(pts, *own).sum()          # the flag grid did cut something away


def test_sub_cloud_selection_with_a_row_stride():
    n, dim = 5000, 3
    a = np.full((n, dim + 3), np.nan, dtype=np.float32)
    a[:, :dim] = _select_cloud(n, dim, 9)
    lo, hi = np.full(dim, -0.7, np.float32), np.full(dim, 0.9, np.float32)
    centers, radii = np.zeros((1, dim)), np.array([0.8])
    lib = _native.load()
    t = _dev(a)
    out = torch.full((n, dim), float("nan"), dtype=torch.float32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    flags = torch.zeros(int(lib.flooder_select_grid_bytes(dim)), dtype=torch.uint8, device=DEV)
    bbox, cbox = _dev(np.concatenate([lo, hi])), _dev(ir.box16(*ir.bbox(a[:, :dim])))
    c, r = _dev(centers.astype(np.float32)), _dev(radii.astype(np.float32))
    _native.check(lib.flooder_box_select_f32(_native.ptr(t), n, dim, dim + 3, _native.ptr(bbox), _native.ptr(cbox),
                                             _native.ptr(c), _native.ptr(r), 1, _native.ptr(flags), _native.ptr(out),
                                             _native.ptr(count), _stream()), "flooder_box_select_f32")
    sel = _host(out)[:int(_host(count)[0])]
    assert ir.check_selection(sel, a[:, :dim], lo, hi, centers, radii) > 0


def test_block_subcloud_keeps_every_nearest_neighbour():
    """``core.block_subcloud`` with farthest-point landmarks: the nearest cloud point (float64 brute force) of every
    lattice sample of the block's simplices is in the sub-cloud, which is a sub-multiset of the cloud."""
    from scipy.spatial import Delaunay

    pts = ir.gaussian(20_000, 3, 31)
    tp = _dev(pts)
    lms = fa.generate_landmarks(tp, 60, start_idx=0)
    lm = _host(lms).astype(np.float64)
    simplices = Delaunay(lm).simplices[:25]
    verts = lm[simplices]                                              # (S, 4, 3)
    sub = _host(core.block_subcloud(tp, _dev(verts.astype(np.float32)), 3))
    have, cloud = ir.multiset(sub), ir.multiset(pts)
    assert 0 < sub.shape[0] < pts.shape[0]
    assert all(key in cloud and c <= cloud[key] for key, c in have.items())
    w = gr.lattice(6, 3).numpy()
    samples = np.einsum("rj,sjk->srk", w, verts).reshape(-1, 3)
    p64 = pts.astype(np.float64)
    nearest = np.unique(np.concatenate([np.argmin(((samples[a:a + 64, None, :] - p64[None, :, :]) ** 2).sum(axis=2), axis=1)
                                        for a in range(0, samples.shape[0], 64)]))
    missing = [int(j) for j in nearest if ir.row_keys(pts[j:j + 1])[0].tobytes() not in have]
    assert not missing, missing
