"""The reference of the point index (``index_reference``) and the inputs of ``test_gpu_index_exact.py``, checked on the
host: the defining properties of the curve codes on full lattices, the level table of the box tree, the reference tree
against a plain loop, the cloud-kind words against a plain loop, and the conditions the device tests rely on (exact
quantisation of the lattice inputs, exact grid cells of the integer clouds, the cap on ambiguous leaves of the random
float clouds)."""

import functools

import numpy as np
import pytest

import index_reference as ir

LATTICES, LEVEL_TABLE = ir.LATTICES, ir.LEVEL_TABLE


@pytest.mark.parametrize("dim,bits", LATTICES)
def test_curve_codes_on_the_full_lattice(dim, bits):
    """Both codes are bijections onto [0, 2^(bits dim)) with code 0 at the origin; consecutive Hilbert codes are
    lattice neighbours at L1 distance exactly 1."""
    cells = ir.full_lattice(dim, bits)
    n = cells.shape[0]
    assert n == 1 << (bits * dim)
    for curve in (1, 0):
        codes = ir.curve_codes(cells, bits, curve)
        assert np.array_equal(np.sort(codes), np.arange(n, dtype=np.uint64)), (dim, bits, curve)
        assert not cells[np.argmin(codes)].any()
    walk = cells[np.argsort(ir.hilbert_codes(cells, bits))].astype(np.int64)
    assert (np.abs(np.diff(walk, axis=0)).sum(axis=1) == 1).all()


def test_morton_codes_are_the_bit_interleave():
    rng = np.random.default_rng(0)
    cells = rng.integers(0, 1 << 7, (200, 3)).astype(np.uint64)
    codes = ir.morton_codes(cells, 7)
    for row, code in zip(cells.tolist(), codes.tolist()):
        want = 0
        for k, v in enumerate(row):
            for b in range(7):
                want |= ((v >> b) & 1) << (3 * b + k)
        assert code == want


def test_wide_codes_stay_injective():
    """The wide cases of the device test (more than 32 key bits) on random cells: distinct cells, distinct codes, all
    below 2^(bits dim)."""
    rng = np.random.default_rng(1)
    for dim, bits in ((3, 11), (3, 21), (8, 7)):
        cells = np.unique(rng.integers(0, 1 << bits, (20_000, dim)).astype(np.uint64), axis=0)
        for curve in (1, 0):
            codes = ir.curve_codes(cells, bits, curve)
            assert np.unique(codes).size == cells.shape[0]
            assert int(codes.max()) < 1 << (bits * dim)


def test_curve_bits():
    assert [ir.curve_bits(d) for d in range(1, 9)] == [21, 12, 8, 12, 12, 10, 9, 7]
    assert ir.curve_bits(3, 21) == 21 and ir.curve_bits(3, 11) == 11 and ir.curve_bits(8, 12) == 7
    assert ir.curve_bits(1, 6) == 21          # one axis keeps its cap whatever the option says


@pytest.mark.parametrize("dim,bits", LATTICES)
def test_lattice_inputs_quantise_exactly(dim, bits):
    """With the box (0, 2^bits - 1) the scale is exactly 1 and every lattice point is its own cell; points outside
    land in the rim cells; an axis of no extent gives cell 0."""
    b = ir.curve_bits(dim, bits)              # (one axis: 21 bits whatever was asked for)
    cells = ir.full_lattice(dim, bits)
    lo, hi = np.zeros(dim, np.float32), np.full(dim, (1 << b) - 1, np.float32)
    assert np.array_equal(ir.quantise(cells.astype(np.float32), lo, hi, b), cells)
    out = np.array([[-5.0] * dim, [float(1 << b) + 3.0] * dim], dtype=np.float32)
    assert np.array_equal(ir.quantise(out, lo, hi, b), np.array([[0] * dim, [(1 << b) - 1] * dim], dtype=np.uint64))
    flat_hi = hi.copy()
    flat_hi[dim - 1] = 0.0
    assert (ir.quantise(cells.astype(np.float32), lo, flat_hi, b)[:, dim - 1] == 0).all()


@pytest.mark.parametrize("n,levels", sorted(LEVEL_TABLE.items()))
def test_level_table(n, levels):
    lv, total = ir.make_levels(n)
    assert len(lv) == levels
    assert lv[0] == (0, (n + 15) // 16)
    for (off, count), (off2, count2) in zip(lv, lv[1:]):
        assert off2 == off + (count + 63) // 64 * 64 and count2 == (count + 63) // 64 and count > 64
    assert lv[-1][1] <= 64 and total == lv[-1][0] + 64
    assert all(off % 64 == 0 for off, _ in lv)


def test_1024_points_are_exactly_64_leaves():
    assert ir.make_levels(1024) == ([(0, 64)], 64)
    assert ir.make_levels(1025) == ([(0, 65), (128, 2)], 192)
    assert ir.make_levels(65_536)[0] == [(0, 4096), (4096, 64)]
    assert ir.make_levels(65_537)[0] == [(0, 4097), (4160, 65), (4288, 2)]


@pytest.mark.parametrize("n,dim", [(1, 3), (17, 2), (1025, 5), (66_561, 3)])
def test_reference_tree_against_a_plain_loop(n, dim):
    rows = ir.gaussian(n, dim, 5)
    nodes = ir.tree_nodes(rows)
    dp = ir.padded_dim(dim)
    lv, total = ir.make_levels(n)
    assert nodes.shape == (total, 2 * dp)
    empty = np.concatenate([np.full(dp, np.inf), np.full(dp, -np.inf)]).astype(np.float32)
    want = np.tile(empty, (total, 1))
    for leaf in range(lv[0][1]):
        part = rows[16 * leaf:16 * leaf + 16]
        want[leaf, :dim], want[leaf, dp:dp + dim] = part.min(axis=0), part.max(axis=0)
    for (off, count), (poff, pcount) in zip(lv[1:], lv):
        for i in range(count):
            kids = want[poff + 64 * i:poff + min(64 * i + 64, pcount)]
            want[off + i, :dim], want[off + i, dp:dp + dim] = kids[:, :dim].min(axis=0), kids[:, dp:dp + dim].max(axis=0)
    assert np.array_equal(nodes, want)
    # every box contains its rows, the root level contains everything
    top_off, top_count = lv[-1]
    assert np.array_equal(nodes[top_off:top_off + top_count, :dim].min(axis=0), rows.min(axis=0))
    assert np.array_equal(nodes[top_off:top_off + top_count, dp:dp + dim].max(axis=0), rows.max(axis=0))
    pr = ir.padded_rows(rows, np.arange(n))
    assert pr.shape == ((n + 15) // 16 * 16, dp)
    assert np.array_equal(pr[:n, :dim], rows) and (pr[:n, dim:] == 0).all() and np.isposinf(pr[n:]).all()


def test_special_cloud_holds_what_it_says():
    for dim in (3, 5):
        p = ir.special_cloud(2100, dim, 7)
        tiny = np.finfo(np.float32).tiny
        assert (np.signbit(p) & (p == 0)).any()
        assert ((np.abs(p) < tiny) & (p != 0)).sum() > 100
        assert (p == np.float32(3e38)).any() and (p == np.float32(-3e38)).any()
        assert np.isfinite(p).all()
        lo, hi = ir.leaf_boxes(p)
        assert ((np.abs(lo) < tiny) & (lo != 0)).any() and ((np.abs(hi) < tiny) & (hi != 0)).any()   # denormal bounds
    s = ir.special_rows(4)
    assert np.signbit(s[0]).all() and s[1, 0] == np.finfo(np.float32).max and s[2, 0] == -s[1, 0] and 0 < s[3, 0] < 1e-44


@functools.lru_cache(maxsize=None)
def _ordered(name):
    dim, make = ir.FLOAT_CLOUDS[name]
    pts = make()
    lo, hi = ir.bbox(pts)
    order = ir.curve_order(pts, lo, hi, ir.curve_bits(dim))
    return pts[order], lo, hi


@pytest.mark.parametrize("name", sorted(ir.FLOAT_CLOUDS))
def test_few_leaves_of_the_float_clouds_are_ambiguous(name):
    """The condition of the per-cell comparison on random float clouds: at most 1 % of the leaves of the curve-ordered
    cloud have the centre of their box within 2^-12 cell of an inner cell boundary (expected 2 dim 2^-12)."""
    rows, lo, hi = _ordered(name)
    share = ir.ambiguous_share(rows, lo, hi)
    print(f"{name}: ambiguous leaves {100 * share:.3f} %")
    assert share <= 0.01
    grid = ir.density_grid(rows, lo, hi)
    assert grid.sum() == rows.shape[0]
    assert ir.check_density_grid(grid, rows, lo, hi) == round(share * ((rows.shape[0] + 15) // 16))


@pytest.mark.parametrize("dim", [2, 3])
def test_integer_clouds_fall_into_exact_cells(dim):
    """Integer coordinates in [0, G]^dim with both extremes on every axis: the float32 evaluation of the cell - scale
    G / (hi - lo), centre 0.5 (lo + hi) - is exact, so the device must give the reference's cell for every leaf."""
    g = ir.grid_cells(dim)
    for n in ir.INTEGER_SIZES:
        p = ir.integer_cloud(n, dim, 100 + dim)
        lo, hi = ir.bbox(p)
        assert (lo == 0).all() and (hi == g).all() and (p == np.rint(p)).all()
        rows = p[ir.curve_order(p, lo, hi, ir.curve_bits(dim))]
        llo, lhi = ir.leaf_boxes(rows)
        scale = np.float32(g) / (hi - lo)
        assert (scale == 1).all()
        centre32 = (np.float32(0.5) * (llo + lhi) - lo) * scale
        assert np.array_equal(centre32.astype(np.float64), 0.5 * (llo.astype(np.float64) + lhi.astype(np.float64)))
        _, cell, _ = ir.leaf_cells(rows, lo, hi)
        assert np.array_equal(cell, np.minimum(centre32.astype(np.int64), g - 1))


def _kind_by_loop(grid, dim):
    g = ir.grid_cells(dim)
    c = g // 4
    fine = np.asarray(grid).reshape((g,) * dim)
    coarse = np.zeros((c,) * dim, dtype=np.int64)
    for idx in np.ndindex(*fine.shape):
        coarse[tuple(i // 4 for i in idx)] += fine[idx]
    inner = 0
    for idx in np.ndindex(*coarse.shape):
        if coarse[idx] == 0:
            continue
        ok = True
        for k in range(dim):
            for s in (-1, 1):
                j = list(idx)
                j[k] += s
                if 0 <= j[k] < c and coarse[tuple(j)] == 0:
                    ok = False
        inner += coarse[idx] if ok else 0
    return int(inner), int(coarse.sum())


@pytest.mark.parametrize("dim", [2, 3])
def test_cloud_kind_words_against_a_plain_loop(dim):
    rng = np.random.default_rng(dim)
    g = ir.grid_cells(dim)
    for fill in (0.02, 0.3, 0.9):
        grid = (rng.random(g ** dim) < fill) * rng.integers(1, 40, g ** dim)
        assert ir.cloud_kind(grid, dim) == _kind_by_loop(grid, dim)
    full = np.ones(g ** dim, dtype=np.int64)
    assert ir.cloud_kind(full, dim) == (g ** dim, g ** dim)       # no neighbour missing at the rims
    one = np.zeros(g ** dim, dtype=np.int64)
    one[0] = 7
    assert ir.cloud_kind(one, dim) == (0, 7)


def test_cloud_kind_tells_the_float_clouds_apart():
    share = {}
    for name in ("gauss3", "torus3", "cheese3"):
        rows, lo, hi = _ordered(name)
        inner, total = ir.cloud_kind(ir.density_grid(rows, lo, hi), 3)
        assert total == rows.shape[0]
        share[name] = inner / total
    assert share["gauss3"] > 0.85 and share["cheese3"] > 0.85 and share["torus3"] < 0.35, share


def test_selection_reference():
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((500, 3)).astype(np.float32)
    pts[10] = pts[11]
    lo, hi = np.full(3, -0.5, np.float32), np.full(3, 0.5, np.float32)
    centers, radii = np.zeros((1, 3), np.float32), np.array([0.4], np.float32)
    inside = ir.inside_box(pts, lo, hi)
    need = ir.check_selection(pts[inside], pts, lo, hi, centers, radii)
    assert 0 < need < inside.sum()
    with pytest.raises(AssertionError):
        ir.check_selection(pts[inside][1:], pts, lo, hi)                  # a row of the box left out
    with pytest.raises(AssertionError):
        ir.check_selection(np.concatenate([pts[inside], pts[inside][:1]]), pts, lo, hi)      # a row twice
    with pytest.raises(AssertionError):
        ir.check_selection(pts, pts, lo, hi)                              # rows outside the box
    with pytest.raises(AssertionError):
        ir.check_selection(pts[inside] + np.float32(1e-3), pts, lo, hi)   # rows that are no rows of the cloud
    z = np.array([[0.0, -0.0, 0.0]], np.float32)
    assert ir.multiset(z) != ir.multiset(np.zeros((1, 3), np.float32))    # bit equality
