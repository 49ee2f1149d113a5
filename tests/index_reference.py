"""Reference of the point index in plain numpy (float64 or integers; no torch, no device): the bounding box, the curve
codes (Skilling's axes-to-transpose transform and the plain bit interleave), the padded rows, the implicit box tree,
the density grid with its cloud-kind words and the sub-cloud selection.  ``test_index_reference_cpu.py`` checks this
module and the inputs on the host, ``test_gpu_index_exact.py`` compares the library with it.

NaN and infinite coordinates are out of scope everywhere here: the library documents no behaviour for them."""

import numpy as np

# (dim, bits per axis) of the full lattices on which the curve codes are checked, on the host and on the device
LATTICES = [(1, 6), (2, 6), (3, 4), (4, 3), (5, 3), (6, 2), (7, 2), (8, 2), (2, 1), (3, 1)]

# n -> levels of the box tree: the sizes at the level boundaries
LEVEL_TABLE = {1: 1, 15: 1, 16: 1, 17: 1, 1023: 1, 1024: 1, 1025: 2, 65_535: 2, 65_536: 2, 65_537: 3, 66_561: 3,
               4_194_305: 4}

LEAF = 16        # points per leaf
FAN = 64         # children per inner node; every level is padded to a multiple of it
MAX_LEVELS = 6
INF = np.float32(np.inf)


def padded_dim(dim):
    return 2 if dim <= 2 else (4 if dim <= 4 else 8)


# ---------------------------------------------------------------------------------------------- bounding box
def bbox(pts):
    """(lo, hi) of the rows, float32, by ``np.min`` / ``np.max``."""
    pts = np.asarray(pts)
    return pts.min(axis=0), pts.max(axis=0)


def box16(lo, hi):
    """The library's 16-float box: [0:dim] minima, [8:8+dim] maxima."""
    out = np.zeros(16, dtype=np.float32)
    out[:len(lo)] = lo
    out[8:8 + len(hi)] = hi
    return out


# ---------------------------------------------------------------------------------------------- curve codes
def curve_bits(dim, option=0):
    """Bits per axis of the codes: option ``curve_bits`` (0: 8 in three dimensions, 12 elsewhere), one axis keeps its
    cap; never more than floor(63 / dim) and 21."""
    cap = min(63 // dim, 21)
    b = option if option > 0 else (8 if dim == 3 else 12)
    if dim == 1:
        b = cap
    return min(b, cap)


def quantise(pts, lo, hi, bits):
    """Cells of the points on the 2^bits lattice over the box, in float32 and in the order of operations of the
    library: scale = (2^bits - 1) / (hi - lo) (0 on an axis of no extent), t = (p - lo) * scale clamped to
    [0, 2^bits - 1], truncated.  Every step is one correctly rounded float32 operation in numpy as on the device."""
    pts = np.asarray(pts, dtype=np.float32)
    lo = np.asarray(lo, dtype=np.float32)
    hi = np.asarray(hi, dtype=np.float32)
    top = np.float32((1 << bits) - 1)
    ext = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(ext > 0, top / ext, np.float32(0)).astype(np.float32)
    t = (pts - lo[None, :]) * scale[None, :]
    assert t.dtype == np.float32
    t = np.where(t < 0, np.float32(0), t)
    t = np.where(t > top, top, t)
    return t.astype(np.uint64)


def hilbert_transpose(cells, bits):
    """Skilling's AxestoTranspose (AIP Conf. Proc. 707, 2004) on every row of ``cells`` (n, dim) unsigned integers
    below 2^bits: returns the transposed Hilbert index, one word per axis."""
    x = np.array(cells, dtype=np.uint64)
    n_axes = x.shape[1]
    one = np.uint64(1)
    q = one << np.uint64(bits - 1)
    m = q
    while q > one:                          # inverse undo
        p = q - one
        for i in range(n_axes):
            hit = (x[:, i] & q) != 0
            x[hit, 0] ^= p                                   # invert
            t = (x[:, 0] ^ x[:, i]) & p                      # exchange
            t[hit] = 0
            x[:, 0] ^= t
            x[:, i] ^= t
        q >>= one
    for i in range(1, n_axes):              # Gray encode
        x[:, i] ^= x[:, i - 1]
    t = np.zeros(x.shape[0], dtype=np.uint64)
    q = m
    while q > one:
        hit = (x[:, n_axes - 1] & q) != 0
        t[hit] ^= q - one
        q >>= one
    x ^= t[:, None]
    return x


def hilbert_codes(cells, bits):
    """Hilbert index of every lattice cell: the transposed form read bit plane by bit plane from the top, axis 0
    first (most significant).  One axis: the cell itself."""
    cells = np.asarray(cells, dtype=np.uint64)
    n_axes = cells.shape[1]
    if n_axes == 1:
        return cells[:, 0].copy()
    x = hilbert_transpose(cells, bits)
    code = np.zeros(cells.shape[0], dtype=np.uint64)
    for b in range(bits - 1, -1, -1):
        for k in range(n_axes):
            code = (code << np.uint64(1)) | ((x[:, k] >> np.uint64(b)) & np.uint64(1))
    return code


def morton_codes(cells, bits):
    """Plain bit interleave: bit b of axis k is bit b * dim + k of the code."""
    cells = np.asarray(cells, dtype=np.uint64)
    n_axes = cells.shape[1]
    code = np.zeros(cells.shape[0], dtype=np.uint64)
    for b in range(bits):
        for k in range(n_axes):
            code |= ((cells[:, k] >> np.uint64(b)) & np.uint64(1)) << np.uint64(b * n_axes + k)
    return code


def curve_codes(cells, bits, curve=1):
    return hilbert_codes(cells, bits) if curve == 1 else morton_codes(cells, bits)


def point_codes(pts, lo, hi, bits, curve=1):
    return curve_codes(quantise(pts, lo, hi, bits), bits, curve)


def curve_order(pts, lo, hi, bits, curve=1):
    """Stable argsort of the codes: equal codes stay in ascending original index."""
    return np.argsort(point_codes(pts, lo, hi, bits, curve), kind="stable")


def full_lattice(dim, bits):
    """All (2^bits)^dim integer points, axis 0 fastest."""
    side = 1 << bits
    idx = np.arange(side ** dim, dtype=np.uint64)
    return np.stack([(idx // np.uint64(side ** k)) % np.uint64(side) for k in range(dim)], axis=1)


# ---------------------------------------------------------------------------------------------- rows and the box tree
def make_levels(n):
    """[(offset, count)] of the levels, leaves first, and the total node count: 16 points per leaf, fan-out 64, every
    level padded to a multiple of 64; the top level has at most 64 nodes."""
    c = max((n + LEAF - 1) // LEAF, 1)
    levels, off = [], 0
    while True:
        levels.append((off, c))
        off += (c + FAN - 1) // FAN * FAN
        if c <= FAN or len(levels) == MAX_LEVELS:
            break
        c = (c + FAN - 1) // FAN
    return levels, off


def padded_rows(pts, order):
    """Rows ``pts[order]`` in the padded layout: pad columns 0.0, then +inf rows up to a multiple of 16."""
    pts = np.asarray(pts, dtype=np.float32)
    n, dim = pts.shape
    dp = padded_dim(dim)
    n_pad = (n + LEAF - 1) // LEAF * LEAF
    out = np.full((n_pad, dp), INF, dtype=np.float32)
    out[:n] = 0.0
    out[:n, :dim] = pts[np.asarray(order, dtype=np.int64)]
    return out


def _group_boxes(lo, hi, group, n_out):
    """Boxes of consecutive groups of ``group`` boxes; missing members count as empty (+inf, -inf)."""
    n, dim = lo.shape
    full = n_out * group
    a = np.full((full, dim), INF, dtype=np.float32)
    b = np.full((full, dim), -INF, dtype=np.float32)
    a[:n] = lo
    b[:n] = hi
    return a.reshape(n_out, group, dim).min(axis=1), b.reshape(n_out, group, dim).max(axis=1)


def tree_nodes(rows):
    """The whole node array of the tree over the real rows (n, dim) in their order: (total, 2 * DP) float32, lo then
    hi; empty nodes and pad lanes k >= dim are (+inf, -inf)."""
    rows = np.asarray(rows, dtype=np.float32)
    n, dim = rows.shape
    dp = padded_dim(dim)
    levels, total = make_levels(n)
    nodes = np.empty((total, 2 * dp), dtype=np.float32)
    nodes[:, :dp] = INF
    nodes[:, dp:] = -INF
    lo, hi = _group_boxes(rows, rows, LEAF, levels[0][1])
    for l, (off, count) in enumerate(levels):
        if l > 0:
            lo, hi = _group_boxes(lo, hi, FAN, count)
        assert lo.shape[0] == count
        nodes[off:off + count, :dim] = lo
        nodes[off:off + count, dp:dp + dim] = hi
    return nodes


def leaf_boxes(rows):
    rows = np.asarray(rows, dtype=np.float32)
    return _group_boxes(rows, rows, LEAF, (rows.shape[0] + LEAF - 1) // LEAF)


# ---------------------------------------------------------------------------------------------- density grid
def grid_cells(dim):
    return 256 if dim == 2 else 64


AMBIGUOUS = 2.0 ** -12   # cell units: about four float32 roundings at 2 G = 512


def leaf_cells(rows, lo, hi):
    """Per leaf of the rows: its real row count, the cell under the centre of its box per axis (float64 arithmetic on
    the float32 boxes, G cells per axis over the box (lo, hi), clamped at the rims) and, per axis, whether the centre
    lies within ``AMBIGUOUS`` of an inner cell boundary (+1 / -1: the neighbouring cell it may round into, 0: none)."""
    rows = np.asarray(rows, dtype=np.float32)
    n, dim = rows.shape
    g = grid_cells(dim)
    llo, lhi = leaf_boxes(rows)
    counts = np.minimum(LEAF, n - LEAF * np.arange(llo.shape[0], dtype=np.int64))
    lo64, hi64 = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    ext = hi64 - lo64
    scale = np.where(ext > 0, g / np.where(ext > 0, ext, 1.0), 0.0)
    pos = (0.5 * (llo.astype(np.float64) + lhi.astype(np.float64)) - lo64[None, :]) * scale[None, :]
    cell = np.clip(np.floor(pos), 0, g - 1).astype(np.int64)
    near = np.rint(pos)
    close = (np.abs(pos - near) <= AMBIGUOUS) & (near >= 1) & (near <= g - 1)
    other = np.where(close, np.where(cell >= near, -1, 1), 0).astype(np.int64)
    return counts, cell, other


def flat_cell(cell, dim):
    g = grid_cells(dim)
    flat = np.zeros(cell.shape[0], dtype=np.int64)
    for k in range(dim - 1, -1, -1):
        flat = flat * g + cell[:, k]
    return flat


def density_grid(rows, lo, hi, only=None):
    """G^dim counts: every leaf adds its real row count to the cell under the centre of its box (axis 0 fastest)."""
    dim = np.asarray(rows).shape[1]
    counts, cell, _ = leaf_cells(rows, lo, hi)
    flat = flat_cell(cell, dim)
    if only is not None:
        counts, flat = counts[only], flat[only]
    return np.bincount(flat, weights=counts, minlength=grid_cells(dim) ** dim).astype(np.int64)


def ambiguous_share(rows, lo, hi):
    _, _, other = leaf_cells(rows, lo, hi)
    return float((other != 0).any(axis=1).mean())


def check_density_grid(got, rows, lo, hi):
    """``got`` against the reference where a leaf is unambiguous, and either of its candidate cells where it is not.
    Returns the number of ambiguous leaves.

    An ambiguous leaf whose candidate cells no other ambiguous leaf shares is checked on its own: its count must sit
    in those cells.  Ambiguous leaves that share a candidate cell get the aggregate checks only - no cell below its
    unambiguous count, nothing outside the union of the candidate cells, the right total - which is the weaker
    guarantee; with about 0.1 % of the leaves ambiguous such sharing is rare."""
    rows = np.asarray(rows)
    n, dim = rows.shape
    g = grid_cells(dim)
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == (g ** dim,)
    assert got.sum() == n, (int(got.sum()), n)
    counts, cell, other = leaf_cells(rows, lo, hi)
    amb = (other != 0).any(axis=1)
    base = np.bincount(flat_cell(cell[~amb], dim), weights=counts[~amb], minlength=g ** dim).astype(np.int64)
    rest = got - base
    assert (rest >= 0).all(), "a cell holds fewer points than its unambiguous leaves"
    cand = []                                    # candidate cells of every ambiguous leaf
    for i in np.nonzero(amb)[0]:
        cells = [cell[i].copy()]
        for k in range(dim):
            if other[i, k] != 0:
                moved = [c.copy() for c in cells]
                for c in moved:
                    c[k] += other[i, k]
                cells += moved
        cand.append((int(counts[i]), set(int(f) for f in flat_cell(np.array(cells), dim))))
    allowed = set().union(*[c for _, c in cand]) if cand else set()
    assert set(int(f) for f in np.nonzero(rest)[0]) <= allowed, "points in a cell no leaf can reach"
    assert rest.sum() == sum(c for c, _ in cand)
    for j, (c, cells) in enumerate(cand):
        if all(j == i or not (cells & o) for i, (_, o) in enumerate(cand)):
            assert sum(int(rest[f]) for f in cells) == c, "an ambiguous leaf is in neither of its cells"
    return int(amb.sum())


def cloud_kind(grid, dim):
    """Words [2] and [3] behind the grid: pool 4 fine cells per axis; a coarse cell is interior when it is occupied and
    all its axis neighbours inside the grid are occupied; (points in interior cells, all points)."""
    g = grid_cells(dim)
    c = g // 4
    fine = np.asarray(grid, dtype=np.int64).reshape((g,) * dim)
    coarse = fine.reshape(sum(((c, 4) for _ in range(dim)), ())).sum(axis=tuple(range(1, 2 * dim, 2)))
    occ = coarse > 0
    interior = occ.copy()
    for k in range(dim):
        for shift in (1, -1):
            nb = np.roll(occ, shift, axis=k)
            rim = [slice(None)] * dim
            rim[k] = 0 if shift == 1 else c - 1
            nb[tuple(rim)] = True                 # no neighbour inside the grid: no condition
            interior &= nb
    return int(coarse[interior].sum()), int(coarse.sum())


# ---------------------------------------------------------------------------------------------- sub-cloud selection
def row_keys(rows):
    """One opaque key per row: its bytes (bit equality; -0.0 and 0.0 differ)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).reshape(-1)


def multiset(rows):
    keys, counts = np.unique(row_keys(rows), return_counts=True)
    return dict(zip((k.tobytes() for k in keys), (int(c) for c in counts)))


def inside_box(pts, lo, hi):
    pts = np.asarray(pts, dtype=np.float32)
    return ((pts >= np.asarray(lo, np.float32)[None]) & (pts <= np.asarray(hi, np.float32)[None])).all(axis=1)


def inside_balls(pts, centers, radii, margin=1e-6, chunk=1 << 16):
    """Rows within radius * (1 - margin) of some centre, float64."""
    p = np.asarray(pts, dtype=np.float64)
    c = np.asarray(centers, dtype=np.float64)
    r = np.asarray(radii, dtype=np.float64) * (1.0 - margin)
    out = np.zeros(p.shape[0], dtype=bool)
    for a in range(0, p.shape[0], chunk):
        d2 = ((p[a:a + chunk, None, :] - c[None, :, :]) ** 2).sum(axis=2)
        out[a:a + chunk] = (d2 <= (r * r)[None, :]).any(axis=1)
    return out


def check_selection(selected, pts, lo, hi, centers=None, radii=None):
    """The properties of a selected sub-cloud; returns the number of rows the reference demands."""
    pts = np.asarray(pts, dtype=np.float32)
    selected = np.asarray(selected, dtype=np.float32)
    assert not np.isnan(selected).any()
    have, cloud = multiset(selected), multiset(pts)
    for key, c in have.items():
        assert key in cloud, "a selected row is no row of the cloud"
        assert c <= cloud[key], "a row was emitted more often than the cloud holds it"
    if selected.shape[0]:
        assert inside_box(selected, lo, hi).all(), "a selected row lies outside the box"
    must = inside_box(pts, lo, hi)
    if centers is not None:
        must &= inside_balls(pts, centers, radii)
    for key, c in multiset(pts[must]).items() if must.any() else ():
        assert have.get(key, 0) >= c, "a row inside the box and a ball was left out"
    return int(must.sum())


# ---------------------------------------------------------------------------------------------- inputs
def special_rows(dim):
    """Rows holding -0.0, the largest finite float32 of both signs and denormals."""
    big = np.finfo(np.float32).max
    tiny = np.float32(1e-45)                    # the smallest denormal
    rows = np.zeros((6, dim), dtype=np.float32)
    rows[0, :] = -0.0
    rows[1, :] = big
    rows[2, :] = -big
    rows[3, :] = tiny
    rows[4, :] = -tiny
    rows[5, :] = np.float32(-1e-40)
    return rows


def gaussian(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def special_cloud(n, dim, seed):
    """Small values around zero with -0.0, denormals of both signs and +-3e38 among them: a box bound that is flushed
    to zero no longer contains its row."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n, dim)) * 1e-38).astype(np.float32)      # many denormals (below 1.18e-38)
    p[rng.integers(0, n, n // 7), rng.integers(0, dim, n // 7)] = -0.0
    p[rng.integers(0, n, n // 9)] = 0.0
    p[n // 2, :] = np.float32(3e38)
    p[n // 3, :] = np.float32(-3e38)
    p[n - 1, 0] = np.float32(1e-45)
    p[0, dim - 1] = np.float32(-1e-45)
    return p


def torus(n, seed, R=2.0, r=0.7, noise=0.03):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)
    return (p + noise * rng.standard_normal((n, 3))).astype(np.float32)


def swiss_cheese(n, seed, dim=3, holes=6):
    """Uniform in the unit cube with ``holes`` balls cut out."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0.2, 0.8, (holes, dim))
    radii = rng.uniform(0.1, 0.2, holes)
    out = np.empty((0, dim))
    while out.shape[0] < n:
        p = rng.uniform(0, 1, (n, dim))
        keep = (((p[:, None, :] - centers[None]) ** 2).sum(axis=2) > (radii ** 2)[None]).all(axis=1)
        out = np.concatenate([out, p[keep]])
    return out[:n].astype(np.float32)


def annulus(n, seed):
    rng = np.random.default_rng(seed)
    a, rad = rng.uniform(0, 2 * np.pi, n), np.sqrt(rng.uniform(0.25, 1.0, n))
    return np.stack([rad * np.cos(a), rad * np.sin(a)], axis=1).astype(np.float32)


def integer_cloud(n, dim, seed):
    """Integer coordinates in [0, G]^dim with both extremes present on every axis: the grid's scale is exactly 1 and
    the centre of every leaf box a half-integer."""
    g = grid_cells(dim)
    p = np.random.default_rng(seed).integers(0, g + 1, (n, dim)).astype(np.float32)
    p[0, :] = 0.0
    if n > 1:
        p[n - 1, :] = float(g)
    return p


# the random float clouds of the density and cloud-kind tests: name -> (dim, maker)
FLOAT_CLOUDS = {
    "gauss3": (3, lambda: gaussian(300_000, 3, 11)),
    "torus3": (3, lambda: torus(300_000, 12)),
    "cheese3": (3, lambda: swiss_cheese(300_000, 13)),
    "gauss2": (2, lambda: gaussian(300_000, 2, 14)),
    "annulus2": (2, lambda: annulus(300_000, 15)),
}
INTEGER_SIZES = (1025, 65_537, 300_000)
