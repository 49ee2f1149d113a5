"""The leaf cull of the cell sweep (csrc/flood_planes.hpp: node_meets_slabs; called from csrc/flood_cell.hip on the
leaves a gather has collected), held to account WITHOUT tolerance: with the float32 replicas of
tests/gather_planes_reference.py - the node test and the fma chain of keep_point, both in the kernel's order - no box
that the node test rejects contains a point that keep_point keeps.

Simplices: the random, sliver, flat, axis-parallel and dyadic ones of wit_reference.simplices in 2-D and 3-D and their
copies offset by 1e3; scaled by 2^-20 and 2^20; planes disabled by scale (a needle whose faces fail the row's `ok`
test, a face of lower dimension: every plane off); repeated vertices.  Regions: the whole lattice of a simplex and a
patch of it, cell sizes from 2 % of the extent to the extent.

Boxes and probe points:
  random boxes   centres in and around the region, half sizes over four decades, some of them degenerate (lo = hi on
                 an axis); probed at their corners, edge and face midpoints and at random points inside;
  pinned boxes   a point x0 and a plane f; the slab limit of f is SET to keep_point's own dd_f(x0) - x0 lies exactly on
                 the limit and is kept - and the box has x0 as the corner nearest to the slab and extends away from it.
                 The node test must keep every such box.  With the pad set to 0, or its sign flipped, it rejects some
                 of them: the pad is needed, and the test bites.

The witness sweep's gather has no such cull (it was left out of the change that brought this one), so there is no
witness variant to check here."""
import itertools

import numpy as np
import pytest

from gather_planes_reference import PAD_ABS, PAD_REL, Region, keeps, lattice, node_meets_slabs, plane_dd, samples
from wit_reference import f32
from wit_reference import simplices as _simplices

N_RANDOM_BOXES = 1500
N_INSIDE = 38          # random points per box, beside the 3^dim structured ones
N_PINNED = 3000


def _cases(dim):
    rng = np.random.default_rng(40 + dim)
    out = list(_simplices(dim))
    base = [v for name, v in out if name in ("random 0", "sliver 0", "flat", "unit, dyadic")]
    for v in base:
        out.append(("scaled 2^-20", (v * f32(2.0 ** -20)).astype(f32)))
        out.append(("scaled 2^20", (v * f32(2.0 ** 20)).astype(f32)))
    needle = rng.standard_normal((dim + 1, dim)).astype(f32)        # all vertices within 1e-6 of one line: faces fail `ok`
    needle[1:] = needle[0] + np.linspace(0.2, 1.0, dim)[:, None].astype(f32) * (needle[1] - needle[0]) \
        + f32(1e-6) * rng.standard_normal((dim, dim)).astype(f32)
    out.append(("needle (planes off by scale)", needle.astype(f32)))
    out.append(("lower-dimensional face (every plane off)", rng.standard_normal((dim, dim)).astype(f32)))
    rep = rng.standard_normal((dim + 1, dim)).astype(f32)
    rep[dim] = rep[0]
    out.append(("repeated vertex", rep))
    out.append(("all vertices equal", np.repeat(rng.standard_normal((1, dim)).astype(f32), dim + 1, 0)))
    return out


def _regions(vs):
    w = lattice(vs.shape[0], 6)
    p = samples(vs, w)
    ext = max(float((p.max(0) - p.min(0)).max()), float(np.abs(vs).max()) * 1e-6, 1e-30)
    patch = p[np.argsort(((p - p[0]) ** 2).sum(1), kind="stable")[: max(2, len(p) // 4)]]
    for pts, frac in ((p, 0.02), (p, 0.3), (patch, 0.1), (patch, 1.0)):
        yield Region(vs, pts, f32(frac * ext)), ext


def _probes(lo, hi, rng):
    """(n, m, dim) float32 points inside the boxes: 3^dim lattice of corners / edge, face and body midpoints + random"""
    n, dim = lo.shape
    mid = np.clip((f32(0.5) * lo + f32(0.5) * hi).astype(f32), lo, hi)
    tri = np.stack([lo, mid, hi], 0)                                    # (3, n, dim)
    pts = [np.stack([tri[c[k], :, k] for k in range(dim)], -1) for c in itertools.product(range(3), repeat=dim)]
    t = rng.random((N_INSIDE, n, dim)).astype(f32)
    inside = np.clip((lo[None] + t * (hi - lo)[None]).astype(f32), lo[None], hi[None])
    return np.concatenate([np.stack(pts, 0), inside], 0).transpose(1, 0, 2)


def _random_boxes(rg, ext, rng, n):
    dim = rg.dim
    grow = f32(2.5) * rg.c + f32(0.3 * ext)
    ctr = rng.uniform(rg.blo - grow, rg.bhi + grow, (n, dim)).astype(f32)
    half = (f32(ext) * (10.0 ** rng.uniform(-4, 0, (n, dim))).astype(f32)).astype(f32)
    half[rng.random((n, dim)) < 0.05] = 0                               # degenerate on an axis
    lo, hi = (ctr - half).astype(f32), (ctr + half).astype(f32)
    return lo, hi


def _pinned_boxes(rg, ext, rng, n):
    """boxes with a corner x0 exactly on a slab limit, and that limit: returns lo, hi, slab_lo, slab_hi (one row per box)"""
    dim = rg.dim
    grow = rg.c + f32(0.1 * ext)
    x0 = rng.uniform(rg.blo - grow, rg.bhi + grow, (n, dim)).astype(f32)
    dd = rg.dd(x0)
    with np.errstate(invalid="ignore"):
        slab_lo = np.fmin(np.broadcast_to(rg.slab_lo, dd.shape), dd).astype(f32)   # x0 passes every other plane
        slab_hi = np.fmax(np.broadcast_to(rg.slab_hi, dd.shape), dd).astype(f32)
    f = rng.integers(0, dim + 1, n)
    upper = rng.random(n) < 0.5
    rows = np.arange(n)
    slab_hi[rows[upper], f[upper]] = dd[rows[upper], f[upper]]
    slab_lo[rows[~upper], f[~upper]] = dd[rows[~upper], f[~upper]]
    e = (f32(ext) * (10.0 ** rng.uniform(-4, 0, (n, dim))).astype(f32)).astype(f32)
    # upper limit: the box's minimum along pn[f] is at x0 - the box goes towards +pn; lower limit: towards -pn
    towards = np.where(upper[:, None], rg.pn[f] >= 0, rg.pn[f] < 0)
    lo = np.where(towards, x0, (x0 - e).astype(f32)).astype(f32)
    hi = np.where(towards, (x0 + e).astype(f32), x0).astype(f32)
    return x0, lo, hi, slab_lo, slab_hi


def _sweep(dim, pad_rel=PAD_REL, pad_abs=PAD_ABS, random_boxes=True):
    """-> pairs probed, random boxes rejected, kept points inside rejected random boxes, pinned boxes, pinned boxes rejected"""
    pairs = rejected = bad = pinned = pinned_rejected = 0
    for ci, (name, vs) in enumerate(_cases(dim)):
        for ri, (rg, ext) in enumerate(_regions(vs)):
            rng = np.random.default_rng(10_000 * dim + 10 * ci + ri)
            lo, hi = _random_boxes(rg, ext, rng, N_RANDOM_BOXES if random_boxes else 1)
            meets = node_meets_slabs(lo, hi, rg.pn, rg.po, rg.org, rg.slab_lo, rg.slab_hi, pad_rel, pad_abs)
            pairs += lo.shape[0] * (3 ** dim + N_INSIDE)
            rej = ~meets
            rejected += int(rej.sum())
            if rej.any():   # (a box the test keeps cannot violate anything: only the rejected ones are probed)
                x = _probes(lo[rej], hi[rej], rng).reshape(-1, dim)
                bad += int(keeps(rg.dd(x), rg.slab_lo, rg.slab_hi).sum())
            x0, lo, hi, slo, shi = _pinned_boxes(rg, ext, rng, N_PINNED)
            assert keeps(rg.dd(x0), slo, shi).all(), name                 # x0 is a kept point of its box
            assert ((x0 >= lo) & (x0 <= hi)).all(), name
            meets = node_meets_slabs(lo, hi, rg.pn, rg.po, rg.org, slo, shi, pad_rel, pad_abs)
            pinned += lo.shape[0]
            pinned_rejected += int((~meets).sum())
    return pairs, rejected, bad, pinned, pinned_rejected


@pytest.fixture(scope="module")
def swept():
    return {dim: _sweep(dim) for dim in (2, 3)}


@pytest.mark.parametrize("dim", [2, 3])
def test_no_rejected_box_holds_a_kept_point(swept, dim):
    pairs, rejected, bad, pinned, pinned_rejected = swept[dim]
    print(f"dim {dim}: {pairs} box-point pairs, {rejected} random boxes rejected, {pinned} pinned boxes")
    assert rejected > 10_000                      # the test does cull on these inputs
    assert bad == 0 and pinned_rejected == 0


def test_on_the_order_of_ten_million_pairs(swept):
    assert swept[2][0] + swept[3][0] >= 10_000_000


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("pad", ["zero", "flipped"])
def test_without_the_pad_or_with_its_sign_flipped_the_check_fails(dim, pad):
    rel, ab = (f32(0), f32(0)) if pad == "zero" else (-PAD_REL, -PAD_ABS)
    _, _, _, pinned, pinned_rejected = _sweep(dim, rel, ab, random_boxes=False)
    print(f"dim {dim}, pad {pad}: {pinned_rejected} of {pinned} pinned boxes rejected")
    assert pinned_rejected > 0


def test_what_is_not_a_number_keeps_the_node():
    vs = _simplices(3)[0][1]
    rg = next(_regions(vs))[0]
    lo = np.array([[0.1, 0.2, 0.3]], f32)
    hi = lo + f32(0.5)
    far = (lo + f32(1e6), hi + f32(1e6))
    assert not node_meets_slabs(*far, rg.pn, rg.po, rg.org, rg.slab_lo, rg.slab_hi)[0]          # (a box it does reject)
    nan4 = np.full(4, np.nan, f32)
    assert node_meets_slabs(*far, rg.pn, rg.po, rg.org, nan4, nan4)[0]                         # NaN slab limits
    assert node_meets_slabs(*far, rg.pn, np.full(4, np.nan, f32), rg.org, rg.slab_lo, rg.slab_hi)[0]   # NaN offsets
    assert node_meets_slabs(*far, np.full((4, 3), np.nan, f32), rg.po, rg.org, rg.slab_lo, rg.slab_hi)[0]
    empty = (np.full((1, 3), np.inf, f32), np.full((1, 3), -np.inf, f32))                      # pad row of the tree
    assert node_meets_slabs(*empty, rg.pn, rg.po, rg.org, rg.slab_lo, rg.slab_hi)[0]
    inf_row = (np.full((1, 3), np.inf, f32), np.full((1, 3), np.inf, f32))                     # +inf pad row
    assert node_meets_slabs(*inf_row, rg.pn, rg.po, rg.org, rg.slab_lo, rg.slab_hi)[0]
    # a plane row switched off (pn = 0, po = 3e38) rejects nothing that keep_point keeps: every point has dd = -po
    off = Region(vs[:3], samples(vs[:3], lattice(3, 4)), f32(0.1))
    assert (off.po > f32(1e37)).all() and (off.pn == 0).all()
    assert node_meets_slabs(lo, hi, off.pn, off.po, off.org, off.slab_lo, off.slab_hi)[0]
    assert keeps(plane_dd(lo, off.pn, off.po, off.org), off.slab_lo, off.slab_hi)[0]
