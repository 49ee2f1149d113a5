"""Early exit of the witness sweep's pair loops over the ordered stage (csrc/flood_wit.hip, phases 3 and 5), held to
account without tolerance: a float32 numpy replica of the plane table (flood_planes.hpp), of `Region`, `Excess`, the
binning `(int)(excess(x) * bin_scale)` and `Region::limit(slack(p), k / bin_scale)`.

The kernel leaves a pair loop at stage slot j once every sample p of the wave has a running minimum
<= limit(slack(p), k / bin_scale), k the smallest excess bin among the points from j on.  That is exact if and only if
EVERY point x of bin k or higher has an evaluated squared distance to p STRICTLY above that limit - which is what is
asserted here for every (sample, point) pair, on random and on degenerate simplices (slivers with one edge 1e-3 of the
others, coordinates offset by 1e3), with points placed exactly on bin boundaries and on the polytope's faces among the
inputs.  The same check with the kernel's factor 0.999 replaced by 1.001 must FAIL on these inputs: the test bites.
The statement is about the bins k >= 1; bin 0 - the points inside the polytope - carries no bound at all, and the
kernel never leaves a loop on it (last test).

The replica lives in tests/wit_reference.py (fmaf correctly rounded, every other operation a float32 numpy operation in
the kernel's order); tests/test_gpu_plane_rows.py and tests/test_gpu_wit_probe.py show on the GPU that it computes the
plane rows the kernels write and the Region / Excess / bin / limit words the sweep's own code forms."""
import numpy as np
import pytest

from wit_reference import NBIN, Region, f32, pair_d2
from wit_reference import points as _points
from wit_reference import simplices as _simplices


def _violations(dim, factor, bins="outside"):
    """number of (sample, point) pairs whose evaluated d2 is NOT strictly above the limit of the point's bin; over the
    points of the bins k >= 1 (which violate a side of the polytope by at least k / bin_scale), or of bin 0 alone"""
    bad, pairs, boundary = 0, 0, 0
    worst = []
    for si, (name, vs) in enumerate(_simplices(dim)):
        for cmax_frac in (0.6, 0.15):
            rg = Region(vs, cmax_frac)
            x = _points(rg, np.random.default_rng(1000 * dim + si))
            eb = (rg.excess(x) * rg.bin_scale).astype(f32)
            keep = (eb < f32(NBIN)) & ((eb >= f32(1)) if bins == "outside" else (eb < f32(1)))
            x, eb = x[keep], eb[keep]
            k = eb.astype(np.int32)          # (int)eb
            boundary += int((eb == k).sum())
            c = (k.astype(f32) / rg.bin_scale).astype(f32)
            p = rg.samples()
            dl = rg.slack(p)
            lim = Region.limit(dl[:, None], c[None, :], factor)
            d2 = pair_d2(p, x)
            nb = ~(d2 > lim)
            pairs += d2.size
            if nb.any():
                bad += int(nb.sum())
                worst.append((name, cmax_frac, int(nb.sum())))
    return bad, pairs, boundary, worst


@pytest.mark.parametrize("dim", [2, 3])
def test_points_of_a_bin_are_strictly_beyond_its_limit(dim):
    bad, pairs, boundary, worst = _violations(dim, 0.999)
    print(f"dim {dim}: {pairs} pairs, {boundary} points exactly on a bin boundary, {bad} not beyond the limit {worst[:5]}")
    assert pairs > 1_000_000 and boundary > 100
    assert bad == 0, worst[:10]


@pytest.mark.parametrize("dim", [2, 3])
def test_the_check_bites_with_a_factor_above_one(dim):
    bad, pairs, _, worst = _violations(dim, 1.001)
    print(f"dim {dim}: factor 1.001: {bad} of {pairs} pairs not beyond the limit")
    assert bad > 0


@pytest.mark.parametrize("dim", [2, 3])
def test_bin_zero_carries_no_bound(dim):
    """Bin 0 holds the points INSIDE the polytope (and within c_max / 64 of it): they violate no side, and a sample's
    slack says nothing about them - a point may sit on the sample.  The kernel notes c = -inf for a group of stage slots
    that starts in bin 0, which makes the limit overflow, and an overflowed limit never lets a wave leave."""
    bad, pairs, _, _ = _violations(dim, 0.999, bins="zero")
    print(f"dim {dim}: bin 0: {bad} of {pairs} pairs within the limit a bound c = 0 would give")
    assert bad > 0
    with np.errstate(over="ignore", invalid="ignore"):
        lim = Region.limit(np.array([0.0, 0.25, 1e30], f32), f32(-np.inf))
    assert np.isinf(lim).all() and (lim > 0).all()
