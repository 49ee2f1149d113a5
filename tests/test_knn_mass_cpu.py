"""``distance_to_weighted_measure`` and ``voxel_measure`` on CPU tensors, the refusals and the wiring of
``flooder_knn_mass_f32`` (no GPU): the rule against ``distance_to_measure`` at unit masses, hand cases for the ">="
crossing, zero masses and a heavy site, the not-reached rule, the coreset against a numpy reference, and the stability
bound of the distance to a measure on a torus coreset."""

import os
import re

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, build, core

import knn_mass_reference as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 1e-6)])
@pytest.mark.parametrize("stat", ["dtm", "kth"])
def test_unit_masses_are_distance_to_measure(dtype, tol, stat):
    torch.manual_seed(3)
    pts = torch.rand(700, 3, dtype=dtype)
    qs = torch.rand(90, 3, dtype=dtype)
    ones = torch.ones(700, dtype=dtype)
    for k in (1, 7, 49, 64, 65, 300):
        want, w_ids, w_dist = fa.distance_to_measure(pts, qs, neighbors=k, neighbor_stat=stat, return_neighbors=True)
        got, ids, dist, count = fa.distance_to_weighted_measure(pts, ones, qs, mass=k / 700, neighbor_stat=stat,
                                                                return_neighbors=True)
        assert got.dtype == dtype and ids.dtype == torch.int64 and count.dtype == torch.int64 and dist.dtype == dtype
        assert ids.shape == dist.shape == (90, 1024) and count.shape == (90,)
        assert bool((count == k).all()), k
        assert torch.equal(ids[:, :k], w_ids) and bool((ids[:, k:] == -1).all()) and bool(torch.isinf(dist[:, k:]).all())
        assert float(((got - want).abs() / want.clamp_min(1e-30)).max()) <= tol, (k, stat)
        assert float((dist[:, :k] - w_dist).abs().max()) <= tol
        plain = fa.distance_to_weighted_measure(pts, ones, qs, mass=k / 700, neighbor_stat=stat)
        assert torch.equal(plain, got)


def test_hand_cases():
    # sites on a line, the query at 0: distances 1, 2, 3, 4
    pts = torch.tensor([[1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [4.0, 0.0]], dtype=torch.float64)
    q = torch.zeros(1, 2, dtype=torch.float64)

    def run(mu, mass, stat="dtm", **kw):
        return fa.distance_to_weighted_measure(pts, torch.tensor(mu, dtype=torch.float64), q, mass=mass,
                                               neighbor_stat=stat, return_neighbors=True, **kw)

    # one site holds more than tau: count 1, the value is its distance (both statistics)
    for stat in ("dtm", "kth"):
        v, ids, dist, count = run([6.0, 1.0, 1.0, 2.0], 0.5, stat)           # tau = 5 < 6
        assert count.tolist() == [1] and ids[0, :2].tolist() == [0, -1] and float(v) == 1.0
    # tau EQUALS a prefix sum: the crossing is AT that position (">=")
    v, ids, dist, count = run([2.0, 3.0, 1.0, 4.0], 0.5)                      # tau = 5 = 2 + 3
    assert count.tolist() == [2] and float(v) == pytest.approx(np.sqrt((2 * 1 + 3 * 4) / 5), abs=1e-14)
    assert float(run([2.0, 3.0, 1.0, 4.0], 0.5, "kth")[0]) == 2.0
    # ... and just above it the next site enters with the residual weight
    v, ids, dist, count = run([2.0, 3.0, 1.0, 4.0], 0.55)                     # tau = 5.5
    assert count.tolist() == [3] and float(v) == pytest.approx(np.sqrt((2 * 1 + 3 * 4 + 0.5 * 9) / 5.5), abs=1e-14)
    # zero-mass sites before the crossing: listed, counted, and they add nothing
    v, ids, dist, count = run([0.0, 0.0, 3.0, 3.0], 0.5)                      # tau = 3: crosses at the third site
    assert count.tolist() == [3] and ids[0, :4].tolist() == [0, 1, 2, -1] and float(v) == 3.0
    assert dist[0, :3].tolist() == [1.0, 2.0, 3.0] and bool(torch.isinf(dist[0, 3:]).all())
    assert float(run([0.0, 0.0, 3.0, 3.0], 0.75)[0]) == pytest.approx(np.sqrt((3 * 9 + 1.5 * 16) / 4.5), abs=1e-14)
    # squared
    v2 = run([2.0, 3.0, 1.0, 4.0], 0.55, squared=True)
    assert float(v2[0]) == pytest.approx((2 * 1 + 3 * 4 + 0.5 * 9) / 5.5, abs=1e-14) and v2[2][0, :3].tolist() == [1.0, 4.0, 9.0]
    # queries=None: the sites themselves; every site is its own nearest neighbour
    mu = torch.tensor([6.0, 1.0, 1.0, 2.0], dtype=torch.float64)
    own = fa.distance_to_weighted_measure(pts, mu, mass=0.1, neighbor_stat="kth")      # tau = 1
    assert own.tolist() == [0.0, 0.0, 0.0, 0.0]
    own, ids, _, count = fa.distance_to_weighted_measure(pts, mu, mass=0.2, neighbor_stat="kth", return_neighbors=True)
    assert own.tolist() == [0.0, 1.0, 1.0, 0.0] and count.tolist() == [1, 2, 2, 1]      # tau = 2: the unit sites need a second
    assert ids[:, 0].tolist() == [0, 1, 2, 3]
    # no queries
    e = fa.distance_to_weighted_measure(pts, mu, pts[:0], mass=0.5, return_neighbors=True)
    assert [tuple(t.shape) for t in e] == [(0,), (0, 1024), (0, 1024), (0,)]
    assert fa.distance_to_weighted_measure(pts, mu, pts[:0], mass=0.5).shape == (0,)


def test_not_reached():
    torch.manual_seed(5)
    pts = torch.rand(200, 2, dtype=torch.float64)
    qs = torch.rand(17, 2, dtype=torch.float64)
    ones = torch.ones(200, dtype=torch.float64)
    for stat in ("dtm", "kth"):
        v, ids, dist, count = fa.distance_to_weighted_measure(pts, ones, qs, mass=65 / 200, neighbor_stat=stat,
                                                              max_neighbors=64, return_neighbors=True)
        assert ids.shape == (17, 64)
        assert bool(torch.isinf(v).all()) and bool((v > 0).all()) and bool((count == 64).all())
        assert bool((ids[:, 63] >= 0).all()) and bool(torch.isfinite(dist).all())
        assert torch.equal(ids, fa.distance_to_measure(pts, qs, neighbors=64, return_neighbors=True)[1])
    # one more neighbour allowed (65 rounds up to 128): reached
    v, ids, _, count = fa.distance_to_weighted_measure(pts, ones, qs, mass=65 / 200, max_neighbors=65,
                                                       return_neighbors=True)
    assert ids.shape == (17, 128) and bool(torch.isfinite(v).all()) and bool((count == 65).all())
    # fewer sites than the capacity: the whole cloud is looked at
    v, ids, _, count = fa.distance_to_weighted_measure(pts[:10], ones[:10], qs, mass=1.0, return_neighbors=True)
    assert bool((count == 10).all()) and bool((ids[:, 10:] == -1).all()) and bool(torch.isfinite(v).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_voxel_measure(dtype):
    pts = fa.generate_noisy_torus_points_3d(6000, seed=2).to(dtype)
    cell = 0.25
    sites, mu = fa.voxel_measure(pts, cell)
    assert sites.dtype == dtype and mu.dtype == dtype and sites.shape == (mu.shape[0], 3)
    assert float(mu.sum()) == 6000 and bool((mu >= 1).all())
    again = fa.voxel_measure(pts, cell)
    assert torch.equal(again[0], sites) and torch.equal(again[1], mu)
    r_sites, r_counts, r_cells = km.voxel_measure(pts.numpy(), cell)
    assert np.array_equal(mu.numpy().astype(np.int64), r_counts)
    ulp = np.spacing(np.abs(r_sites).astype(np.float32)).astype(np.float64)     # one float32 ulp of the coordinate
    assert np.all(np.abs(sites.numpy().astype(np.float64) - r_sites) <= ulp)
    # rows ascend by cell, axis 0 most significant, and every site lies in its cell (up to its rounding to the dtype)
    order = np.lexsort(r_cells.T[::-1])
    assert np.array_equal(order, np.arange(len(r_cells)))
    lo = pts.numpy().astype(np.float64).min(axis=0)
    rel = (sites.numpy().astype(np.float64) - lo) / cell
    assert np.all(rel >= r_cells - 1e-5) and np.all(rel <= r_cells + 1 + 1e-5)
    # a cell larger than the extent: one site, the mean
    one, m1 = fa.voxel_measure(pts, 100.0)
    assert one.shape == (1, 3) and m1.tolist() == [6000.0]
    mean = pts.numpy().astype(np.float64).mean(axis=0)
    assert np.all(np.abs(one.numpy().astype(np.float64)[0] - mean) <= np.spacing(np.abs(mean).astype(np.float32)) + 100.0 * 2.0 ** -37)


def test_stability_on_the_torus_coreset():
    """|d_coreset - d_cloud| <= W_2 / sqrt(m) <= cell * sqrt(3) / sqrt(m): every point moves by at most the diagonal of its
    cell.  The exact value is the plain k-nearest DTM at k = m * N = 400; every query is reached at the default capacity."""
    t = km.torus_coreset()
    pts, qs, m = t["points"].double(), t["queries"].double(), t["mass"]
    assert core.mass_neighbors(m, pts.shape[0]) == 400
    exact = fa.distance_to_measure(pts, qs, m)
    got, ids, dist, count = fa.distance_to_weighted_measure(t["sites"].double(), t["masses"].double(), qs, mass=m,
                                                            return_neighbors=True)
    assert bool(torch.isfinite(got).all()) and int(count.max()) < 1024, "a query was not reached"
    bound = t["cell"] * np.sqrt(3.0) / np.sqrt(m)
    err = float((got - exact).abs().max())
    print(f"sites {t['sites'].shape[0]}, neighbours median {int(count.median())} max {int(count.max())}, "
          f"|weighted - exact| max {err:.4g} (bound {bound:.4g}), median value {float(exact.median()):.4g}")
    assert err <= bound
    assert int(count.max()) < 400      # fewer list entries than the 400 points they stand for


def test_refusals():
    pts = torch.rand(50, 3)
    mu = torch.ones(50)
    f = fa.distance_to_weighted_measure
    with pytest.raises(ValueError, match=r"point_masses must be a \(50,\) tensor, one mass per point"):
        f(pts, mu[:49], mass=0.5)
    with pytest.raises(ValueError, match=r"point_masses must be a \(50,\) tensor"):
        f(pts, [1.0] * 50, mass=0.5)
    with pytest.raises(ValueError, match=r"point_masses\.dtype \(torch\.float64\) != points\.dtype \(torch\.float32\)"):
        f(pts, mu.double(), mass=0.5)
    with pytest.raises(ValueError, match="needs mass"):
        f(pts, mu)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"mass must be in \(0, 1\]"):
            f(pts, mu, mass=bad)
    with pytest.raises(TypeError, match="mass must be a real number"):
        f(pts, mu, mass="0.5")
    for bad in (torch.full((50,), float("nan")), -mu, torch.full((50,), float("inf"))):
        with pytest.raises(ValueError, match="point_masses must be finite and non-negative"):
            f(pts, bad, mass=0.5)
    with pytest.raises(ValueError, match="point_masses must have a positive total"):
        f(pts, torch.zeros(50), mass=0.5)
    with pytest.raises(ValueError, match=r"max_neighbors must be in 1\.\.1024"):
        f(pts, mu, mass=0.5, max_neighbors=1025)
    with pytest.raises(ValueError, match=r"max_neighbors must be in 1\.\.1024"):
        f(pts, mu, mass=0.5, max_neighbors=0)
    with pytest.raises(TypeError, match="max_neighbors must be an integer"):
        f(pts, mu, mass=0.5, max_neighbors=64.0)
    with pytest.raises(ValueError, match="neighbor_stat"):
        f(pts, mu, mass=0.5, neighbor_stat="mean")
    with pytest.raises(RuntimeError, match=r"queries must be a \(Q, 3\) tensor"):
        f(pts, mu, torch.rand(4, 2), mass=0.5)
    with pytest.raises(RuntimeError, match=r"queries\.dtype"):
        f(pts, mu, torch.rand(4, 3).double(), mass=0.5)
    with pytest.raises(RuntimeError, match="points must be a non-empty"):
        f(pts[:0], mu[:0], mass=0.5)
    with pytest.raises(TypeError, match="not supported"):
        f(pts.half(), mu.half(), mass=0.5)
    # not differentiable: inputs that require grad are used detached
    out = f(pts.clone().requires_grad_(), mu, mass=0.5)
    assert not out.requires_grad
    # voxel_measure
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cell_size must be positive and finite"):
            fa.voxel_measure(pts, bad)
    with pytest.raises(TypeError, match="cell_size must be a positive real number"):
        fa.voxel_measure(pts, "0.1")
    with pytest.raises(RuntimeError, match="points must be a non-empty"):
        fa.voxel_measure(pts[:0], 0.1)


def test_float64_on_rocm_is_refused_in_the_family_wording():
    """Without a GPU: the refusal is ``_check_points``', made under this function's name (the GPU test raises it)."""
    from flooder_amd import neighbors

    src = open(os.path.join(ROOT, "flooder_amd", "neighbors.py")).read()
    assert '_check_points(points, "distance_to_weighted_measure")' in src
    assert "needs float32: the k-nearest sweep has no float64 kernel" in src
    assert neighbors.distance_to_weighted_measure is fa.distance_to_weighted_measure


def test_wiring():
    for name in ("distance_to_weighted_measure", "voxel_measure"):
        assert name in fa.__all__ and getattr(fa, name) is getattr(fa.neighbors, name)
    assert "flood_knn_mass.hip" in build.HIP_SOURCES and "flood_knn_wide.hip" in build.HIP_SOURCES
    assert os.path.exists(os.path.join(ROOT, "flooder_amd", "csrc", "flood_knn_mass.hip"))
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert re.search(r"^int flooder_knn_mass_f32\(const flooder_knn_wide_t\* p, const float\* masses, const double\* target, "
                     r"int32_t ld_out,\n\s+int32_t\* out_count, void\* stream\);", header, re.M)
    res, args = _native.SIGNATURES["flooder_knn_mass_f32"]
    # the block of the wide entry plus what this one adds: no thirteenth argument, no twelfth block
    assert len(args) == 6 and args[0]._type_ is _native.KnnWide and res is _native.c_int
    assert args[1:] == [_native.c_void_p, _native.c_void_p, _native.c_int32, _native.c_void_p, _native.c_void_p]
