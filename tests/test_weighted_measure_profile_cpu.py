"""``distance_to_weighted_measure_profile`` and ``dtm_profile(cell_size=...)`` on CPU tensors (no GPU): every column is
the single ``distance_to_weighted_measure`` call, exactly, counts included - float32 and float64, 2-D and 4-D, zero-mass
sites, columns that are not reached, ``squared=True`` -; the coreset profile against ``flood_complex(point_weights=...)``
of the single weighted calls; a mass above 1024 points, which the plain profile refuses; the refusals and their wording;
the new entry in the built library, in ``_native`` and in the header."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core, neighbors, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("dtm", "kth")


def _cloud(n, dim, dtype, seed=0):
    return torch.randn(n, dim, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def _annulus_with_strays(n, strays, seed=0):
    clean = fa.generate_annulus_points_2d(n, radius=1.0, width=0.2, seed=seed).float()
    g = torch.Generator().manual_seed(seed + 1)
    r, t = 0.7 * torch.sqrt(torch.rand(strays, generator=g)), 2 * np.pi * torch.rand(strays, generator=g)
    return torch.cat([clean, torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1)])


def _assert_columns(sites, mu, queries, masses, stats, **kw):
    """Every column and its count against the single call -> the (values, counts) of the profile."""
    single_kw = {k: v for k, v in kw.items() if k != "index"}
    values, counts = fa.distance_to_weighted_measure_profile(sites, mu, queries, masses, neighbor_stat=stats,
                                                             return_counts=True, **kw)
    only = fa.distance_to_weighted_measure_profile(sites, mu, queries, masses, neighbor_stat=stats, **kw)
    Q = (sites if queries is None else queries).shape[0]
    cols = [(m, s) for m in masses for s in stats]
    assert values.shape == counts.shape == (Q, len(cols)) and torch.equal(only, values)
    assert values.dtype == sites.dtype and counts.dtype == torch.int64 and not values.requires_grad
    for c, (m, s) in enumerate(cols):
        v, _, _, n = fa.distance_to_weighted_measure(sites, mu, queries, mass=m, neighbor_stat=s, return_neighbors=True,
                                                     **single_kw)
        assert torch.equal(values[:, c], v), (m, s)
        assert torch.equal(counts[:, c], n), (m, s)
    return values, counts


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
@pytest.mark.parametrize("dim", (2, 4))
def test_columns_are_the_single_calls(dim, dtype):
    pts = _cloud(3000, dim, dtype, seed=dim)
    sites, mu = fa.voxel_measure(pts, 0.3 if dim == 2 else 0.9)
    queries = _cloud(400, dim, dtype, seed=10 + dim) * 1.3
    masses = (0.004, 0.05, 0.2)
    for squared in (False, True):
        values, _ = _assert_columns(sites, mu, queries, masses, STATS, squared=squared)
        assert bool(torch.isfinite(values).all())
    # the sites themselves as queries; one mass, one name; a capacity that leaves some queries not reached at some masses
    _assert_columns(sites, mu, None, (0.05,), ("kth",))
    out = fa.distance_to_weighted_measure_profile(sites, mu, queries, 0.05, neighbor_stat="dtm")
    assert out.shape == (400, 1)
    assert torch.equal(out[:, 0], fa.distance_to_weighted_measure(sites, mu, queries, 0.05))
    values, counts = _assert_columns(sites, mu, queries, (0.5, 0.004, 0.05), STATS, max_neighbors=40)
    missed = torch.isinf(values).sum(dim=0)
    L = min(64, sites.shape[0])
    assert int(missed[0]) > 0 and int(missed[2]) == 0, missed.tolist()
    assert bool((counts[:, 0][torch.isinf(values[:, 0])] == L).all())
    # a row that is not reached at the largest mass still has its smaller columns
    assert bool(torch.isfinite(values[torch.isinf(values[:, 0])][:, 2:4]).all())


def test_zero_mass_sites_and_requires_grad():
    pts = _cloud(2000, 2, torch.float32, seed=3)
    sites, mu = fa.voxel_measure(pts, 0.2)
    mu = mu.clone()
    mu[::2] = 0.0
    queries = _cloud(300, 2, torch.float32, seed=4)
    _, counts = _assert_columns(sites, mu, queries, (0.01, 0.1), STATS)
    assert int(counts.min()) >= 1
    values = fa.distance_to_weighted_measure_profile(sites.clone().requires_grad_(), mu.clone().requires_grad_(),
                                                     queries.clone().requires_grad_(), (0.01, 0.1))
    assert not values.requires_grad and values.grad_fn is None


def test_empty_queries():
    sites, mu = fa.voxel_measure(_cloud(500, 3, torch.float64), 0.5)
    values, counts = fa.distance_to_weighted_measure_profile(sites, mu, sites[:0], (0.1, 0.2), neighbor_stat=STATS,
                                                             return_counts=True)
    assert values.shape == counts.shape == (0, 4) and values.dtype == torch.float64 and counts.dtype == torch.int64
    assert fa.distance_to_weighted_measure_profile(sites, mu, sites[:0], 0.1).shape == (0, 1)


def test_refusals():
    sites, mu = fa.voxel_measure(_cloud(500, 3, torch.float32), 0.5)
    f = fa.distance_to_weighted_measure_profile
    with pytest.raises(ValueError, match="distance_to_weighted_measure_profile needs masses"):
        f(sites, mu)
    with pytest.raises(ValueError, match="masses must not be empty"):
        f(sites, mu, None, ())
    with pytest.raises(ValueError, match="neighbor_stat must not be empty"):
        f(sites, mu, None, 0.1, neighbor_stat=())
    with pytest.raises(TypeError, match="masses must be a number or a sequence of numbers"):
        f(sites, mu, None, "0.1")
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match=r"mass must be in \(0, 1\]"):
            f(sites, mu, None, (0.1, bad))
    for bad in (True, "a", None):
        with pytest.raises(TypeError, match=r"mass must be a real number in \(0, 1\]"):
            f(sites, mu, None, (0.1, bad))
    with pytest.raises(ValueError, match="masses lists a value twice"):
        f(sites, mu, None, (0.1, 0.2, 0.1))
    with pytest.raises(ValueError, match="neighbor_stat lists a name twice"):
        f(sites, mu, None, 0.1, neighbor_stat=("dtm", "dtm"))
    with pytest.raises(ValueError, match="neighbor_stat"):
        f(sites, mu, None, 0.1, neighbor_stat=("dtm", "mean"))
    # what distance_to_weighted_measure says of the points, their masses, the queries and max_neighbors
    with pytest.raises(ValueError, match=r"point_masses must be a \(\d+,\) tensor"):
        f(sites, mu[:-1], None, 0.1)
    with pytest.raises(ValueError, match="point_masses.dtype"):
        f(sites, mu.double(), None, 0.1)
    with pytest.raises(ValueError, match="point_masses must be finite and non-negative"):
        f(sites, -mu, None, 0.1)
    with pytest.raises(ValueError, match="point_masses must have a positive total"):
        f(sites, torch.zeros_like(mu), None, 0.1)
    with pytest.raises(RuntimeError, match=r"queries must be a \(Q, 3\) tensor"):
        f(sites, mu, sites[:, :2], 0.1)
    with pytest.raises(ValueError, match=r"max_neighbors must be in 1\.\.1024"):
        f(sites, mu, None, 0.1, max_neighbors=2000)
    with pytest.raises(TypeError, match="max_neighbors must be an integer"):
        f(sites, mu, None, 0.1, max_neighbors=64.0)
    with pytest.raises(RuntimeError, match="points must be a non-empty"):
        f(sites[:0], mu[:0], None, 0.1)


def test_rocm_refusals_without_a_device():
    """What ROCm tensors are told, without a device: the checks look at ``is_cuda``, the dtype and the shape only."""
    class Fake(torch.Tensor):
        is_cuda = True

    f = fa.distance_to_weighted_measure_profile
    p64 = _cloud(50, 3, torch.float64).as_subclass(Fake)
    with pytest.raises(ValueError, match="distance_to_weighted_measure on ROCm tensors needs float32"):
        f(p64, torch.ones(50, dtype=torch.float64), None, 0.1)
    p9 = _cloud(50, 9, torch.float32).as_subclass(Fake)
    with pytest.raises(ValueError, match="ROCm tensors needs ambient dimension 2 to 8"):
        f(p9, torch.ones(50), None, 0.1)
    p = _cloud(50, 3, torch.float32).as_subclass(Fake)
    many = [i / 100 for i in range(1, 34)]
    with pytest.raises(ValueError, match="distance_to_weighted_measure_profile on ROCm tensors takes at most 64 columns, "
                                         "got 66"):
        f(p, torch.ones(50).as_subclass(Fake), None, many, neighbor_stat=STATS)


@pytest.fixture(scope="module")
def annulus():
    pts = _annulus_with_strays(5000, 50)
    lms = fa.generate_landmarks(pts, 100)
    return pts, lms


def test_dtm_profile_over_the_coreset_is_the_single_calls(annulus):
    pts, lms = annulus
    masses, cell, kw = (0.004, 0.02, 0.3), 0.05, dict(points_per_edge=10)
    prof = fa.dtm_profile(pts, lms, masses, cell_size=cell, neighbor_stat=STATS, **kw)
    ks = [core.mass_neighbors(m, pts.shape[0]) for m in masses]
    assert ks[-1] > core.KNN_WIDE_MAX                                      # a mass the plain profile refuses
    assert prof.columns == tuple((k, s) for k in ks for s in STATS)
    assert prof.masses == tuple(m for m in masses for _ in STATS)
    sites, mu = fa.voxel_measure(pts, cell)
    for (k, s), m in zip(prof.columns, prof.masses):
        w = fa.distance_to_weighted_measure(sites, mu, pts, mass=m, neighbor_stat=s)
        assert prof[(k, s)] == fa.flood_complex(pts, lms, point_weights=w, **kw), (k, s)
    # max_neighbors goes to the weighted call; simplex trees compare by their arrays
    trees = fa.dtm_profile(pts, lms, masses[:2], cell_size=cell, max_neighbors=128, return_simplex_tree=True, **kw)
    for (k, s), m in zip(trees.columns, trees.masses):
        w = fa.distance_to_weighted_measure(sites, mu, pts, mass=m, neighbor_stat=s, max_neighbors=128)
        ref = fa.flood_complex(pts, lms, point_weights=w, return_simplex_tree=True, **kw)
        for d in range(3):
            assert np.array_equal(trees[(k, s)].simplices_of_dimension(d), ref.simplices_of_dimension(d))
            assert np.array_equal(trees[(k, s)].filtrations_of_dimension(d), ref.filtrations_of_dimension(d))


def test_dtm_profile_refusals(annulus):
    pts, lms = annulus
    with pytest.raises(ValueError, match="^dtm_profile: max_neighbors is the list capacity of the coreset's weighted "
                                         "measure and needs cell_size"):
        fa.dtm_profile(pts, lms, (0.01,), max_neighbors=64)
    with pytest.raises(ValueError, match="^dtm_profile: a coreset is addressed by mass - pass masses, not neighbors, with "
                                         "cell_size"):
        fa.dtm_profile(pts, lms, neighbors=(5,), cell_size=0.05)
    with pytest.raises(ValueError, match="dtm_profile needs masses"):
        fa.dtm_profile(pts, lms, cell_size=0.05)
    with pytest.raises(ValueError, match="masses lists a value twice"):
        fa.dtm_profile(pts, lms, (0.01, 0.010001), cell_size=0.05)          # two masses, one k
    with pytest.raises(ValueError, match="cell_size must be positive and finite"):
        fa.dtm_profile(pts, lms, (0.01,), cell_size=0.0)
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match="point_weights needs the tree sweep"):
            fa.dtm_profile(pts, lms, (0.01,), cell_size=0.05, method=method)
    # a column in which some point is not reached: the mass, how many of the N points, and the two remedies
    n_pts = pts.shape[0]
    with pytest.raises(ValueError) as err:
        fa.dtm_profile(pts, lms, (0.004, 0.5), cell_size=0.02, max_neighbors=64, points_per_edge=10)
    said = str(err.value)
    assert said.startswith("dtm_profile: ") and f"of {n_pts} points were not reached at mass 0.5" in said
    assert "coarsen cell_size or lower the mass" in said
    assert 0 < int(re.search(r"(\d+) of ", said).group(1)) <= n_pts


def test_a_mass_above_the_wall():
    """30 000 points, mass 0.05: k = 1500 neighbours, which the plain profile refuses and the coreset runs."""
    pts = _annulus_with_strays(30_000, 0, seed=2)
    with pytest.raises(ValueError, match="above KNN_WIDE_MAX = 1024"):
        fa.dtm_profile(pts, 30, (0.01, 0.05), points_per_edge=5)
    prof = fa.dtm_profile(pts, 30, (0.01, 0.05), points_per_edge=5, cell_size=0.05)
    assert prof.columns == ((300, "dtm"), (1500, "dtm")) and prof.masses == (0.01, 0.05)
    assert all(np.isfinite(list(prof[c].values())).all() for c in prof.columns)


def test_dtm_profile_without_the_new_keywords_is_what_it_was():
    params = list(inspect.signature(fa.dtm_profile).parameters.values())
    names = [p.name for p in params]
    assert names == ["points", "landmarks", "masses", "max_dimension", "points_per_edge", "num_rand", "start_idx",
                     "neighbors", "neighbor_stat", "return_simplex_tree", "method", "index", "cell_size", "max_neighbors"]
    by = {p.name: p for p in params}
    assert [by[n].default for n in names[2:]] == [None, None, 30, None, 0, None, "dtm", False, None, None, None, None]
    assert all(by[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[7:])
    assert all(by[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:7])
    pts = _cloud(400, 2, torch.float32, seed=9)
    prof = fa.dtm_profile(pts, 20, (0.02, 0.1), points_per_edge=5)
    assert prof.columns == ((8, "dtm"), (40, "dtm"))
    w = fa.distance_to_measure(pts, mass=0.1)
    assert prof[(40, "dtm")] == fa.flood_complex(pts, 20, points_per_edge=5, point_weights=w)


def test_names_are_exported_and_bound():
    name = "distance_to_weighted_measure_profile"
    assert name in fa.__all__ and getattr(fa, name) is getattr(neighbors, name)
    entry = "flooder_knn_mass_profile_f32"
    res, args = _native.SIGNATURES[entry]
    assert res is ctypes.c_int and len(args) == 8 and len(args) <= 12
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), entry) and hasattr(_native.load(), entry)
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert re.search(r"^int flooder_knn_mass_profile_f32\(const flooder_knn_wide_t\* p, const float\* masses, int n_cols, "
                     r"const double\* targets,\s+const int32_t\* col_stat, int64_t plane_stride, int32_t\* out_count, "
                     r"void\* stream\);", header, re.M)
    assert "distance_to_weighted_measure_profile" in (fa.distance_to_weighted_measure.__doc__ or "")
    assert profile.dtm_profile is fa.dtm_profile


def test_readme_scan_past_the_wall():
    """README, "Above 1024 neighbours": the annulus with 100 strays, five masses over the coreset at cell 0.02."""
    import math

    from flooder_amd.persistence import persistence_pairs

    clean = fa.generate_annulus_points_2d(20000, radius=1.0, width=0.2, seed=0).float()
    g = torch.Generator()
    r, t = 0.7 * torch.sqrt(torch.rand(100, generator=g.manual_seed(1))), 2 * math.pi * torch.rand(100, generator=g)
    dirty = torch.cat([clean, torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1)])
    masses = (0.006, 0.02, 0.04, 0.08, 0.16)
    with pytest.raises(ValueError, match="mass=0.08 is 1608 neighbours of 20100 points, above KNN_WIDE_MAX"):
        fa.dtm_profile(dirty, 200, masses, points_per_edge=20)
    prof = fa.dtm_profile(dirty, 200, masses, points_per_edge=20, return_simplex_tree=True, cell_size=0.02)
    assert [k for k, _ in prof.columns] == [121, 402, 804, 1608, 3216] and prof.masses == masses
    longest, second = [], []
    for col in prof.columns:
        h1 = persistence_pairs(prof[col])[1]
        lengths = sorted((h1[:, 1] - h1[:, 0]).tolist(), reverse=True) + [0.0]
        longest.append(lengths[0])
        second.append(lengths[1])
    assert np.allclose(longest, [0.520, 0.540, 0.529, 0.491, 0.400], atol=1e-3)
    assert np.allclose(second[:2], [3.2e-4, 4.4e-5], rtol=0.05) and second[2:] == [0.0, 0.0, 0.0]
