"""``distance_to_measure_profile``, ``power_profile`` and ``dtm_profile`` on CPU tensors: every column is the single
call, exactly; the refusals come before any work and in the single calls' words; the README's scan over the mass."""

import math

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import core, neighbors, profile
from flooder_amd.persistence import persistence_pairs


def _cloud(n, dim, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, dim, generator=g).to(dtype)


@pytest.mark.parametrize("dim,dtype", [(2, torch.float32), (3, torch.float64), (6, torch.float32)])
def test_distance_to_measure_profile_columns_are_the_single_calls(dim, dtype):
    pts = _cloud(900, dim, dtype, dim)
    q = _cloud(70, dim, dtype, 50 + dim)
    ks = (1, 7, 64, 65, 300)
    for queries in (None, q):
        for squared in (False, True):
            out = fa.distance_to_measure_profile(pts, queries, neighbors=ks, neighbor_stat=("kth", "dtm"), squared=squared)
            cols = [(k, s) for k in ks for s in ("kth", "dtm")]
            assert out.shape == ((900 if queries is None else 70), len(cols)) and out.dtype == dtype
            for c, (k, s) in enumerate(cols):
                one = fa.distance_to_measure(pts, queries, neighbors=k, neighbor_stat=s, squared=squared)
                assert torch.equal(out[:, c], one), (k, s, squared)
    # by mass: the k of every mass, one statistic by name, a single number in place of a list
    masses = (0.01, 0.05, 0.3)
    out = fa.distance_to_measure_profile(pts, q, masses)
    for c, m in enumerate(masses):
        assert torch.equal(out[:, c], fa.distance_to_measure(pts, q, m))
    assert torch.equal(fa.distance_to_measure_profile(pts, q, 0.05)[:, 0], fa.distance_to_measure(pts, q, 0.05))
    assert fa.distance_to_measure_profile(pts, q[:0], masses).shape == (0, 3)


def _same_result(a, b):
    if isinstance(a, dict):
        assert a == b
    else:
        for d in range(a.dimension() + 1):
            assert np.array_equal(a.simplices_of_dimension(d), b.simplices_of_dimension(d))
            assert np.array_equal(a.filtrations_of_dimension(d), b.filtrations_of_dimension(d))


@pytest.mark.parametrize("dim,dtype,n_cols", [(2, torch.float32, 3), (3, torch.float64, 1), (3, torch.float32, 9)])
def test_power_profile_columns_are_the_single_calls(dim, dtype, n_cols):
    pts = _cloud(600, dim, dtype, 7 * dim)
    g = torch.Generator().manual_seed(3)
    w = (torch.rand(600, n_cols, generator=g) * 0.4).to(dtype)
    w[:, 0] = 0                                     # the plain filtration among the columns
    if n_cols > 1:
        w[:, 1] = -w[:, 1]                          # the sign does not matter
    lms = pts[:25].clone()
    prof = fa.power_profile(pts, lms, w, points_per_edge=6)
    assert prof.columns == tuple((c, "power") for c in range(n_cols)) and len(prof) == n_cols
    for c in range(n_cols):
        one = fa.flood_complex(pts, lms, points_per_edge=6, point_weights=w[:, c].contiguous())
        assert prof[c] == one and prof[(c, "power")] is prof[c]
    assert prof[0] == fa.flood_complex(pts, lms, points_per_edge=6)
    simp, vals = prof.table(1)
    assert vals.shape == (simp.shape[0], n_cols)
    assert all(vals[i, c] == prof[c][tuple(s)] for c in range(n_cols) for i, s in enumerate(simp.tolist()[:20]))
    # integer landmarks with a start index, drawn samples under a seed, simplex trees
    torch.manual_seed(11)
    prof = fa.power_profile(pts, 20, w, max_dimension=dim - 1, num_rand=9, start_idx=5, return_simplex_tree=True)
    for c in range(n_cols):
        torch.manual_seed(11)
        _same_result(prof[c], fa.flood_complex(pts, 20, max_dimension=dim - 1, num_rand=9, start_idx=5,
                                               return_simplex_tree=True, point_weights=w[:, c].contiguous()))


@pytest.mark.parametrize("dim,dtype", [(2, torch.float32), (3, torch.float64), (6, torch.float32)])
def test_dtm_profile_columns_are_the_recipe(dim, dtype):
    pts = _cloud(500, dim, dtype, 3 * dim)
    masses = (0.004, 0.05, 0.2)
    md = min(dim, 3)
    prof = fa.dtm_profile(pts, 18, masses, max_dimension=md, points_per_edge=5, neighbor_stat=("dtm", "kth"))
    ks = [core.mass_neighbors(m, 500) for m in masses]
    assert prof.columns == tuple((k, s) for k in ks for s in ("dtm", "kth"))
    assert prof.masses == tuple(m for m in masses for _ in range(2))
    for k, s in prof.columns:
        w = fa.distance_to_measure(pts, neighbors=k, neighbor_stat=s)
        assert prof[(k, s)] == fa.flood_complex(pts, 18, max_dimension=md, points_per_edge=5, point_weights=w)
    prof = fa.dtm_profile(pts, pts[:12].clone(), neighbors=(3, 40), max_dimension=1, points_per_edge=5)
    assert prof.columns == ((3, "dtm"), (40, "dtm")) and prof.masses is None
    w = fa.distance_to_measure(pts, neighbors=40)
    assert prof[1] == fa.flood_complex(pts, pts[:12].clone(), max_dimension=1, points_per_edge=5, point_weights=w)


def test_one_kdtree_query_and_one_complex_serve_every_column(monkeypatch):
    pts = _cloud(400, 2, torch.float32, 1)
    calls = []
    real = neighbors._kdtree_query
    monkeypatch.setattr(neighbors, "_kdtree_query", lambda p, q, k: calls.append(k) or real(p, q, k))
    fa.distance_to_measure_profile(pts, neighbors=(5, 90, 33), neighbor_stat=("dtm", "kth"))
    assert calls == [90]
    built = []
    real_complex = core._cell_complex
    monkeypatch.setattr(core, "_cell_complex", lambda *a: built.append(1) or real_complex(*a))
    fa.dtm_profile(pts, 15, neighbors=(5, 90, 33), points_per_edge=5)
    assert built == [1] and calls == [90, 90]


def test_refusals_come_before_any_work(monkeypatch):
    pts = _cloud(300, 3, torch.float32)
    w = torch.rand(300, 2)

    def no_work(*a, **k):
        raise AssertionError("work was done before the arguments were judged")

    monkeypatch.setattr(core, "_cell_complex", no_work)
    monkeypatch.setattr(neighbors, "_kdtree_query", no_work)
    for f in (lambda **kw: fa.distance_to_measure_profile(pts, **kw), lambda **kw: fa.dtm_profile(pts, 10, **kw)):
        with pytest.raises(ValueError, match="exactly one of masses and neighbors"):
            f()
        with pytest.raises(ValueError, match="exactly one of masses and neighbors"):
            f(masses=(0.1,), neighbors=(3,))
        with pytest.raises(ValueError, match="masses must not be empty"):
            f(masses=())
        with pytest.raises(ValueError, match="neighbors must not be empty"):
            f(neighbors=[])
        with pytest.raises(ValueError, match="neighbor_stat must not be empty"):
            f(neighbors=(3,), neighbor_stat=())
        with pytest.raises(ValueError, match="lists a value twice"):
            f(neighbors=(3, 8, 3))
        with pytest.raises(ValueError, match="lists a value twice"):      # two masses, one k
            f(masses=(0.1, 0.0999))      # (both are 30 of 300 points)
        with pytest.raises(ValueError, match="lists a name twice"):
            f(neighbors=(3,), neighbor_stat=("dtm", "dtm"))
        # ... every entry in the words of distance_to_measure
        with pytest.raises(ValueError, match=r"neighbors must be in 1\.\.1024"):
            f(neighbors=(3, 1025))
        with pytest.raises(ValueError, match=r"neighbors=301 exceeds the number of points \(300\)"):
            f(neighbors=(3, 301))
        with pytest.raises(TypeError, match="neighbors must be an integer"):
            f(neighbors=(3, 2.5))
        with pytest.raises(ValueError, match=r"mass must be in \(0, 1\]"):
            f(masses=(0.1, 1.5))
        with pytest.raises(TypeError, match="mass must be a real number"):
            f(masses=("0.1",))
        with pytest.raises(ValueError, match="neighbor_stat must be one of"):
            f(neighbors=(3,), neighbor_stat=("dtm", "mean"))
    big = _cloud(30_000, 2, torch.float32)
    with pytest.raises(ValueError, match="above KNN_WIDE_MAX = 1024"):
        fa.distance_to_measure_profile(big, masses=(0.001, 0.05))
    # power_profile: (N, M) weights, each column judged by flood_complex's check
    with pytest.raises(ValueError, match=r"point_weights must be a \(300, M\) tensor"):
        fa.power_profile(pts, 10, w[:, 0])
    with pytest.raises(ValueError, match=r"point_weights must be a \(300, M\) tensor"):
        fa.power_profile(pts, 10, w[:, :0])
    with pytest.raises(ValueError, match=r"point_weights must be a \(300,\) tensor"):
        fa.power_profile(pts, 10, w[:200])
    with pytest.raises(ValueError, match="point_weights.dtype"):
        fa.power_profile(pts, 10, w.double())
    with pytest.raises(ValueError, match="point_weights must be finite"):
        fa.power_profile(pts, 10, torch.where(w > 0.99, torch.tensor(float("inf")), w))
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match="point_weights needs the tree sweep"):
            fa.power_profile(pts, 10, w, method=method)
        with pytest.raises(ValueError, match="point_weights needs the tree sweep"):
            fa.dtm_profile(pts, 10, (0.1,), method=method)
    with pytest.raises(ValueError, match="method must be"):
        fa.power_profile(pts, 10, w, method="tree")


def test_rocm_float64_wording_is_the_shared_checks(monkeypatch):
    """What a ROCm float64 tensor is told, without a device: the checks look at ``is_cuda`` and the dtype only."""
    class Fake(torch.Tensor):
        is_cuda = True

    pts = _cloud(50, 3, torch.float64).as_subclass(Fake)
    with pytest.raises(ValueError, match="distance_to_measure on ROCm tensors needs float32"):
        fa.distance_to_measure_profile(pts, neighbors=(3, 5))
    with pytest.raises(ValueError, match="distance_to_measure on ROCm tensors needs float32"):
        fa.dtm_profile(pts, 10, neighbors=(3, 5))
    with pytest.raises(ValueError, match="point_weights on ROCm tensors needs float32"):
        fa.power_profile(pts, 10, torch.rand(50, 2, dtype=torch.float64).as_subclass(Fake))
    pts9 = _cloud(50, 9, torch.float32).as_subclass(Fake)
    with pytest.raises(ValueError, match="ROCm tensors needs ambient dimension 2 to 8"):
        fa.distance_to_measure_profile(pts9, neighbors=(3,))


def test_names_are_exported_and_bound():
    from flooder_amd import _native

    for name in ("distance_to_measure_profile", "power_profile", "dtm_profile"):
        assert name in fa.__all__ and callable(getattr(fa, name))
    for name in ("flooder_knn_wide_profile_f32", "flooder_node_min_cols_f32", "flooder_sweep_power_profile_f32"):
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) <= 12
    assert _native.POWER_COLS_MAX == core.POWER_COLS_MAX == 8
    assert profile.dtm_profile is fa.dtm_profile


def test_readme_scan_over_the_mass():
    """README, "Choosing the mass": the annulus with 100 strays in its hole, one ``dtm_profile`` over eight masses."""
    clean = fa.generate_annulus_points_2d(20000, radius=1.0, width=0.2, seed=0).float()
    g = torch.Generator()
    r, t = 0.7 * torch.sqrt(torch.rand(100, generator=g.manual_seed(1))), 2 * math.pi * torch.rand(100, generator=g)
    dirty = torch.cat([clean, torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1)])
    masses = (0.0005, 0.001, 0.002, 0.004, 0.006, 0.01, 0.02, 0.04)
    prof = fa.dtm_profile(dirty, 200, masses, points_per_edge=20, return_simplex_tree=True)
    assert [k for k, _ in prof.columns] == [11, 21, 41, 81, 121, 201, 402, 804] and prof.masses == masses
    longest, second = [], []
    for col in prof.columns:
        h1 = persistence_pairs(prof[col])[1]
        lengths = sorted((h1[:, 1] - h1[:, 0]).tolist(), reverse=True) + [0.0]
        longest.append(lengths[0])
        second.append(lengths[1])
    assert np.allclose(longest, [0.236, 0.285, 0.354, 0.446, 0.519, 0.536, 0.540, 0.529], atol=6e-4)
    assert np.allclose(second[:6], [0.0492, 0.0319, 0.00407, 0.00115, 0.000325, 0.000482], rtol=0.02)
    assert second[6] == second[7] == 0.0                     # from mass 0.02 on the hole's interval is the only one
    # the column at mass 0.006 is the README's single recipe
    w = fa.distance_to_measure(dirty, mass=0.006)
    one = fa.flood_complex(dirty, 200, points_per_edge=20, return_simplex_tree=True, point_weights=w)
    h1 = persistence_pairs(one)[1]
    assert float((h1[:, 1] - h1[:, 0]).max()) == longest[4]
