"""``distance_to_weighted_measure_profile`` and ``dtm_profile(cell_size=...)`` on ROCm tensors: every column is the
single ``distance_to_weighted_measure`` call, ``torch.equal``, counts included - on the 20 000-point torus and its
coreset, with a capacity that leaves some queries not reached, with the sites as their own queries and with query groups
forced by a small workspace -; the launches are counted (ONE profile entry per group, the single entry never); the
coreset profile equals ``flood_complex(point_weights=...)`` of the single weighted calls; the refusals; and both public
calls on a side stream while the default stream is held."""

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import knn_mass_reference as km
import streams_helper as sh
from test_gpu_streams import free_streams, lib, side  # noqa: F401  (fixtures: the side streams that run during a hold)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
STATS = ("dtm", "kth")
MASSES = (0.02, 0.002, 0.0055)     # 400, 40 and 110 of the torus' points; the largest is not the last
CAPS = (64, 1024)


def _counted(monkeypatch, name, record):
    lib_ = _native.load()
    real = getattr(lib_, name)
    calls = []

    def counted(blk, *rest):
        calls.append(record(blk._obj, *rest))
        return real(blk, *rest)

    monkeypatch.setattr(lib_, name, counted)
    return calls


@pytest.fixture(scope="module")
def torus():
    t = km.torus_coreset()
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


@pytest.fixture(scope="module")
def singles(torus):
    """{(cap, mass, stat, squared): (value, count)} of the single calls, computed once."""
    out = {}
    for cap in CAPS:
        for m in MASSES:
            for s in STATS:
                for squared in (False, True):
                    v, _, _, n = fa.distance_to_weighted_measure(torus["sites"], torus["masses"], torus["queries"], mass=m,
                                                                 neighbor_stat=s, squared=squared, max_neighbors=cap,
                                                                 return_neighbors=True)
                    out[(cap, m, s, squared)] = (v, n)
    return out


def test_both_kinds_of_query_occur_says_the_cpu_path():
    """At 64 neighbours the torus' queries are all reached at mass 0.002, none at 0.02, and some at 0.0055."""
    t = km.torus_coreset()
    v = fa.distance_to_weighted_measure_profile(t["sites"], t["masses"], t["queries"], MASSES, max_neighbors=64)
    missed = torch.isinf(v).sum(dim=0).tolist()
    Q = t["queries"].shape[0]
    assert missed[0] == Q and missed[1] == 0 and 0 < missed[2] < Q, missed
    v = fa.distance_to_weighted_measure_profile(t["sites"], t["masses"], t["queries"], MASSES, max_neighbors=1024)
    assert bool(torch.isfinite(v).all())


@pytest.mark.parametrize("cap", CAPS)
def test_columns_are_the_single_calls(cap, torus, singles, monkeypatch):
    sites, mu, q = torus["sites"], torus["masses"], torus["queries"]
    Q, cols = q.shape[0], [(m, s) for m in MASSES for s in STATS]
    profile_calls = _counted(monkeypatch, "flooder_knn_mass_profile_f32",
                             lambda b, masses, n_cols, targets, col_stat, stride, *rest: (int(b.n_simplices), int(b.k),
                                                                                         int(n_cols), int(stride)))
    single_calls = _counted(monkeypatch, "flooder_knn_mass_f32", lambda b, *rest: int(b.k))
    index = core.PointIndex(sites)
    whole = core.SORTED_WORKSPACE_BYTES
    for squared in (False, True):
        for workspace, idx in ((whole, None), ((24 + 8 * len(cols)) * 700, index)):
            monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", workspace)
            del profile_calls[:]
            values, counts = fa.distance_to_weighted_measure_profile(sites, mu, q, MASSES, neighbor_stat=STATS,
                                                                     squared=squared, max_neighbors=cap,
                                                                     return_counts=True, index=idx)
            assert values.shape == counts.shape == (Q, len(cols)) and values.is_contiguous() and counts.is_contiguous()
            assert values.dtype == torch.float32 and counts.dtype == torch.int64 and not values.requires_grad
            for c, (m, s) in enumerate(cols):
                v, n = singles[(cap, m, s, squared)]
                assert torch.equal(values[:, c], v), (m, s, squared, workspace)
                assert torch.equal(counts[:, c], n), (m, s, squared, workspace)
            # ONE launch per group of queries, for all the columns, planes Q words apart
            groups = [Q] if idx is None else [700] * (Q // 700) + ([Q % 700] if Q % 700 else [])
            assert profile_calls == [(g, cap, len(cols), Q) for g in groups]
    assert single_calls == []
    if cap == 64:       # (the kinds the CPU path promised)
        missed = torch.isinf(values).sum(dim=0).tolist()
        assert missed[0] == missed[1] == Q and missed[2] == missed[3] == 0 and 0 < missed[4] == missed[5] < Q, missed
        assert bool((counts[:, 0] == 64).all())


def test_the_sites_as_their_own_queries_one_column_and_no_queries(torus):
    sites, mu = torus["sites"], torus["masses"]
    values, counts = fa.distance_to_weighted_measure_profile(sites, mu, None, (0.004, 0.001), neighbor_stat=STATS,
                                                             max_neighbors=256, return_counts=True)
    c = 0
    for m in (0.004, 0.001):
        for s in STATS:
            v, _, _, n = fa.distance_to_weighted_measure(sites, mu, None, mass=m, neighbor_stat=s, max_neighbors=256,
                                                         return_neighbors=True)
            assert torch.equal(values[:, c], v) and torch.equal(counts[:, c], n), (m, s)
            c += 1
    one = fa.distance_to_weighted_measure_profile(sites, mu, torus["queries"], 0.004)
    assert one.shape == (torus["queries"].shape[0], 1)
    assert torch.equal(one[:, 0], fa.distance_to_weighted_measure(sites, mu, torus["queries"], 0.004))
    values, counts = fa.distance_to_weighted_measure_profile(sites, mu, sites[:0], (0.004, 0.001), return_counts=True)
    assert values.shape == counts.shape == (0, 2) and values.device == sites.device and counts.dtype == torch.int64
    many = [i / 100 for i in range(1, 34)]
    with pytest.raises(ValueError, match="on ROCm tensors takes at most 64 columns, got 66"):
        fa.distance_to_weighted_measure_profile(sites, mu, None, many, neighbor_stat=STATS)
    with pytest.raises(ValueError, match="masses lists a value twice"):
        fa.distance_to_weighted_measure_profile(sites, mu, None, (0.01, 0.01))
    with pytest.raises(ValueError, match="distance_to_weighted_measure on ROCm tensors needs float32"):
        fa.distance_to_weighted_measure_profile(sites.double(), mu.double(), None, 0.01)


def _annulus_with_strays(n, strays, seed=0):
    clean = fa.generate_annulus_points_2d(n, radius=1.0, width=0.2, seed=seed).float()
    g = torch.Generator().manual_seed(seed + 1)
    r, t = 0.7 * torch.sqrt(torch.rand(strays, generator=g)), 2 * np.pi * torch.rand(strays, generator=g)
    return torch.cat([clean, torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1)])


@pytest.fixture(scope="module")
def annulus():
    pts = _annulus_with_strays(5000, 50).to(DEV)
    return pts, fa.generate_landmarks(pts, 100)


def test_dtm_profile_over_the_coreset_is_the_single_calls(annulus, monkeypatch):
    pts, lms = annulus
    masses, cell, kw = (0.3, 0.004, 0.02), 0.05, dict(points_per_edge=10)
    profile_calls = _counted(monkeypatch, "flooder_knn_mass_profile_f32", lambda b, m, n_cols, *rest: int(n_cols))
    single_calls = _counted(monkeypatch, "flooder_knn_mass_f32", lambda b, *rest: int(b.k))
    prof = fa.dtm_profile(pts, lms, masses, cell_size=cell, neighbor_stat=STATS, **kw)
    assert profile_calls == [6] and single_calls == []
    ks = [core.mass_neighbors(m, pts.shape[0]) for m in masses]
    assert ks[0] > core.KNN_WIDE_MAX                                       # a mass the plain profile refuses
    assert prof.columns == tuple((k, s) for k in ks for s in STATS)
    assert prof.masses == tuple(m for m in masses for _ in STATS)
    sites, mu = fa.voxel_measure(pts, cell)
    for (k, s), m in zip(prof.columns, prof.masses):
        w = fa.distance_to_weighted_measure(sites, mu, pts, mass=m, neighbor_stat=s)
        assert prof[(k, s)] == fa.flood_complex(pts, lms, point_weights=w, **kw), (k, s)
    trees = fa.dtm_profile(pts, lms, masses[1:], cell_size=cell, max_neighbors=128, return_simplex_tree=True, **kw)
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
    with pytest.raises(ValueError, match=r"^dtm_profile: \d+ of 5050 points were not reached at mass 0.5 - .*coarsen "
                                         "cell_size or lower the mass"):
        fa.dtm_profile(pts, lms, (0.004, 0.5), cell_size=0.02, max_neighbors=64, points_per_edge=10)
    with pytest.raises(ValueError, match="above KNN_WIDE_MAX = 1024"):
        fa.dtm_profile(pts, lms, (0.004, 0.3), points_per_edge=10)


def weighted_profile(p, q, cell, masses, cap):
    sites, mu = fa.voxel_measure(p, cell)
    values, counts = fa.distance_to_weighted_measure_profile(sites, mu, q, masses, neighbor_stat=STATS, max_neighbors=cap,
                                                             return_counts=True)
    return [sites, mu, values, counts]


def coreset_profile(p):
    prof = fa.dtm_profile(p, 40, (0.05, 0.005), points_per_edge=8, cell_size=0.1, max_neighbors=256)
    return [prof.table(d)[1] for d in range(4)]


def test_held_weighted_measure_profile(side):
    """The integer-valued clouds of the held neighbour family: dense in the middle, single points far out."""
    clouds = []
    for seed in (80, 90):
        g = torch.Generator().manual_seed(seed)
        clouds.append((torch.round(8 * torch.randn(20_000, 3, generator=g)).to(DEV),
                       torch.round(10 * torch.randn(3000, 3, generator=g)).to(DEV)))
    ref = sh.held_call("distance_to_weighted_measure_profile", lambda p, q: weighted_profile(p, q, 2.0, (0.02, 0.002), 64),
                       clouds[0], clouds[1], side)
    missed = np.isinf(ref[2]).sum(axis=0)
    assert 0 < missed[0] < ref[2].shape[0], f"{missed.tolist()} of {ref[2].shape[0]} queries not reached: both kinds are needed"


def test_held_dtm_profile_over_the_coreset(side):
    """Uniform clouds in the unit cube: 1000 cells of about 20 points, so 256 sites hold the mass 0.05 everywhere."""
    real, decoy = (torch.rand(20_000, 3, generator=torch.Generator().manual_seed(s)).to(DEV) for s in (100, 101))
    ref = sh.held_call("dtm_profile cell_size", coreset_profile, (real,), (decoy,), side)
    assert all(np.isfinite(t).all() for t in ref) and ref[3].shape[1] == 2
