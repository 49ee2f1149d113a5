"""``distance_to_measure_profile``, ``power_profile`` and ``dtm_profile`` on ROCm tensors: every column is the single
call, exactly, in 2-D, 3-D and 6-D - with query groups and simplex groups forced by small workspaces, nine weight
columns (two column groups), drawn samples under a seed and a reused index - and the calls are counted: ONE wide entry
per group of queries, one profile sweep per dimension pass, column group and simplex group."""

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DIMS = (2, 3, 6)
KS = (1, 33, 64, 65, 200)
STATS = ("kth", "dtm")


def _cloud(n, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, dim, generator=g).to(DEV)


def _counted(monkeypatch, name, record):
    lib = _native.load()
    real = getattr(lib, name)
    calls = []

    def counted(blk, *rest):
        calls.append(record(blk._obj, *rest))
        return real(blk, *rest)

    monkeypatch.setattr(lib, name, counted)
    return calls


@pytest.mark.parametrize("dim", DIMS)
def test_distance_to_measure_profile_columns_are_the_single_calls(dim, monkeypatch):
    pts, q = _cloud(4000, dim, dim), _cloud(700, dim, 40 + dim) * 1.5
    cols = [(k, s) for k in KS for s in STATS]
    want = {}
    for queries in (None, q):
        for squared in (False, True):
            want[(queries is None, squared)] = [fa.distance_to_measure(pts, queries, neighbors=k, neighbor_stat=s,
                                                                       squared=squared) for k, s in cols]
    profile_calls = _counted(monkeypatch, "flooder_knn_wide_profile_f32", lambda b, n_cols, *rest: (int(b.n_simplices), int(b.k), int(n_cols)))
    single_calls = _counted(monkeypatch, "flooder_knn_wide_f32", lambda b, *rest: int(b.k))
    index = core.PointIndex(pts)
    whole = core.SORTED_WORKSPACE_BYTES
    for queries in (None, q):
        for squared in (False, True):
            for workspace, idx in ((whole, None), ((24 + 4 * len(cols)) * 300, index)):
                monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", workspace)
                del profile_calls[:]
                out = fa.distance_to_measure_profile(pts, queries, neighbors=KS, neighbor_stat=STATS, squared=squared,
                                                     index=idx)
                Q = 4000 if queries is None else 700
                assert out.shape == (Q, len(cols)) and out.is_contiguous()
                for c in range(len(cols)):
                    assert torch.equal(out[:, c], want[(queries is None, squared)][c]), (cols[c], squared, workspace)
                # ONE wide walk per group of queries, at the largest k, for all the columns
                groups = [Q] if idx is None else [300] * (Q // 300) + ([Q % 300] if Q % 300 else [])
                assert profile_calls == [(n, 200, len(cols)) for n in groups]
    assert single_calls == []
    masses = (0.002, 0.01, 0.05)
    out = fa.distance_to_measure_profile(pts, q, masses)
    for c, m in enumerate(masses):
        assert torch.equal(out[:, c], fa.distance_to_measure(pts, q, m))
    assert fa.distance_to_measure_profile(pts, q[:0], masses).shape == (0, 3)


def _counted_passes(monkeypatch):
    """One entry per dimension pass that goes through ``core._sweep_dimension_power_profile``."""
    real = core._sweep_dimension_power_profile
    passes = []
    monkeypatch.setattr(core, "_sweep_dimension_power_profile", lambda *a, **k: passes.append(1) or real(*a, **k))
    return passes


def _same_result(a, b):
    if isinstance(a, dict):
        assert a == b
    else:
        for d in range(a.dimension() + 1):
            assert np.array_equal(a.simplices_of_dimension(d), b.simplices_of_dimension(d))
            assert np.array_equal(a.filtrations_of_dimension(d), b.filtrations_of_dimension(d))


@pytest.mark.parametrize("dim,n_cols", [(2, 3), (3, 9), (6, 2), (3, 1)])
def test_power_profile_columns_are_the_single_calls(dim, n_cols, monkeypatch):
    pts = _cloud(5000, dim, 7 * dim)
    g = torch.Generator().manual_seed(n_cols)
    w = (torch.rand(5000, n_cols, generator=g) * 0.5).to(DEV)
    w[:, 0] = 0                                      # the plain filtration's values among the columns
    if n_cols > 1:
        w[:, 1] = -3.0 * w[:, 1]                     # heavy, and the sign does not matter
    if n_cols > 2:
        w[:, 2] = 50.0                               # a beacon column: one light point far out
        w[int(pts.norm(dim=1).argmax()), 2] = 0.0
    md = min(dim, 3)
    kw = dict(max_dimension=md, points_per_edge=8)
    lms = fa.generate_landmarks(pts, 24)
    want = [fa.flood_complex(pts, lms, point_weights=w[:, c].contiguous(), **kw) for c in range(n_cols)]
    sweeps = _counted(monkeypatch, "flooder_sweep_power_profile_f32", lambda b, n_cols, *rest: (int(n_cols), int(b.R), int(b.n_simplices)))
    index = core.PointIndex(pts)
    passes = _counted_passes(monkeypatch)
    for workspace, idx in ((core.PROFILE_WORKSPACE_BYTES, None), (4 * 8 * 40 * 7, index)):   # (the whole pass, then groups)
        monkeypatch.setattr(core, "PROFILE_WORKSPACE_BYTES", workspace)
        del sweeps[:], passes[:]
        prof = fa.power_profile(pts, lms, w, index=idx, **kw)
        assert prof.columns == tuple((c, "power") for c in range(n_cols))
        for c in range(n_cols):
            assert prof[c] == want[c], c
        if n_cols == 1:
            assert sweeps == []                      # one column: the single sweep itself
            continue
        # one profile sweep per dimension pass, column group and simplex group
        sizes = {}
        for m, R, S_g in sweeps:
            sizes.setdefault((m, R), []).append(S_g)
        col_groups = [8, n_cols - 8] if n_cols > 8 else [n_cols]
        n_simplices = {}
        for key in want[0]:
            n_simplices[len(key) - 1] = n_simplices.get(len(key) - 1, 0) + 1
        # (a lattice pass delivers the faces of its simplices as well: the passes are fewer than the dimensions)
        assert sorted({m for m, _ in sizes}) == sorted(set(col_groups))
        assert len(sizes) == len(col_groups) * len(passes) and 1 <= len(passes) <= md + 1
        for (m, R), got in sizes.items():
            S = sum(got)
            per = max(1, min(S, workspace // (4 * m * R)))
            assert got == [per] * (S // per) + ([S % per] if S % per else []), (m, R, got)
            assert S in n_simplices.values()
        if idx is not None:
            assert max(len(got) for got in sizes.values()) >= 2      # the small workspace did cut the passes
    # drawn samples under a seed, integer landmarks, simplex trees
    torch.manual_seed(5)
    prof = fa.power_profile(pts, 20, w, max_dimension=2, num_rand=70, start_idx=3, return_simplex_tree=True)
    for c in range(n_cols):
        torch.manual_seed(5)
        _same_result(prof[c], fa.flood_complex(pts, 20, max_dimension=2, num_rand=70, start_idx=3,
                                               return_simplex_tree=True, point_weights=w[:, c].contiguous()))


@pytest.mark.parametrize("dim", DIMS)
def test_dtm_profile_columns_are_the_recipe(dim, monkeypatch):
    pts = _cloud(5000, dim, 3 * dim)
    masses = (0.002, 0.013, 0.04)
    md = min(dim, 3)
    kw = dict(max_dimension=md, points_per_edge=8)
    wide = _counted(monkeypatch, "flooder_knn_wide_profile_f32", lambda b, *rest: (int(b.n_simplices), int(b.k)))
    sweeps = _counted(monkeypatch, "flooder_sweep_power_profile_f32", lambda b, n_cols, *rest: int(n_cols))
    passes = _counted_passes(monkeypatch)
    built = []
    real_init = core.PointIndex.__init__
    monkeypatch.setattr(core.PointIndex, "__init__", lambda self, *a, **k: built.append(1) or real_init(self, *a, **k))
    prof = fa.dtm_profile(pts, 24, masses, neighbor_stat=("dtm", "kth"), **kw)
    built_by_profile = list(built)
    ks = [core.mass_neighbors(m, 5000) for m in masses]
    assert ks == [10, 65, 200]
    assert prof.columns == tuple((k, s) for k in ks for s in ("dtm", "kth"))
    assert prof.masses == tuple(m for m in masses for _ in range(2))
    # ONE index for the weights, the landmark selection and the sweep; ONE wide walk; one sweep per dimension pass
    assert built_by_profile == [1] and wide == [(5000, 200)] and sweeps == [6] * len(passes) and passes
    for k, s in prof.columns:
        w = fa.distance_to_measure(pts, neighbors=k, neighbor_stat=s)
        assert prof[(k, s)] == fa.flood_complex(pts, 24, point_weights=w, **kw), (k, s)
    index = core.PointIndex(pts)
    lms = fa.generate_landmarks(pts, 16, index=index)
    prof = fa.dtm_profile(pts, lms, neighbors=(5, 300), max_dimension=1, points_per_edge=8, index=index)
    assert prof.columns == ((5, "dtm"), (300, "dtm")) and prof.masses is None
    w = fa.distance_to_measure(pts, neighbors=300, index=index)
    assert prof[1] == fa.flood_complex(pts, lms, max_dimension=1, points_per_edge=8, point_weights=w, index=index)
