"""Neighbour profile on the CPU path: ``flood_profile`` against one ``flood_complex`` call per column (equal dicts, equal
tree arrays), its table, the validation, the ABI of ``flooder_sweep_knn_profile_f32``'s parameter block, the entry
point's refusals (no device needed) and the CLI flags of the robust filtration."""

import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, cli, core, profile

from helpers import header_numbers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 3, 8, 17, 32)
STATS = ("kth", "dtm")


def _cloud(dim, n, dtype, seed=0, doubled=False):
    g = torch.Generator().manual_seed(seed + 10 * dim)
    pts = torch.rand(n, dim, generator=g, dtype=torch.float64).to(dtype)
    if doubled:
        pts = torch.cat([pts, pts[: n // 3]])[torch.randperm(n + n // 3, generator=g)]
    return pts.contiguous()


# (dim, points, landmarks, points_per_edge, max_dimension)
CONTRACT_CASES = [(2, 2000, 30, 8, None), (3, 600, 14, 5, None), (3, 1500, 20, 6, 2), (5, 300, 12, 5, 2)]


# ------------------------------------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dim,n,n_lms,ppe,max_dim", CONTRACT_CASES)
def test_every_column_is_the_single_call(dim, n, n_lms, ppe, max_dim, dtype):
    pts = _cloud(dim, n, dtype, doubled=(dim == 3 and n == 600))
    lms = fa.generate_landmarks(pts, n_lms, start_idx=0)
    prof = fa.flood_profile(pts, lms, max_dim, ppe, neighbors=KS, neighbor_stat=STATS)
    assert prof.columns == tuple((k, s) for k in KS for s in STATS) and len(prof) == 12
    for i, (k, s) in enumerate(prof.columns):
        want = fa.flood_complex(pts, lms, max_dim, ppe, neighbors=k, neighbor_stat=s)
        assert prof[(k, s)] == want, (k, s)
        assert prof[i] is prof[(k, s)]
    assert prof[-1] is prof[(32, "dtm")]
    with pytest.raises(KeyError):
        prof[(4, "kth")]
    with pytest.raises(IndexError):
        prof[12]


def test_integer_landmarks_one_statistic_and_start_idx():
    pts = _cloud(3, 500, torch.float32, seed=2)
    prof = fa.flood_profile(pts, 15, None, 5, None, 7, neighbors=(5, 2), neighbor_stat="dtm")
    assert prof.columns == ((5, "dtm"), (2, "dtm"))
    for k, s in prof.columns:
        assert prof[(k, s)] == fa.flood_complex(pts, 15, None, 5, None, start_idx=7, neighbors=k, neighbor_stat=s)
    one = fa.flood_profile(pts, 15, points_per_edge=5, neighbors=3)               # an int: one column
    assert one.columns == ((3, "kth"),)
    assert one[0] == fa.flood_complex(pts, 15, points_per_edge=5, neighbors=3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_num_rand_under_the_same_seed(dtype):
    pts = _cloud(3, 800, dtype, seed=3)
    lms = fa.generate_landmarks(pts, 16, start_idx=0)
    torch.manual_seed(17)
    prof = fa.flood_profile(pts, lms, points_per_edge=None, num_rand=30, neighbors=(1, 4, 32), neighbor_stat=STATS)
    for k, s in prof.columns:
        torch.manual_seed(17)
        assert prof[(k, s)] == fa.flood_complex(pts, lms, points_per_edge=None, num_rand=30, neighbors=k, neighbor_stat=s)


def test_simplex_trees_hold_equal_arrays():
    pts = _cloud(3, 700, torch.float32, seed=4)
    lms = fa.generate_landmarks(pts, 18, start_idx=0)
    prof = fa.flood_profile(pts, lms, points_per_edge=6, neighbors=(1, 8, 17), neighbor_stat=STATS, return_simplex_tree=True)
    for k, s in prof.columns:
        want = fa.flood_complex(pts, lms, points_per_edge=6, neighbors=k, neighbor_stat=s, return_simplex_tree=True)
        got = prof[(k, s)]
        assert isinstance(got, fa.SimplexTree) and got.num_simplices() == want.num_simplices()
        for d in range(4):
            assert np.array_equal(got.simplices_of_dimension(d), want.simplices_of_dimension(d))
            assert np.array_equal(got.filtrations_of_dimension(d), want.filtrations_of_dimension(d))
    # the trees do not share their values
    a, b = prof[(8, "kth")], prof[(17, "kth")]
    assert not np.array_equal(a.filtrations_of_dimension(3), b.filtrations_of_dimension(3))


def test_a_profile_of_k_one_is_flood_complex_itself(monkeypatch):
    pts = _cloud(3, 400, torch.float32)
    lms = fa.generate_landmarks(pts, 15, start_idx=0)
    base = fa.flood_complex(pts, lms, points_per_edge=5)
    calls = []
    real = core.flood_complex
    monkeypatch.setattr(core, "flood_complex", lambda *a, **kw: calls.append(kw) or real(*a, **kw))
    prof = fa.flood_profile(pts, lms, points_per_edge=5, neighbors=1, neighbor_stat=STATS)
    assert len(calls) == 2 and prof.columns == ((1, "kth"), (1, "dtm"))
    assert prof[0] == base and prof[(1, "dtm")] == base
    simp, vals = prof.table(2)
    assert vals.shape == (simp.shape[0], 2) and [base[tuple(r)] for r in simp.tolist()] == vals[:, 0].tolist()


# ------------------------------------------------------------------------------------------------ 2. table(d)
def test_table_agrees_with_the_columns_and_grows_with_k():
    pts = _cloud(3, 900, torch.float32, seed=6)
    lms = fa.generate_landmarks(pts, 20, start_idx=0)
    ks = (1, 2, 3, 5, 8, 16, 32)
    prof = fa.flood_profile(pts, lms, points_per_edge=6, neighbors=ks, neighbor_stat=STATS)
    total = 0
    for d in range(4):
        simp, vals = prof.table(d)
        assert simp.dtype == np.int64 and simp.shape[1] == d + 1 and vals.dtype == np.float64
        assert vals.shape == (simp.shape[0], len(prof.columns)) and simp.shape[0] > 0
        total += simp.shape[0]
        for c, col in enumerate(prof.columns):
            fc = prof[col]
            assert [fc[tuple(r)] for r in simp.tolist()] == vals[:, c].tolist()
        # d_(k) and the mean of the k smallest grow with k; maxima and the monotone pass keep the order
        for s in STATS:
            cols = [prof.columns.index((k, s)) for k in ks]
            assert (np.diff(vals[:, cols], axis=1) >= 0).all(), (d, s)
        assert (vals[:, prof.columns.index((32, "dtm"))] <= vals[:, prof.columns.index((32, "kth"))]).all()
    assert total == len(prof[0])


# ------------------------------------------------------------------------------------------------ 3. validation
def test_refusals_come_before_any_work(monkeypatch):
    pts = _cloud(3, 40, torch.float32)

    def no_work(*a, **kw):
        raise AssertionError("work was done before the arguments were validated")

    monkeypatch.setattr(core, "generate_landmarks", no_work)
    monkeypatch.setattr(core, "_build_complex", no_work)
    monkeypatch.setattr(core, "flood_complex", no_work)
    monkeypatch.setattr(profile, "delaunay_cells", no_work)
    for bad in ((), []):
        with pytest.raises(ValueError, match="neighbors"):
            fa.flood_profile(pts, 10, neighbors=bad)
    for bad in ((2, 2), (1, 8, 1), [4, 5, 4]):
        with pytest.raises(ValueError, match="twice"):
            fa.flood_profile(pts, 10, neighbors=bad)
    for bad in (0, 33, (2, 0), (33, 2), 41):
        with pytest.raises(ValueError, match="neighbors must be in 1..32"):
            fa.flood_profile(pts, 10, neighbors=bad)
    for bad in (2.0, True, (2, 2.0), (True, 2), "2", None):
        with pytest.raises(TypeError, match="integer"):
            fa.flood_profile(pts, 10, neighbors=bad)
    for bad in ("mean", ("kth", "mean"), ()):
        with pytest.raises(ValueError, match="neighbor_stat"):
            fa.flood_profile(pts, 10, neighbors=(1, 2), neighbor_stat=bad)
    with pytest.raises(ValueError, match="twice"):
        fa.flood_profile(pts, 10, neighbors=(1, 2), neighbor_stat=("kth", "kth"))
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match="nearest point only"):
            fa.flood_profile(pts, 10, neighbors=(1, 2), method=method)
    with pytest.raises(ValueError, match="method must be"):
        fa.flood_profile(pts, 10, neighbors=(1, 2), method="octree")
    with pytest.raises(ValueError, match="number of points"):
        fa.flood_profile(pts[:20], 10, neighbors=(2, 21))


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_knn_profile_block_has_the_layout_of_the_header(tmp_path):
    """(size and offsets against the header: test_host.py, test_parameter_block_has_the_layout_of_the_header)"""
    cname, cls = "flooder_knn_profile_t", _native.KnnProfile
    out = header_numbers(tmp_path, extra={"cols_max": "FLOODER_KNN_COLS_MAX", "col_k": f"sizeof((({cname}*)0)->col_k)",
                                          "col_stat": f"sizeof((({cname}*)0)->col_stat)"})
    assert out["cols_max"] == _native.KNN_COLS_MAX == 64
    assert out["col_k"] == 4 * 64 == cls.col_k.size and out["col_stat"] == 4 * 64 == cls.col_stat.size
    names = {f for f, _ in cls._fields_}
    single = {f for f, _ in _native.KnnSweep._fields_}
    # the single sweep's fields without k and stat (and its padding word), the column list in their place
    assert names == (single - {"k", "stat", "reserved"}) | {"n_cols", "col_k", "col_stat"}
    blk = cls([(8, 0), (3, 1), (32, 0)], n_pts=7, R=3)
    assert blk.size == ctypes.sizeof(cls) and blk.abi == 1 and (blk.n_pts, blk.R, blk.n_cols) == (7, 3, 3)
    assert list(blk.col_k[:4]) == [8, 3, 32, 0] and list(blk.col_stat[:4]) == [0, 1, 0, 0]
    assert not blk.out_bits
    with pytest.raises(TypeError):
        cls(no_such_field=1)
    with pytest.raises(ValueError):
        cls([(1, 0)] * 65)


def test_knn_profile_is_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "flooder_sweep_knn_profile_f32(" in header and "#define FLOODER_KNN_COLS_MAX 64" in header
    res, args = _native.SIGNATURES["flooder_sweep_knn_profile_f32"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_native.KnnProfile), ctypes.c_void_p]
    from flooder_amd import build
    assert "flood_knn.hip" in build.HIP_SOURCES
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "flooder_sweep_knn_profile_f32")
    assert core.PROFILE_WORKSPACE_BYTES == core.SORTED_WORKSPACE_BYTES
    assert fa.flood_profile is profile.flood_profile and "flood_profile" in fa.__all__


def test_knn_profile_refuses_foreign_blocks_and_bad_columns():
    """Every refusal returns before a pointer is looked at or a kernel is launched (no device needed)."""
    lib = _native.load()
    call = lambda blk: lib.flooder_sweep_knn_profile_f32(ctypes.byref(blk), None)
    good = dict(n_pts=100, dim=3, k1=4, R=10, n_simplices=0)
    cols = [(8, 0), (8, 1), (1, 0), (32, 1)]
    assert call(_native.KnnProfile(cols, **good)) == 0             # nothing to sweep: accepted, nothing launched
    assert call(_native.KnnProfile(cols, **{**good, "n_simplices": 4, "R": 0})) == 0
    assert call(_native.KnnProfile([(k, s) for k in range(1, 33) for s in (0, 1)], **good)) == 0   # all 64 columns
    for mutate in (lambda b: setattr(b, "abi", 2), lambda b: setattr(b, "size", ctypes.sizeof(b) + 8),
                   lambda b: setattr(b, "size", 4)):
        blk = _native.KnnProfile(cols, **good)
        mutate(blk)
        assert call(blk) != 0 and b"abi / size" in lib.flooder_last_error()
    for n_cols in (0, -1, 65):
        blk = _native.KnnProfile(cols, **good)
        blk.n_cols = n_cols
        assert call(blk) != 0 and b"n_cols must be in 1..64" in lib.flooder_last_error()
    for k in (0, -1, 33):
        assert call(_native.KnnProfile([(2, 0), (k, 0)], **good)) != 0
        assert b"col_k must be in 1..32" in lib.flooder_last_error()
    for stat in (2, -1):
        assert call(_native.KnnProfile([(2, 0), (3, stat)], **good)) != 0
        assert b"col_stat" in lib.flooder_last_error()
    assert call(_native.KnnProfile([(2, 0), (3, 1), (2, 0)], **good)) != 0
    assert b"listed twice" in lib.flooder_last_error()
    assert call(_native.KnnProfile([(2, 0), (2, 1)], **good)) == 0          # the same k with the other statistic is fine
    for dim in (0, 1, 9):
        assert call(_native.KnnProfile(cols, **{**good, "dim": dim})) != 0
        assert b"dim must be in 2..8" in lib.flooder_last_error()
    assert call(_native.KnnProfile(cols, **{**good, "n_pts": 31})) != 0
    assert b"fewer points than the largest k" in lib.flooder_last_error()
    assert call(_native.KnnProfile(cols, **{**good, "n_simplices": 5})) != 0   # null pointers with work to do


# ------------------------------------------------------------------------------------------------ 5. CLI
def test_cli_flags_reach_flood_complex(tmp_path, monkeypatch):
    pts = fa.generate_noisy_torus_points_3d(400, seed=0).numpy()
    path = tmp_path / "cloud.npy"
    np.save(path, pts.astype(np.float32))
    a = cli.build_parser().parse_args(["--input-file", "x.npy"])
    assert (a.neighbors, a.neighbor_stat) == (1, "kth")                    # the call as it was
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--input-file", "x.npy", "--neighbor-stat", "mean"])
    seen = []
    real = fa.flood_complex
    monkeypatch.setattr(fa, "flood_complex", lambda *a, **kw: seen.append(kw) or real(*a, **kw))
    out = tmp_path / "robust.pkl"
    rc = cli.main(["--input-file", str(path), "--num-landmarks", "40", "--points-per-edge", "6", "--device", "cpu",
                   "--output-file", str(out), "--max-dimension", "2", "--neighbors", "3", "--neighbor-stat", "dtm"])
    assert rc == 0 and len(seen) == 1 and (seen[0]["neighbors"], seen[0]["neighbor_stat"]) == (3, "dtm")
    payload = pickle.load(open(out, "rb"))
    assert (payload["meta"]["neighbors"], payload["meta"]["neighbor_stat"]) == (3, "dtm")
    st = real(torch.from_numpy(pts), 40, max_dimension=2, points_per_edge=6, return_simplex_tree=True, neighbors=3,
              neighbor_stat="dtm")
    st.compute_persistence()
    plain = real(torch.from_numpy(pts), 40, max_dimension=2, points_per_edge=6, return_simplex_tree=True)
    plain.compute_persistence()
    for d in range(2):
        want = np.asarray(st.persistence_intervals_in_dimension(d)).reshape(-1, 2)
        got = np.asarray(payload["diagrams"][d]).reshape(-1, 2)
        assert np.array_equal(np.sort(got, axis=0), np.sort(want, axis=0))
    assert not np.array_equal(np.asarray(plain.persistence_intervals_in_dimension(1)),
                              np.asarray(st.persistence_intervals_in_dimension(1)))
    # without the flags: neighbors=1, the plain filtration
    rc = cli.main(["--input-file", str(path), "--num-landmarks", "40", "--points-per-edge", "6", "--device", "cpu",
                   "--max-dimension", "2"])
    assert rc == 0 and (seen[1]["neighbors"], seen[1]["neighbor_stat"]) == (1, "kth")
    with pytest.raises(ValueError, match="neighbors must be in 1..32"):
        cli.main(["--input-file", str(path), "--num-landmarks", "40", "--device", "cpu", "--neighbors", "33"])
