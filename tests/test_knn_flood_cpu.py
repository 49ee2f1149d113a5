"""Robust filtration on the CPU path: ``flood_complex(neighbors=k, neighbor_stat=...)`` against a float64 brute force
over all points (``torch.cdist`` + ``topk``), the order relations between the statistics, the annulus with outliers,
the refusals, and the ABI of ``flooder_sweep_knn_f32``'s parameter block."""

import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from flooder_amd.persistence import persistence_pairs
from flooder_amd.synthetic import generate_annulus_points_2d

from helpers import assert_close_filtration, header_numbers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ brute force
def brute_statistic(points: torch.Tensor, samples: torch.Tensor, k: int, stat: str) -> torch.Tensor:
    """Per row of ``samples``: the distance to the k-th nearest point (``kth``) or the root of the mean of the k
    smallest squared distances (``dtm``), float64, over ALL points (a point that occurs twice counts twice)."""
    d = torch.cdist(samples.double(), points.double(), compute_mode="donot_use_mm_for_euclid_dist")
    small = torch.topk(d, k, dim=1, largest=False).values
    return small.max(dim=1).values if stat == "kth" else small.pow(2).mean(dim=1).sqrt()


def brute_filtration(fc, points, landmarks, k, stat, points_per_edge=None, weights_by_dim=None):
    """The value of every simplex of the dict ``fc`` from the brute force: the maximum of the statistic over the
    lattice of the simplex's own dimension (``core.generate_grid``) or over the drawn weights ``weights_by_dim[d]``,
    then the monotone pass over the faces (a no-op for lattices: a face's lattice is part of its coface's)."""
    by_dim = {}
    for key in fc:
        by_dim.setdefault(len(key) - 1, []).append(key)
    ref = {}
    for d in sorted(by_dim):
        keys = by_dim[d]
        if weights_by_dim is not None:
            w = weights_by_dim[d]
        elif d == 0:
            w = torch.ones((1, 1), dtype=points.dtype)     # a vertex is its own single sample
        else:
            w = core.generate_grid(points_per_edge, d, "cpu", points.dtype)[0]
        verts = landmarks.double()[torch.tensor(keys, dtype=torch.long)]            # (S, d+1, dim)
        samples = torch.einsum("rk,skd->srd", w.double(), verts)
        g = brute_statistic(points, samples.reshape(-1, points.shape[1]), k, stat).reshape(len(keys), -1)
        for key, v in zip(keys, g.max(dim=1).values.tolist()):
            for face in itertools.combinations(key, d) if d > 0 else ():
                v = max(v, ref[face])
            ref[key] = v
    return ref


def _cloud(dim, n, dtype, doubled=False, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * dim)
    pts = torch.rand(n, dim, generator=g, dtype=torch.float64).to(dtype)
    if doubled:
        pts = torch.cat([pts, pts])[torch.randperm(2 * n, generator=g)]
    return pts.contiguous()


N_LMS = {2: 14, 3: 12, 5: 10}


# ------------------------------------------------------------------------------------------------ 1. default unchanged
@pytest.mark.parametrize("stat", ["kth", "dtm"])
def test_one_neighbor_is_the_default_call(stat):
    pts = _cloud(3, 400, torch.float32)
    lms = fa.generate_landmarks(pts, 15, start_idx=0)
    assert fa.flood_complex(pts, lms, points_per_edge=5) == \
        fa.flood_complex(pts, lms, points_per_edge=5, neighbors=1, neighbor_stat=stat)
    torch.manual_seed(3)
    a = fa.flood_complex(pts, lms, points_per_edge=None, num_rand=20)
    torch.manual_seed(3)
    b = fa.flood_complex(pts, lms, points_per_edge=None, num_rand=20, neighbors=1, neighbor_stat=stat)
    assert a == b


# ------------------------------------------------------------------------------------------------ 2. brute force
@pytest.mark.parametrize("stat", ["kth", "dtm"])
@pytest.mark.parametrize("k", [2, 5, 32])
@pytest.mark.parametrize("mode", ["lattice", "num_rand"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dim", [2, 3, 5])
def test_cpu_values_match_the_brute_force(dim, dtype, mode, k, stat):
    pts = _cloud(dim, 300, dtype)
    lms = pts[:N_LMS[dim]].clone()
    _check_against_brute_force(pts, lms, mode, k, stat, f"{dim}-D {dtype} {mode} k={k} {stat}")


@pytest.mark.parametrize("stat", ["kth", "dtm"])
@pytest.mark.parametrize("k", [2, 5, 32])
@pytest.mark.parametrize("mode", ["lattice", "num_rand"])
def test_cpu_values_count_doubled_points_twice(mode, k, stat):
    pts = _cloud(3, 150, torch.float32, doubled=True)
    lms = torch.unique(pts, dim=0)[:12].clone()
    fc = _check_against_brute_force(pts, lms, mode, k, stat, f"doubled {mode} k={k} {stat}")
    if stat == "kth" and mode == "lattice":
        # every point twice: the 2j-th and the (2j-1)-th nearest are the same point
        single = torch.unique(pts, dim=0)
        if k == 2:
            assert fc == fa.flood_complex(single, lms, points_per_edge=4)
        odd = fa.flood_complex(pts, lms, points_per_edge=4, neighbors=k - 1 if k % 2 == 0 else k + 1)
        assert fc == odd


def _check_against_brute_force(pts, lms, mode, k, stat, what):
    dim = pts.shape[1]
    if mode == "lattice":
        fc = fa.flood_complex(pts, lms, points_per_edge=4, neighbors=k, neighbor_stat=stat)
        ref = brute_filtration(fc, pts, lms, k, stat, points_per_edge=4)
    else:
        torch.manual_seed(11)
        fc = fa.flood_complex(pts, lms, points_per_edge=None, num_rand=25, neighbors=k, neighbor_stat=stat)
        torch.manual_seed(11)    # the draws of the call, dimension by dimension, in its order
        present = sorted({len(key) - 1 for key in fc})
        assert present == list(range(dim + 1))
        weights = {d: core.generate_uniform_weights(25, d, "cpu", pts.dtype) for d in present}
        ref = brute_filtration(fc, pts, lms, k, stat, weights_by_dim=weights)
    keys = sorted(fc)
    assert len(keys) > 3 * lms.shape[0]
    assert_close_filtration([fc[key] for key in keys], [ref[key] for key in keys], pts.numpy(), what)
    return fc


# ------------------------------------------------------------------------------------------------ 3. order relations
def test_order_relations_between_the_statistics():
    pts = _cloud(3, 500, torch.float32, seed=5)
    lms = fa.generate_landmarks(pts, 20, start_idx=0)
    default = fa.flood_complex(pts, lms, points_per_edge=6)
    keys = sorted(default)
    prev = None
    for k in (1, 2, 3, 5, 8, 16, 32):
        kth = fa.flood_complex(pts, lms, points_per_edge=6, neighbors=k, neighbor_stat="kth")
        dtm = fa.flood_complex(pts, lms, points_per_edge=6, neighbors=k, neighbor_stat="dtm")
        assert sorted(kth) == keys and sorted(dtm) == keys
        a = np.array([kth[key] for key in keys])
        b = np.array([dtm[key] for key in keys])
        if k == 1:
            assert kth == default and dtm == default
        else:
            assert (a >= prev).all(), f"kth decreases from the previous k to k={k}"
            assert (a > prev).any()
        assert (b <= a).all(), f"dtm above kth at k={k}"
        prev = a


# ------------------------------------------------------------------------------------------------ 4. robustness
def _longest_h1(pts, **kw):
    st = fa.flood_complex(pts, 200, points_per_edge=20, start_idx=0, return_simplex_tree=True, **kw)
    if hasattr(st, "compute_persistence") and not isinstance(st, fa.SimplexTree):   # a gudhi tree
        st.compute_persistence()
        h1 = st.persistence_intervals_in_dimension(1)
    else:
        h1 = persistence_pairs(st).get(1, np.zeros((0, 2)))
    length = np.sort(h1[:, 1] - h1[:, 0])[::-1]
    return float(length[0]), length


def test_outliers_in_the_hole_of_an_annulus():
    clean = generate_annulus_points_2d(20000, radius=1.0, width=0.2, seed=0).to(torch.float32)
    g = torch.Generator().manual_seed(1)
    r = 0.7 * torch.sqrt(torch.rand(30, generator=g))
    t = 2 * math.pi * torch.rand(30, generator=g)
    dirty = torch.cat([clean, torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1).to(torch.float32)])
    l_clean, _ = _longest_h1(clean)
    l_dirty, _ = _longest_h1(dirty)
    l_robust, all_robust = _longest_h1(dirty, neighbors=32, neighbor_stat="kth")
    print(f"longest H1: clean {l_clean:.4f}, dirty k=1 {l_dirty:.4f} ({l_dirty / l_clean:.3f}), "
          f"dirty k=32 kth {l_robust:.4f} ({l_robust / l_clean:.3f}), next {all_robust[1:3]}")
    assert l_dirty <= 0.5 * l_clean
    assert l_robust >= 0.9 * l_clean


# ------------------------------------------------------------------------------------------------ 5. validation
def test_refusals_come_before_any_work(monkeypatch):
    pts = _cloud(3, 40, torch.float32)

    def no_work(*a, **kw):
        raise AssertionError("landmarks selected before the arguments were validated")

    monkeypatch.setattr(core, "generate_landmarks", no_work)
    monkeypatch.setattr(core, "_build_complex", no_work)
    assert core.KNN_MAX == 32
    for bad in (0, -1, 33, 41):                       # (41: also more than the 40 points)
        with pytest.raises(ValueError, match="neighbors"):
            fa.flood_complex(pts, 10, neighbors=bad)
    with pytest.raises(ValueError, match="number of points"):
        fa.flood_complex(pts[:20], 10, neighbors=21)
    for bad in (2.0, "2", None, True):
        with pytest.raises(TypeError, match="integer"):
            fa.flood_complex(pts, 10, neighbors=bad)
    for k in (1, 2):
        with pytest.raises(ValueError, match="neighbor_stat"):
            fa.flood_complex(pts, 10, neighbors=k, neighbor_stat="mean")
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match="nearest point only"):
            fa.flood_complex(pts, 10, neighbors=2, method=method)
    with pytest.raises(ValueError, match="reduce_hook"):
        fa.flood_complex(pts, 10, neighbors=2, reduce_hook=lambda t: None)
    with pytest.raises(ValueError, match="shard_blocks"):
        fa.flood_complex(pts, 10, neighbors=2, simplex_shard=(0, 2), shard_blocks=True)
    with pytest.raises(ValueError, match="method must be"):
        fa.flood_complex(pts, 10, neighbors=2, method="octree")


def test_simplex_shards_combine_to_the_unsharded_values_cpu():
    pts = _cloud(3, 300, torch.float32)
    lms = fa.generate_landmarks(pts, 14, start_idx=0)
    whole = fa.flood_complex(pts, lms, points_per_edge=5, neighbors=5, neighbor_stat="dtm")
    parts = []

    def collect(face):
        parts.append(face.clone())
        if len(parts) == 2:
            face.copy_(torch.minimum(parts[0], parts[1]))

    fa.flood_complex(pts, lms, points_per_edge=5, neighbors=5, neighbor_stat="dtm", simplex_shard=(0, 2),
                     face_reduce_hook=collect)
    both = fa.flood_complex(pts, lms, points_per_edge=5, neighbors=5, neighbor_stat="dtm", simplex_shard=(1, 2),
                            face_reduce_hook=collect)
    assert both == whole


# ------------------------------------------------------------------------------------------------ 6. ABI
def test_knn_sweep_block_has_the_layout_of_the_header(tmp_path):
    """(size and offsets against the header: test_host.py, test_parameter_block_has_the_layout_of_the_header)"""
    cls = _native.KnnSweep
    assert header_numbers(tmp_path, extra={"knn_max": "FLOODER_KNN_MAX"}) == {"knn_max": core.KNN_MAX}
    for needed in ("size", "abi", "pts_sorted", "n_pts", "dim", "nodes", "verts", "weights", "k1", "R", "n_simplices", "k",
                   "stat", "queue", "out_bits", "stats"):
        assert hasattr(cls, needed), needed
    blk = cls(n_pts=7, R=3, k=5, stat=1)
    assert blk.size == ctypes.sizeof(cls) and blk.abi == 1 and (blk.n_pts, blk.R, blk.k, blk.stat) == (7, 3, 5, 1)
    assert not blk.out_bits
    with pytest.raises(TypeError):
        cls(no_such_field=1)


def test_knn_sweep_is_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "flooder_sweep_knn_f32(" in header
    assert len(_native.SIGNATURES["flooder_sweep_knn_f32"][1]) == 2
    from flooder_amd import build
    assert "flood_knn.hip" in build.HIP_SOURCES
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "flooder_sweep_knn_f32")


def test_knn_sweep_refuses_foreign_blocks_and_bad_ranges():
    """Every refusal returns before a pointer is looked at or a kernel is launched (no device needed)."""
    lib = _native.load()
    call = lambda blk: lib.flooder_sweep_knn_f32(ctypes.byref(blk), None)
    good = dict(n_pts=100, dim=3, k1=4, R=10, n_simplices=0, k=8, stat=0)
    assert call(_native.KnnSweep(**good)) == 0                     # nothing to sweep: accepted, nothing launched
    blk = _native.KnnSweep(**good)
    blk.abi = 2
    assert call(blk) != 0
    blk = _native.KnnSweep(**good)
    blk.size = ctypes.sizeof(blk) + 8
    assert call(blk) != 0
    blk = _native.KnnSweep(**good)
    blk.size = 4
    assert call(blk) != 0
    for k in (0, -1, 33):
        assert call(_native.KnnSweep(**{**good, "k": k})) != 0
        assert b"k must be in 1..32" in lib.flooder_last_error()
    for dim in (0, 1, 9):
        assert call(_native.KnnSweep(**{**good, "dim": dim})) != 0
        assert b"dim must be in 2..8" in lib.flooder_last_error()
    assert call(_native.KnnSweep(**{**good, "stat": 2})) != 0
    assert call(_native.KnnSweep(**{**good, "n_simplices": 5})) != 0   # null pointers with work to do
