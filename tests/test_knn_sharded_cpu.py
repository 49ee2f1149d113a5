"""The robust filtration over point shards, the parts that need no GPU: the parameter block of
``flooder_knn_merge_f32`` against the header, the declaration, the CPU refusal of ``neighbor_reduce_hook`` - and the
exactness argument itself, on numpy: the k smallest of the union of every shard's k smallest squared distances are the
k smallest over the whole cloud (``KDTree.query(k)``), for interleaved and for spatial partitions."""

import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.spatial import KDTree

import flooder_amd as fa
from flooder_amd import _native, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_merge_block_has_the_layout_of_the_header():
    """(size and offsets against the header: test_host.py, test_parameter_block_has_the_layout_of_the_header)"""
    cls = _native.KnnMerge
    blk = cls(n_cells=7, n_lists=3, k=5, stat=1)
    assert blk.size == ctypes.sizeof(cls) and blk.abi == 1 and (blk.n_cells, blk.n_lists, blk.k, blk.stat) == (7, 3, 5, 1)
    assert not blk.lists and not blk.out_bits
    with pytest.raises(TypeError):
        cls(no_such_field=1)


def test_knn_merge_is_declared_exported_and_listed_for_the_build():
    from flooder_amd import build

    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "flooder_knn_merge_f32(const flooder_knn_merge_t* p, void* stream)" in header
    res, args = _native.SIGNATURES["flooder_knn_merge_f32"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_native.KnnMerge), ctypes.c_void_p]
    assert "flood_knn_merge.hip" in build.HIP_SOURCES
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "flooder_knn_merge_f32")


def test_knn_merge_refuses_a_foreign_block_without_a_device():
    lib = _native.load()
    for change in (dict(abi=2), dict(size=ctypes.sizeof(_native.KnnMerge) + 8)):
        blk = _native.KnnMerge(n_cells=4, n_lists=2, k=2)
        for f, v in change.items():
            setattr(blk, f, v)
        assert lib.flooder_knn_merge_f32(ctypes.byref(blk), None) == -1
    for k in (0, 33):
        assert lib.flooder_knn_merge_f32(ctypes.byref(_native.KnnMerge(n_cells=4, n_lists=2, k=k)), None) == -1


def test_neighbor_reduce_hook_on_cpu_tensors_is_refused():
    g = torch.Generator().manual_seed(1)
    pts = torch.rand(100, 3, generator=g)

    def hook(lists):
        return lists[None]

    with pytest.raises(ValueError, match="neighbor_reduce_hook needs ROCm tensors"):
        fa.flood_complex(pts, pts[:8].clone(), points_per_edge=4, neighbors=3, neighbor_reduce_hook=hook)
    with pytest.raises(ValueError, match="neighbor_reduce_hook needs neighbors > 1"):
        fa.flood_complex(pts, pts[:8].clone(), points_per_edge=4, neighbor_reduce_hook=hook)
    # the hook lifts "k <= points of this shard" and nothing else of the k > 1 rules
    with pytest.raises(ValueError, match="exceeds the number of points"):
        core._check_neighbors(pts[:2], 3, "kth", None)
    with pytest.raises(ValueError, match="needs ROCm tensors"):
        core._check_neighbors(pts[:2], 3, "kth", None, neighbor_reduce_hook=hook)
    assert core.KNN_MERGE_WORKSPACE_BYTES == core.PROFILE_WORKSPACE_BYTES


def _merge_model(lists, k):
    """numpy model of flooder_knn_merge_f32's selection: (W, n, k) ascending lists -> the k smallest of each cell's
    W * k values, ascending.  Values only - no ids, no tie rule."""
    W, n, _ = lists.shape
    return np.sort(lists.transpose(1, 0, 2).reshape(n, W * k), axis=1)[:, :k]


@pytest.mark.parametrize("partition", ["interleaved", "spatial"])
@pytest.mark.parametrize("dim,n,W,k", [(2, 400, 2, 5), (3, 1000, 3, 8), (3, 90, 4, 32), (6, 700, 5, 17)])
def test_k_best_of_the_shards_k_best_is_the_k_best_of_the_cloud(dim, n, W, k, partition):
    rng = np.random.default_rng(dim * 1000 + n)
    P = rng.random((n, dim))
    P[n // 2:n // 2 + n // 10] = P[:n // 10]          # doubled points: they count twice
    Q = rng.random((300, dim))
    want = KDTree(P).query(Q, k=k)[0] ** 2             # (300, k) ascending, over the whole cloud
    if partition == "interleaved":
        shards = [P[r::W] for r in range(W)]
    else:
        order = np.argsort(P[:, 0])
        shards = [P[order[n * r // W:n * (r + 1) // W]] for r in range(W)]
    lists = np.full((W, Q.shape[0], k), np.inf)
    for w, sh in enumerate(shards):
        kl = min(k, sh.shape[0])                        # a shard smaller than k: its list ends in +inf
        d = KDTree(sh).query(Q, k=kl)[0] ** 2
        lists[w, :, :kl] = d.reshape(Q.shape[0], kl)
    if k == 32:
        assert all(sh.shape[0] < k for sh in shards)
    got = _merge_model(lists, k)
    assert np.array_equal(got, want)
    perm = rng.permutation(W)
    assert np.array_equal(_merge_model(lists[perm], k), want)
