"""The robust filtration's statistic at arbitrary query points: the k-distance and the distance to the empirical measure.

``flood_complex(neighbors=k)`` evaluates these only at lattice samples of Delaunay simplices.  ``neighbor_distance``
evaluates them at the cloud's own points (an outlier score before landmark selection - farthest-point sampling picks
stray points first) or at any other points (a function on a grid).  ROCm tensors run the k-nearest sweep over sorted
tiles (``flooder_sweep_knn_sorted_f32`` in its query form: every query is a "simplex" of one vertex with one sample).
"""

from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _native, core


def _check_queries(queries: torch.Tensor, points: torch.Tensor) -> None:
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != points.shape[1]:
        got = tuple(queries.shape) if isinstance(queries, torch.Tensor) else type(queries).__name__
        raise RuntimeError(f"queries must be a (Q, {points.shape[1]}) tensor, got {got}")
    if queries.device != points.device:
        raise RuntimeError(f"queries.device ({queries.device}) != points.device ({points.device})")
    if queries.dtype != points.dtype:
        raise RuntimeError(f"queries.dtype ({queries.dtype}) != points.dtype ({points.dtype})")


def neighbor_distance(points: torch.Tensor, queries: Optional[torch.Tensor] = None, neighbors: int = 1,
                      neighbor_stat: str = "kth", *, squared: bool = False,
                      index: Optional[core.PointIndex] = None) -> torch.Tensor:
    """Per query the k-distance or the distance to the empirical measure of ``points`` -> (Q,) tensor of ``points``'
    dtype on its device.

    ``neighbor_stat="kth"``: d_(k), the distance to the k-th nearest point of ``points``; ``"dtm"``:
    sqrt(mean of d_(1)^2 .. d_(k)^2) with k = ``neighbors`` (1..32, at most the number of points).  A point that occurs
    twice counts twice - the convention of ``flood_complex(neighbors=k)``, whose vertex values are
    ``neighbor_distance(points, landmarks, k, stat)``.  ``squared=True`` returns the statistic before the root.

    ``queries``: (Q, d) on the device of ``points`` and of its dtype; they must be finite (not checked on the device).
    ``None``: the cloud's own points, in input order.  A point of the cloud is its own nearest neighbour (k = 1 gives
    0): pass ``neighbors=k + 1`` to leave it out.  Q = 0 gives an empty tensor.

    CPU tensors (float32, float64; any dimension) query scipy's kd-tree.  ROCm tensors must be float32 in 2 to 8
    dimensions (``ValueError`` otherwise: the k-nearest sweep has no float64 kernel); ``index``: a ``PointIndex`` of
    these very points (as for ``flood_complex``), else one is built - or recalled, in ``INDEX_CACHE`` mode.  Only the
    argument checks synchronise with the host.
    """
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[0] == 0:
        got = tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__
        raise RuntimeError(f"points must be a non-empty (N, d) tensor, got shape {got}")
    if points.dtype not in core.SUPPORTED_DTYPES:
        raise TypeError(f"dtype ({points.dtype}) not supported")
    if points.device.type not in ("cuda", "cpu"):
        raise RuntimeError("Device not supported.")
    on_gpu = points.is_cuda
    if on_gpu and points.dtype is torch.float64:
        raise ValueError("neighbor_distance on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel")
    if on_gpu and not 2 <= points.shape[1] <= 8:
        raise ValueError("neighbor_distance on ROCm tensors needs ambient dimension 2 to 8")
    neighbors, _ = core._check_neighbors(points, neighbors, neighbor_stat, None)
    if queries is None:
        queries = points
    else:
        _check_queries(queries, points)
    if index is not None:
        core._check_index(index, points, on_gpu, "ROCm tensors")
    if queries.shape[0] == 0:
        return torch.empty(0, dtype=points.dtype, device=points.device)
    if on_gpu:
        return _neighbor_distance_hip(points, queries, neighbors, neighbor_stat, squared, index)

    from scipy.spatial import KDTree

    dist, _ = KDTree(np.asarray(points.detach())).query(np.asarray(queries.detach()), k=neighbors,
                                                         workers=core.CPU_WORKERS)
    dist = np.asarray(dist).reshape(queries.shape[0], neighbors)     # (Q, k) ascending (scipy drops the axis at k = 1)
    if squared:
        d2 = np.square(dist.astype(np.float64))
        val = d2[:, -1] if neighbor_stat == "kth" else d2.sum(axis=1) / neighbors
    else:
        val = core._robust_stat(dist, neighbors, neighbor_stat)
    return torch.as_tensor(np.ascontiguousarray(val)).to(points.dtype)


def _neighbor_distance_hip(points: torch.Tensor, queries: torch.Tensor, k: int, stat: str, squared: bool,
                           index: Optional[core.PointIndex]) -> torch.Tensor:
    """Keys of the queries inside the cloud's box (queries outside it get clamped keys: order only) -> radix sort ->
    ``flooder_sweep_knn_sorted_f32`` with k1 = R = 1 (fma(1.0f, q, 0.0f) is q) -> square root by
    ``flooder_face_values_f32``, the root of the dimension pass's face epilogue.  Groups of queries keep the keys, the
    orders and the sort's scratch (24 B per query) within ``core.SORTED_WORKSPACE_BYTES``."""
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    if index is None:
        index = core._recall_index(points)
        if index is None:
            index = core.PointIndex(points)
            core._remember_index(points, index)
    q = queries.detach().contiguous()
    Q, dim = q.shape
    one = torch.ones((1, 1), dtype=torch.float32, device=dev)
    bits = torch.empty(Q, dtype=torch.int32, device=dev)
    key_bits = int(lib.flooder_sample_key_bits(dim))
    per_group = max(1, min(Q, int(core.SORTED_WORKSPACE_BYTES) // 24, (1 << 32) - 3))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        verts = q[a:b].unsqueeze(1)                  # (b - a, 1, dim): one vertex per "simplex"
        queue, sort_state = core._zeroed_queue(lib, dev, b - a)
        order = core._sorted_sample_order(lib, st, index, verts, one, sort_state, None, key_bits)
        blk = _native.KnnSorted(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=1, nodes=index.nodes, verts=verts,
                                weights=one, R=1, k=k, n_simplices=b - a, stat=core.NEIGHBOR_STATS.index(stat),
                                queue=queue, out_bits=bits[a:b], sample_order=order)
        _native.check(lib.flooder_sweep_knn_sorted_f32(ctypes.byref(blk), st), "flooder_sweep_knn_sorted_f32")
    if squared:
        return bits.view(torch.float32)
    out = torch.empty(Q, dtype=torch.float32, device=dev)
    _native.check(lib.flooder_face_values_f32(_native.ptr(bits), Q, _native.ptr(out), st), "flooder_face_values_f32")
    return out
