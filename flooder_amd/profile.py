"""Neighbour profile of the robust Flood filtration: every ``(k, stat)`` of a list from ONE pass over the samples.

``flood_profile(points, landmarks, ..., neighbors=(1, 2, 4, 8, 16, 32), neighbor_stat=("kth", "dtm"))`` returns, per
column ``(k, stat)``, what ``flood_complex(..., neighbors=k, neighbor_stat=stat)`` returns - the same dict, the same
simplex tree arrays - for the price of one call at the largest k: one landmark selection, one Delaunay complex, one
point index, one queue order and sample plan per dimension, and one tree sweep whose lanes end a tile with their
k_max smallest squared distances sorted in registers (``flooder_sweep_knn_profile_f32``, csrc/flood_knn.hip).  Every
``"kth"`` and ``"dtm"`` statistic with k' <= k_max is a function of those registers, so the planes it writes are, word
for word, the buffers of the single sweeps.  On CPU tensors one ``KDTree.query(k=k_max)`` serves all columns.

What a scan over k is for: choosing ``neighbors`` (README, "Choosing k").  Sharding, ``reduce_hook`` and gradients are
not part of this function (``flood_complex`` / ``flood_filtration`` with one k have them).
"""

from __future__ import annotations

import copy
from numbers import Integral
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native, core
from .simplex_tree import SimplexTree, delaunay_cells

Column = Tuple[int, str]


def _clone_tree(tree: SimplexTree) -> SimplexTree:
    """A tree over the same (shared, read-only) simplex tables with value arrays of its own."""
    out = copy.copy(tree)
    out._rows = dict(tree._rows)
    out._vals = {d: v.copy() for d, v in tree._vals.items()}
    out._pending = {}
    out._lazy = set(tree._lazy)
    out._cell_faces = dict(tree._cell_faces)
    out._persistence = None
    return out


class FloodProfile:
    """Result of ``flood_profile``.  ``columns``: ``((k, stat), ...)`` in the caller's order.  ``prof[(k, stat)]`` or
    ``prof[i]``: what ``flood_complex`` returns for that column (a dict, or a simplex tree when the profile was asked
    for with ``return_simplex_tree=True``).  ``table(d)``: the simplices of dimension d and their values in every
    column, after the monotone pass."""

    def __init__(self, columns: Sequence[Column], trees: Optional[List[SimplexTree]], results: Optional[list],
                 return_simplex_tree: bool):
        self.columns: Tuple[Column, ...] = tuple(columns)
        self._trees = trees          # one tree per column (values of their own, simplex tables shared) ...
        self._results = results      # ... or what flood_complex itself returned (largest k = 1, gudhi trees)
        self._as_tree = bool(return_simplex_tree)
        self._dicts: Dict[int, dict] = {}

    def __len__(self) -> int:
        return len(self.columns)

    def _position(self, key) -> int:
        if isinstance(key, Integral) and not isinstance(key, bool):
            if not -len(self.columns) <= key < len(self.columns):
                raise IndexError(f"column {key} out of range for {len(self.columns)} columns")
            return int(key) % len(self.columns)
        try:
            k, stat = key
            return self.columns.index((int(k), stat))
        except (TypeError, ValueError):
            raise KeyError(f"no column {key!r}; columns are {self.columns}") from None

    def __getitem__(self, key):
        c = self._position(key)
        if self._results is not None:
            return self._results[c]
        if self._as_tree:
            return self._trees[c]
        if c not in self._dicts:
            self._dicts[c] = self._trees[c].to_dict()
        return self._dicts[c]

    def __iter__(self):
        return iter(self.columns)

    def items(self):
        return ((col, self[i]) for i, col in enumerate(self.columns))

    def table(self, d: int) -> Tuple[np.ndarray, np.ndarray]:
        """``(simplices (n_d, d + 1) int64, values (n_d, n_cols) float64)`` of dimension ``d``: column c holds the
        final (non-decreasing) filtration values of ``columns[c]``, rows in the order of the simplex table."""
        if self._results is not None:
            trees = self._results if self._as_tree else None
            if trees is None or not all(isinstance(t, SimplexTree) for t in trees):
                # dicts (or foreign trees): rows in lexicographic order of the simplices
                dicts = [r if isinstance(r, dict) else dict((tuple(s), v) for s, v in r.get_simplices())
                         for r in self._results]
                keys = sorted(key for key in dicts[0] if len(key) == d + 1)
                simp = np.array(keys, dtype=np.int64).reshape(-1, d + 1)
                vals = np.array([[dc[key] for dc in dicts] for key in keys], dtype=np.float64).reshape(-1, len(dicts))
                return simp, vals
        else:
            trees = self._trees
        simp = np.asarray(trees[0].simplices_of_dimension(d), dtype=np.int64)
        vals = np.stack([np.asarray(t.filtrations_of_dimension(d), dtype=np.float64) for t in trees], axis=1)
        return simp, vals.reshape(simp.shape[0], len(trees))


def _check_columns(points: torch.Tensor, neighbors, neighbor_stat, method):
    """``neighbors`` (an int or a non-empty sequence of distinct ints) x ``neighbor_stat`` (a name or a non-empty
    sequence of distinct names), every k judged by ``core._check_neighbors`` with the call's ``method`` - the messages
    are ``flood_complex``'s -> (ks, stats, columns, method of the k > 1 columns)."""
    if isinstance(neighbors, (str, bytes)) or (not isinstance(neighbors, Integral) and not hasattr(neighbors, "__iter__")):
        raise TypeError(f"neighbors must be an integer or a sequence of integers, got {neighbors!r}")
    ks = [neighbors] if isinstance(neighbors, Integral) else list(neighbors)
    stats = [neighbor_stat] if isinstance(neighbor_stat, str) or not hasattr(neighbor_stat, "__iter__") else list(neighbor_stat)
    if not ks:
        raise ValueError("neighbors must not be empty")
    if not stats:
        raise ValueError("neighbor_stat must not be empty")
    knn_method = method
    checked = []
    for k in ks:
        for stat in stats:
            k_int, m = core._check_neighbors(points, k, stat, method)
            if k_int > 1:
                knn_method = m
        checked.append(k_int)
    if len(set(checked)) != len(checked):
        raise ValueError(f"neighbors lists a value twice: {ks!r}")
    if len(set(stats)) != len(stats):
        raise ValueError(f"neighbor_stat lists a name twice: {stats!r}")
    columns = [(k, s) for k in checked for s in stats]
    return checked, stats, columns, knn_method


def flood_profile(points: torch.Tensor, landmarks: Union[int, torch.Tensor], max_dimension: Optional[int] = None,
                  points_per_edge: Optional[int] = 30, num_rand: Optional[int] = None, start_idx: Optional[int] = 0, *,
                  neighbors=(1, 2, 4, 8, 16, 32), neighbor_stat="kth", return_simplex_tree: bool = False,
                  method: Optional[str] = None, index: Optional["core.PointIndex"] = None) -> FloodProfile:
    """The robust Flood filtration for every ``(k, stat)`` with k in ``neighbors`` and stat in ``neighbor_stat`` (a name
    or a sequence of names), from one pass: for every column,

        ``prof[(k, stat)] == flood_complex(points, landmarks, max_dimension, points_per_edge, num_rand,
        start_idx=start_idx, neighbors=k, neighbor_stat=stat, method=method, index=index,
        return_simplex_tree=return_simplex_tree)``

    exactly - ROCm and CPU tensors, the ``(1, *)`` columns (the plain filtration) included; with ``num_rand`` under
    the same seed of the global CPU generator (the weights of a dimension are drawn once and serve every column);
    with ``return_simplex_tree=True`` the per-dimension simplex and filtration arrays are equal.  ``columns`` is
    ``[(k, s) for k in neighbors for s in stats]``.

    Every k is judged as ``flood_complex`` judges it, before any work is done (1 <= k <= 32, k <= number of points; a
    k > 1 column needs the tree sweep: ROCm float32 in 2 to 8 dimensions, ``method`` None / "auto" / "bvh").  A profile
    whose largest k is 1 calls ``flood_complex`` itself.  On ROCm tensors the plane buffer of the sweep (4 bytes x
    columns x simplices x samples) is bounded by ``core.PROFILE_WORKSPACE_BYTES``; above it the simplices of a
    dimension are swept in groups."""
    ks, stats, columns, knn_method = _check_columns(points, neighbors, neighbor_stat, method)
    if max(ks) == 1:
        results = [core.flood_complex(points, landmarks, max_dimension, points_per_edge, num_rand, start_idx=start_idx,
                                      neighbors=k, neighbor_stat=s, method=method, index=index,
                                      return_simplex_tree=return_simplex_tree) for k, s in columns]
        return FloodProfile(columns, None, results, return_simplex_tree)
    method = knn_method
    if points.dim() != 2 or points.shape[0] == 0:
        raise RuntimeError(f"points must be a non-empty (N, d) tensor, got shape {tuple(points.shape)}")
    if method != "bvh":
        raise ValueError(f"method must be 'cell', 'bvh' or 'ball', got {method!r}")
    if points.dtype not in core.SUPPORTED_DTYPES:
        raise TypeError(f"dtype ({points.dtype}) not supported")
    if points.device.type not in ("cuda", "cpu"):
        raise RuntimeError("Device not supported.")
    on_gpu = points.is_cuda
    dim = points.shape[1]
    if max_dimension is None:
        max_dimension = dim
    if index is not None:
        core._check_index(index, points, on_gpu, "ROCm tensors")
    if on_gpu:
        _native.load()   # raises ImportError with the build hint: no fallback
        torch.cuda.set_device(points.device)
        if index is None:
            index = core._recall_index(points)
            if index is None:
                index = core.PointIndex(points.to(torch.float32))
                core._remember_index(points, index)
    if isinstance(landmarks, Integral):
        landmarks = core.generate_landmarks(points, min(int(landmarks), points.shape[0]), None, start_idx=start_idx,
                                            index=index)
    core._check_landmarks(landmarks, points)

    lm_host = landmarks.detach().cpu().numpy()
    tree, simplices = core._cell_complex(delaunay_cells(lm_host), lm_host.shape[0], max_dimension)
    # per column: the hand-off items of flood_complex, pass after pass
    items = [[] for _ in columns]
    if on_gpu:
        passes = core._dimension_passes(simplices, landmarks.detach().to(torch.float32), core._widest_axis(points, index.box),
                                        points_per_edge, num_rand, "tree")
    else:
        from scipy.spatial import KDTree

        kdtree = KDTree(np.asarray(points))
        k_max = max(ks)
        passes = core._dimension_passes(simplices, landmarks.detach(), core._widest_axis(points), points_per_edge,
                                        num_rand, "ball")
    for p in passes:
        if on_gpu:
            face_cols = core._sweep_dimension_knn_profile(index, p.verts, p.weights, p.faces, columns, plan=p.plan)
        else:
            samples = p.weights.unsqueeze(0) @ p.verts
            dist_all, _ = kdtree.query(np.asarray(samples), k=k_max, workers=core.CPU_WORKERS)   # (S, R, k_max), ascending
            # (scipy's k' nearest are the first k' of its k_max)
            face_cols = [core._face_max_cpu(torch.as_tensor(np.ascontiguousarray(
                dist_all[..., 0] if k == 1 else core._robust_stat(dist_all[..., :k], k, stat))), p.faces)
                for k, stat in columns]
        for c, face in enumerate(face_cols):
            items[c] += core._handoff_items(tree, p, face.cpu().numpy().astype(np.float64))
    trees = []
    for c in range(len(columns)):
        trees.append(_clone_tree(tree))
        core._apply_items(trees[c], items[c])
        trees[c].make_filtration_non_decreasing()
    return FloodProfile(columns, trees, None, return_simplex_tree)
