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


def power_profile(points: torch.Tensor, landmarks: Union[int, torch.Tensor], point_weights: torch.Tensor,
                  max_dimension: Optional[int] = None, points_per_edge: Optional[int] = 30,
                  num_rand: Optional[int] = None, start_idx: Optional[int] = 0, *, return_simplex_tree: bool = False,
                  method: Optional[str] = None, index: Optional["core.PointIndex"] = None) -> FloodProfile:
    """The weighted Flood filtration for every column of ``point_weights`` (N, M), from one pass: for every c,

        ``prof[c] == flood_complex(points, landmarks, max_dimension, points_per_edge, num_rand, start_idx=start_idx,
        point_weights=point_weights[:, c], method=method, index=index, return_simplex_tree=return_simplex_tree)``

    exactly - ROCm and CPU tensors; with ``num_rand`` under the same seed of the global CPU generator; with
    ``return_simplex_tree=True`` the per-dimension simplex and filtration arrays are equal.  ``columns`` is
    ``((0, "power"), ..., (M - 1, "power"))``; ``prof[i]`` and ``table(d)`` as in ``flood_profile``.

    Every column is judged as ``flood_complex`` judges its ``point_weights``, before any work is done.  One landmark
    selection, one Delaunay complex, one point index, one sample plan per dimension.  ROCm float32 tensors in 2 to 8
    dimensions sweep the columns in groups of at most 8 (``flooder_sweep_power_profile_f32``: one walk of the tree, one
    squared distance per pair, one fma and one minimum per column), the simplices of a dimension in groups within
    ``core.PROFILE_WORKSPACE_BYTES``; the weights must be finite (not checked).  CPU tensors: one lifted kd-tree per
    column.  Not differentiable, not sharded, no hooks (``flood_complex`` / ``power_filtration`` with one column)."""
    if not isinstance(point_weights, torch.Tensor) or point_weights.dim() != 2 or point_weights.shape[1] == 0:
        got = tuple(point_weights.shape) if isinstance(point_weights, torch.Tensor) else type(point_weights).__name__
        n = points.shape[0] if isinstance(points, torch.Tensor) and points.dim() == 2 else "N"
        raise ValueError(f"point_weights must be a ({n}, M) tensor, one column of weights per filtration (M >= 1), got "
                         f"{got}")
    n_cols = point_weights.shape[1]
    for c in range(n_cols):
        bvh = core._check_point_weights(points, point_weights[:, c], method)
    columns = [(c, "power") for c in range(n_cols)]
    return _power_profile(points, landmarks, point_weights, columns, max_dimension, points_per_edge, num_rand, start_idx,
                          return_simplex_tree, bvh, index)


def _power_profile(points, landmarks, point_weights, columns, max_dimension, points_per_edge, num_rand, start_idx,
                   return_simplex_tree, method, index) -> FloodProfile:
    """The body of ``power_profile`` and ``dtm_profile`` (checked weights (N, M), ``method`` as
    ``core._check_point_weights`` returned it); it follows ``flood_profile``."""
    if method != "bvh":
        raise ValueError(f"method must be 'cell', 'bvh' or 'ball', got {method!r}")
    if points.dtype not in core.SUPPORTED_DTYPES:
        raise TypeError(f"dtype ({points.dtype}) not supported")
    if points.device.type not in ("cuda", "cpu"):
        raise RuntimeError("Device not supported.")
    on_gpu = points.is_cuda
    n_cols = len(columns)
    if max_dimension is None:
        max_dimension = points.shape[1]
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
    items = [[] for _ in columns]
    if on_gpu:
        # the weights in tree-row order and their node minima, once per call: per column, or interleaved per group of 8
        w = point_weights.detach()
        single = core._power_weights(index, w[:, 0]) if n_cols == 1 else None
        groups = [] if n_cols == 1 else [(min(core.POWER_COLS_MAX, n_cols - a),
                                          *core._power_weight_columns(index, w[:, a:a + core.POWER_COLS_MAX]))
                                         for a in range(0, n_cols, core.POWER_COLS_MAX)]
        passes = core._dimension_passes(simplices, landmarks.detach().to(torch.float32), core._widest_axis(points, index.box),
                                        points_per_edge, num_rand, "tree")
    else:
        from scipy.spatial import KDTree

        pts_np = np.asarray(points.detach())
        w_np = np.asarray(point_weights.detach().abs())
        # (|p - x|^2 + w_x^2 is the squared distance from (p, 0) to the lifted point (x, |w_x|))
        kdtrees = [KDTree(np.concatenate([pts_np, w_np[:, c:c + 1]], axis=1)) for c in range(n_cols)]
        passes = core._dimension_passes(simplices, landmarks.detach(), core._widest_axis(points), points_per_edge,
                                        num_rand, "ball")
    for p in passes:
        if on_gpu and n_cols == 1:
            face_cols = [core._sweep_dimension_power(index, p.verts, p.weights, p.faces, *single, plan=p.plan)[0]]
        elif on_gpu:
            face_cols = core._sweep_dimension_power_profile(index, p.verts, p.weights, p.faces, groups, plan=p.plan)
        else:
            samples = p.weights.unsqueeze(0) @ p.verts
            lifted = np.asarray(torch.cat([samples, samples.new_zeros(samples.shape[:-1] + (1,))], dim=-1))
            face_cols = [core._face_max_cpu(torch.as_tensor(kd.query(lifted, workers=core.CPU_WORKERS)[0]), p.faces)
                         for kd in kdtrees]
        for c, face in enumerate(face_cols):
            items[c] += core._handoff_items(tree, p, face.cpu().numpy().astype(np.float64))
    trees = []
    for c in range(n_cols):
        trees.append(_clone_tree(tree))
        core._apply_items(trees[c], items[c])
        trees[c].make_filtration_non_decreasing()
    return FloodProfile(columns, trees, None, return_simplex_tree)


def dtm_profile(points: torch.Tensor, landmarks: Union[int, torch.Tensor], masses=None,
                max_dimension: Optional[int] = None, points_per_edge: Optional[int] = 30,
                num_rand: Optional[int] = None, start_idx: Optional[int] = 0, *, neighbors=None, neighbor_stat="dtm",
                return_simplex_tree: bool = False, method: Optional[str] = None,
                index: Optional["core.PointIndex"] = None, cell_size: Optional[float] = None,
                max_neighbors: Optional[int] = None) -> FloodProfile:
    """The DTM-weighted Flood filtration for every mass of a list, from one pass: ``power_profile`` with
    ``distance_to_measure_profile(points, masses=masses, neighbors=neighbors, neighbor_stat=neighbor_stat)`` as its
    weights.  For every column ``(k, stat)`` of ``prof.columns`` (``[(k, s) for k in ks for s in stats]``, k the
    neighbours of a mass),

        ``prof[(k, stat)] == flood_complex(points, landmarks, ..., point_weights=distance_to_measure(points,
        neighbors=k, neighbor_stat=stat))``

    exactly.  ``prof.masses``: the caller's masses aligned with the columns, ``None`` when called with ``neighbors``.
    Exactly one of ``masses`` and ``neighbors`` is given; every entry is judged as ``distance_to_measure`` judges it.
    One ``PointIndex`` serves the weights, the landmark selection and the sweep; the weights cost one wide k-nearest
    sweep at the largest k, the filtrations one weighted sweep per group of 8 columns.  What a scan over the mass is
    for: choosing it (README, "Choosing the mass").

    ``cell_size=c``: the weights over the cloud's CORESET, for masses of more than 1024 points - ``(sites, mu) =
    voxel_measure(points, c)`` once, one index of the sites, and ``distance_to_weighted_measure_profile(sites, mu,
    points, masses, neighbor_stat=neighbor_stat, max_neighbors=max_neighbors)`` as the weights: one walk of the sites
    per point at the largest mass.  The columns are still ``(k, stat)`` with k = ``core.mass_neighbors(m, N)``, the number
    of POINTS the mass stands for (it may be far above 1024; two masses that give the same k are refused), and

        ``prof[(k, stat)] == flood_complex(points, landmarks, ..., point_weights=distance_to_weighted_measure(sites, mu,
        points, mass=m, neighbor_stat=stat, max_neighbors=max_neighbors))``

    exactly.  A coreset is addressed by mass: ``neighbors`` together with ``cell_size`` is refused, and so is
    ``max_neighbors`` (the list capacity of ``distance_to_weighted_measure``) without ``cell_size``.  The weighted sweep
    needs finite weights: a mass at which some point's ``max_neighbors`` nearest sites do not hold it raises a
    ``ValueError`` that names the mass."""
    from .neighbors import (_check_points, _measure_columns, _weighted_columns, distance_to_measure_profile,
                            distance_to_weighted_measure_profile, voxel_measure)

    if cell_size is None and max_neighbors is not None:
        raise ValueError("dtm_profile: max_neighbors is the list capacity of the coreset's weighted measure and needs "
                         "cell_size")
    if cell_size is not None and neighbors is not None:
        raise ValueError("dtm_profile: a coreset is addressed by mass - pass masses, not neighbors, with cell_size")
    on_gpu = _check_points(points, "distance_to_measure")
    if cell_size is not None:
        entries, stats, _ = _weighted_columns(masses, neighbor_stat, "dtm_profile")
        n = points.shape[0]
        ks = [core.mass_neighbors(m, n) for m in entries]
        if len(set(ks)) != len(ks):
            raise ValueError(f"masses lists a value twice: {entries!r} gives k = {ks!r}")
        columns = [(k, s) for k in ks for s in stats]
        aligned = tuple(m for m in entries for _ in stats)
    else:
        _, _, columns, aligned = _measure_columns(points, masses, neighbors, neighbor_stat, "dtm_profile")
    if method in ("cell", "ball"):   # (before the weights are computed; the other refusals of the weighted sweep are
        raise ValueError(core._POWER_REFUSALS["method"].format(method=method))   # _check_points' for these tensors)
    bvh = "bvh" if method is None or method == "auto" else method
    if index is not None:
        core._check_index(index, points, on_gpu, "ROCm tensors")
    if on_gpu and index is None:
        index = core._recall_index(points)
        if index is None:
            index = core.PointIndex(points.to(torch.float32))
            core._remember_index(points, index)
    if cell_size is not None:
        sites, mu = voxel_measure(points.detach(), cell_size)
        weights = distance_to_weighted_measure_profile(sites, mu, points.detach(), entries, neighbor_stat=stats,
                                                       max_neighbors=max_neighbors)
        missed = (~torch.isfinite(weights)).sum(dim=0).tolist()
        for c, m in enumerate(missed):
            if m:
                raise ValueError(f"dtm_profile: {m} of {n} points were not reached at mass {aligned[c]!r} - their nearest "
                                 f"sites of the coreset do not hold it; coarsen cell_size or lower the mass")
    else:
        weights = distance_to_measure_profile(points, None, masses, neighbors=neighbors, neighbor_stat=neighbor_stat,
                                              index=index)
    prof = _power_profile(points, landmarks, weights, columns, max_dimension, points_per_edge, num_rand, start_idx,
                          return_simplex_tree, bvh, index)
    prof.masses = aligned
    return prof


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
