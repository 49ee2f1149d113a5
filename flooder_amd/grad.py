"""Differentiable Flood filtration: exact witnesses of every filtration value and their gradients.

For a simplex tau with landmark vertices L_0..L_k the Flood filtration value is

    f(tau) = |p* - x*|,   p* = sum_i w*_i L_i   (the sample on tau whose nearest-point distance is largest)
                          x* = points[j*]      (the point of the cloud nearest to p*)

so, for f > 0 and u = (p* - x*) / f,  df/dpoints[j*] = -u  and  df/dL_i = w*_i u  (0 for f = 0).  ``flood_filtration``
runs the sweep of ``flood_complex`` and recovers (w*, j*) exactly: on ROCm tensors from the per-sample minimum d2 bits
of the unfused sweep (``csrc/flood_grad.hip``: face argmax, witness search in the box tree of the cloud), on CPU tensors
from the indices of the kd-tree query.  The values themselves are the ones ``flood_complex`` returns.  See DESIGN.md,
"Witnesses and gradients".

``neighbors=k`` (the robust filtration): the witness is p* and its k nearest points x_(1) .. x_(k), ordered by (distance,
id) - on ROCm tensors recovered exactly by ``flooder_witness_knn`` from the bits of the k-nearest sweep's statistic.
``"kth"``: f = |p* - x_(k)|, the formulas above at x_(k); ``"dtm"``: f = sqrt(mean_i |p* - x_(i)|^2),
df/dpoints[id_(i)] = -(p* - x_(i)) / (k f), df/dL_j = w*_j (p* - mean x) / f.

``power_filtration`` (the weighted filtration, ``flood_complex(point_weights=w)``): f = sqrt(|p* - x*|^2 + w*^2) with x*
the POWER-nearest point of p* - on ROCm tensors recovered exactly by ``flooder_witness_power`` from the bits of the
power-distance sweep -, u = (p* - x*) / f: df/dpoints[j*] = -u, df/dL_i = w*_i u, df/dpoint_weights[j*] = w_j* / f.

``dtm_filtration`` (the DTM filtration by mass): ``power_filtration`` with w = ``distance_to_measure(points, mass=m,
differentiable=True)``, whose gradient chains on into the points for every k up to 1024.
"""

from __future__ import annotations

import ctypes
from numbers import Integral
from typing import Dict, List, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native
from . import core
from .persistence import persistence_pairs_simplices
from .simplex_tree import SimplexTree, delaunay_cells

__all__ = ["FloodFiltration", "flood_filtration", "power_filtration", "dtm_filtration"]


class FloodFiltration:
    """Result of ``flood_filtration``, ``power_filtration`` and ``dtm_filtration``: per dimension d (lists indexed by d)

    ``simplices[d]``        (n_d, d+1) int64 CPU: the rows of ``tree.simplices_of_dimension(d)`` (vertex ids ascending)
    ``values[d]``           (n_d,) on the points' device and dtype, differentiable w.r.t. points and landmarks
    ``witness_point[d]``    (n_d,) int64: j*, the row of ``points`` nearest to the witness sample (-1: none)
    ``witness_weights[d]``  (n_d, d+1): barycentric weights w* of the witness sample over the simplex's OWN vertices
    ``witness_neighbors[d]`` (n_d, k) int64: the ``neighbors`` = k nearest points of the witness sample, ascending by
                            (distance, id) (-1: none); its last column is ``witness_point[d]``, the k-th nearest
    ``neighbors``, ``neighbor_stat``  the robust filtration's arguments (1, "kth": the plain filtration)
    ``point_weights``       the weighted filtration's (N,) tensor (``power_filtration``: ``witness_point`` is then the
                            POWER-nearest point of the witness sample; ``dtm_filtration``: the distance to the measure
                            at every point, with grad when the points require it); None from ``flood_filtration``
    ``tree``                the ``flooder_amd.SimplexTree`` with the (detached) values
    """

    def __init__(self, tree: SimplexTree, simplices, values, witness_point, witness_weights, landmark_ids,
                 faces_not_found: int = 0, witness_neighbors=None, neighbors: int = 1, neighbor_stat: str = "kth",
                 point_weights: Optional[torch.Tensor] = None):
        self.tree = tree
        self.simplices: List[torch.Tensor] = simplices
        self.values: List[torch.Tensor] = values
        self.witness_point: List[torch.Tensor] = witness_point
        self.witness_weights: List[torch.Tensor] = witness_weights
        self.landmark_ids = landmark_ids   # int64 rows of `points` the landmarks were taken from (integer landmarks)
        self.faces_not_found = faces_not_found   # faces the device witness search found no point for (0; else it raises)
        self.witness_neighbors: List[torch.Tensor] = (witness_neighbors if witness_neighbors is not None
                                                      else [p.unsqueeze(1) for p in witness_point])
        self.neighbors = neighbors
        self.neighbor_stat = neighbor_stat
        self.point_weights = point_weights

    def to_dict(self) -> Dict[tuple, float]:
        """``{simplex: value}``, what ``flood_complex`` returns for the same arguments."""
        return self.tree.to_dict()

    def diagrams(self, min_persistence: float = 0.0, persistence_dim_max: bool = False) -> Dict[int, torch.Tensor]:
        """``{dim: (m, 2) tensor}`` of persistence intervals, rows sorted as ``tree.persistence_intervals_in_dimension``
        sorts them; births and finite deaths are entries of ``values`` (differentiable), essential classes die at inf."""
        top = self.tree.dimension()
        if top >= len(self.values):
            raise ValueError(f"diagrams() needs every dimension of the complex: the filtration covers dimensions "
                             f"0..{len(self.values) - 1}, the complex has dimension {top} (pass max_dimension={top})")
        pairs = persistence_pairs_simplices(self.tree, min_persistence=min_persistence,
                                            persistence_dim_max=persistence_dim_max)
        flat = torch.cat(self.values)
        offs = np.concatenate([[0], np.cumsum([v.shape[0] for v in self.values])]).astype(np.int64)
        inf = flat.new_tensor(float("inf"))
        out: Dict[int, torch.Tensor] = {}
        for dim, pr in pairs.items():
            birth = flat[torch.as_tensor(offs[pr[:, 0]] + pr[:, 1], device=flat.device)]
            ess = pr[:, 2] < 0
            dpos = np.where(ess, 0, offs[np.maximum(pr[:, 2], 0)] + pr[:, 3])
            death = torch.where(torch.as_tensor(ess, device=flat.device), inf,
                                flat[torch.as_tensor(dpos, device=flat.device)])
            iv = torch.stack((birth, death), dim=1)
            key = iv.detach().cpu().double().numpy()
            order = np.lexsort((key[:, 1], key[:, 0]))
            out[dim] = iv[torch.as_tensor(order, device=iv.device)]
        return out


def _check_args(points: torch.Tensor, method: Optional[str]):
    if points.dim() != 2 or points.shape[0] == 0:
        raise RuntimeError(f"points must be a non-empty (N, d) tensor, got shape {tuple(points.shape)}")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"dtype ({points.dtype}) not supported")
    if method == "ball":
        raise ValueError("flood_filtration: method 'ball' has no exact witnesses (use 'cell' or 'bvh')")
    if method not in (None, "auto", "cell", "bvh"):
        raise ValueError(f"method must be 'cell' or 'bvh', got {method!r}")
    dim = points.shape[1]
    if points.is_cuda:
        if points.dtype is torch.float64:
            raise TypeError("flood_filtration: ROCm float64 tensors are not supported (pass float32)")
        if not 2 <= dim <= 8:
            raise ValueError("flood_filtration: ROCm tensors need ambient dimension 2 to 8")
        if method in (None, "auto"):
            method = core._auto_method(points)
        if method == "cell" and dim not in (2, 3):
            raise ValueError("method 'cell' supports ambient dimension 2 and 3 only")
    elif points.device.type != "cpu":
        raise RuntimeError("Device not supported.")
    return method


def flood_filtration(points: torch.Tensor, landmarks, max_dimension: Optional[int] = None, points_per_edge: int = 30,
                     num_rand: Optional[int] = None, start_idx: Optional[int] = 0, *, method: Optional[str] = None,
                     index: Optional["core.PointIndex"] = None, neighbors: int = 1,
                     neighbor_stat: str = "kth") -> FloodFiltration:
    """Flood filtration with exact witnesses: the values of ``flood_complex(points, landmarks, max_dimension,
    points_per_edge, num_rand, start_idx=start_idx, method=method, index=index, neighbors=neighbors,
    neighbor_stat=neighbor_stat)``, differentiable w.r.t. ``points`` and ``landmarks``.  Integer ``landmarks``:
    farthest-point sampling as ``flood_complex`` does it, the landmarks are ``points.index_select(0, idx)`` (their
    gradient flows into ``points``).  CPU tensors (float32, float64) and ROCm float32 in ambient dimension 2 to 8,
    methods ``"cell"`` / ``"bvh"``.

    ``neighbors=k`` / ``neighbor_stat``: the robust filtration of ``flood_complex``, judged by the same rules with the
    same messages (k > 1 on ROCm: the tree sweep, ``method`` None / "auto" / "bvh").  The witness of a value is then the
    sample p* with the largest statistic and its k nearest points x_(1) .. x_(k), ``witness_neighbors``, ordered by
    (distance, id); ``"kth"``: f = |p* - x_(k)| with the plain gradient at x_(k); ``"dtm"``: f = sqrt(mean_i |p* - x_(i)|^2),
    df/dx_(i) = -(p* - x_(i)) / (k f), df/dp* = (p* - mean x) / f.  On ROCm tensors the k are the k smallest by (d2 in
    the sweep's float32 arithmetic, id): among points equidistant at the k-th place the smallest ids.  On CPU tensors
    they are what ``scipy.spatial.KDTree.query(k=neighbors)`` returns, stably sorted by (distance, id): WHICH of
    several points equidistant at the k-th place is among them is scipy's choice.  ``neighbors=1`` is the call without
    the argument, whichever statistic is named."""
    neighbors, method = core._check_neighbors(points, neighbors, neighbor_stat, method)
    method = _check_args(points, method)
    return _filtration(points, landmarks, max_dimension, points_per_edge, num_rand, start_idx, method, index, neighbors,
                       neighbor_stat)


def power_filtration(points: torch.Tensor, landmarks, point_weights: torch.Tensor, max_dimension: Optional[int] = None,
                     points_per_edge: int = 30, num_rand: Optional[int] = None, start_idx: Optional[int] = 0, *,
                     method: Optional[str] = None, index: Optional["core.PointIndex"] = None) -> FloodFiltration:
    """Weighted Flood filtration with exact witnesses: the values of ``flood_complex(points, landmarks, max_dimension,
    points_per_edge, num_rand, start_idx=start_idx, method=method, index=index, point_weights=point_weights)``,
    differentiable w.r.t. ``points``, ``landmarks`` AND ``point_weights``.  With ``point_weights =
    neighbor_distance(points, neighbors=k, neighbor_stat="dtm")`` (differentiable itself) the robust filtration of the
    literature sits in a loss end to end at the cost of a k = 1 sweep.

    The arguments are judged as ``flood_complex(point_weights=...)`` judges them, with the same messages
    (``core._check_point_weights``): ``method`` None / "auto" / "bvh"; CPU tensors (float32, float64, any dimension) and
    ROCm float32 in ambient dimension 2 to 8.  Integer ``landmarks``: farthest-point sampling as ``flood_filtration``
    does it (their gradient flows into ``points``).

    The witness of a value is the sample p* with the largest power distance (among equal ones the smallest sample row)
    and j* = ``witness_point``, the point that attains min_x |p* - x|^2 + w_x^2.  With f = sqrt(|p* - x*|^2 + w*^2) and
    u = (p* - x*) / f: df/dpoints[j*] = -u, df/dL_i = lambda_i u over the barycentric weights of p*,
    df/dpoint_weights[j*] = w_j* / f with the caller's signed weight; all 0 where f = 0.  On ROCm tensors j* is the
    smallest id among the points whose word fmaf(w, w, d2), in the sweep's float32 arithmetic, has the bits of the
    minimum (``flooder_witness_power``), and the three gradients are summed in a fixed order: bit-identical run to run.
    On CPU tensors j* is the index scipy's kd-tree over the lifted cloud ``[points, |w|]`` returns for ``[p*, 0]``: which of
    several tied points is scipy's choice."""
    method = core._check_point_weights(points, point_weights, method)
    method = _check_args(points, method)
    return _filtration(points, landmarks, max_dimension, points_per_edge, num_rand, start_idx, method, index, 1, "kth",
                       point_weights)


def dtm_filtration(points: torch.Tensor, landmarks, mass: Optional[float] = None, max_dimension: Optional[int] = None,
                   points_per_edge: int = 30, num_rand: Optional[int] = None, start_idx: Optional[int] = 0, *,
                   neighbors: Optional[int] = None, neighbor_stat: str = "dtm", method: Optional[str] = None,
                   index: Optional["core.PointIndex"] = None, cell_size: Optional[float] = None,
                   max_neighbors: Optional[int] = None) -> FloodFiltration:
    """The DTM filtration by mass, differentiable end to end: ``power_filtration(points, landmarks, w, ...)`` with
    ``w = distance_to_measure(points, mass=mass, neighbors=neighbors, neighbor_stat=neighbor_stat, differentiable=True,
    index=index)`` at the cloud's own points - the literature's robust filtration (k = mass * N up to 1024 neighbours)
    at the cost of one wide k-nearest sweep over the cloud and a k = 1 sweep over the samples.

    The arguments are judged by those two functions' own checks, with their messages (exactly one of ``mass`` and
    ``neighbors``).  The values are those of ``flood_complex(points, landmarks, ..., point_weights=
    distance_to_measure(points, mass=mass))``, on ROCm tensors bit for bit.  ``F.point_weights`` is w and carries grad
    when ``points`` requires it: one backward adds the three gradients of ``power_filtration`` into ``points`` (as
    witness points, as landmarks taken from the cloud, and through the weights, chained through the closed form of
    ``distance_to_measure``).  On ROCm tensors the ``PointIndex`` is built once (or recalled, or ``index``) and serves
    both steps and the landmark selection; every sum has a fixed order: bit-identical run to run.

    ``cell_size=c``: the weights over the cloud's CORESET, for a mass of more than 1024 points - ``w =
    distance_to_weighted_measure(sites, mu, queries=points, mass=mass, neighbor_stat=neighbor_stat,
    max_neighbors=max_neighbors, differentiable=True)`` with ``(sites, mu) = voxel_measure(points, c,
    differentiable=True)``.  The sites get a ``PointIndex`` of their own; the cloud's index serves the landmark selection
    and ``power_filtration`` as before.  A coreset is addressed by mass: ``neighbors`` together with ``cell_size`` is
    refused, and so is ``max_neighbors`` (the list capacity of ``distance_to_weighted_measure``) without ``cell_size``.
    ``power_filtration`` needs finite weights, so a point whose ``max_neighbors`` nearest sites do not hold the mass
    raises a ``ValueError`` (the function synchronises with the host anyway, for the Delaunay step).  One backward then
    adds into ``points.grad`` the witness and landmark gradients and the weight gradient, chained through the weighted
    measure in both roles of the cloud: as its queries, and through the centroids of its cells."""
    from .neighbors import (_check_points, _index_of, distance_to_measure, distance_to_weighted_measure,
                            voxel_measure)

    if cell_size is None and max_neighbors is not None:
        raise ValueError("dtm_filtration: max_neighbors is the list capacity of the coreset's weighted measure and "
                         "needs cell_size")
    if cell_size is not None and neighbors is not None:
        raise ValueError("dtm_filtration: a coreset is addressed by mass - pass mass, not neighbors, with cell_size")
    on_gpu = _check_points(points, "distance_to_measure")
    if cell_size is not None:
        sites, mu = voxel_measure(points, cell_size, differentiable=True)
        w = distance_to_weighted_measure(sites, mu, points, mass, neighbor_stat=neighbor_stat,
                                         max_neighbors=max_neighbors, differentiable=True)
        missed = int((~torch.isfinite(w.detach())).sum())
        if missed:
            raise ValueError(f"dtm_filtration: {missed} of {points.shape[0]} points were not reached - their nearest "
                             f"sites of the coreset do not hold the mass {mass!r}; coarsen cell_size or lower mass")
    if on_gpu and index is None:
        index = _index_of(points.detach(), None)
    if cell_size is None:
        w = distance_to_measure(points, None, mass, neighbors=neighbors, neighbor_stat=neighbor_stat,
                                differentiable=True, index=index)
    return power_filtration(points, landmarks, w, max_dimension, points_per_edge, num_rand, start_idx, method=method,
                            index=index)


def _filtration(points, landmarks, max_dimension, points_per_edge, num_rand, start_idx, method, index, neighbors,
                neighbor_stat, point_weights=None) -> FloodFiltration:
    """The checked call of ``flood_filtration`` (``point_weights`` None) or ``power_filtration``."""
    if index is not None:
        core._check_index(index, points, points.is_cuda, "ROCm tensors")
    dim = points.shape[1]
    if max_dimension is None:
        max_dimension = dim
    landmark_ids = None
    if isinstance(landmarks, Integral):
        n_l = int(landmarks)
        if n_l <= 0:
            raise RuntimeError(f"Number of landmarks ({n_l}) must be positive")
        if start_idx is None:
            start_idx = int(torch.randint(points.shape[0], (1,)).item())
        if not (0 <= start_idx < points.shape[0]):
            raise RuntimeError(f"start_idx ({start_idx}) out of range for {points.shape[0]} points")
        with torch.no_grad():
            if points.is_cuda and index is None:
                index = core.PointIndex(points.detach().to(torch.float32))
            landmark_ids = core.fps_indices(points.detach(), min(n_l, points.shape[0]), start_idx, index=index)
        landmarks = points.index_select(0, landmark_ids)
    core._check_landmarks(landmarks, points)

    with torch.no_grad():
        pts = points.detach()
        lms = landmarks.detach()
        lm_np = lms.cpu().numpy()
        tree, simplices = core._cell_complex(delaunay_cells(lm_np), lm_np.shape[0], max_dimension)
        n_dims = max_dimension + 1
        own_val = [np.full(s.shape[0], np.nan) for s in simplices]
        own_pt = [np.full(s.shape[0], -1, dtype=np.int64) for s in simplices]
        own_w = [np.zeros((s.shape[0], d + 1)) for d, s in enumerate(simplices)]
        # (neighbors > 1: the k nearest points of every witness sample; own_pt is then its last column)
        own_nb = [np.full((s.shape[0], neighbors), -1, dtype=np.int64) for s in simplices] if neighbors > 1 else None
        knn = (neighbors, neighbor_stat, own_nb) if neighbors > 1 else None
        not_found = 0
        if points.is_cuda:
            not_found = _sweep_gpu(pts, lms, tree, simplices, points_per_edge, num_rand, method, index,
                                   own_val, own_pt, own_w, knn, point_weights)
        else:
            _sweep_cpu(pts, lms, tree, simplices, points_per_edge, num_rand, own_val, own_pt, own_w, knn, point_weights)
        for d in range(n_dims):
            vals = tree.filtrations_of_dimension(d)
            if vals.shape[0]:
                vals[:] = own_val[d]
        tree._persistence = None
        tree.make_filtration_non_decreasing()
        wp, ww, wn = _inherit(tree, own_val, own_pt, own_w, n_dims, own_nb)

    dev, dt = points.device, points.dtype
    vals_t = [torch.as_tensor(tree.filtrations_of_dimension(d), dtype=dt).to(dev) for d in range(n_dims)]
    F = FloodFiltration(tree, [torch.as_tensor(s) for s in simplices], None,
                        [torch.as_tensor(p).to(dev) for p in wp], [torch.as_tensor(w, dtype=dt).to(dev) for w in ww],
                        landmark_ids, not_found, None if wn is None else [torch.as_tensor(n).to(dev) for n in wn],
                        neighbors, neighbor_stat, point_weights)
    # (the context keeps the witness tensors, not F: F holds the outputs of this very node - a cycle through autograd's
    # C++ graph that the garbage collector cannot break)
    witnesses = (F.simplices, F.witness_point, F.witness_weights)
    if neighbors > 1 and neighbor_stat == "dtm":    # ("kth": the gradient sits at witness_point, the k-th nearest)
        witnesses += (F.witness_neighbors,)
    if point_weights is not None:
        flat = _PowerValues.apply(points, landmarks, point_weights, torch.cat(vals_t), witnesses)
    else:
        flat = _FloodValues.apply(points, landmarks, torch.cat(vals_t), witnesses)
    F.values = list(torch.split(flat, [v.shape[0] for v in vals_t]))
    return F


# ---------------------------------------------------------------------------------------------------- the sweeps
def _face_groups(p: "core.DimensionPass"):
    """[(first column of the group in the face table, v_idx)] of a pass; random samples: one face, the simplex itself."""
    if p.v_idx_np is None:
        return [(0, np.arange(p.d + 1, dtype=np.int64).reshape(1, -1))]
    out, col = [], 0
    for v_idx in p.v_idx_np:
        out.append((col, v_idx))
        col += v_idx.shape[0]
    return out


def _pick_copies(key: torch.Tensor, rows: torch.Tensor, n_rows: int):
    """Per table row: among its copies (entries of ``rows``), the largest d2 bits (high word of ``key``), then the
    smallest flat (queue position, face) index - the smallest queue position, a simplex has a face once; inside the
    copy, ``key`` already names its smallest sample row.  Returns (covered rows, winning flat positions)."""
    dev = key.device
    bits = key >> 32
    bmax = torch.full((n_rows,), -1, dtype=torch.int64, device=dev)
    bmax.scatter_reduce_(0, rows, bits, reduce="amax")
    pos = torch.arange(key.shape[0], device=dev, dtype=torch.int64)
    big = torch.iinfo(torch.int64).max
    cand = torch.where(bits == bmax[rows], pos, torch.full_like(pos, big))
    win = torch.full((n_rows,), big, dtype=torch.int64, device=dev)
    win.scatter_reduce_(0, rows, cand, reduce="amin")
    covered = torch.nonzero(win != big).reshape(-1)
    return covered, win[covered]


def _grad_face_rows(plan: "core.SamplePlan"):
    """(face CSR in swept columns (``rows_perm``) with every face's segment ascending - a face that spans the row is read
    coalesced -, the weight-table row of every swept column), kept on the plan: a grid plan is cached per
    points_per_edge."""
    got = getattr(plan, "_grad_rows", None)
    if got is None:
        ptr = plan.faces.ptr.cpu().numpy()
        rp = plan.rows_perm.cpu().numpy().copy()
        for f in range(plan.faces.n_faces):
            rp[ptr[f]:ptr[f + 1]].sort()
        dev = plan.rows_perm.device
        got = plan._grad_rows = (torch.as_tensor(rp, device=dev),
                                 torch.as_tensor(np.asarray(plan._perm, dtype=np.int32), device=dev))
    return got


def _sweep_gpu(pts, lms, tree, simplices, points_per_edge, num_rand, method, index, own_val, own_pt, own_w, knn=None,
               point_weights=None):
    lib = _native.load()
    dev = pts.device
    torch.cuda.set_device(dev)
    pts32 = pts.to(torch.float32).contiguous()
    if index is None:
        index = core.PointIndex(pts32)
    dim = pts.shape[1]
    axis = core._widest_axis(pts, index.box)
    st = _native.current_stream_ptr(dev)
    not_found = torch.zeros(1, dtype=torch.int32, device=dev)
    if point_weights is not None:   # the weights in tree-row order and their node minima, once per call
        w_sorted, node_w = core._power_weights(index, point_weights)
    for p in core._dimension_passes(simplices, lms.to(torch.float32), axis, points_per_edge, num_rand, "tree"):
        d, sv, weights, faces = p.d, p.verts, p.weights, p.faces
        plan = p.plan if p.plan is not None else core.SamplePlan(weights, faces)   # (random samples: the gather below needs it)
        S, R = sv.shape[0], weights.shape[0]
        got = []
        if knn is not None:    # (S, R) bits of the squared statistic instead of the minimum d2
            face_dev, _ = core._sweep_dimension_knn(index, sv, weights, faces, knn[0], knn[1], plan=plan, keep=got.append)
        elif point_weights is not None:    # (S, R) bits of the squared power distance
            face_dev, _ = core._sweep_dimension_power(index, sv, weights, faces, w_sorted, node_w, plan=plan,
                                                      keep=got.append)
        else:
            sweep = core._sweep_dimension_cell if method == "cell" else core._sweep_dimension_bvh
            face_dev, _ = sweep(index, sv, weights, faces, got.append, plan=plan)
        d2 = got[0]
        F = faces.n_faces
        keys = torch.empty((S, F), dtype=torch.int64, device=dev)
        face_rows, row_id = _grad_face_rows(plan)
        _native.check(lib.flooder_face_argmax_f32(_native.ptr(d2), S, R, _native.ptr(faces.ptr), _native.ptr(face_rows),
                                                  _native.ptr(row_id), F, _native.ptr(keys), st),
                      "flooder_face_argmax_f32")
        for col, v_idx in _face_groups(p):
            nf, k = v_idx.shape
            rows_np = core._face_table_rows(tree, p, v_idx)
            n_rows = simplices[k - 1].shape[0]
            rows = torch.as_tensor(np.ascontiguousarray(rows_np, dtype=np.int64), device=dev).reshape(-1)
            key = keys[:, col:col + nf].reshape(-1)
            val = face_dev[:, col:col + nf].reshape(-1)
            ok = rows >= 0
            if not bool(ok.all()):
                sel = torch.nonzero(ok).reshape(-1)
                rows, key, val = rows[sel], key[sel], val[sel]
            else:
                sel = None
            covered, win = _pick_copies(key, rows, n_rows)
            flat = win if sel is None else sel[win]         # position in the (S, nf) block
            s_q = torch.div(flat, nf, rounding_mode="floor")
            j_q = flat - s_q * nf
            kw = key[win]
            r_w = 0xFFFFFFFF - (kw & 0xFFFFFFFF)              # the winning row of the weight table
            ok_r = r_w < R
            r_q = torch.where(ok_r, plan.inv[torch.where(ok_r, r_w, 0)], -1)   # ... and its swept column (-1: none)
            bits = (kw >> 32)
            n_q = int(covered.shape[0])
            q_s = s_q.to(torch.int32).contiguous()
            q_r = r_q.to(torch.int32).contiguous()
            q_b = bits.to(torch.int32).contiguous()
            cov = covered.cpu().numpy()
            if knn is not None:
                out_nb = torch.empty((n_q, knn[0]), dtype=torch.int64, device=dev)
                blk = _native.WitnessKnn(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=d + 1, nodes=index.nodes,
                                         order=index.order32, verts=sv, weights=plan.w_perm, R=R, k=knn[0], n_simplices=S,
                                         n_queries=n_q, q_simplex=q_s, q_row=q_r, q_stat=q_b, out_ids=out_nb,
                                         not_found=not_found, stat=core.NEIGHBOR_STATS.index(knn[1]))
                _native.check(lib.flooder_witness_knn(ctypes.byref(blk), st), "flooder_witness_knn")
                knn[2][k - 1][cov] = out_nb.cpu().numpy()
                out_pt = out_nb[:, -1]
            else:
                out_pt = torch.empty(n_q, dtype=torch.int64, device=dev)
                blk = _native.WitnessSearch(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=d + 1, nodes=index.nodes,
                                            order=index.order32, verts=sv, weights=plan.w_perm, R=R, n_simplices=S, n_queries=n_q,
                                            q_simplex=q_s, q_row=q_r, q_d2=q_b, out_point=out_pt, not_found=not_found)
                if point_weights is not None:
                    _native.check(lib.flooder_witness_power(ctypes.byref(blk), _native.ptr(w_sorted), _native.ptr(node_w),
                                                            st), "flooder_witness_power")
                else:
                    _native.check(lib.flooder_witness_search(ctypes.byref(blk), st), "flooder_witness_search")
            own_val[k - 1][cov] = val[win].cpu().numpy().astype(np.float64)
            own_pt[k - 1][cov] = out_pt.cpu().numpy()
            w_full = plan.w_perm[r_q.clamp(min=0)]           # (n_q, d+1) over the swept simplex's vertices
            vi = torch.as_tensor(v_idx, device=dev)[j_q]     # (n_q, k) the face's vertex positions
            own_w[k - 1][cov] = torch.gather(w_full, 1, vi).cpu().numpy().astype(np.float64)
    missing = int(not_found.item())
    if missing:
        who = "flood_filtration" if point_weights is None else "power_filtration"
        raise RuntimeError(f"{who}: the witness search found no point at the exact distance for {missing} faces")
    return missing


def _sweep_cpu(pts, lms, tree, simplices, points_per_edge, num_rand, own_val, own_pt, own_w, knn=None,
               point_weights=None):
    from scipy.spatial import KDTree

    # (weighted: |p - x|^2 + w_x^2 is the squared distance from (p, 0) to the lifted point (x, |w_x|), as flood_complex)
    kdtree = KDTree(np.asarray(pts) if point_weights is None
                    else np.concatenate([np.asarray(pts), np.asarray(point_weights.detach().abs())[:, None]], axis=1))
    for p in core._dimension_passes(simplices, lms, core._widest_axis(pts), points_per_edge, num_rand, "ball"):
        weights, faces, S = p.weights, p.faces, p.verts.shape[0]
        samples = weights.unsqueeze(0) @ p.verts
        if point_weights is not None:   # the lifted samples (p, 0)
            samples = torch.cat([samples, samples.new_zeros(samples.shape[:-1] + (1,))], dim=-1)
        if knn is not None:
            dist_k, idx_k = kdtree.query(np.asarray(samples), k=knn[0], workers=core.CPU_WORKERS)   # (S, R, k), ascending
            dist = core._robust_stat(dist_k, knn[0], knn[1])
            idx = idx_k[..., -1]
        else:
            dist, idx = kdtree.query(np.asarray(samples), workers=core.CPU_WORKERS)
        fptr = faces.ptr.numpy()
        frows = faces.rows.numpy()
        w_np = weights.numpy()
        for col, v_idx in _face_groups(p):
            nf, k = v_idx.shape
            rows = core._face_table_rows(tree, p, v_idx).reshape(-1)
            arg = np.empty((S, nf), dtype=np.int64)
            val = np.empty((S, nf))
            for j in range(nf):
                fr = frows[fptr[col + j]:fptr[col + j + 1]]
                a = np.argmax(dist[:, fr], axis=1)           # first maximum: the smallest sample row
                arg[:, j] = fr[a]
                val[:, j] = dist[np.arange(S), fr[a]]
            ok = rows >= 0
            pos = np.nonzero(ok)[0]
            # per table row: the largest value, then the smallest (queue position, face) copy
            order = np.lexsort((pos, -val.reshape(-1)[pos], rows[pos]))
            srt = pos[order]
            first = np.ones(srt.shape[0], dtype=bool)
            first[1:] = rows[srt[1:]] != rows[srt[:-1]]
            win = srt[first]
            s_q, j_q = win // nf, win % nf
            r_q = arg.reshape(-1)[win]
            tr = rows[win]
            own_val[k - 1][tr] = val.reshape(-1)[win]
            own_pt[k - 1][tr] = idx[s_q, r_q]
            own_w[k - 1][tr] = w_np[r_q[:, None], v_idx[j_q]]
            if knn is not None:   # the k neighbours, stably sorted by (distance, id)
                dk, ik = dist_k[s_q, r_q], idx_k[s_q, r_q].astype(np.int64)
                by_id = np.argsort(ik, axis=1, kind="stable")
                dk, ik = np.take_along_axis(dk, by_id, axis=1), np.take_along_axis(ik, by_id, axis=1)
                by_d = np.argsort(dk, axis=1, kind="stable")
                ik = np.take_along_axis(ik, by_d, axis=1)
                knn[2][k - 1][tr] = ik
                own_pt[k - 1][tr] = ik[:, -1]


def _facet_rows(tree: SimplexTree, d: int) -> np.ndarray:
    fr = tree._facet_rows(d)
    if fr is not None:
        return fr
    rows = tree.simplices_of_dimension(d)
    return np.stack([tree._locate(d - 1, np.delete(rows, j, axis=1)) for j in range(d + 1)], axis=1)


def _inherit(tree: SimplexTree, own_val, own_pt, own_w, n_dims: int, own_nb=None):
    """Witnesses of the final (monotone) values: a simplex that ``make_filtration_non_decreasing`` raised to a facet's
    value takes that facet's witness (the first facet, omitting vertex j, that holds the value), its weights
    re-expressed over the simplex's own vertices (0 at the omitted one).  ``own_nb`` (the k nearest points of the
    witness samples, neighbors > 1) goes along with the witness point."""
    wp = [p.copy() for p in own_pt]
    ww = [w.copy() for w in own_w]
    wn = [n.copy() for n in own_nb] if own_nb is not None else None
    for d in range(1, n_dims):
        n = wp[d].shape[0]
        if n == 0 or wp[d - 1].shape[0] == 0:
            continue
        fin = tree.filtrations_of_dimension(d)
        own = own_val[d]
        raised = np.isnan(own) | (fin > own)
        if not raised.any():
            continue
        sel = np.nonzero(raised)[0]
        facets = _facet_rows(tree, d)[sel]
        fv = tree.filtrations_of_dimension(d - 1)[np.maximum(facets, 0)]
        hit = (facets >= 0) & (fv == fin[sel, None])
        has = hit.any(axis=1)
        j = np.argmax(hit, axis=1)
        sel, j = sel[has], j[has]
        src = facets[np.nonzero(has)[0], j]
        wp[d][sel] = wp[d - 1][src]
        if wn is not None:
            wn[d][sel] = wn[d - 1][src]
        w = np.zeros((sel.shape[0], d + 1))
        for m in range(d + 1):
            take = np.nonzero(j != m)[0]
            col = np.where(m < j[take], m, m - 1)
            w[take, m] = ww[d - 1][src[take], col]
        ww[d][sel] = w
    return wp, ww, wn


# ---------------------------------------------------------------------------------------------------- autograd
class _FloodValues(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, landmarks, values, witnesses):
        ctx.witnesses = witnesses
        ctx.save_for_backward(points, landmarks)
        return values.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        points, landmarks = ctx.saved_tensors
        gp, gl = witness_backward(*ctx.witnesses[:3], points.detach(), landmarks.detach(), grad, *ctx.witnesses[3:])
        return (gp if ctx.needs_input_grad[0] else None), (gl if ctx.needs_input_grad[1] else None), None, None


class _PowerValues(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, landmarks, point_weights, values, witnesses):
        ctx.witnesses = witnesses
        ctx.save_for_backward(points, landmarks, point_weights)
        return values.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        points, landmarks, point_weights = ctx.saved_tensors
        got = power_witness_backward(*ctx.witnesses, points.detach(), landmarks.detach(), point_weights.detach(), grad)
        return tuple(g if need else None for g, need in zip(got, ctx.needs_input_grad)) + (None, None)


def witness_backward(simplices, witness_point, witness_weights, points: torch.Tensor, landmarks: torch.Tensor,
                     grad: torch.Tensor, witness_neighbors=None):
    """(grad_points (n, dim), grad_landmarks (L, dim)) of sum(grad * values), in the input dtype.  ROCm tensors: the
    contributions are summed per target row in a fixed order (``flooder_segment_sum_f32``): bit-identical run to run.
    ``witness_neighbors`` (per dimension (n_d, k)): the values are distances to the empirical measure of those k
    points, f = sqrt(mean_i |p* - x_(i)|^2); without it f = |p* - points[witness_point]| (the nearest point, or the
    k-th nearest of the k-distance)."""
    return _witness_backward(simplices, witness_point, witness_weights, points, landmarks, grad, witness_neighbors)[:2]


def power_witness_backward(simplices, witness_point, witness_weights, points: torch.Tensor, landmarks: torch.Tensor,
                           point_weights: torch.Tensor, grad: torch.Tensor):
    """``witness_backward`` of the weighted filtration -> (grad_points (n, dim), grad_landmarks (L, dim),
    grad_point_weights (n,)): f = sqrt(|p* - x*|^2 + w*^2) at x* = points[witness_point], the power-nearest point,
    u = (p* - x*) / f; a value adds -g u to row j* of the points, g lambda_i u to landmark i and g w_j* / f to weight j*
    (the caller's signed weight: d(w^2)/dw = 2 w); nothing where f = 0.  ROCm tensors: all three summed in a fixed order."""
    return _witness_backward(simplices, witness_point, witness_weights, points, landmarks, grad, None, point_weights)


def _witness_backward(simplices, witness_point, witness_weights, points, landmarks, grad, witness_neighbors=None,
                      point_weights=None):
    """(grad_points, grad_landmarks, grad_point_weights or None): the body of the two functions above."""
    dev, dt = points.device, points.dtype
    dim = points.shape[1]
    tg_p, vl_p, tg_l, vl_l, vl_w = [], [], [], [], []
    off = 0
    for d, simp in enumerate(simplices):
        n = simp.shape[0]
        g = grad[off:off + n].to(dt)
        off += n
        if n == 0:
            continue
        jp = witness_point[d]
        keep = torch.nonzero((g != 0) & (jp >= 0)).reshape(-1)
        if keep.numel() == 0:
            continue
        g = g[keep]
        jp = jp[keep]
        V = simp.to(dev)[keep]                                 # (m, d+1) landmark ids
        W = witness_weights[d][keep]                           # (m, d+1)
        p = (W.unsqueeze(2) * landmarks[V]).sum(dim=1)         # p* (m, dim)
        if witness_neighbors is not None:
            nb = witness_neighbors[d][keep]                    # (m, k) ids, ascending by (distance, id)
            kk = nb.shape[1]
            diffs = p.unsqueeze(1) - points[nb]                # (m, k, dim)
            f = ((diffs * diffs).sum(dim=2).sum(dim=1, keepdim=True) / kk).sqrt()
            safe = torch.where(f > 0, f, torch.ones_like(f))
            # df/dx_(i) = -(p* - x_(i)) / (k f);  df/dp* = (p* - mean x) / f, the sum of the k terms
            each = torch.where(f.unsqueeze(2) > 0, g.reshape(-1, 1, 1) * diffs / (kk * safe).unsqueeze(2),
                               torch.zeros_like(diffs))
            gu = each.sum(dim=1)
            tg_p.append(nb.reshape(-1))
            vl_p.append(-each.reshape(-1, dim))
        else:
            diff = p - points[jp]
            f = diff.norm(dim=1, keepdim=True)
            if point_weights is not None:
                # (where w = 0 f stays the norm itself, not the root of its square: the plain filtration's bits)
                wj = point_weights[jp].unsqueeze(1)
                f = torch.where(wj == 0, f, torch.sqrt(f * f + wj * wj))
                vl_w.append(torch.where(f > 0, g.unsqueeze(1) * wj / torch.where(f > 0, f, torch.ones_like(f)),
                                        torch.zeros_like(f)))
            u = torch.where(f > 0, diff / torch.where(f > 0, f, torch.ones_like(f)), torch.zeros_like(diff))
            gu = g.unsqueeze(1) * u
            tg_p.append(jp)
            vl_p.append(-gu)
        nz = W != 0
        rows_i, cols_i = torch.nonzero(nz, as_tuple=True)
        tg_l.append(V[rows_i, cols_i])
        vl_l.append(W[rows_i, cols_i].unsqueeze(1) * gu[rows_i])
    gp = _scatter_rows(tg_p, vl_p, points.shape[0], dim, dev, dt)
    gl = _scatter_rows(tg_l, vl_l, landmarks.shape[0], dim, dev, dt)
    gw = None if point_weights is None else _scatter_rows(tg_p, vl_w, points.shape[0], 1, dev, dt).reshape(-1)
    return gp, gl, gw


def _scatter_rows(targets, vals, n_out: int, dim: int, dev, dt) -> torch.Tensor:
    out = torch.zeros((n_out, dim), dtype=dt, device=dev)
    if not targets:
        return out
    tg = torch.cat(targets)
    vl = torch.cat(vals).contiguous()
    if tg.numel() == 0:
        return out
    if dev.type != "cuda":
        out.index_add_(0, tg, vl)    # (sequential on the host: deterministic)
        return out
    lib = _native.load()
    srt, order = torch.sort(tg, stable=True)
    uniq, counts = torch.unique_consecutive(srt, return_counts=True)
    seg_ptr = torch.zeros(uniq.shape[0] + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=seg_ptr[1:])
    vl32 = vl.to(torch.float32).contiguous()
    _native.check(lib.flooder_segment_sum_f32(_native.ptr(vl32), dim, _native.ptr(order.contiguous()), _native.ptr(seg_ptr),
                                              _native.ptr(uniq.contiguous()), uniq.shape[0], _native.ptr(out),
                                              _native.current_stream_ptr(dev)), "flooder_segment_sum_f32")
    return out
