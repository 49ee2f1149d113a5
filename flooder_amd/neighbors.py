"""The robust filtration's statistic at arbitrary query points: the k-distance and the distance to the empirical measure.

``flood_complex(neighbors=k)`` evaluates these only at lattice samples of Delaunay simplices.  ``neighbor_distance``
evaluates them at the cloud's own points (an outlier score before landmark selection - farthest-point sampling picks
stray points first) or at any other points (a function on a grid).  ROCm tensors run the k-nearest sweep over sorted
tiles (``flooder_sweep_knn_sorted_f32`` in its query form: every query is a "simplex" of one vertex with one sample).

``nearest_neighbors`` says WHICH points those k are (``flooder_knn_ids_sorted_f32``: the same sweep keeping (d2 word,
original id) keys), and with them ``neighbor_distance`` is differentiable in the cloud and in the queries.

``power_distance`` is the weighted filtration's function, min_x |q - x|^2 + w_x^2, ``power_nearest`` says WHICH point
attains it (``flooder_witness_power``), and with it ``power_distance`` is differentiable in the cloud, the weights and
the queries.

``distance_to_measure`` speaks in MASS (k = mass * N, up to 1024 neighbours): ``flooder_knn_wide_f32``, one wave per query
with its k best in LDS, values and neighbours; detached by default, with ``differentiable=True`` the closed form of
``neighbor_distance`` for every k, its backward two kernels of ``csrc/flood_dtm_grad.hip`` over the sweep's int32 ids.

``distance_to_weighted_measure`` takes SITES WITH MASSES (the coreset of ``voxel_measure``) and a mass that may be far
more than 1024 points: ``flooder_knn_mass_f32``, the wide kernel's walk up to the site at which the cumulative mass
reaches the target; detached by default, with ``differentiable=True`` the closed form of the rule in the sites, their
masses and the queries, its backward two kernels of ``csrc/flood_mass_grad.hip`` over the sweep's int32 rows and counts.
``voxel_measure(differentiable=True)`` carries the gradient of the sites on to the cloud they are the centroids of.
``distance_to_weighted_measure_profile`` evaluates several masses at once (``flooder_knn_mass_profile_f32``: one walk to
the largest target, one crossing scan per column), every column equal to the single call.
"""

from __future__ import annotations

import ctypes
from numbers import Integral, Real
from typing import Optional, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native, core


def _check_queries(queries: torch.Tensor, points: torch.Tensor) -> None:
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != points.shape[1]:
        got = tuple(queries.shape) if isinstance(queries, torch.Tensor) else type(queries).__name__
        raise RuntimeError(f"queries must be a (Q, {points.shape[1]}) tensor, got {got}")
    if queries.device != points.device:
        raise RuntimeError(f"queries.device ({queries.device}) != points.device ({points.device})")
    if queries.dtype != points.dtype:
        raise RuntimeError(f"queries.dtype ({queries.dtype}) != points.dtype ({points.dtype})")


def _check_points(points, who: str) -> bool:
    """``points`` as every function here takes it -> on a ROCm device?  ``who`` names the function in the refusals."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[0] == 0:
        got = tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__
        raise RuntimeError(f"points must be a non-empty (N, d) tensor, got shape {got}")
    if points.dtype not in core.SUPPORTED_DTYPES:
        raise TypeError(f"dtype ({points.dtype}) not supported")
    if points.device.type not in ("cuda", "cpu"):
        raise RuntimeError("Device not supported.")
    on_gpu = points.is_cuda
    if on_gpu and points.dtype is torch.float64:
        raise ValueError(f"{who} on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel")
    if on_gpu and not 2 <= points.shape[1] <= 8:
        raise ValueError(f"{who} on ROCm tensors needs ambient dimension 2 to 8")
    return on_gpu


def _check_queries_and_index(points, queries, index, on_gpu: bool) -> torch.Tensor:
    """-> queries (``points`` itself for None)."""
    if queries is None:
        queries = points
    else:
        _check_queries(queries, points)
    if index is not None:
        core._check_index(index, points, on_gpu, "ROCm tensors")
    return queries


def _check_arguments(points, queries, neighbors, neighbor_stat, index) -> Tuple[torch.Tensor, int]:
    """The argument checks of ``neighbor_distance`` and ``nearest_neighbors`` (one set of refusals, one wording) ->
    (queries: ``points`` itself for None, neighbors as int)."""
    on_gpu = _check_points(points, "neighbor_distance")
    neighbors, _ = core._check_neighbors(points, neighbors, neighbor_stat, None)
    return _check_queries_and_index(points, queries, index, on_gpu), neighbors


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

    Differentiable: when ``points`` or ``queries`` requires grad (and grad mode is on) the result carries a
    ``grad_fn``.  With f the value and x_(1) .. x_(k) the neighbours of a query q, ``"kth"`` has df/dq =
    (q - x_(k)) / f and sends the negative to x_(k); ``"dtm"`` has df/dq = sum_i (q - x_(i)) / (k f) and sends
    -(q - x_(i)) / (k f) to each x_(i); ``squared=True`` has 2 in place of 1 / f; the gradient is 0 where f is 0; with
    ``queries=None`` both roles accumulate into ``points.grad``.  The neighbours are those of ``nearest_neighbors``
    (on ROCm tensors one sweep gives them and the values, which are bit for bit those of the call without grad) and
    the backward on ROCm tensors is bit-identical run to run.  Without grad nothing changes: no ids are computed.
    """
    own = queries is None
    queries, neighbors = _check_arguments(points, queries, neighbors, neighbor_stat, index)
    if queries.shape[0] == 0:
        return torch.empty(0, dtype=points.dtype, device=points.device)
    if torch.is_grad_enabled() and (points.requires_grad or queries.requires_grad):
        return _NeighborDistance.apply(points, None if own else queries, neighbors, neighbor_stat, bool(squared), index)
    if points.is_cuda:
        _, _, bits = _query_sweep_hip(points, queries, neighbors, neighbor_stat, index, False, False, True)
        return _root_of_bits(_native.load(), bits, squared, _native.current_stream_ptr(points.device))
    dist, _ = _kdtree_query(points, queries, neighbors)
    return _cpu_statistic(dist, neighbors, neighbor_stat, squared).to(points.dtype)


def nearest_neighbors(points: torch.Tensor, queries: Optional[torch.Tensor] = None, neighbors: int = 1, *,
                      squared: bool = False, index: Optional[core.PointIndex] = None):
    """The k nearest points of ``points`` per query -> (``ids`` (Q, k) int64: rows of ``points`` in input order,
    ``dist`` (Q, k) of ``points``' dtype: their distances, squared with ``squared=True``), both ascending by
    (distance, id) and on the device of ``points``.

    Arguments as ``neighbor_distance`` (same checks, same refusals): k = ``neighbors`` in 1..32, at most the number of
    points; a point that occurs twice is two ids.  ``queries=None``: the cloud's own points - column 0 is then the
    point itself, or a copy of it with a smaller id.  Q = 0 gives empty (0, k) tensors.

    ROCm tensors (float32, 2 to 8 dimensions) run ``flooder_knn_ids_sorted_f32``: exact in the sweeps' float32
    arithmetic, and among points at the same float32 squared distance the smaller id comes first - the k-th place
    included - the rule of ``flood_filtration``'s witnesses.  ``dist[:, k - 1]`` is ``neighbor_distance(..., "kth")``
    bit for bit.  Only the argument checks synchronise with the host.

    CPU tensors (float32, float64; any dimension) query scipy's kd-tree: which of several equidistant points sits at
    the k-th place, and their order among themselves, is scipy's choice.
    """
    queries, neighbors = _check_arguments(points, queries, neighbors, "kth", index)
    if queries.shape[0] == 0:
        return _no_neighbors(points, neighbors)
    if points.is_cuda:
        ids, dist, _ = _knn_ids_hip(points, queries, neighbors, "kth", index, want_d2=True, want_bits=False)
    else:
        dist, ids = _kdtree_query(points, queries, neighbors)
    return _neighbor_pair(points, ids, dist, squared)


def distance_to_measure(points: torch.Tensor, queries: Optional[torch.Tensor] = None, mass: Optional[float] = None, *,
                        neighbors: Optional[int] = None, neighbor_stat: str = "dtm", squared: bool = False,
                        return_neighbors: bool = False, index: Optional[core.PointIndex] = None,
                        differentiable: bool = False):
    """Per query the distance to the empirical measure of ``points`` at mass ``mass`` -> (Q,) tensor of ``points``'
    dtype on its device.

    The literature's parametrisation (gudhi's ``DistanceToMeasure``): with k = ``core.mass_neighbors(mass, N)`` =
    max(1, ceil(mass * N - 1e-6)) the value is sqrt(mean of d_(1)^2 .. d_(k)^2) (``neighbor_stat="dtm"``) or the
    k-distance d_(k) (``"kth"``); a point that occurs twice counts twice.  Exactly one of ``mass`` (a real number in
    (0, 1]) and ``neighbors`` (k itself, 1..``core.KNN_WIDE_MAX`` = 1024, at most the number of points) is given.
    ``squared=True`` returns the statistic before the root.  ``return_neighbors=True`` returns ``(value, ids (Q, k)
    int64, dist (Q, k))``: the k nearest points per query, ascending by (distance, id), ``dist`` squared with
    ``squared=True``.  ``queries`` (None: the cloud's own points), ``index`` and the checks on them are those of
    ``neighbor_distance``; Q = 0 gives empty results.

    ROCm tensors (float32, 2 to 8 dimensions) run ``flooder_knn_wide_f32`` - one wave per query, its k best in LDS -
    for every k: exact in the sweeps' float32 arithmetic, among points at the same float32 squared distance the smaller
    id first.  Up to k = 32 values and neighbours are those of ``neighbor_distance`` and ``nearest_neighbors`` bit for
    bit; above 64 ``"dtm"`` adds the k squared distances in the strided order stated in ``include/flooder_hip.h``
    (within 78 * 2^-24 relative of the exact mean).  ``flood_complex(..., neighbor_mass=m)`` has these values at its
    vertices.  CPU tensors (float32, float64; any dimension) query scipy's kd-tree.

    By default inputs that require grad are used detached.  ``differentiable=True``: when ``points`` or ``queries``
    requires grad (and grad mode is on) the value carries a ``grad_fn`` with the closed form of ``neighbor_distance``
    over m terms, m = k for ``"dtm"`` and m = 1 (x_(k) alone) for ``"kth"``: with f the value, (q - x_(i)) has the
    coefficient grad_out / (f m), 0 where f = 0, and grad_out * 2 / m with ``squared=True``; dq is their sum, its
    negative goes term by term to the x_(i); with ``queries=None`` both roles accumulate into ``points.grad``.  The
    values (and ``ids``, ``dist`` of ``return_neighbors=True``; ``dist`` is detached) are bit for bit those of the call
    without grad; without an input that requires grad the keyword changes nothing.  ROCm tensors keep the wide sweep's
    int32 ids and run ``flooder_dtm_grad_queries_f32`` and ``flooder_dtm_grad_points_f32`` (csrc/flood_dtm_grad.hip): no
    (Q, k, dim) tensor, no float atomics, groups of query rows within ``core.DTM_GRAD_WORKSPACE_BYTES`` - the gradient
    is bit-identical run to run and does not depend on the groups.  CPU tensors: the kd-tree's ids and ``index_add_``.
    """
    on_gpu = _check_points(points, "distance_to_measure")
    if (mass is None) == (neighbors is None):
        raise ValueError("distance_to_measure needs exactly one of mass and neighbors")
    k = _measure_neighbors(points, mass, neighbors, neighbor_stat)
    own = queries is None
    queries = _check_queries_and_index(points, queries, index, on_gpu)
    with_grad = bool(differentiable) and torch.is_grad_enabled() and (points.requires_grad or queries.requires_grad)
    grad_points, grad_queries = points, queries
    points, queries = points.detach(), queries.detach()
    if queries.shape[0] == 0:
        value = torch.empty(0, dtype=points.dtype, device=points.device)
        return (value, *_no_neighbors(points, k)) if return_neighbors else value
    if on_gpu:
        ids, dist, bits = _query_sweep_hip(points, queries, k, neighbor_stat, index, return_neighbors or with_grad,
                                           return_neighbors, True, wide=True)
        value = _root_of_bits(_native.load(), bits, squared, _native.current_stream_ptr(points.device))
    else:
        dist, ids = _kdtree_query(points, queries, k)
        value = _cpu_statistic(dist, k, neighbor_stat, squared).to(points.dtype)
    if with_grad:   # (ROCm tensors: the sweep's int32 ids as they are)
        saved = ids if on_gpu else torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64))
        value = _DistanceToMeasure.apply(grad_points, None if own else grad_queries, value, saved, neighbor_stat,
                                         bool(squared))
    return (value, *_neighbor_pair(points, ids, dist, squared)) if return_neighbors else value


def _measure_neighbors(points: torch.Tensor, mass, neighbors, neighbor_stat) -> int:
    """k of ``distance_to_measure`` from ONE of ``mass`` and ``neighbors`` (the other None), judged in its wording."""
    core._check_neighbor_stat(neighbor_stat)
    n = points.shape[0]
    if mass is not None:
        k, _ = core._check_robust(points, 1, neighbor_stat, mass, None, queries=True)
    else:
        if isinstance(neighbors, bool) or not isinstance(neighbors, Integral):
            raise TypeError(f"neighbors must be an integer, got {neighbors!r}")
        k = int(neighbors)
        if not 1 <= k <= core.KNN_WIDE_MAX:
            raise ValueError(f"neighbors must be in 1..{core.KNN_WIDE_MAX} (KNN_WIDE_MAX: the k best of a query live in "
                             f"the LDS of one wave), got {k}")
    if k > n:
        raise ValueError(f"neighbors={k} exceeds the number of points ({n})")
    return k


def _measure_columns(points: torch.Tensor, masses, neighbors, neighbor_stat, who: str):
    """The columns of a mass profile: exactly one of ``masses`` and ``neighbors`` (a value or a non-empty sequence), every
    entry judged by ``_measure_neighbors`` with every name of ``neighbor_stat`` (a name or a non-empty sequence of
    distinct names) -> (ks, stats, columns ``[(k, s) for k in ks for s in stats]``, the masses aligned with the columns
    or None)."""
    if (masses is None) == (neighbors is None):
        raise ValueError(f"{who} needs exactly one of masses and neighbors")
    by_mass = masses is not None
    given = masses if by_mass else neighbors
    name = "masses" if by_mass else "neighbors"
    if isinstance(given, (str, bytes)):
        raise TypeError(f"{name} must be a number or a sequence of numbers, got {given!r}")
    entries = list(given) if hasattr(given, "__iter__") else [given]
    stats = [neighbor_stat] if isinstance(neighbor_stat, str) or not hasattr(neighbor_stat, "__iter__") else list(neighbor_stat)
    if not entries:
        raise ValueError(f"{name} must not be empty")
    if not stats:
        raise ValueError("neighbor_stat must not be empty")
    ks = []
    for e in entries:
        for stat in stats:
            k = _measure_neighbors(points, e if by_mass else None, None if by_mass else e, stat)
        ks.append(k)
    if len(set(ks)) != len(ks):
        raise ValueError(f"{name} lists a value twice: {entries!r} gives k = {ks!r}")
    if len(set(stats)) != len(stats):
        raise ValueError(f"neighbor_stat lists a name twice: {stats!r}")
    columns = [(k, s) for k in ks for s in stats]
    aligned = tuple(float(m) for m in entries for _ in stats) if by_mass else None
    return ks, stats, columns, aligned


def distance_to_measure_profile(points: torch.Tensor, queries: Optional[torch.Tensor] = None, masses=None, *,
                                neighbors=None, neighbor_stat="dtm", squared: bool = False,
                                index: Optional[core.PointIndex] = None) -> torch.Tensor:
    """``distance_to_measure`` for several masses from ONE pass over the queries -> (Q, n_cols) tensor of ``points``'
    dtype on its device.

    Exactly one of ``masses`` and ``neighbors`` (a value or a non-empty sequence) is given; ``neighbor_stat`` is a name
    or a sequence of names.  Every entry is judged as ``distance_to_measure`` judges it, in its words, before any work
    is done; two entries that give the same k are refused ("lists a value twice").  The columns are
    ``[(k, s) for k in ks for s in stats]`` and column c is ``torch.equal`` to ``distance_to_measure(points, queries,
    neighbors=k_c, neighbor_stat=s_c, squared=squared)``.  ``queries`` (None: the cloud's own points), ``index`` and the
    checks on them are those of ``neighbor_distance``; Q = 0 gives an empty (0, n_cols) tensor.  Detached, not
    differentiable (``distance_to_measure(differentiable=True)`` with one mass is).

    ROCm tensors (float32, 2 to 8 dimensions) run ``flooder_knn_wide_profile_f32``: ONE wide sweep per group of queries
    at the largest k, no ids - the list a wave ends with holds the k_max smallest keys ascending, its first k' entries
    are the k' smallest, and both statistics are fixed by the sorted words alone.  The price is that of the one call
    at the largest k.  At most 64 columns.  CPU tensors (float32, float64; any dimension): one kd-tree query at the
    largest k, the statistic of the leading k' distances per column."""
    on_gpu = _check_points(points, "distance_to_measure")
    ks, stats, columns, _ = _measure_columns(points, masses, neighbors, neighbor_stat, "distance_to_measure_profile")
    if on_gpu and len(columns) > _native.KNN_COLS_MAX:
        raise ValueError(f"distance_to_measure_profile on ROCm tensors takes at most {_native.KNN_COLS_MAX} columns, got "
                         f"{len(columns)}")
    queries = _check_queries_and_index(points, queries, index, on_gpu)
    points, queries = points.detach(), queries.detach()
    Q, n_cols = queries.shape[0], len(columns)
    if Q == 0:
        return torch.empty((0, n_cols), dtype=points.dtype, device=points.device)
    if on_gpu:
        bits = _query_profile_hip(points, queries, columns, index)                     # (n_cols, Q) int32
        value = _root_of_bits(_native.load(), bits, squared, _native.current_stream_ptr(points.device))
        return value.t().contiguous()
    dist, _ = _kdtree_query(points, queries, max(ks))
    # (scipy's k' nearest are the first k' of its k_max)
    return torch.stack([_cpu_statistic(dist[:, :k], k, s, squared).to(points.dtype) for k, s in columns], dim=1)


def _query_profile_hip(points: torch.Tensor, queries: torch.Tensor, columns, index: Optional[core.PointIndex]):
    """``_query_sweep_hip`` in its wide form for every (k, stat) of ``columns`` at once -> (n_cols, Q) int32 words of the
    squared statistics.  Per group of queries (24 B of keys, orders and sort scratch + 4 B per column each, within
    ``core.SORTED_WORKSPACE_BYTES``) ONE ``flooder_knn_wide_profile_f32`` at the largest k; a group's slice of a plane
    is contiguous, its planes are Q words apart: the entry's ``plane_stride``."""
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    index = _index_of(points, index)
    q = queries.detach().contiguous()
    Q, dim = q.shape
    cols = [(int(k), core.NEIGHBOR_STATS.index(s)) for k, s in columns]
    k_max = max(k for k, _ in cols)
    n_cols, col_k, col_stat = _native.column_arrays(cols)
    one = torch.ones((1, 1), dtype=torch.float32, device=dev)
    bits = torch.empty((len(cols), Q), dtype=torch.int32, device=dev)
    key_bits = int(lib.flooder_sample_key_bits(dim))
    per_group = max(1, min(Q, int(core.SORTED_WORKSPACE_BYTES) // (24 + 4 * len(cols)), (1 << 32) - 3))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        verts = q[a:b].unsqueeze(1)                  # (b - a, 1, dim): one vertex per "simplex"
        _, sort_state = core._zeroed_queue(lib, dev, b - a)
        order = core._sorted_sample_order(lib, st, index, verts, one, sort_state, None, key_bits)
        blk = _native.KnnWide(k=k_max, stat=0, sample_order=order, out_bits=_native.ptr(bits) + 4 * a,
                              **core._knn_block_fields(index, verts, one))
        _native.check(lib.flooder_knn_wide_profile_f32(ctypes.byref(blk), n_cols, col_k, col_stat, Q, st),
                      "flooder_knn_wide_profile_f32")
    return bits


_CAPACITIES = (64, 128, 256, 512, 1024)   # mirrors with_list_slots (csrc/flood_knn_list.hpp): the list capacities of the wide and mass entries


def _list_capacity(max_neighbors) -> int:
    """``max_neighbors`` (None: ``core.KNN_WIDE_MAX``) rounded up to the capacity ladder 64, 128, 256, 512, 1024."""
    if max_neighbors is None:
        return core.KNN_WIDE_MAX
    if isinstance(max_neighbors, bool) or not isinstance(max_neighbors, Integral):
        raise TypeError(f"max_neighbors must be an integer, got {max_neighbors!r}")
    if not 1 <= int(max_neighbors) <= core.KNN_WIDE_MAX:
        raise ValueError(f"max_neighbors must be in 1..{core.KNN_WIDE_MAX} (KNN_WIDE_MAX: the neighbours of a query live "
                         f"in the LDS of one wave), got {int(max_neighbors)}")
    return next(c for c in _CAPACITIES if c >= int(max_neighbors))


def _check_point_masses(points: torch.Tensor, point_masses) -> None:
    n = points.shape[0]
    if not isinstance(point_masses, torch.Tensor) or tuple(point_masses.shape) != (n,):
        got = tuple(point_masses.shape) if isinstance(point_masses, torch.Tensor) else type(point_masses).__name__
        raise ValueError(f"point_masses must be a ({n},) tensor, one mass per point, got {got}")
    if point_masses.dtype != points.dtype:
        raise ValueError(f"point_masses.dtype ({point_masses.dtype}) != points.dtype ({points.dtype})")
    if point_masses.device != points.device:
        raise ValueError(f"point_masses.device ({point_masses.device}) != points.device ({points.device})")
    if not points.is_cuda:   # (on ROCm tensors a check would synchronise with the host: the caller's contract)
        point_masses = point_masses.detach()
        if not bool(torch.isfinite(point_masses).all()) or bool((point_masses < 0).any()):
            raise ValueError("point_masses must be finite and non-negative")
        if not float(point_masses.sum(dtype=torch.float64)) > 0.0:
            raise ValueError("point_masses must have a positive total")


def _mass_target(point_masses: torch.Tensor, mass: float, total: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tau = mass * sum(point_masses) as a (1,) float64 tensor on the masses' device, without a host synchronisation.
    A tau within 1e-12 relative of an integer is that integer: (k / N) * N is k, so that unit masses at ``mass=k / N``
    cross at the k-th neighbour whatever the rounding of the product.  ``total``: that sum, when the caller has it (a
    profile forms it once for all its masses)."""
    if total is None:
        total = point_masses.detach().sum(dtype=torch.float64)
    tau = (total * float(mass)).reshape(1)
    near = torch.round(tau)
    return torch.where((near >= 1) & ((tau - near).abs() <= 1e-12 * tau), near, tau).contiguous()


def distance_to_weighted_measure(points: torch.Tensor, point_masses: torch.Tensor, queries: Optional[torch.Tensor] = None,
                                 mass: Optional[float] = None, *, neighbor_stat: str = "dtm", squared: bool = False,
                                 max_neighbors: Optional[int] = None, return_neighbors: bool = False,
                                 index: Optional[core.PointIndex] = None, differentiable: bool = False):
    """Per query the distance to the WEIGHTED measure sum_i mu_i delta_(x_i) (x_i = ``points[i]``, mu_i =
    ``point_masses[i]`` >= 0) at mass ``mass`` -> (Q,) tensor of ``points``' dtype on its device.

    With T = sum mu_i and the target tau = ``mass`` * T (``mass``: a real number in (0, 1]; a tau within 1e-12 relative
    of an integer is that integer), the sites are ordered per query by (distance, id); M_j = mu_(0) + ... + mu_(j) is
    the cumulative mass and j* the first position with M_j* >= tau.  ``neighbor_stat="dtm"``: sqrt(( sum_(i < j*) mu_(i)
    d_(i)^2 + (tau - M_(j*-1)) d_(j*)^2 ) / tau), the distance to the measure of Chazal, Cohen-Steiner and Merigot;
    ``"kth"``: d_(j*), the radius at which the ball around the query holds the mass tau.  Sites of mass 0 are listed but
    add nothing.  With unit masses and ``mass=k / N`` this is ``distance_to_measure(points, queries, neighbors=k)``.
    ``squared=True`` returns the statistic before the root.

    The number of neighbours j* + 1 differs from query to query and is NOT bounded by k = mass * (number of points the
    sites stand for): a site of ``voxel_measure`` that stands for 20 points makes its entry count 20-fold, so a mass
    that is thousands of points - above ``core.KNN_WIDE_MAX``, where ``distance_to_measure`` refuses - is tens of sites.
    The DTM is stable: |d_(mu,m) - d_(nu,m)| <= W_2(mu, nu) / sqrt(m), and the coreset of cell size c is within
    W_2 <= c * sqrt(d) of the cloud.  At most L neighbours are looked at, L = ``max_neighbors`` rounded up to 64, 128,
    256, 512 or 1024 (default ``core.KNN_WIDE_MAX`` = 1024) - and at most the number of sites.  A query whose L nearest
    sites do not hold the mass tau is NOT REACHED and gets +inf; this is documented, not raised (on ROCm tensors a check
    would synchronise with the host - the policy of ``point_weights``): coarsen the coreset or lower the mass.

    ``return_neighbors=True`` returns ``(value, ids (Q, L) int64, dist (Q, L), count (Q,) int64)``: per query its
    first ``count`` = j* + 1 sites ascending by (distance, id) (not reached: all min(L, N) looked at), then -1 / +inf;
    ``dist`` is squared with ``squared=True``.  ``queries`` (None: the sites themselves), ``index`` and the checks on them
    are those of ``neighbor_distance``; Q = 0 gives empty results.  ``point_masses``: an (N,) tensor of the points' dtype
    on their device; CPU tensors refuse non-finite or negative masses and a zero total, ROCm tensors are not checked (it
    would synchronise): there these are the caller's contract.

    ROCm tensors (float32, 2 to 8 dimensions; float64 is refused) run ``flooder_knn_mass_f32``: one wave per query, the
    walk of the wide k-nearest kernel whose cull bound is the key at which the cumulative mass (a float64 scan) crosses
    tau; exact in the sweeps' float32 arithmetic, ``"dtm"`` within (ceil(count / 64) + 67) * 2^-24 relative on the
    squared value (``include/flooder_hip.h``); tau is formed on the device, only the argument checks synchronise.  With
    integer masses (the coreset's counts) the crossing is exact.  CPU tensors (float32, float64; any dimension) query
    scipy's kd-tree at min(L, N) neighbours and evaluate the rule in float64.

    By default inputs that require grad are used detached.  ``differentiable=True``: when ``points``, ``point_masses``
    or ``queries`` requires grad (and grad mode is on) the value carries a ``grad_fn`` with the closed form of the rule.
    Per reached query the listed sites y_(0) .. y_(j*) have the entry coefficients a_t = mu_(t) for t < j* and a_(j*) =
    rho = tau - M_(j*-1) (they add up to tau).  ``"dtm"``, squared value F = sum_t a_t d_(t)^2 / tau: dF/dq = (2 / tau)
    sum_t a_t (q - y_(t)), its negative goes entry by entry to the y_(t); dF/dmu_l = (d_(l)^2 - d_(j*)^2) / tau for a site
    listed before the crossing, and every mass, listed or not, also gets ``mass`` * (d_(j*)^2 - F) / tau (tau depends on
    every mass).  ``"kth"``, F = d_(j*)^2: dF/dq = 2 (q - y_(j*)), its negative to y_(j*) alone, nothing to the masses
    (the radius is piecewise constant in them).  The un-squared value f has these times 1 / (2 f), 0 where f = 0.  A
    query that is not reached (+inf) adds exactly nothing to any gradient, whatever its incoming gradient.  With
    ``queries=None`` both roles of a site accumulate into ``points.grad``.  The rule is piecewise smooth: this is its
    gradient wherever the crossing position does not move (almost everywhere); the gradient through the crossing
    position itself is out of scope.  The values (and ``ids``, ``dist``, ``count`` of ``return_neighbors=True``, which
    are detached) are bit for bit those of the call without grad; without an input that requires grad the keyword changes
    nothing.  ROCm tensors keep the sweep's int32 rows and counts and run ``flooder_mass_grad_queries_f32``,
    ``flooder_mass_grad_points_f32`` and ``flooder_mass_grad_masses_f32`` (csrc/flood_mass_grad.hip; ``"kth"``: ``flooder_dtm_grad_*_f32`` on the column of
    crossing ids): no (Q, L, dim) tensor, no float atomics, groups of query rows within
    ``core.DTM_GRAD_WORKSPACE_BYTES`` - the gradient is bit-identical run to run and does not depend on the groups; with
    unit masses and ``mass=k / N`` it is that of ``distance_to_measure(neighbors=k, differentiable=True)`` bit for bit.
    CPU tensors: the kd-tree's ids, the closed form in float64 torch and ``index_add_``.

    Several masses at once: ``distance_to_weighted_measure_profile`` (one walk of the sites at the largest mass, every
    column equal to the call here), and over a cloud's coreset ``dtm_profile(cell_size=...)``; ``power_profile`` takes any
    (N, M) weights, these included.  Out of scope here: ``flood_complex(neighbor_mass=...)`` over a weighted cloud (pass
    the result as ``point_weights`` instead: ``flood_complex(points, L, point_weights=w)``, or use
    ``dtm_filtration(cell_size=...)``), sharding, a float64 kernel.
    """
    on_gpu = _check_points(points, "distance_to_weighted_measure")
    core._check_neighbor_stat(neighbor_stat)
    _check_point_masses(points, point_masses)
    if mass is None:
        raise ValueError("distance_to_weighted_measure needs mass (a real number in (0, 1])")
    core.mass_neighbors(mass, 1)   # (the checks of a mass, in the family's wording)
    cap = _list_capacity(max_neighbors)
    own = queries is None
    queries = _check_queries_and_index(points, queries, index, on_gpu)
    with_grad = bool(differentiable) and torch.is_grad_enabled() and (
        points.requires_grad or point_masses.requires_grad or queries.requires_grad)
    grad_points, grad_masses, grad_queries = points, point_masses, queries
    points, point_masses, queries = points.detach(), point_masses.detach(), queries.detach()
    Q = queries.shape[0]
    if Q == 0:
        value = torch.empty(0, dtype=points.dtype, device=points.device)
        if not return_neighbors:
            return value
        return (value, *_no_neighbors(points, cap), torch.empty(0, dtype=torch.int64, device=points.device))
    tau = _mass_target(point_masses, mass)
    if on_gpu:
        lib, st = _native.load(), _native.current_stream_ptr(points.device)
        ids, d2, count, bits = _weighted_sweep_hip(points, point_masses, queries, tau, cap, neighbor_stat, index,
                                                   return_neighbors or with_grad, return_neighbors)
        value = _root_of_bits(lib, bits, squared, st)
        if with_grad:   # (the sweep's int32 rows and counts as they are; the squared words tell reached from not)
            value = _WeightedMeasure.apply(grad_points, grad_masses, None if own else grad_queries, value,
                                           bits.view(torch.float32), ids, count, tau, float(mass), neighbor_stat,
                                           bool(squared))
        if not return_neighbors:
            return value
        return value, ids.long(), _root_of_bits(lib, d2, squared, st), count.long()
    value, ids, dist, count = _weighted_measure_cpu(points, point_masses, queries, float(tau[0]), cap, neighbor_stat,
                                                    squared)
    value = torch.as_tensor(value).to(points.dtype)
    ids, count = torch.as_tensor(ids), torch.as_tensor(count)
    if with_grad:
        value = _WeightedMeasure.apply(grad_points, grad_masses, None if own else grad_queries, value, None, ids, count,
                                       tau, float(mass), neighbor_stat, bool(squared))
    if not return_neighbors:
        return value
    return value, ids, torch.as_tensor(dist).to(points.dtype), count


def _weighted_measure_cpu(points, point_masses, queries, tau: float, cap: int, stat: str, squared: bool):
    """The rule of ``distance_to_weighted_measure`` in float64 numpy over the kd-tree's min(cap, N) nearest -> (value
    (Q,), ids (Q, cap) int64 padded with -1, dist (Q, cap) padded with +inf, count (Q,) int64)."""
    Q, kq = queries.shape[0], min(cap, points.shape[0])
    dist, ids = _kdtree_query(points, queries, kq)
    dist = dist.astype(np.float64)
    d2 = np.square(dist)
    mu = np.asarray(point_masses, dtype=np.float64)[ids]
    val, count = _weighted_rule_cpu(d2, mu, np.cumsum(mu, axis=1), tau, stat, squared)
    listed = np.arange(cap)[None, :] < count[:, None]
    out_ids = np.full((Q, cap), -1, dtype=np.int64)
    out_dist = np.full((Q, cap), np.inf)
    out_ids[:, :kq] = ids
    out_dist[:, :kq] = d2 if squared else dist
    out_ids[~listed] = -1
    out_dist[~listed] = np.inf
    return val, out_ids, out_dist, count


def _weighted_rule_cpu(d2: np.ndarray, mu: np.ndarray, M: np.ndarray, tau: float, stat: str, squared: bool):
    """The rule at ONE target over the (Q, kq) squared distances ``d2`` of the nearest sites ascending, their masses
    ``mu`` and the cumulative masses ``M`` (all float64) -> (value (Q,), +inf where the kq sites do not hold ``tau``;
    count (Q,) int64: the crossing position + 1, kq where not reached).  ``distance_to_weighted_measure`` and every
    column of its profile are this function: the same operations on the same numbers."""
    Q, kq = d2.shape
    crossed = M >= tau
    reached = crossed.any(axis=1)
    j = np.argmax(crossed, axis=1)                                # the first crossing (0 where there is none)
    rows = np.arange(Q)
    if stat == "kth":
        val = d2[rows, j]
    else:
        before = np.arange(kq)[None, :] < j[:, None]
        m_prev = np.where(j > 0, M[rows, np.maximum(j - 1, 0)], 0.0)
        val = ((mu * d2 * before).sum(axis=1) + (tau - m_prev) * d2[rows, j]) / tau
    val = np.where(reached, val if squared else np.sqrt(val), np.inf)
    count = np.where(reached, j + 1, kq).astype(np.int64)
    return val, count


def _weighted_sweep_hip(points, point_masses, queries, tau: torch.Tensor, cap: int, stat: str,
                        index: Optional[core.PointIndex], want_neighbors: bool, want_d2: Optional[bool] = None):
    """``_query_sweep_hip``'s wide form for ``flooder_knn_mass_f32``: the same ``PointIndex``, the queries sorted by curve
    key in groups (24 B of keys, orders and sort scratch, 8 B of value and count and, with ``want_neighbors``, 8 * cap
    bytes of rows per query, within ``core.SORTED_WORKSPACE_BYTES``), one launch per group -> (ids (Q, cap) int32 or
    None, their d2 words (Q, cap) int32 or None, count (Q,) int32, the words of the squared statistic (Q,) int32).
    ``want_d2`` (None: as ``want_neighbors``) False: the ids without their d2 words - what a forward with grad keeps."""
    want_d2 = want_neighbors if want_d2 is None else (want_neighbors and want_d2)
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    index = _index_of(points, index)
    q = queries.contiguous()
    Q, dim = q.shape
    masses = point_masses.to(torch.float32).contiguous()
    one = torch.ones((1, 1), dtype=torch.float32, device=dev)
    ids = torch.empty((Q, cap), dtype=torch.int32, device=dev) if want_neighbors else None
    d2 = torch.empty((Q, cap), dtype=torch.int32, device=dev) if want_d2 else None
    count = torch.empty(Q, dtype=torch.int32, device=dev)
    bits = torch.empty(Q, dtype=torch.int32, device=dev)
    key_bits = int(lib.flooder_sample_key_bits(dim))
    per_query = 24 + 8 + (8 * cap if want_neighbors else 0)
    per_group = max(1, min(Q, int(core.SORTED_WORKSPACE_BYTES) // per_query, (1 << 32) - 3))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        verts = q[a:b].unsqueeze(1)                  # (b - a, 1, dim): one vertex per "simplex"
        _, sort_state = core._zeroed_queue(lib, dev, b - a)
        order = core._sorted_sample_order(lib, st, index, verts, one, sort_state, None, key_bits)
        blk = _native.KnnWide(k=cap, stat=core.NEIGHBOR_STATS.index(stat), order=index.order32, sample_order=order,
                              out_bits=bits[a:b], out_ids=None if ids is None else ids[a:b],
                              out_d2=None if d2 is None else d2[a:b], **core._knn_block_fields(index, verts, one))
        _native.check(lib.flooder_knn_mass_f32(ctypes.byref(blk), _native.ptr(masses), _native.ptr(tau), cap,
                                               _native.ptr(count[a:b]), st), "flooder_knn_mass_f32")
    return ids, d2, count, bits


def _weighted_columns(masses, neighbor_stat, who: str):
    """The columns of a weighted mass profile: ``masses`` (a number or a non-empty sequence, every entry judged as
    ``distance_to_weighted_measure`` judges ``mass``) x ``neighbor_stat`` (a name or a non-empty sequence of names); an
    entry listed twice is refused -> (masses as floats, stats, columns ``[(m, s) for m in masses for s in stats]``)."""
    if masses is None:
        raise ValueError(f"{who} needs masses (real numbers in (0, 1])")
    if isinstance(masses, (str, bytes)):
        raise TypeError(f"masses must be a number or a sequence of numbers, got {masses!r}")
    entries = list(masses) if hasattr(masses, "__iter__") else [masses]
    stats = [neighbor_stat] if isinstance(neighbor_stat, str) or not hasattr(neighbor_stat, "__iter__") else list(neighbor_stat)
    if not entries:
        raise ValueError("masses must not be empty")
    if not stats:
        raise ValueError("neighbor_stat must not be empty")
    for stat in stats:
        core._check_neighbor_stat(stat)
    for m in entries:
        core.mass_neighbors(m, 1)   # (the checks of a mass, in the family's wording)
    entries = [float(m) for m in entries]
    if len(set(entries)) != len(entries):
        raise ValueError(f"masses lists a value twice: {entries!r}")
    if len(set(stats)) != len(stats):
        raise ValueError(f"neighbor_stat lists a name twice: {stats!r}")
    return entries, stats, [(m, s) for m in entries for s in stats]


def distance_to_weighted_measure_profile(points: torch.Tensor, point_masses: torch.Tensor,
                                         queries: Optional[torch.Tensor] = None, masses=None, *, neighbor_stat="dtm",
                                         squared: bool = False, max_neighbors: Optional[int] = None,
                                         return_counts: bool = False, index: Optional[core.PointIndex] = None):
    """``distance_to_weighted_measure`` for several masses from ONE walk of the sites per query -> (Q, n_cols) tensor of
    ``points``' dtype on its device; with ``return_counts=True`` ``(values, counts (Q, n_cols) int64)``.

    ``masses`` is a number or a non-empty sequence, ``neighbor_stat`` a name or a sequence of names; every entry is
    judged as ``distance_to_weighted_measure`` judges it, in its words, before any work is done, and an entry listed
    twice is refused ("lists a value twice").  The columns are ``[(m, s) for m in masses for s in stats]`` and column c
    is ``torch.equal`` to ``distance_to_weighted_measure(points, point_masses, queries, mass=m_c, neighbor_stat=s_c,
    squared=squared, max_neighbors=max_neighbors)``, its count that call's ``count`` - a query that is not reached at a
    mass (+inf, count min(L, N)) included, whatever the other columns of its row are.  ``points``, ``point_masses``,
    ``queries`` (None: the sites themselves), ``max_neighbors``, ``index`` and the checks on them are those of
    ``distance_to_weighted_measure``; Q = 0 gives empty results.  Detached, not differentiable
    (``distance_to_weighted_measure(differentiable=True)`` with one mass is).

    ROCm tensors (float32, 2 to 8 dimensions) run ``flooder_knn_mass_profile_f32``: one launch per group of queries, the
    walk of ``flooder_knn_mass_f32`` to the LARGEST target - the list a wave ends with holds every site up to that
    crossing in order, so the crossing of every smaller target lies in it, and the cumulative mass at a place depends on
    the places in front of it alone: the epilogue scans the list once per column.  The targets are formed on the device
    by the single call's rule, each bit for bit its tau; only the argument checks synchronise.  At most 64 columns.  CPU
    tensors (float32, float64; any dimension): one kd-tree query at min(L, N) neighbours - what the single call queries
    whatever the mass - and the float64 rule per column."""
    who = "distance_to_weighted_measure_profile"
    on_gpu = _check_points(points, "distance_to_weighted_measure")
    _check_point_masses(points, point_masses)
    entries, stats, columns = _weighted_columns(masses, neighbor_stat, who)
    if on_gpu and len(columns) > _native.KNN_COLS_MAX:
        raise ValueError(f"{who} on ROCm tensors takes at most {_native.KNN_COLS_MAX} columns, got {len(columns)}")
    cap = _list_capacity(max_neighbors)
    queries = _check_queries_and_index(points, queries, index, on_gpu)
    points, point_masses, queries = points.detach(), point_masses.detach(), queries.detach()
    Q, n_cols = queries.shape[0], len(columns)
    if Q == 0:
        value = torch.empty((0, n_cols), dtype=points.dtype, device=points.device)
        return (value, torch.empty((0, n_cols), dtype=torch.int64, device=points.device)) if return_counts else value
    total = point_masses.sum(dtype=torch.float64)
    taus = [_mass_target(point_masses, m, total) for m in entries]          # each the single call's tau, bit for bit
    if on_gpu:
        targets = torch.cat([t for t in taus for _ in stats]).contiguous()
        bits, count = _weighted_profile_hip(points, point_masses, queries, targets,
                                            [core.NEIGHBOR_STATS.index(s) for _, s in columns], cap, index)
        value = _root_of_bits(_native.load(), bits, squared, _native.current_stream_ptr(points.device))
        value = value.t().contiguous()
        return (value, count.t().contiguous().long()) if return_counts else value
    kq = min(cap, points.shape[0])
    dist, ids = _kdtree_query(points, queries, kq)
    d2 = np.square(dist.astype(np.float64))
    mu = np.asarray(point_masses, dtype=np.float64)[ids]
    M = np.cumsum(mu, axis=1)
    cols = [_weighted_rule_cpu(d2, mu, M, float(tau[0]), s, squared) for tau in taus for s in stats]
    value = torch.stack([torch.as_tensor(v).to(points.dtype) for v, _ in cols], dim=1)
    return (value, torch.stack([torch.as_tensor(c) for _, c in cols], dim=1)) if return_counts else value


def _weighted_profile_hip(points, point_masses, queries, targets: torch.Tensor, col_stats, cap: int,
                          index: Optional[core.PointIndex]):
    """``_weighted_sweep_hip`` for every (target, stat) column at once -> ((n_cols, Q) int32 words of the squared
    statistics, (n_cols, Q) int32 counts).  Per group of queries (24 B of keys, orders and sort scratch + 8 B per column
    each, within ``core.SORTED_WORKSPACE_BYTES``) ONE ``flooder_knn_mass_profile_f32``; a group's slice of a plane is
    contiguous, its planes are Q words apart: the entry's ``plane_stride``."""
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    index = _index_of(points, index)
    q = queries.contiguous()
    Q, dim = q.shape
    n_cols = len(col_stats)
    col_stat = (ctypes.c_int32 * n_cols)(*[int(s) for s in col_stats])
    masses = point_masses.to(torch.float32).contiguous()
    one = torch.ones((1, 1), dtype=torch.float32, device=dev)
    bits = torch.empty((n_cols, Q), dtype=torch.int32, device=dev)
    count = torch.empty((n_cols, Q), dtype=torch.int32, device=dev)
    key_bits = int(lib.flooder_sample_key_bits(dim))
    per_group = max(1, min(Q, int(core.SORTED_WORKSPACE_BYTES) // (24 + 8 * n_cols), (1 << 32) - 3))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        verts = q[a:b].unsqueeze(1)                  # (b - a, 1, dim): one vertex per "simplex"
        _, sort_state = core._zeroed_queue(lib, dev, b - a)
        order = core._sorted_sample_order(lib, st, index, verts, one, sort_state, None, key_bits)
        blk = _native.KnnWide(k=cap, stat=0, order=index.order32, sample_order=order, out_bits=_native.ptr(bits) + 4 * a,
                              **core._knn_block_fields(index, verts, one))
        _native.check(lib.flooder_knn_mass_profile_f32(ctypes.byref(blk), _native.ptr(masses), n_cols,
                                                       _native.ptr(targets), col_stat, Q, _native.ptr(count) + 4 * a, st),
                      "flooder_knn_mass_profile_f32")
    return bits, count


def voxel_measure(points: torch.Tensor, cell_size: float, differentiable: bool = False):
    """The coreset of a cloud on a grid of cubes of edge ``cell_size`` -> (``sites`` (M, d), ``masses`` (M,)), both of
    ``points``' dtype on its device: per occupied cell the centroid of its points and their number - the weighted
    measure ``distance_to_weighted_measure`` takes, within W_2 <= cell_size * sqrt(d) of the cloud's empirical measure.

    The cell of x is floor((x - min x) * (1 / cell_size)) per axis, in float64 (one multiplication by the reciprocal:
    the same result on every device).  Rows are ascending by cell, axis 0 most significant.  Deterministic, with no
    float atomics: the points are sorted by cell, their offsets inside the cell - fixed point, 36 fractional bits, so
    a centroid is within 2^-37 of a cell of the float64 mean - are summed as INTEGERS (a cumulative sum and differences
    at the cell boundaries: exact in any order), and the centroid is rounded once to ``points``' dtype.  Two runs, and
    a CPU and a ROCm run, agree (sites to the last bit of float64 before that rounding).  One host synchronisation (the
    number M of occupied cells) is taken.  Up to 2^27 points.

    By default ``points`` is used detached.  ``differentiable=True``: when ``points`` requires grad (and grad mode is on)
    ``sites`` carries a ``grad_fn``: a site is the mean of its cell's points, so ``points.grad[i] = sites.grad[cell(i)] /
    count[cell(i)]`` - one ``index_select`` over the cell of every point, deterministic, no further synchronisation (the
    assignment of points to cells is piecewise constant).  The masses never carry grad, and the bits of both outputs are
    those of the plain call.
    """
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[0] == 0 or points.shape[1] == 0:
        got = tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__
        raise RuntimeError(f"points must be a non-empty (N, d) tensor, got shape {got}")
    if points.dtype not in core.SUPPORTED_DTYPES:
        raise TypeError(f"dtype ({points.dtype}) not supported")
    if isinstance(cell_size, bool) or not isinstance(cell_size, Real):
        raise TypeError(f"cell_size must be a positive real number, got {cell_size!r}")
    cell_size = float(cell_size)
    if not (np.isfinite(cell_size) and cell_size > 0.0):
        raise ValueError(f"cell_size must be positive and finite, got {cell_size!r}")
    if points.shape[0] > 1 << 27:
        raise ValueError(f"voxel_measure takes at most 2^27 points (the integer sums of a cell), got {points.shape[0]}")
    x = points.detach().to(torch.float64)
    lo = x.min(dim=0).values
    scaled = (x - lo) * (1.0 / cell_size)
    cell_f = torch.floor(scaled)
    offs = torch.floor((scaled - cell_f) * float(1 << 36) + 0.5).to(torch.int64)      # 0 .. 2^36
    cells, inverse, counts = torch.unique(cell_f.to(torch.int64), dim=0, return_inverse=True, return_counts=True)
    by_cell = torch.sort(inverse.reshape(-1), stable=True).indices
    sums = torch.cumsum(offs[by_cell], dim=0)                                          # int64: exact
    ends = torch.cumsum(counts, dim=0)
    last = sums[ends - 1]
    total = last - torch.cat([torch.zeros_like(last[:1]), last[:-1]])
    frac = total.to(torch.float64) / (counts.to(torch.float64).unsqueeze(1) * float(1 << 36))
    sites = lo + (cells.to(torch.float64) + frac) * cell_size
    sites = sites.to(points.dtype).contiguous()
    if differentiable and torch.is_grad_enabled() and points.requires_grad:
        sites = _VoxelSites.apply(points, sites, inverse.reshape(-1), counts)
    return sites, counts.to(points.dtype)


class _VoxelSites(torch.autograd.Function):
    """``voxel_measure(differentiable=True)``: the computed ``sites`` with the gradient of a mean per cell."""

    @staticmethod
    def forward(ctx, points, sites, inverse, counts):
        ctx.save_for_backward(inverse, counts)
        return sites.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_sites):
        inverse, counts = ctx.saved_tensors
        share = grad_sites / counts.to(grad_sites.dtype).unsqueeze(1)
        return share.index_select(0, inverse), None, None, None


def power_distance(points: torch.Tensor, point_weights: torch.Tensor, queries: Optional[torch.Tensor] = None, *,
                   squared: bool = False, index: Optional[core.PointIndex] = None) -> torch.Tensor:
    """Per query the power distance sqrt(min_x |q - x|^2 + w_x^2) to the weighted cloud -> (Q,) tensor of ``points``'
    dtype on its device: the function whose sublevel sets ``flood_complex(points, landmarks, point_weights=w)``
    filters (its vertex values are ``power_distance(points, w, landmarks)``, bit for bit on ROCm tensors).

    ``point_weights``: (N,) of the points' dtype and device, one weight per point; it enters squared, so its sign does
    not matter.  With ``w = distance_to_measure(points, mass=m)`` this is the witnessed k-distance, an approximation of
    the distance to the measure from N numbers.  ``queries`` (None: the cloud's own points), ``index`` and the checks on
    them are those of ``neighbor_distance``; ``squared=True`` returns the value before the root; Q = 0 gives an empty
    tensor.

    ROCm tensors (float32, 2 to 8 dimensions) run ``flooder_sweep_power_f32`` in its query form (k1 = R = 1, sorted
    query keys as ``neighbor_distance``); the weights must be finite (not checked on the device).  CPU tensors
    (float32, float64; any dimension) query scipy's kd-tree over the lifted cloud ``[points, |w|]`` with ``[q, 0]`` and
    refuse non-finite weights.

    Differentiable: when ``points``, ``point_weights`` or ``queries`` requires grad (and grad mode is on) the result
    carries a ``grad_fn``.  With f the value, x* = points[j*] the power-nearest point of a query q (``power_nearest``)
    and w* its weight: df/dq = (q - x*) / f, the negative goes to x*, df/dw* = w* / f with the caller's signed weight;
    ``squared=True`` has 2 in place of 1 / f; the gradient is 0 where f is 0; with ``queries=None`` both roles
    accumulate into ``points.grad``.  The values are bit for bit those of the call without grad and the backward on
    ROCm tensors is bit-identical run to run.  Without grad nothing changes: no witness is searched.
    """
    own = queries is None
    on_gpu = _check_points(points, "power_distance")
    core._check_point_weights(points, point_weights, None)
    queries = _check_queries_and_index(points, queries, index, on_gpu)
    if queries.shape[0] == 0:
        return torch.empty(0, dtype=points.dtype, device=points.device)
    if torch.is_grad_enabled() and (points.requires_grad or point_weights.requires_grad or queries.requires_grad):
        return _PowerDistance.apply(points, point_weights, None if own else queries, bool(squared), index)
    return _power_query(points, point_weights, queries, index, squared, False)[1]


def power_nearest(points: torch.Tensor, point_weights: torch.Tensor, queries: Optional[torch.Tensor] = None, *,
                  index: Optional[core.PointIndex] = None):
    """The power-nearest point of the weighted cloud per query -> (``ids`` (Q,) int64: the row of ``points`` that
    attains min_x |q - x|^2 + w_x^2, ``dist`` (Q,) of ``points``' dtype: ``power_distance(points, point_weights,
    queries)``, bit for bit), both on the device of ``points``.  Arguments and checks as ``power_distance``; Q = 0
    gives empty tensors.

    ROCm tensors: the query-form sweep of ``power_distance`` for the bits of the minimum, then
    ``flooder_witness_power`` in the same groups of queries - exact in the sweep's float32 arithmetic, among points
    whose word fmaf(w, w, d2) has the minimum's bits the smallest id, the rule of ``power_filtration``'s witnesses (its
    vertex witnesses are ``power_nearest(points, w, landmarks)[0]``).  CPU tensors: the index scipy's kd-tree over the
    lifted cloud returns; which of several tied points is scipy's choice."""
    on_gpu = _check_points(points, "power_distance")
    core._check_point_weights(points, point_weights, None)
    queries = _check_queries_and_index(points, queries, index, on_gpu)
    if queries.shape[0] == 0:
        return (torch.empty(0, dtype=torch.int64, device=points.device),
                torch.empty(0, dtype=points.dtype, device=points.device))
    return _power_query(points, point_weights, queries, index, False, True)


def _power_query(points, point_weights, queries, index, squared: bool, want_ids: bool):
    """(ids (Q,) int64 or None, the power distance (Q,), squared with ``squared``) of Q > 0 checked queries."""
    points, point_weights, queries = points.detach(), point_weights.detach(), queries.detach()
    Q = queries.shape[0]
    if not points.is_cuda:
        from scipy.spatial import KDTree

        lifted = np.concatenate([np.asarray(points), np.asarray(point_weights.abs())[:, None]], axis=1)
        q = np.concatenate([np.asarray(queries), np.zeros((Q, 1), dtype=lifted.dtype)], axis=1)
        dist, ids = KDTree(lifted).query(q, workers=core.CPU_WORKERS)
        dist = np.asarray(dist, dtype=np.float64).reshape(Q)
        ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64).reshape(Q)) if want_ids else None
        return ids, torch.as_tensor(np.square(dist) if squared else dist).to(points.dtype)
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    index = _index_of(points, index)
    w_sorted, node_w = core._power_weights(index, point_weights)
    q = queries.contiguous()
    one = torch.ones((1, 1), dtype=torch.float32, device=dev)
    bits = torch.empty(Q, dtype=torch.int32, device=dev)
    ids = torch.empty(Q, dtype=torch.int64, device=dev) if want_ids else None
    not_found = torch.zeros(1, dtype=torch.int32, device=dev) if want_ids else None
    key_bits = int(lib.flooder_sample_key_bits(q.shape[1]))
    # (as _query_sweep_hip; the witness names a query by an int32)
    per_group = max(1, min(Q, int(core.SORTED_WORKSPACE_BYTES) // 24, (1 << 31) - 1))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        verts = q[a:b].unsqueeze(1)                  # (b - a, 1, dim): one vertex per "simplex"
        queue, sort_state = core._zeroed_queue(lib, dev, b - a)
        order = core._sorted_sample_order(lib, st, index, verts, one, sort_state, None, key_bits)
        blk = _native.KnnSorted(k=1, stat=0, sample_order=order, queue=queue, out_bits=bits[a:b],
                                **core._knn_block_fields(index, verts, one))
        _native.check(lib.flooder_sweep_power_f32(ctypes.byref(blk), _native.ptr(w_sorted), _native.ptr(node_w), st),
                      "flooder_sweep_power_f32")
        if want_ids:   # the witness search in its query form: query i is sample (i, 0) with the word just written
            q_s = torch.arange(b - a, dtype=torch.int32, device=dev)
            blk = _native.WitnessSearch(pts_sorted=index.pts, n_pts=index.n, dim=index.dim, k1=1, nodes=index.nodes,
                                        order=index.order32, verts=verts, weights=one, R=1, n_simplices=b - a,
                                        n_queries=b - a, q_simplex=q_s, q_row=torch.zeros_like(q_s), q_d2=bits[a:b],
                                        out_point=ids[a:b], not_found=not_found)
            _native.check(lib.flooder_witness_power(ctypes.byref(blk), _native.ptr(w_sorted), _native.ptr(node_w), st),
                          "flooder_witness_power")
    if want_ids and int(not_found.item()):
        raise RuntimeError(f"power_nearest: the witness search found no point at the exact power distance for "
                           f"{int(not_found.item())} queries")
    return ids, _root_of_bits(lib, bits, squared, st)


def _no_neighbors(points: torch.Tensor, k: int):
    """(ids, dist) of no queries."""
    return (torch.empty((0, k), dtype=torch.int64, device=points.device),
            torch.empty((0, k), dtype=points.dtype, device=points.device))


def _neighbor_pair(points: torch.Tensor, ids, dist, squared: bool):
    """(ids, their d2 words (ROCm tensors: both (Q, k) int32) or the kd-tree's distances (CPU: numpy), squared) -> the
    (ids int64, dist of ``points``' dtype) that ``nearest_neighbors`` and ``distance_to_measure`` return."""
    if points.is_cuda:
        dist = _root_of_bits(_native.load(), dist, squared, _native.current_stream_ptr(points.device))
        return ids.long(), dist
    if squared:
        dist = np.square(dist.astype(np.float64))
    return torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)), torch.as_tensor(np.ascontiguousarray(dist)).to(points.dtype)


def _kdtree_query(points: torch.Tensor, queries: torch.Tensor, k: int):
    """(dist, ids) of scipy's kd-tree query, both (Q, k), distances ascending (scipy drops the axis at k = 1)."""
    from scipy.spatial import KDTree

    dist, ids = KDTree(np.asarray(points.detach())).query(np.asarray(queries.detach()), k=k, workers=core.CPU_WORKERS)
    Q = queries.shape[0]
    return np.asarray(dist).reshape(Q, k), np.asarray(ids).reshape(Q, k)


def _cpu_statistic(dist: np.ndarray, k: int, stat: str, squared: bool) -> torch.Tensor:
    if squared:
        d2 = np.square(dist.astype(np.float64))
        val = d2[:, -1] if stat == "kth" else d2.sum(axis=1) / k
    else:
        val = core._robust_stat(dist, k, stat)
    return torch.as_tensor(np.ascontiguousarray(val))


def _index_of(points: torch.Tensor, index: Optional[core.PointIndex]) -> core.PointIndex:
    if index is None:
        index = core._recall_index(points)
        if index is None:
            index = core.PointIndex(points)
            core._remember_index(points, index)
    return index


def _query_sweep_hip(points: torch.Tensor, queries: torch.Tensor, k: int, stat: str, index: Optional[core.PointIndex],
                     want_ids: bool, want_d2: bool, want_bits: bool, wide: bool = False):
    """Keys of the queries inside the cloud's box (queries outside it get clamped keys: order only) -> radix sort ->
    a k-nearest sweep in its query form, k1 = R = 1 (fma(1.0f, q, 0.0f) is q), the sorted order its ``sample_order``
    (queries that follow each other walk the same part of the tree): ``flooder_sweep_knn_sorted_f32`` over sorted tiles,
    with ``want_ids`` ``flooder_knn_ids_sorted_f32``, with ``wide`` (k up to ``core.KNN_WIDE_MAX``, no work queue)
    ``flooder_knn_wide_f32`` -> (ids (Q, k) int32 or None, their d2 words (Q, k) int32 or None, the words of the squared
    statistic (Q,) int32 or None).  Groups of queries keep the keys, the orders and the sort's scratch (24 B per query)
    and, in the ids and wide forms, their share of the outputs within ``core.SORTED_WORKSPACE_BYTES``."""
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    index = _index_of(points, index)
    q = queries.detach().contiguous()
    Q, dim = q.shape
    one = torch.ones((1, 1), dtype=torch.float32, device=dev)
    ids = torch.empty((Q, k), dtype=torch.int32, device=dev) if want_ids else None
    d2 = torch.empty((Q, k), dtype=torch.int32, device=dev) if want_ids and want_d2 else None
    bits = torch.empty(Q, dtype=torch.int32, device=dev) if want_bits else None
    key_bits = int(lib.flooder_sample_key_bits(dim))
    with_order = want_ids or wide          # the forms whose block has order, out_ids and out_d2: they count their outputs
    out_bytes = 4 * k * ((ids is not None) + (d2 is not None)) + (4 if want_bits else 0)
    per_query = 24 + (out_bytes if with_order else 0)
    per_group = max(1, min(Q, int(core.SORTED_WORKSPACE_BYTES) // per_query, (1 << 32) - 3))
    entry, block = (("flooder_knn_wide_f32", _native.KnnWide) if wide
                    else ("flooder_knn_ids_sorted_f32", _native.KnnIds) if want_ids
                    else ("flooder_sweep_knn_sorted_f32", _native.KnnSorted))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        verts = q[a:b].unsqueeze(1)                  # (b - a, 1, dim): one vertex per "simplex"
        queue, sort_state = core._zeroed_queue(lib, dev, b - a)
        order = core._sorted_sample_order(lib, st, index, verts, one, sort_state, None, key_bits)
        outs = dict(out_bits=None if bits is None else bits[a:b])
        if not wide:
            outs.update(queue=queue)
        if with_order:
            outs.update(order=index.order32, out_ids=None if ids is None else ids[a:b],
                        out_d2=None if d2 is None else d2[a:b])
        blk = block(k=k, stat=core.NEIGHBOR_STATS.index(stat), sample_order=order, **outs,
                    **core._knn_block_fields(index, verts, one))
        _native.check(getattr(lib, entry)(ctypes.byref(blk), st), entry)
    return ids, d2, bits


def _knn_ids_hip(points: torch.Tensor, queries: torch.Tensor, k: int, stat: str, index: Optional[core.PointIndex],
                 want_d2: bool, want_bits: bool):
    """The ids form of ``_query_sweep_hip``: what ``nearest_neighbors`` and a forward with grad run."""
    return _query_sweep_hip(points, queries, k, stat, index, True, want_d2, want_bits)


def _root_of_bits(lib, bits: torch.Tensor, squared: bool, st) -> torch.Tensor:
    if squared:
        return bits.view(torch.float32)
    out = torch.empty(bits.shape, dtype=torch.float32, device=bits.device)
    _native.check(lib.flooder_face_values_f32(_native.ptr(bits), bits.numel(), _native.ptr(out), st),
                  "flooder_face_values_f32")
    return out


class _NeighborDistance(torch.autograd.Function):
    """``neighbor_distance`` with its closed-form backward.  ``queries`` None: the cloud's own points (both roles of a
    point accumulate into the gradient of ``points``)."""

    @staticmethod
    def forward(ctx, points, queries, k, stat, squared, index):
        own = queries is None
        qs = points if own else queries
        if points.is_cuda:
            ids, _, bits = _knn_ids_hip(points, qs, k, stat, index, want_d2=False, want_bits=True)
            value = _root_of_bits(_native.load(), bits, squared, _native.current_stream_ptr(points.device))
            ids = ids.long()
        else:
            dist, ids = _kdtree_query(points, qs, k)
            value = _cpu_statistic(dist, k, stat, squared).to(points.dtype)
            ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64))
        ctx.save_for_backward(points, qs, ids, value)
        ctx.own, ctx.k, ctx.stat, ctx.squared = own, k, stat, squared
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from .grad import _scatter_rows

        points, qs, ids, value = ctx.saved_tensors
        own, k, stat, squared = ctx.own, ctx.k, ctx.stat, ctx.squared
        need_p = ctx.needs_input_grad[0]
        need_q = own or ctx.needs_input_grad[1]
        Q, dim = qs.shape
        dt, dev = points.dtype, points.device
        if stat == "kth":
            ids = ids[:, -1:]                                  # x_(k) alone
        m = ids.shape[1]
        # coefficient of (q - x_(i)): grad_out * (1 / f, 0 where f == 0; or 2) / (number of terms of the mean)
        if squared:
            coef = grad_out * (2.0 / m)
        else:
            coef = torch.where(value > 0, grad_out / (value * m), torch.zeros_like(value))
        contrib = (qs.detach().unsqueeze(1) - points.detach()[ids]) * coef.view(Q, 1, 1)      # (Q, m, dim)
        grad_q = contrib.sum(dim=1) if need_q else None
        targets, vals = [], []
        if need_p:
            targets.append(ids.reshape(-1))
            vals.append(-contrib.reshape(Q * m, dim))
            if own:
                targets.append(torch.arange(Q, dtype=torch.int64, device=dev))
                vals.append(grad_q)
        grad_p = _scatter_rows(targets, vals, points.shape[0], dim, dev, dt) if need_p else None
        return grad_p, (None if own or not ctx.needs_input_grad[1] else grad_q), None, None, None, None


class _DistanceToMeasure(torch.autograd.Function):
    """``distance_to_measure(differentiable=True)``: the computed ``value`` with the closed-form backward of
    ``_NeighborDistance`` over the ``ids`` (Q, k) the forward found (int32 on ROCm tensors, int64 on CPU tensors), for
    every k.  ``queries`` None: the cloud's own points."""

    @staticmethod
    def forward(ctx, points, queries, value, ids, stat, squared):
        own = queries is None
        ctx.save_for_backward(points, points if own else queries, ids, value)
        ctx.own, ctx.stat, ctx.squared = own, stat, squared
        return value.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        points, qs, ids, value = ctx.saved_tensors
        own, squared = ctx.own, ctx.squared
        need_p = ctx.needs_input_grad[0]
        need_q = own or ctx.needs_input_grad[1]
        k = ids.shape[1]
        m = 1 if ctx.stat == "kth" else k                      # "kth": x_(k) alone, the column k - 1
        # coefficient of (q - x_(i)): grad_out * (1 / f, 0 where f == 0; or 2) / (number of terms of the mean)
        if squared:
            coef = grad_out * (2.0 / m)
        else:
            coef = torch.where(value > 0, grad_out / (value * m), torch.zeros_like(value))
        backward = _dtm_backward_hip if points.is_cuda else _dtm_backward_cpu
        grad_p, grad_q = backward(points.detach(), qs.detach(), ids, k - m, m, coef, own, need_p, need_q)
        return grad_p, (None if own or not ctx.needs_input_grad[1] else grad_q), None, None, None, None


def _dtm_backward_cpu(points, qs, ids, first: int, m: int, coef, own: bool, need_p: bool, need_q: bool):
    """(grad_points or None, grad_queries or None) over the columns ``first`` .. ``first + m - 1`` of ``ids``: plain torch,
    ``index_add_`` (sequential on the host: deterministic), in groups of query rows that keep the (rows, m, dim)
    contributions of a group near 256 MB."""
    Q, dim = qs.shape
    grad_q = torch.empty_like(qs) if need_q else None
    grad_p = torch.zeros_like(points) if need_p else None
    per_group = max(1, (256 << 20) // (m * dim * points.element_size()))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        nb = ids[a:b, first:first + m]
        contrib = (qs[a:b].unsqueeze(1) - points[nb]) * coef[a:b].view(-1, 1, 1)      # (rows, m, dim)
        if need_q:
            grad_q[a:b] = contrib.sum(dim=1)
        if need_p:
            grad_p.index_add_(0, nb.reshape(-1), -contrib.reshape(-1, dim))
    if need_p and own:
        grad_p += grad_q
    return grad_p, grad_q


def _dtm_backward_hip(points, qs, ids, first: int, m: int, coef, own: bool, need_p: bool, need_q: bool):
    """The same on ROCm float32 tensors: ``flooder_dtm_grad_queries_f32`` over all queries, then per group of ascending
    query rows the (target, query row) pairs as packed int64 keys, sorted (the keys are distinct: one sorted list, however
    it is sorted), the segment of every row of ``points`` by a binary search, and ``flooder_dtm_grad_points_f32``,
    which continues the sequential sum per (target, axis) from group to group - the gradient does not depend on
    ``core.DTM_GRAD_WORKSPACE_BYTES``.  ``queries=None``: one further addition per word, grad_queries onto grad_points."""
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    pts, q = points.contiguous(), qs.contiguous()
    coef = coef.to(torch.float32).contiguous()
    (Q, dim), n, k = q.shape, pts.shape[0], ids.shape[1]
    grad_q = grad_p = None
    if need_q:
        grad_q = torch.empty((Q, dim), dtype=torch.float32, device=dev)
        _native.check(lib.flooder_dtm_grad_queries_f32(_native.ptr(pts), n, _native.ptr(q), Q, dim,
                                                       _native.ptr(ids) + 4 * first, k, m, _native.ptr(coef),
                                                       _native.ptr(grad_q), st), "flooder_dtm_grad_queries_f32")
    if need_p:
        grad_p = torch.zeros((n, dim), dtype=torch.float32, device=dev)
        bounds = torch.arange(n + 1, dtype=torch.int64, device=dev) << 32
        per_group = max(1, min(Q, int(core.DTM_GRAD_WORKSPACE_BYTES) // (64 * m), ((1 << 31) - 1) // m))
        for a in range(0, Q, per_group):
            b = min(Q, a + per_group)
            rows = torch.arange(b - a, dtype=torch.int64, device=dev).unsqueeze(1)
            keys = ((ids[a:b, first:first + m].to(torch.int64) << 32) | rows).reshape(-1)
            keys = torch.sort(keys).values
            seg_ptr = torch.searchsorted(keys, bounds)
            _native.check(lib.flooder_dtm_grad_points_f32(_native.ptr(pts), n, _native.ptr(q[a:b]), b - a, dim,
                                                          _native.ptr(coef[a:b]), _native.ptr(keys), _native.ptr(seg_ptr),
                                                          None, n, _native.ptr(grad_p), st),
                          "flooder_dtm_grad_points_f32")
        if own:
            grad_p += grad_q
    return grad_p, grad_q


class _WeightedMeasure(torch.autograd.Function):
    """``distance_to_weighted_measure(differentiable=True)``: the computed ``value`` with the closed-form backward over
    the ``ids`` (Q, L) and ``count`` (Q,) the forward found (int32 on ROCm tensors, int64 padded with -1 on CPU tensors).
    ``value_sq``: the squared statistic (ROCm tensors; None on CPU tensors, which evaluate it again in float64);
    ``tau``: the (1,) float64 target on the device.  ``queries`` None: the sites themselves."""

    @staticmethod
    def forward(ctx, points, point_masses, queries, value, value_sq, ids, count, tau, mass, stat, squared):
        own = queries is None
        saved = [points, point_masses, points if own else queries, value, ids, count, tau]
        if value_sq is not None:
            saved.append(value_sq)
        ctx.save_for_backward(*saved)
        ctx.own, ctx.mass, ctx.stat, ctx.squared = own, mass, stat, squared
        return value.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        points, masses, qs, value, ids, count, tau, *rest = ctx.saved_tensors
        own = ctx.own
        need_p, need_m = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_q = own or ctx.needs_input_grad[2]
        backward = _mass_backward_hip if points.is_cuda else _mass_backward_cpu
        grad_p, grad_m, grad_q = backward(points.detach(), masses.detach(), qs.detach(), value, rest[0] if rest else None,
                                          ids, count, tau, ctx.mass, ctx.stat, ctx.squared, grad_out, own, need_p,
                                          need_m, need_q)
        return (grad_p, grad_m, (None if own or not ctx.needs_input_grad[2] else grad_q), None, None, None, None, None,
                None, None, None)


def _mass_backward_cpu(points, masses, qs, value, value_sq, ids, count, tau, mass: float, stat: str, squared: bool,
                       grad_out, own: bool, need_p: bool, need_m: bool, need_q: bool):
    """(grad_points, grad_masses, grad_queries; None where not needed) of the weighted measure on CPU tensors: the closed
    form in float64 torch on the kd-tree's ids, ``index_add_`` (sequential on the host: deterministic), in groups of
    query rows that keep the (rows, columns, dim) contributions of a group near 256 MB.  Rows that were not reached
    (value +inf) are masked out with ``torch.where``: they add exact zeros."""
    dt = points.dtype
    Q, dim = qs.shape
    n = points.shape[0]
    reached = torch.isfinite(value)
    g = torch.where(reached, grad_out.to(torch.float64), torch.zeros((), dtype=torch.float64))
    t = float(tau[0])
    x, q, mu = points.to(torch.float64), qs.to(torch.float64), masses.to(torch.float64)
    cnt = torch.where(reached, count, torch.zeros_like(count))
    width = max(1, int(cnt.max()))                     # (columns beyond the longest reached list hold nothing)
    last = (cnt - 1).clamp(min=0)
    if stat == "kth":                                  # y_(j*) alone: the form of distance_to_measure at m = 1
        cross = ids.gather(1, last.unsqueeze(1)).clamp(min=0)
        f = torch.where(reached, value.to(torch.float64), torch.ones((), dtype=torch.float64))
        coef = g * 2.0 if squared else torch.where(f > 0, g / torch.where(f > 0, f, torch.ones_like(f)), torch.zeros_like(f))
        grad_p, grad_q = _dtm_backward_cpu(x, q, cross, 0, 1, coef, own, need_p, need_q)
        return (None if grad_p is None else grad_p.to(dt), torch.zeros_like(masses) if need_m else None,
                None if grad_q is None else grad_q.to(dt))
    grad_q = torch.zeros((Q, dim), dtype=torch.float64) if need_q else None
    grad_p = torch.zeros((n, dim), dtype=torch.float64) if need_p else None
    grad_m = torch.zeros(n, dtype=torch.float64) if need_m else None
    dense = torch.zeros((), dtype=torch.float64)
    cols = torch.arange(width).unsqueeze(0)
    per_group = max(1, (256 << 20) // (width * dim * 8))
    for a in range(0, Q, per_group):
        b = min(Q, a + per_group)
        nb = ids[a:b, :width].clamp(min=0)
        before = cols < last[a:b].unsqueeze(1)                         # listed before the crossing
        at = (cols == last[a:b].unsqueeze(1)) & reached[a:b].unsqueeze(1)
        before = before & reached[a:b].unsqueeze(1)
        m_nb = torch.where(before, mu[nb], torch.zeros((), dtype=torch.float64))
        rho = t - m_nb.sum(dim=1)
        coeffs = m_nb + torch.where(at, rho.unsqueeze(1), torch.zeros((), dtype=torch.float64))      # a_t, 0 elsewhere
        diff = q[a:b].unsqueeze(1) - x[nb]                             # (rows, width, dim)
        d2 = diff.square().sum(dim=2)
        F = (coeffs * d2).sum(dim=1) / t
        if squared:
            c = g[a:b] * (2.0 / t)
        else:
            f = torch.sqrt(F)
            c = torch.where(f > 0, g[a:b] / (torch.where(f > 0, f, torch.ones_like(f)) * t), torch.zeros_like(f))
        contrib = (c.unsqueeze(1) * coeffs).unsqueeze(2) * diff
        if need_q:
            grad_q[a:b] = contrib.sum(dim=1)
        if need_p:
            grad_p.index_add_(0, nb.reshape(-1), -contrib.reshape(-1, dim))
        if need_m:
            h = 0.5 * c
            dstar2 = d2.gather(1, last[a:b].unsqueeze(1))
            listed = torch.where(before, h.unsqueeze(1) * (d2 - dstar2), torch.zeros((), dtype=torch.float64))
            grad_m.index_add_(0, nb.reshape(-1), listed.reshape(-1))
            dense = dense + (h * (dstar2.squeeze(1) - F)).sum()
    if need_p and own:
        grad_p += grad_q
    if need_m:
        grad_m += mass * dense
    return (None if grad_p is None else grad_p.to(dt), None if grad_m is None else grad_m.to(dt),
            None if grad_q is None else grad_q.to(dt))


def _mass_backward_hip(points, masses, qs, value, value_sq, ids, count, tau, mass: float, stat: str, squared: bool,
                       grad_out, own: bool, need_p: bool, need_m: bool, need_q: bool):
    """The same on ROCm float32 tensors.  ``"dtm"``: ``flooder_mass_grad_queries_f32`` over all queries (the query
    gradient and the crossing row - rho, the crossing id, dstar2 - of every query), then per group of ascending query rows
    the (target, query row) pairs of the PADDED rows as packed int64 keys - rows that were not reached masked to -1, and
    every negative key sorts in front of ``searchsorted``'s first bound and drops out -, sorted, the segment of every site
    by a binary search, and ``flooder_mass_grad_points_f32`` and (for the masses) ``flooder_mass_grad_masses_f32``, which
    continue the sequential sums per word from group to group: the gradient does not depend on ``core.DTM_GRAD_WORKSPACE_BYTES``.  The term every mass gets (tau depends on each) is one float64
    ``torch.sum``.  ``"kth"``: ``_dtm_backward_hip`` on the (Q, 1) column of crossing ids.  tau stays on the device;
    nothing here synchronises with the host."""
    lib = _native.load()
    dev = points.device
    torch.cuda.set_device(dev)
    st = _native.current_stream_ptr(dev)
    pts, q = points.contiguous(), qs.contiguous()
    (Q, dim), n, L = q.shape, pts.shape[0], ids.shape[1]
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    reached = torch.isfinite(value_sq)
    g = torch.where(reached, grad_out.to(torch.float32), zero)
    cnt = torch.where(reached, count, torch.zeros_like(count)).contiguous()
    if stat == "kth":
        cross = torch.where(reached, ids.gather(1, (cnt.long() - 1).clamp(min=0).unsqueeze(1)).squeeze(1),
                            torch.full_like(cnt, -1)).reshape(Q, 1).contiguous()
        coef = g * 2.0 if squared else torch.where(reached & (value > 0), g / value, zero)
        grad_p, grad_q = _dtm_backward_hip(pts, q, cross, 0, 1, coef, own, need_p, need_q)
        return grad_p, (torch.zeros_like(masses) if need_m else None), grad_q
    tau32 = tau.to(torch.float32)
    # coefficient of a_t (q - y_(t)): with unit masses (tau = k) the words of _DistanceToMeasure
    if squared:
        coef = g * (2.0 / tau32)
    else:
        coef = torch.where(reached & (value > 0), g / (value * tau32), zero)
    # the two layouts of csrc/flood_mass_grad.hip: a site's row is its coordinates, then its mass; a query's crossing row
    # is its coefficient, then what the first kernel writes - rho, the crossing id and dstar2
    sites = torch.cat([pts, masses.to(torch.float32).unsqueeze(1)], dim=1).contiguous()
    qrow = torch.empty((Q, 4), dtype=torch.float32, device=dev)
    qrow[:, 0] = coef
    grad_q = torch.empty((Q, dim), dtype=torch.float32, device=dev)
    _native.check(lib.flooder_mass_grad_queries_f32(_native.ptr(sites), n, _native.ptr(q), Q, dim, _native.ptr(ids), L,
                                                    _native.ptr(cnt), _native.ptr(tau), _native.ptr(qrow),
                                                    _native.ptr(grad_q), st), "flooder_mass_grad_queries_f32")
    grad_p = grad_m = None
    if need_p or need_m:
        grad_p = torch.zeros((n, dim), dtype=torch.float32, device=dev) if need_p else None
        grad_m = torch.zeros(n, dtype=torch.float32, device=dev) if need_m else None
        bounds = torch.arange(n + 1, dtype=torch.int64, device=dev) << 32
        per_group = max(1, min(Q, int(core.DTM_GRAD_WORKSPACE_BYTES) // (64 * L), ((1 << 31) - 1) // L))
        for a in range(0, Q, per_group):
            b = min(Q, a + per_group)
            rows = torch.arange(b - a, dtype=torch.int64, device=dev).unsqueeze(1)
            targets = torch.where(reached[a:b].unsqueeze(1), ids[a:b], torch.full_like(ids[a:b], -1)).to(torch.int64)
            keys = torch.sort(((targets << 32) | rows).reshape(-1)).values
            seg_ptr = torch.searchsorted(keys, bounds)
            for out, name in ((grad_p, "flooder_mass_grad_points_f32"), (grad_m, "flooder_mass_grad_masses_f32")):
                if out is not None:
                    _native.check(getattr(lib, name)(_native.ptr(sites), n, _native.ptr(q[a:b]), b - a, dim,
                                                     _native.ptr(qrow[a:b]), _native.ptr(keys), _native.ptr(seg_ptr),
                                                     None, n, _native.ptr(out), st), name)
        if need_p and own:
            grad_p += grad_q
        if need_m:      # what every mass gets because tau depends on it: mass * sum_q h_q (dstar2_q - F_q)
            spread = torch.where(reached, (0.5 * coef).double() * (qrow[:, 3].double() - value_sq.double()),
                                 torch.zeros((), dtype=torch.float64, device=dev))
            grad_m += (spread.sum() * mass).to(torch.float32)
    return grad_p, grad_m, (grad_q if need_q else None)


class _PowerDistance(torch.autograd.Function):
    """``power_distance`` with its closed-form backward.  ``queries`` None: the cloud's own points (both roles of a
    point accumulate into the gradient of ``points``)."""

    @staticmethod
    def forward(ctx, points, point_weights, queries, squared, index):
        own = queries is None
        qs = points if own else queries
        ids, value = _power_query(points, point_weights, qs, index, squared, True)
        ctx.save_for_backward(points, point_weights, qs, ids, value)
        ctx.own, ctx.squared = own, squared
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from .grad import _scatter_rows

        points, point_weights, qs, ids, value = ctx.saved_tensors
        own, squared = ctx.own, ctx.squared
        need_p, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_q = own or ctx.needs_input_grad[2]
        Q, dim = qs.shape
        dt, dev = points.dtype, points.device
        # coefficient of (q - x*) and of w*: grad_out * (1 / f, 0 where f == 0; or 2)
        coef = grad_out * 2.0 if squared else torch.where(value > 0, grad_out / value, torch.zeros_like(value))
        grad_q = (qs.detach() - points.detach()[ids]) * coef.unsqueeze(1)      # (Q, dim)
        grad_p = grad_w = None
        if need_p:
            targets, vals = [ids], [-grad_q]
            if own:
                targets.append(torch.arange(Q, dtype=torch.int64, device=dev))
                vals.append(grad_q)
            grad_p = _scatter_rows(targets, vals, points.shape[0], dim, dev, dt)
        if need_w:
            grad_w = _scatter_rows([ids], [(point_weights.detach()[ids] * coef).unsqueeze(1)], points.shape[0], 1, dev,
                                   dt).reshape(-1)
        return grad_p, grad_w, (grad_q if need_q and not own else None), None, None
