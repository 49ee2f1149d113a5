"""What the Python layer refuses around the robust filtration, with which exception and which message:
``flood_complex`` (``neighbors``, ``neighbor_stat``, ``neighbor_mass`` with every hook / ``shard_blocks`` / ``method``
combination that is refused), ``distance_to_measure``, ``nearest_neighbors``, ``neighbor_distance``,
``flood_filtration`` and ``flood_profile``.  Every call is refused before any work is done.  A call that is wrong in two
ways gets the message of the check that comes first: the order of the checks is part of the tables.

The expected exception types and whole messages were recorded from the package as it was while ``flood_complex``
still judged a mass by ``_check_neighbor_mass`` and a count by ``_check_neighbors`` one after the other, and
``distance_to_measure`` made its own k-from-mass checks: the tables assert those recorded values, not what the code
gives now (the method of ``test_knn_entry_refusals.py``).

A row is (function, cloud, keyword arguments, exception, whole message).  The clouds are named in ``_clouds``; a
keyword value that starts with "@" stands for an object that has no literal (``_OBJECTS``)."""
import pytest
import torch

import flooder_amd as fa

_OBJECTS = {
    "@hook": lambda t: t,                                   # a reduce / neighbour-reduce / face hook (never called)
    "@notindex": object(),                                  # an index= that is no PointIndex
    "@list": [[0.0, 0.0, 0.0]],                             # queries that are no tensor
}


def _clouds(device, n):
    """``n`` points in 3-D on ``device`` and what the tables derive from them."""
    g = torch.Generator().manual_seed(7)
    base = torch.randn(n, 3, generator=g)
    nine = torch.randn(n, 9, generator=g)
    clouds = {"pts": base, "f64": base.double(), "nine": nine, "few": base[:20], "empty": base[:0], "flat": base[:, 0],
              "half": base.half(), "big": torch.randn(1100, 3, generator=g)}
    clouds = {name: t.to(device).contiguous() for name, t in clouds.items()}
    clouds["notatensor"] = [[0.0, 0.0, 0.0]]
    objects = dict(_OBJECTS)
    qs = torch.randn(5, 3, generator=g)
    objects.update({"@qs2": qs[:, :2].to(device).contiguous(), "@qs64": qs.double().to(device), "@qscpu": qs})
    return clouds, objects, qs.to(device)


def _call(row, clouds, objects, qs):
    """Make the call of a table row -> (exception type name, whole message), or ("no exception", "")."""
    name, cloud, kwargs = row[:3]
    pts = clouds[cloud]
    kwargs = {k: objects[v] if isinstance(v, str) and v.startswith("@") else v for k, v in kwargs.items()}
    try:
        if name in ("flood_complex", "flood_filtration", "flood_profile"):
            base = pts if isinstance(pts, torch.Tensor) and pts.dim() == 2 and pts.shape[0] >= 8 else clouds["pts"]
            lms = base[:8].clone().to(pts.dtype if isinstance(pts, torch.Tensor) else base.dtype)
            getattr(fa, name)(pts, lms, points_per_edge=3, **kwargs)
        else:
            kwargs.setdefault("queries", qs.to(pts.dtype) if isinstance(pts, torch.Tensor) else qs)
            getattr(fa, name)(pts, **kwargs)
    except Exception as exc:   # noqa: BLE001 - the type is part of what is compared
        return type(exc).__name__, str(exc)
    return "no exception", ""


def _wrong(table, device, n):
    clouds, objects, qs = _clouds(device, n)
    return [(row[:3], got, row[3:]) for row in table for got in [_call(row, clouds, objects, qs)] if got != tuple(row[3:])]


CPU_TABLE = [
    ("flood_complex", "pts", dict(neighbors=0), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("flood_complex", "pts", dict(neighbors=33), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("flood_complex", "pts", dict(neighbors=-2), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got -2'),
    ("flood_complex", "pts", dict(neighbors=True), "TypeError",
     'neighbors must be an integer, got True'),
    ("flood_complex", "pts", dict(neighbors=2.0), "TypeError",
     'neighbors must be an integer, got 2.0'),
    ("flood_complex", "pts", dict(neighbors="3"), "TypeError",
     "neighbors must be an integer, got '3'"),
    ("flood_complex", "pts", dict(neighbors=None), "TypeError",
     'neighbors must be an integer, got None'),
    ("flood_complex", "few", dict(neighbors=32), "ValueError",
     'neighbors=32 exceeds the number of points (20)'),
    ("flood_complex", "empty", dict(neighbors=3), "ValueError",
     'neighbors=3 exceeds the number of points (0)'),
    ("flood_complex", "pts", dict(neighbors=1, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_stat=None), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got None"),
    ("flood_complex", "pts", dict(neighbors=0, neighbor_stat="mean"), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("flood_complex", "pts", dict(neighbors=33, method="cell"), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("flood_complex", "few", dict(neighbors=32, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "pts", dict(neighbors=3, method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbors=3, method="ball"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbors=3, method="nonsense"), "ValueError",
     "method must be 'cell', 'bvh' or 'ball', got 'nonsense'"),
    ("flood_complex", "pts", dict(neighbors=3, reduce_hook="@hook"), "ValueError",
     'neighbors > 1 cannot be combined with reduce_hook: a MIN over point shards is not the k-th nearest '
     'of their union'),
    ("flood_complex", "pts", dict(neighbors=3, shard_blocks=True), "ValueError",
     "neighbors > 1 cannot be combined with shard_blocks=True: a block's sub-cloud holds the points inside"
     " its simplices' bounding balls, which bound the nearest point only"),
    ("flood_complex", "pts", dict(neighbors=3, shard_blocks=True, simplex_shard=(0, 2)), "ValueError",
     "neighbors > 1 cannot be combined with shard_blocks=True: a block's sub-cloud holds the points inside"
     " its simplices' bounding balls, which bound the nearest point only"),
    ("flood_complex", "pts", dict(neighbors=3, method="cell", reduce_hook="@hook"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbors=3, reduce_hook="@hook", shard_blocks=True), "ValueError",
     'neighbors > 1 cannot be combined with reduce_hook: a MIN over point shards is not the k-th nearest '
     'of their union'),
    ("flood_complex", "few", dict(neighbors=32, method="cell"), "ValueError",
     'neighbors=32 exceeds the number of points (20)'),
    ("flood_complex", "pts", dict(neighbors=1, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_reduce_hook needs neighbors > 1: with one neighbour the reduction over point shards is a '
     'MIN, which is what reduce_hook is for'),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", reduce_hook="@hook"), "ValueError",
     "neighbor_reduce_hook cannot be combined with reduce_hook: the k-best merge of the shards' lists "
     'replaces the MIN of their minima'),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", shard_blocks=True), "ValueError",
     "neighbor_reduce_hook cannot be combined with shard_blocks=True: a block's sub-cloud holds the points"
     " inside its simplices' bounding balls, which bound the nearest point only"),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook"), "ValueError",
     "neighbor_reduce_hook needs ROCm tensors: the k-best merge of the point shards' lists is a device "
     'kernel and CPU tensors have no sharded k-nearest path'),
    ("flood_complex", "few", dict(neighbors=32, neighbor_reduce_hook="@hook"), "ValueError",
     "neighbor_reduce_hook needs ROCm tensors: the k-best merge of the point shards' lists is a device "
     'kernel and CPU tensors have no sharded k-nearest path'),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", method="cell"), "ValueError",
     "neighbor_reduce_hook needs ROCm tensors: the k-best merge of the point shards' lists is a device "
     'kernel and CPU tensors have no sharded k-nearest path'),
    ("flood_complex", "pts", dict(neighbors=1, neighbor_reduce_hook="@hook", reduce_hook="@hook"), "ValueError",
     'neighbor_reduce_hook needs neighbors > 1: with one neighbour the reduction over point shards is a '
     'MIN, which is what reduce_hook is for'),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "f64", dict(neighbors=3, neighbor_reduce_hook="@hook"), "ValueError",
     "neighbor_reduce_hook needs ROCm tensors: the k-best merge of the point shards' lists is a device "
     'kernel and CPU tensors have no sharded k-nearest path'),
    ("flood_complex", "pts", dict(neighbor_mass=0.2, neighbors=3), "ValueError",
     'neighbor_mass cannot be combined with neighbors=3: the mass fixes the number of neighbours (leave '
     'neighbors at 1)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.2, neighbors=2), "ValueError",
     'neighbor_mass cannot be combined with neighbors=2: the mass fixes the number of neighbours (leave '
     'neighbors at 1)'),
    ("flood_complex", "pts", dict(neighbor_mass=1.5, neighbors=2), "ValueError",
     'neighbor_mass cannot be combined with neighbors=2: the mass fixes the number of neighbours (leave '
     'neighbors at 1)'),
    ("flood_complex", "pts", dict(neighbor_mass="0.2", neighbors=2), "ValueError",
     'neighbor_mass cannot be combined with neighbors=2: the mass fixes the number of neighbours (leave '
     'neighbors at 1)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.2, neighbors=True), "ValueError",
     'neighbor_mass cannot be combined with neighbors=True: the mass fixes the number of neighbours (leave'
     ' neighbors at 1)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.2, neighbors=1.0), "ValueError",
     'neighbor_mass cannot be combined with neighbors=1.0: the mass fixes the number of neighbours (leave '
     'neighbors at 1)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.2, neighbors=0, neighbor_stat="mean"), "ValueError",
     'neighbor_mass cannot be combined with neighbors=0: the mass fixes the number of neighbours (leave '
     'neighbors at 1)'),
    ("flood_complex", "pts", dict(neighbor_mass="0.2"), "TypeError",
     "mass must be a real number in (0, 1], got '0.2'"),
    ("flood_complex", "pts", dict(neighbor_mass=True), "TypeError",
     'mass must be a real number in (0, 1], got True'),
    ("flood_complex", "pts", dict(neighbor_mass=[0.2]), "TypeError",
     'mass must be a real number in (0, 1], got [0.2]'),
    ("flood_complex", "pts", dict(neighbor_mass=0.0), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got 0.0'),
    ("flood_complex", "pts", dict(neighbor_mass=0), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got 0.0'),
    ("flood_complex", "pts", dict(neighbor_mass=-0.5), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got -0.5'),
    ("flood_complex", "pts", dict(neighbor_mass=1.5), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got 1.5'),
    ("flood_complex", "pts", dict(neighbor_mass=float("nan")), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got nan'),
    ("flood_complex", "pts", dict(neighbor_mass=float("inf")), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got inf'),
    ("flood_complex", "empty", dict(neighbor_mass=0.2), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("flood_complex", "empty", dict(neighbor_mass=1.5), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("flood_complex", "flat", dict(neighbor_mass=0.2), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (60,)'),
    ("flood_complex", "empty", dict(neighbor_mass=0.2, neighbor_stat="mean"), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, neighbor_stat="mean", method="cell"), "ValueError",
     "neighbor_mass needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, neighbor_stat="mean", method="cell"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, method="cell"), "ValueError",
     "neighbor_mass needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, method="ball"), "ValueError",
     "neighbor_mass needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, method="nonsense"), "ValueError",
     "method must be 'cell', 'bvh' or 'ball', got 'nonsense'"),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, method="ball"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, method="nonsense"), "ValueError",
     "method must be 'cell', 'bvh' or 'ball', got 'nonsense'"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=1e-09, reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, reduce_hook="@hook", neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, shard_blocks=True), "ValueError",
     'neighbor_mass cannot be combined with shard_blocks=True: a mass is a share of the WHOLE cloud, and a'
     " block's sub-cloud holds only the points inside its simplices' bounding balls"),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, shard_blocks=True, simplex_shard=(0, 2)), "ValueError",
     'neighbor_mass cannot be combined with shard_blocks=True: a mass is a share of the WHOLE cloud, and a'
     " block's sub-cloud holds only the points inside its simplices' bounding balls"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, reduce_hook="@hook", shard_blocks=True), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, reduce_hook="@hook", neighbor_stat="mean"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, reduce_hook="@hook", method="cell"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, shard_blocks=True, method="cell"), "ValueError",
     'neighbor_mass cannot be combined with shard_blocks=True: a mass is a share of the WHOLE cloud, and a'
     " block's sub-cloud holds only the points inside its simplices' bounding balls"),
    ("flood_complex", "pts", dict(neighbor_mass=1.5, reduce_hook="@hook"), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got 1.5'),
    ("flood_complex", "pts", dict(neighbor_mass=0.2, neighbors=2, reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with neighbors=2: the mass fixes the number of neighbours (leave '
     'neighbors at 1)'),
    ("flood_complex", "big", dict(neighbor_mass=1.0), "ValueError",
     'neighbor_mass=1.0 is 1100 neighbours of 1100 points, above KNN_WIDE_MAX = 1024 (the k best of a '
     'sample live in the LDS of one wave): the largest mass that fits this cloud is 0.930909'),
    ("flood_complex", "big", dict(neighbor_mass=0.95), "ValueError",
     'neighbor_mass=0.95 is 1045 neighbours of 1100 points, above KNN_WIDE_MAX = 1024 (the k best of a '
     'sample live in the LDS of one wave): the largest mass that fits this cloud is 0.930909'),
    ("flood_complex", "big", dict(neighbor_mass=1.0, method="cell"), "ValueError",
     'neighbor_mass=1.0 is 1100 neighbours of 1100 points, above KNN_WIDE_MAX = 1024 (the k best of a '
     'sample live in the LDS of one wave): the largest mass that fits this cloud is 0.930909'),
    ("flood_complex", "big", dict(neighbor_mass=1.0, neighbor_stat="mean"), "ValueError",
     'neighbor_mass=1.0 is 1100 neighbours of 1100 points, above KNN_WIDE_MAX = 1024 (the k best of a '
     'sample live in the LDS of one wave): the largest mass that fits this cloud is 0.930909'),
    ("flood_complex", "big", dict(neighbor_mass=1.0, reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "big", dict(neighbor_mass=1.0, shard_blocks=True), "ValueError",
     'neighbor_mass cannot be combined with shard_blocks=True: a mass is a share of the WHOLE cloud, and a'
     " block's sub-cloud holds only the points inside its simplices' bounding balls"),
    ("distance_to_measure", "pts", dict(), "ValueError",
     'distance_to_measure needs exactly one of mass and neighbors'),
    ("distance_to_measure", "pts", dict(mass=0.1, neighbors=30), "ValueError",
     'distance_to_measure needs exactly one of mass and neighbors'),
    ("distance_to_measure", "pts", dict(neighbor_stat="mean"), "ValueError",
     'distance_to_measure needs exactly one of mass and neighbors'),
    ("distance_to_measure", "pts", dict(mass=0.1, neighbors=30, neighbor_stat="mean"), "ValueError",
     'distance_to_measure needs exactly one of mass and neighbors'),
    ("distance_to_measure", "pts", dict(neighbors=0), "ValueError",
     'neighbors must be in 1..1024 (KNN_WIDE_MAX: the k best of a query live in the LDS of one wave), got '
     '0'),
    ("distance_to_measure", "pts", dict(neighbors=-1), "ValueError",
     'neighbors must be in 1..1024 (KNN_WIDE_MAX: the k best of a query live in the LDS of one wave), got '
     '-1'),
    ("distance_to_measure", "pts", dict(neighbors=1025), "ValueError",
     'neighbors must be in 1..1024 (KNN_WIDE_MAX: the k best of a query live in the LDS of one wave), got '
     '1025'),
    ("distance_to_measure", "pts", dict(neighbors=True), "TypeError",
     'neighbors must be an integer, got True'),
    ("distance_to_measure", "pts", dict(neighbors=2.0), "TypeError",
     'neighbors must be an integer, got 2.0'),
    ("distance_to_measure", "pts", dict(neighbors="3"), "TypeError",
     "neighbors must be an integer, got '3'"),
    ("distance_to_measure", "pts", dict(neighbors=61), "ValueError",
     'neighbors=61 exceeds the number of points (60)'),
    ("distance_to_measure", "pts", dict(neighbors=1024), "ValueError",
     'neighbors=1024 exceeds the number of points (60)'),
    ("distance_to_measure", "pts", dict(mass="0.5"), "TypeError",
     "mass must be a real number in (0, 1], got '0.5'"),
    ("distance_to_measure", "pts", dict(mass=True), "TypeError",
     'mass must be a real number in (0, 1], got True'),
    ("distance_to_measure", "pts", dict(mass=1.5), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got 1.5'),
    ("distance_to_measure", "pts", dict(mass=0.0), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got 0.0'),
    ("distance_to_measure", "pts", dict(mass=float("nan")), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got nan'),
    ("distance_to_measure", "pts", dict(mass=0.5, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("distance_to_measure", "pts", dict(mass=1.5, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("distance_to_measure", "pts", dict(neighbors=0, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("distance_to_measure", "pts", dict(neighbors=61, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("distance_to_measure", "big", dict(mass=1.0), "ValueError",
     'mass=1.0 is 1100 neighbours of 1100 points, above KNN_WIDE_MAX = 1024 (the k best of a query live in'
     ' the LDS of one wave): the largest mass that fits this cloud is 0.930909'),
    ("distance_to_measure", "big", dict(mass=0.95, queries=None), "ValueError",
     'mass=0.95 is 1045 neighbours of 1100 points, above KNN_WIDE_MAX = 1024 (the k best of a query live '
     'in the LDS of one wave): the largest mass that fits this cloud is 0.930909'),
    ("distance_to_measure", "big", dict(mass=1.0, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("distance_to_measure", "pts", dict(mass=0.1, queries="@qs2"), "RuntimeError",
     'queries must be a (Q, 3) tensor, got (5, 2)'),
    ("distance_to_measure", "pts", dict(mass=0.1, queries="@qs64"), "RuntimeError",
     'queries.dtype (torch.float64) != points.dtype (torch.float32)'),
    ("distance_to_measure", "pts", dict(mass=0.1, queries="@list"), "RuntimeError",
     'queries must be a (Q, 3) tensor, got list'),
    ("distance_to_measure", "pts", dict(mass=1.5, queries="@qs2"), "ValueError",
     'mass must be in (0, 1] (a share of the cloud), got 1.5'),
    ("distance_to_measure", "pts", dict(neighbors=61, queries="@qs2"), "ValueError",
     'neighbors=61 exceeds the number of points (60)'),
    ("distance_to_measure", "pts", dict(mass=0.1, index="@notindex"), "ValueError",
     'index= applies to ROCm tensors'),
    ("distance_to_measure", "pts", dict(mass=0.1, queries="@qs2", index="@notindex"), "RuntimeError",
     'queries must be a (Q, 3) tensor, got (5, 2)'),
    ("distance_to_measure", "empty", dict(mass=0.1), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("distance_to_measure", "empty", dict(mass=1.5), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("distance_to_measure", "empty", dict(), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("distance_to_measure", "flat", dict(mass=0.1), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (60,)'),
    ("distance_to_measure", "half", dict(mass=0.1), "TypeError",
     'dtype (torch.float16) not supported'),
    ("distance_to_measure", "half", dict(), "TypeError",
     'dtype (torch.float16) not supported'),
    ("distance_to_measure", "notatensor", dict(mass=0.1), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape list'),
    ("nearest_neighbors", "pts", dict(neighbors=0), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("nearest_neighbors", "pts", dict(neighbors=33), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("nearest_neighbors", "pts", dict(neighbors=True), "TypeError",
     'neighbors must be an integer, got True'),
    ("nearest_neighbors", "pts", dict(neighbors=2.0), "TypeError",
     'neighbors must be an integer, got 2.0'),
    ("nearest_neighbors", "few", dict(neighbors=32), "ValueError",
     'neighbors=32 exceeds the number of points (20)'),
    ("nearest_neighbors", "pts", dict(neighbors=3, queries="@qs2"), "RuntimeError",
     'queries must be a (Q, 3) tensor, got (5, 2)'),
    ("nearest_neighbors", "pts", dict(neighbors=3, queries="@qs64"), "RuntimeError",
     'queries.dtype (torch.float64) != points.dtype (torch.float32)'),
    ("nearest_neighbors", "pts", dict(neighbors=0, queries="@qs2"), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("nearest_neighbors", "pts", dict(neighbors=3, index="@notindex"), "ValueError",
     'index= applies to ROCm tensors'),
    ("nearest_neighbors", "empty", dict(neighbors=3), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("nearest_neighbors", "empty", dict(neighbors=0), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("nearest_neighbors", "half", dict(neighbors=3), "TypeError",
     'dtype (torch.float16) not supported'),
    ("nearest_neighbors", "flat", dict(neighbors=3), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (60,)'),
    ("neighbor_distance", "pts", dict(neighbors=0), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("neighbor_distance", "pts", dict(neighbors=33), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("neighbor_distance", "pts", dict(neighbors=True), "TypeError",
     'neighbors must be an integer, got True'),
    ("neighbor_distance", "pts", dict(neighbors="3"), "TypeError",
     "neighbors must be an integer, got '3'"),
    ("neighbor_distance", "few", dict(neighbors=32), "ValueError",
     'neighbors=32 exceeds the number of points (20)'),
    ("neighbor_distance", "pts", dict(neighbors=3, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("neighbor_distance", "pts", dict(neighbors=1, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("neighbor_distance", "pts", dict(neighbors=0, neighbor_stat="mean"), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("neighbor_distance", "few", dict(neighbors=32, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("neighbor_distance", "pts", dict(neighbors=3, queries="@qs2"), "RuntimeError",
     'queries must be a (Q, 3) tensor, got (5, 2)'),
    ("neighbor_distance", "pts", dict(neighbors=3, queries="@qs64"), "RuntimeError",
     'queries.dtype (torch.float64) != points.dtype (torch.float32)'),
    ("neighbor_distance", "pts", dict(neighbors=3, neighbor_stat="mean", queries="@qs2"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("neighbor_distance", "pts", dict(neighbors=3, index="@notindex"), "ValueError",
     'index= applies to ROCm tensors'),
    ("neighbor_distance", "empty", dict(neighbors=3), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("neighbor_distance", "half", dict(neighbors=3), "TypeError",
     'dtype (torch.float16) not supported'),
    ("neighbor_distance", "half", dict(neighbors=3, neighbor_stat="mean"), "TypeError",
     'dtype (torch.float16) not supported'),
    ("flood_filtration", "pts", dict(neighbors=0), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("flood_filtration", "pts", dict(neighbors=33), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("flood_filtration", "pts", dict(neighbors=True), "TypeError",
     'neighbors must be an integer, got True'),
    ("flood_filtration", "few", dict(neighbors=32), "ValueError",
     'neighbors=32 exceeds the number of points (20)'),
    ("flood_filtration", "pts", dict(neighbors=3, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_filtration", "pts", dict(neighbors=0, neighbor_stat="mean"), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("flood_filtration", "pts", dict(neighbors=3, method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_filtration", "pts", dict(neighbors=3, method="ball"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_filtration", "pts", dict(neighbors=1, method="ball"), "ValueError",
     "flood_filtration: method 'ball' has no exact witnesses (use 'cell' or 'bvh')"),
    ("flood_filtration", "pts", dict(neighbors=3, method="nonsense"), "ValueError",
     "method must be 'cell' or 'bvh', got 'nonsense'"),
    ("flood_filtration", "pts", dict(neighbors=1, method="nonsense"), "ValueError",
     "method must be 'cell' or 'bvh', got 'nonsense'"),
    ("flood_filtration", "pts", dict(neighbors=33, method="ball"), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("flood_filtration", "empty", dict(neighbors=3), "ValueError",
     'neighbors=3 exceeds the number of points (0)'),
    ("flood_filtration", "empty", dict(neighbors=1), "RuntimeError",
     'points must be a non-empty (N, d) tensor, got shape (0, 3)'),
    ("flood_filtration", "half", dict(neighbors=3), "TypeError",
     'dtype (torch.float16) not supported'),
    ("flood_filtration", "pts", dict(neighbors=3, index="@notindex"), "ValueError",
     'index= applies to ROCm tensors'),
    ("flood_profile", "pts", dict(neighbors=(1, 0)), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("flood_profile", "pts", dict(neighbors=(1, 33)), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("flood_profile", "pts", dict(neighbors=(2, True)), "TypeError",
     'neighbors must be an integer, got True'),
    ("flood_profile", "pts", dict(neighbors="3"), "TypeError",
     "neighbors must be an integer or a sequence of integers, got '3'"),
    ("flood_profile", "pts", dict(neighbors=2.0), "TypeError",
     'neighbors must be an integer or a sequence of integers, got 2.0'),
    ("flood_profile", "pts", dict(neighbors=()), "ValueError",
     'neighbors must not be empty'),
    ("flood_profile", "pts", dict(neighbors=(1, 2), neighbor_stat=()), "ValueError",
     'neighbor_stat must not be empty'),
    ("flood_profile", "pts", dict(neighbors=(1, 2), neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_profile", "pts", dict(neighbors=(1, 2), neighbor_stat=('kth', 'mean')), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_profile", "pts", dict(neighbors=(1, 0), neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_profile", "pts", dict(neighbors=(2, 2)), "ValueError",
     'neighbors lists a value twice: [2, 2]'),
    ("flood_profile", "pts", dict(neighbors=(1, 2), neighbor_stat=('kth', 'kth')), "ValueError",
     "neighbor_stat lists a name twice: ['kth', 'kth']"),
    ("flood_profile", "pts", dict(neighbors=(2, 2), neighbor_stat=('kth', 'kth')), "ValueError",
     'neighbors lists a value twice: [2, 2]'),
    ("flood_profile", "few", dict(neighbors=(1, 32)), "ValueError",
     'neighbors=32 exceeds the number of points (20)'),
    ("flood_profile", "pts", dict(neighbors=(1, 2), method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_profile", "pts", dict(neighbors=(1, 2), method="ball"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_profile", "pts", dict(neighbors=(1, 2), method="nonsense"), "ValueError",
     "method must be 'cell', 'bvh' or 'ball', got 'nonsense'"),
    ("flood_profile", "pts", dict(neighbors=(2, 33), method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_profile", "empty", dict(neighbors=(1, 2)), "ValueError",
     'neighbors=2 exceeds the number of points (0)'),
    ("flood_profile", "half", dict(neighbors=(1, 2)), "TypeError",
     'dtype (torch.float16) not supported'),
    ("flood_profile", "pts", dict(neighbors=(1, 2), index="@notindex"), "ValueError",
     'index= applies to ROCm tensors'),
]

GPU_TABLE = [
    ("flood_complex", "f64", dict(neighbors=3), "ValueError",
     'neighbors > 1 on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("flood_complex", "f64", dict(neighbors=3, method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "f64", dict(neighbors=3, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "f64", dict(neighbor_mass=0.9), "ValueError",
     'neighbor_mass on ROCm tensors needs float32: the wide k-nearest sweep has no float64 kernel'),
    ("flood_complex", "f64", dict(neighbor_mass=0.1), "ValueError",
     'neighbors > 1 on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("flood_complex", "f64", dict(neighbor_mass=0.9, method="cell"), "ValueError",
     "neighbor_mass needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "f64", dict(neighbor_mass=0.9, neighbor_stat="mean"), "ValueError",
     'neighbor_mass on ROCm tensors needs float32: the wide k-nearest sweep has no float64 kernel'),
    ("flood_complex", "f64", dict(neighbor_mass=0.9, reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "f64", dict(neighbors=3, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_reduce_hook needs float32 ROCm tensors: the k-nearest sweep and the merge of its lists have'
     ' no float64 kernel'),
    ("flood_complex", "f64", dict(neighbors=3, reduce_hook="@hook"), "ValueError",
     'neighbors > 1 cannot be combined with reduce_hook: a MIN over point shards is not the k-th nearest '
     'of their union'),
    ("flood_filtration", "f64", dict(neighbors=3), "ValueError",
     'neighbors > 1 on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("flood_filtration", "f64", dict(neighbors=1), "TypeError",
     'flood_filtration: ROCm float64 tensors are not supported (pass float32)'),
    ("flood_profile", "f64", dict(neighbors=(1, 2)), "ValueError",
     'neighbors > 1 on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("neighbor_distance", "f64", dict(neighbors=3), "ValueError",
     'neighbor_distance on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("neighbor_distance", "f64", dict(neighbors=1), "ValueError",
     'neighbor_distance on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("neighbor_distance", "f64", dict(neighbors=0), "ValueError",
     'neighbor_distance on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("nearest_neighbors", "f64", dict(neighbors=3), "ValueError",
     'neighbor_distance on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("distance_to_measure", "f64", dict(mass=0.9), "ValueError",
     'distance_to_measure on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("distance_to_measure", "f64", dict(neighbors=3), "ValueError",
     'distance_to_measure on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("distance_to_measure", "f64", dict(), "ValueError",
     'distance_to_measure on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("distance_to_measure", "f64", dict(mass=1.5), "ValueError",
     'distance_to_measure on ROCm tensors needs float32: the k-nearest sweep has no float64 kernel'),
    ("flood_complex", "nine", dict(neighbors=3), "ValueError",
     'neighbors > 1 on ROCm tensors needs ambient dimension 2 to 8'),
    ("flood_complex", "nine", dict(neighbors=3, reduce_hook="@hook"), "ValueError",
     'neighbors > 1 cannot be combined with reduce_hook: a MIN over point shards is not the k-th nearest '
     'of their union'),
    ("flood_complex", "nine", dict(neighbor_mass=0.9), "ValueError",
     'neighbor_mass on ROCm tensors needs ambient dimension 2 to 8'),
    ("flood_complex", "nine", dict(neighbor_mass=0.1), "ValueError",
     'neighbors > 1 on ROCm tensors needs ambient dimension 2 to 8'),
    ("flood_complex", "nine", dict(neighbor_mass=0.9, method="ball"), "ValueError",
     "neighbor_mass needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "nine", dict(neighbors=3, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbors > 1 on ROCm tensors needs ambient dimension 2 to 8'),
    ("flood_complex", "nine", dict(neighbors=1), "RuntimeError",
     'flooder_amd: ambient dimension > 8 is not supported by the HIP kernels'),
    ("flood_filtration", "nine", dict(neighbors=3), "ValueError",
     'neighbors > 1 on ROCm tensors needs ambient dimension 2 to 8'),
    ("flood_filtration", "nine", dict(neighbors=1), "ValueError",
     'flood_filtration: ROCm tensors need ambient dimension 2 to 8'),
    ("flood_profile", "nine", dict(neighbors=(1, 2)), "ValueError",
     'neighbors > 1 on ROCm tensors needs ambient dimension 2 to 8'),
    ("neighbor_distance", "nine", dict(neighbors=3), "ValueError",
     'neighbor_distance on ROCm tensors needs ambient dimension 2 to 8'),
    ("neighbor_distance", "nine", dict(neighbors=3, neighbor_stat="mean"), "ValueError",
     'neighbor_distance on ROCm tensors needs ambient dimension 2 to 8'),
    ("nearest_neighbors", "nine", dict(neighbors=3), "ValueError",
     'neighbor_distance on ROCm tensors needs ambient dimension 2 to 8'),
    ("distance_to_measure", "nine", dict(mass=0.9), "ValueError",
     'distance_to_measure on ROCm tensors needs ambient dimension 2 to 8'),
    ("distance_to_measure", "nine", dict(neighbors=0), "ValueError",
     'distance_to_measure on ROCm tensors needs ambient dimension 2 to 8'),
    ("flood_complex", "pts", dict(neighbors=1, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_reduce_hook needs neighbors > 1: with one neighbour the reduction over point shards is a '
     'MIN, which is what reduce_hook is for'),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", reduce_hook="@hook"), "ValueError",
     "neighbor_reduce_hook cannot be combined with reduce_hook: the k-best merge of the shards' lists "
     'replaces the MIN of their minima'),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", shard_blocks=True), "ValueError",
     "neighbor_reduce_hook cannot be combined with shard_blocks=True: a block's sub-cloud holds the points"
     " inside its simplices' bounding balls, which bound the nearest point only"),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", method="ball"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbors=3, neighbor_reduce_hook="@hook", method="nonsense"), "ValueError",
     "method must be 'cell', 'bvh' or 'ball', got 'nonsense'"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, neighbor_reduce_hook="@hook"), "ValueError",
     'neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook: a mass is a share of the '
     'WHOLE cloud, and a shard of the points does not know how many there are (pass neighbors=k to the '
     'sharded call)'),
    ("flood_complex", "pts", dict(neighbors=3, method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbors=3, method="ball"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbors=3, method="nonsense"), "ValueError",
     "method must be 'cell', 'bvh' or 'ball', got 'nonsense'"),
    ("flood_complex", "pts", dict(neighbors=3, reduce_hook="@hook"), "ValueError",
     'neighbors > 1 cannot be combined with reduce_hook: a MIN over point shards is not the k-th nearest '
     'of their union'),
    ("flood_complex", "pts", dict(neighbors=3, shard_blocks=True, simplex_shard=(0, 2)), "ValueError",
     "neighbors > 1 cannot be combined with shard_blocks=True: a block's sub-cloud holds the points inside"
     " its simplices' bounding balls, which bound the nearest point only"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, method="cell"), "ValueError",
     "neighbor_mass needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbor_mass=0.1, method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, method="nonsense"), "ValueError",
     "method must be 'cell', 'bvh' or 'ball', got 'nonsense'"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, shard_blocks=True), "ValueError",
     'neighbor_mass cannot be combined with shard_blocks=True: a mass is a share of the WHOLE cloud, and a'
     " block's sub-cloud holds only the points inside its simplices' bounding balls"),
    ("flood_complex", "pts", dict(neighbor_mass=0.9, neighbor_stat="mean"), "ValueError",
     "neighbor_stat must be one of ('kth', 'dtm'), got 'mean'"),
    ("flood_complex", "pts", dict(neighbors=33), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("flood_filtration", "pts", dict(neighbors=3, method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_filtration", "pts", dict(neighbors=3, method="ball"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'ball' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_profile", "pts", dict(neighbors=(1, 2), method="cell"), "ValueError",
     "neighbors > 1 needs the tree sweep: method 'cell' evaluates the nearest point only (use method=None,"
     " 'auto' or 'bvh')"),
    ("flood_filtration", "pts", dict(neighbors=33), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("neighbor_distance", "pts", dict(neighbors=33), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 33'),
    ("nearest_neighbors", "pts", dict(neighbors=0), "ValueError",
     'neighbors must be in 1..32 (KNN_MAX: the k best of a sample live in registers of the kernel), got 0'),
    ("distance_to_measure", "pts", dict(neighbors=1025), "ValueError",
     'neighbors must be in 1..1024 (KNN_WIDE_MAX: the k best of a query live in the LDS of one wave), got '
     '1025'),
    ("distance_to_measure", "pts", dict(neighbors=65), "ValueError",
     'neighbors=65 exceeds the number of points (64)'),
    ("distance_to_measure", "pts", dict(mass=0.1, queries="@qs2"), "RuntimeError",
     'queries must be a (Q, 3) tensor, got (5, 2)'),
    ("neighbor_distance", "pts", dict(neighbors=3, queries="@qscpu"), "RuntimeError",
     'queries.device (cpu) != points.device (cuda:0)'),
    ("neighbor_distance", "pts", dict(neighbors=3, index="@notindex"), "ValueError",
     'index= is not a PointIndex of these points (shape or device differ)'),
    ("distance_to_measure", "pts", dict(mass=0.5, index="@notindex"), "ValueError",
     'index= is not a PointIndex of these points (shape or device differ)'),
]


def test_tables_cover_what_they_must():
    for table, least in ((CPU_TABLE, 150), (GPU_TABLE, 60)):
        assert len(table) >= least and len({repr(row[:3]) for row in table}) == len(table)
        assert all(row[3] != "no exception" and row[4] for row in table)
    assert {row[0] for row in CPU_TABLE} == {"flood_complex", "flood_filtration", "flood_profile", "distance_to_measure",
                                            "nearest_neighbors", "neighbor_distance"}
    mass = [row for row in CPU_TABLE if row[0] == "flood_complex" and "neighbor_mass" in row[2]]
    assert len(mass) >= 50 and sum(1 for row in mass if len(row[2]) >= 2) >= 30          # wrong in two ways
    assert {row[1] for row in GPU_TABLE} == {"pts", "f64", "nine"}


def test_cpu_refusals_are_the_recorded_ones():
    wrong = _wrong(CPU_TABLE, "cpu", 60)
    assert not wrong, wrong


@pytest.mark.gpu
def test_rocm_refusals_are_the_recorded_ones():
    """float64, ambient dimension 9, ``neighbor_reduce_hook`` and ``method="cell"`` with k > 1 on ROCm tensors of 64
    points: each a refusal before any launch."""
    wrong = _wrong(GPU_TABLE, "cuda", 64)
    assert not wrong, wrong
