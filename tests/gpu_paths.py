"""The table of "every GPU path": the calls, their options and the checks that say which path ran.  Shared by
test_gpu_streams.py (every path on a side stream while the default stream is held) and test_gpu_poisoned_workspaces.py
(every path on poisoned, guarded workspaces).  The cloud size is an argument of the builders: the streams tests pass
their round 20 000 / 8 000, the poisoned tests ragged sizes."""
import warnings

import numpy as np
import torch

import flooder_amd as fa
from flooder_amd import core

DEV = torch.device("cuda:0")


def randn(n, dim, seed, scale=1.0):
    return (scale * torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))).to(DEV)


# --------------------------------------------------------------------------------------------------- index
def index_parts(idx):
    """Rows, box tree, order, density grid, and the lanes of the box that are defined ([0:dim] min, [8:8+dim] max)."""
    return ([idx.pts, idx.nodes, idx.order32, idx.box[:idx.dim], idx.box[8:8 + idx.dim]]
            + ([] if idx.dens is None else [idx.dens]))


# (dim, SORT_STATE_BY_CALLER); 6-D: rows in k-d tree order
INDEX_CASES = [(2, True), (2, False), (3, True), (3, False), (6, True)]

# --------------------------------------------------------------------------------------------------- landmarks
N_LMS = 300
FPS_CASES = {
    # name: (dim, method, FPS_BATCHED, options of the library, launches: None = not the batched entry)
    "brute": (3, "brute", True, {}, None),
    "one_per_launch": (3, "bucket", False, {}, None),
    "batched": (3, "bucket", True, dict(fps_switch=8), "batched"),
    "batched_rounds": (3, "bucket", True, dict(fps_switch=8, fps_rounds=1), "batched"),
    "batched_lane_best": (3, "bucket", True, dict(fps_switch=8, fps_lane_best=1), "batched"),
    "batched_5d": (5, "bucket", True, dict(fps_switch=8), "batched"),
}


# --------------------------------------------------------------------------------------------------- flood_complex
def flood(p, w=None, n_lms=50, **kw):
    if kw.get("num_rand") is not None:
        torch.manual_seed(7)     # (the weights are drawn from the CPU generator)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (float64: the documented warning)
        return fa.flood_complex(p, n_lms, point_weights=w, **kw)


def flood_cases(n):
    """name: (dim, dtype, arguments, the dimension-pass driver of core that must run) for a cloud of ``n`` points."""
    return {
        "2d": (2, torch.float32, dict(points_per_edge=20), "_sweep_dimension_cell"),
        "3d": (3, torch.float32, dict(points_per_edge=12), "_sweep_dimension_cell"),
        "3d_bvh": (3, torch.float32, dict(points_per_edge=12, method="bvh"), "_sweep_dimension_bvh"),
        "3d_ball": (3, torch.float32, dict(points_per_edge=12, method="ball"), "_sweep_dimension_hip"),
        "6d": (6, torch.float32, dict(n_lms=24, max_dimension=2, points_per_edge=8), "_sweep_dimension_bvh"),
        "3d_float64": (3, torch.float64, dict(points_per_edge=10), "_sweep_dimension_f64"),
        "3d_neighbors_4": (3, torch.float32, dict(points_per_edge=10, neighbors=4, neighbor_stat="kth"), "_sweep_dimension_knn"),
        "3d_mass_100": (3, torch.float32, dict(points_per_edge=8, neighbor_mass=100 / n, neighbor_stat="dtm"),
                        "_sweep_dimension_knn"),
        "3d_power": (3, torch.float32, dict(points_per_edge=12), "_sweep_dimension_power"),
        "3d_num_rand": (3, torch.float32, dict(points_per_edge=None, num_rand=300), "_sweep_dimension_cell"),
    }


FLOOD_CASE_NAMES = tuple(flood_cases(1))
SWEEP_DRIVERS = ("_sweep_dimension_cell", "_sweep_dimension_bvh", "_sweep_dimension_hip", "_sweep_dimension_f64",
                 "_sweep_dimension_knn", "_sweep_dimension_power")


def watch_sweeps(monkeypatch):
    """Which dimension-pass drivers of ``core`` run from now on, and with how many neighbours -> (set of names, set of k)."""
    ran, ks = set(), set()
    for name in SWEEP_DRIVERS:
        def watched(*a, _name=name, _f=getattr(core, name), **k):
            ran.add(_name)
            if _name == "_sweep_dimension_knn":
                ks.add(int(a[4]))
            return _f(*a, **k)
        monkeypatch.setattr(core, name, watched)
    return ran, ks


def flood_arguments(case, n, seeds):
    """The argument tuples of ``flood(*args, **kw)`` for ``case`` on clouds of ``n`` points, one per seed offset of
    ``seeds`` (the cloud of seed s + dim; the power case adds weights)."""
    dim, dtype, _, _ = flood_cases(n)[case]
    args = [(randn(n, dim, s + dim).to(dtype),) for s in seeds]
    if case == "3d_power":
        g = torch.Generator().manual_seed(8)
        args = [(p, (0.2 * torch.rand(n, generator=g)).to(DEV)) for (p,) in args]
    return args


def check_flood_path(case, n, ran, ks):
    """The path: the driver the case is about ran, the default cell sweep only where it is the case; the k-nearest cases
    at their k (4: the register ladder; 100 > core.KNN_MAX: flooder_knn_wide_f32)."""
    driver = flood_cases(n)[case][3]
    assert driver in ran and (driver == "_sweep_dimension_cell" or "_sweep_dimension_cell" not in ran), sorted(ran)
    if driver == "_sweep_dimension_knn":
        assert ks == ({4} if case == "3d_neighbors_4" else {100}) and core.KNN_MAX < 100


# --------------------------------------------------------------------------------------------------- neighbours
def weighted_measure(p, q, cell, mass, cap):
    sites, mu = fa.voxel_measure(p, cell)
    v, ids, dist, count = fa.distance_to_weighted_measure(sites, mu, q, mass=mass, max_neighbors=cap, return_neighbors=True)
    return [sites, mu, v, ids, dist, count]


NEIGHBOUR_CALLS = {
    "neighbor_distance k=8 dtm": lambda p, q, w: fa.neighbor_distance(p, q, neighbors=8, neighbor_stat="dtm"),
    "nearest_neighbors k=8": lambda p, q, w: list(fa.nearest_neighbors(p, q, neighbors=8)),
    "distance_to_measure k=16": lambda p, q, w: fa.distance_to_measure(p, q, neighbors=16),
    "distance_to_measure k=100": lambda p, q, w: list(fa.distance_to_measure(p, q, neighbors=100, return_neighbors=True)),
    "distance_to_measure_profile": lambda p, q, w: fa.distance_to_measure_profile(p, q, neighbors=(4, 32, 100)),
    "power_distance": lambda p, q, w: fa.power_distance(p, w, q),
    "power_nearest": lambda p, q, w: list(fa.power_nearest(p, w, q)),
    "distance_to_weighted_measure": lambda p, q, w: weighted_measure(p, q, 2.0, 0.02, 64),
}


def neighbour_clouds(n, n_queries, seeds=(80, 90)):
    """Integer-valued Gaussian clouds (ties are decided by id; dense in the middle, single points far out) and queries
    that reach beyond them; weights for the power distance.  One (points, queries, weights) per seed."""
    out = []
    for seed in seeds:
        g = torch.Generator().manual_seed(seed)
        p = torch.round(8 * torch.randn(n, 3, generator=g)).to(DEV)
        q = torch.round(10 * torch.randn(n_queries, 3, generator=g)).to(DEV)
        w = torch.randint(0, 6, (n,), generator=g).float().to(DEV)
        out.append((p, q, w))
    return out


def check_neighbour_result(call, ref):
    if call == "distance_to_weighted_measure":
        missed = int(np.isinf(ref[2]).sum())
        assert 0 < missed < ref[2].shape[0], f"{missed} of {ref[2].shape[0]} queries not reached: the case needs both kinds"


# --------------------------------------------------------------------------------------------------- profiles
def tables(prof, dim):
    return [prof.table(d)[1] for d in range(dim + 1)]


def profile_calls(n):
    return {
        "flood_profile": lambda p, w: tables(fa.flood_profile(p, 40, points_per_edge=8, neighbors=(1, 4, 16),
                                                              neighbor_stat=("kth", "dtm")), 3),
        "power_profile": lambda p, w: tables(fa.power_profile(p, 40, w, points_per_edge=8), 3),
        "dtm_profile": lambda p, w: tables(fa.dtm_profile(p, 40, masses=(20 / n, 100 / n), points_per_edge=8), 3),
    }


PROFILE_CALL_NAMES = tuple(profile_calls(1))


def profile_arguments(n, count=2):
    g = torch.Generator().manual_seed(11)
    return [(randn(n, 3, 100 + i), (0.2 * torch.rand(n, 3, generator=g)).to(DEV)) for i in range(count)]


# --------------------------------------------------------------------------------------------------- gradients
def with_grad(build):
    """f(points, ...): a leaf made on the current stream, ``build(leaf, ...)`` -> differentiable tensors, the gradient
    of a fixed weighted sum of them; the values and the gradient."""
    def f(p, *rest):
        x = p.clone().requires_grad_(True)
        values = build(x, *rest)
        loss = sum((torch.linspace(0.5, 1.5, v.numel(), device=v.device) * torch.nan_to_num(v, posinf=0.0).flatten()).sum()
                   for v in values)
        (grad,) = torch.autograd.grad(loss, x)
        return [v.detach() for v in values] + [grad]
    return f


GRAD_KW = dict(points_per_edge=8)


def grad_calls(n):
    return {
        "flood_filtration": lambda x: fa.flood_filtration(x, 40, **GRAD_KW).values,
        "flood_filtration 2-D": lambda x: fa.flood_filtration(x[:, :2].contiguous(), 40, points_per_edge=12).values,
        "power_filtration": lambda x: fa.power_filtration(x, 40, 0.1 * x.detach().abs().sum(dim=1), **GRAD_KW).values,
        "dtm_filtration mass": lambda x: fa.dtm_filtration(x, 40, 100 / n, **GRAD_KW).values,
        "dtm_filtration cell_size": lambda x: fa.dtm_filtration(x, 40, 0.05, cell_size=0.1, max_neighbors=256, **GRAD_KW).values,
        "distance_to_measure differentiable k=16": lambda x: [fa.distance_to_measure(x, neighbors=16, differentiable=True)],
        "distance_to_measure differentiable k=100": lambda x: [fa.distance_to_measure(x, neighbors=100, differentiable=True)],
        "distance_to_weighted_measure differentiable": lambda x: [fa.distance_to_weighted_measure(
            *fa.voxel_measure(x, 0.1, differentiable=True), x, 0.05, max_neighbors=256, differentiable=True)],
    }


GRAD_CALL_NAMES = tuple(grad_calls(1))


def grad_clouds(n, seeds=(120, 130)):
    return [torch.rand(n, 3, generator=torch.Generator().manual_seed(s)).to(DEV) for s in seeds]
