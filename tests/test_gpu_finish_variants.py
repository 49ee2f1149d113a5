"""The finish (csrc/flood_finish.hip) under the options that pick its kernel and its launch shape: the wide kernel
(finish_faces_kernel<DIM, false, 8>: eight waves share one staged tree top, "finish_wide_points") in 2-D and 3-D on
clouds of a few ten thousand points, "finish_items_cap", "finish_focus_pct", "finish_refresh", "bvh_refine_pct" and
"bvh_grid" down to one workgroup.

Kernel level: the harness of ``test_gpu_finish_single`` (hand-built flag lists, every sample unsettled from +inf) on
lists shorter and longer than the short-list launch takes; every variant bit for bit the default, the tree sweep, and
within helpers' tolerance the kd-tree; and every case shows through the counters that the per-wave passes - the code
the options reach - did the work.  End to end: ``core._sweep_dimension_cell`` with hard tiles on, under the wide kernel
and under grids of one and three workgroups (the team launch used to get ``bvh_grid / 4`` = 0 workgroups there).
Runs on a real MI355X only (-m gpu)."""
import functools

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from oracle import flood_oracle as fo

import variant_cases as vc
from helpers import assert_close_filtration, get_options
from variant_cases import INT_MAX, Setup, all_tiles, finish, options, single_tiles

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CLOUDS = ("gauss2d", "eight2d", "gauss3d", "eight3d")
# what a variant sets on top of the list's own "bvh_subs"
VARIANTS = {
    "wide": dict(finish_wide_points=1),
    "items_cap": dict(finish_items_cap=1024),
    "focus_0": dict(finish_focus_pct=0), "focus_100": dict(finish_focus_pct=100),
    "refresh_1": dict(finish_refresh=1), "refresh_never": dict(finish_refresh=INT_MAX),
    "refine_always": dict(bvh_refine_pct=1), "refine_never": dict(bvh_refine_pct=INT_MAX),
    "grid_1": dict(bvh_grid=1), "grid_3": dict(bvh_grid=3), "grid_4": dict(bvh_grid=4),
    "wide_grid_1": dict(finish_wide_points=1, bvh_grid=1),
}


def test_variants_are_the_listed_values():
    mine = vc.SET_BY["test_gpu_finish_variants"]
    seen = {}
    for opts in VARIANTS.values():
        for name, v in opts.items():
            seen.setdefault(name, set()).add(v)
    seen["bvh_subs"] = {1}
    assert {k: tuple(sorted(v)) for k, v in seen.items()} == {k: tuple(sorted(v)) for k, v in mine.items()}


def _points(name):
    g = torch.Generator().manual_seed(11 + len(name))
    if name == "gauss2d":
        return torch.randn(30_000, 2, generator=g)
    if name == "gauss3d":
        return torch.randn(40_000, 3, generator=g)
    flat = fa.generate_figure_eight_points_2d(60_000 if name == "eight2d" else 20_000, noise_std=0.02, seed=3).float()
    if name == "eight2d":
        return flat
    return torch.cat([flat, 0.02 * torch.randn(flat.shape[0], 1, generator=g)], dim=1)    # the same curve as a thin sheet


@functools.lru_cache(maxsize=None)
def _setup(name):
    """2-D: 33 points per edge (561 rows, 9 tiles per simplex); 3-D: 17 (969 rows, 16 tiles)."""
    pts = _points(name)
    su = Setup(pts.contiguous(), DEV, 120 if pts.shape[1] == 2 else 80, 33 if pts.shape[1] == 2 else 17)
    assert 20_000 <= pts.shape[0] <= 60_000 and su.R % 64 != 0
    return su


@functools.lru_cache(maxsize=None)
def _baseline(name, kind):
    """(the simplices, the flagged tiles, bvh_subs of the list, face bits of the default run).  "long": more tiles than
    the short-list launch takes - the per-wave passes do all the work under the library's own bvh_subs; "short": fewer,
    with bvh_subs 1, which turns the short-list launch off, so that again the passes do.  The default run is checked
    against the tree sweep bit for bit and against the kd-tree."""
    su, T = _setup(name), single_tiles()
    if kind == "long":
        n_s = T // su.tiles + 8
        subs = get_options(_native.load(), b"bvh_subs")[b"bvh_subs"]
        assert subs > 1
    else:
        n_s, subs = T // su.tiles // 2, 1
    assert su.verts.shape[0] >= n_s, (name, su.verts.shape[0], n_s)
    verts = su.verts[:n_s].contiguous()
    tiles = all_tiles(n_s, su.tiles)
    assert (len(tiles) > T) == (kind == "long")
    bits, stats, left = finish(su, verts, tiles, subs)
    print(name, kind, "S", n_s, "tiles", len(tiles), "stats", stats.tolist(), "left", left)
    assert stats[6] > 0 and left == 0, f"{name} {kind}: the per-wave passes did not do the work: {stats.tolist()}, {left}"
    tree, _ = core._sweep_dimension_bvh(su.index, verts, su.weights, su.faces, None)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits, tree.view(torch.int32).cpu().numpy(), err_msg=f"{name} {kind}: differs from the tree sweep")
    assert_close_filtration(bits.view(np.float32).max(axis=1), su.kdtree_top(verts), su.pts.cpu().numpy(), f"{name} {kind}")
    return verts, tiles, subs, bits


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", ["short", "long"])
@pytest.mark.parametrize("name", CLOUDS)
def test_variant_equals_the_default(name, kind, variant):
    su = _setup(name)
    verts, tiles, subs, want = _baseline(name, kind)
    bits, stats, left = finish(su, verts, tiles, subs, **VARIANTS[variant])
    print(name, kind, variant, stats.tolist(), left)
    assert stats[6] > 0 and stats[0] > 0 and left == 0, f"the per-wave passes did not do the work: {stats.tolist()}, {left}"
    np.testing.assert_array_equal(bits, want, err_msg=f"{name} {kind} {variant}: differs from the default")


@pytest.mark.parametrize("name", CLOUDS)
def test_wide_kernel_without_split_tiles_on_a_long_list(name):
    """The wide kernel with "bvh_subs" 1 on the long list: 64 distinct samples per wave, eight waves per workgroup."""
    su = _setup(name)
    verts, tiles, _, want = _baseline(name, "long")
    bits, stats, left = finish(su, verts, tiles, 1, finish_wide_points=1)
    assert stats[6] > 0 and left == 0, stats.tolist()
    np.testing.assert_array_equal(bits, want, err_msg=f"{name}: wide, bvh_subs 1")


@pytest.mark.parametrize("name", CLOUDS)
def test_short_list_with_the_short_list_launch_on(name):
    """The variants on the short list as the product runs it (the short-list launch first): same bits, whatever is
    left over for the passes behind it."""
    su = _setup(name)
    verts, tiles, _, want = _baseline(name, "short")
    subs = get_options(_native.load(), b"bvh_subs")[b"bvh_subs"]
    for variant, opts in VARIANTS.items():
        bits, stats, left = finish(su, verts, tiles, subs, **opts)
        assert stats[0] > 0 and stats[5] > 0, (variant, stats.tolist())
        np.testing.assert_array_equal(bits, want, err_msg=f"{name} {variant}: short list, short-list launch on")


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _product(dim):
    """The clouds and the lattice of ``test_finish_hard_tiles_and_ordering_change_nothing`` (200 landmarks, 30 points
    per edge), and of their top simplices the few nearest the middle of the cloud - the hole of the torus, the crossing of
    the figure eight: long searches.  Few, because a tile is hard when it evaluates more leaves than ``finish_budget``
    times the tiles per wave of the launch: under a grid of one workgroup a list of thousands of tiles has no hard tile
    at all, a list of a few dozen has (measured: 2 tetrahedra flag 156 tiles, 1200 to 2500 hard rounds under every grid;
    16 triangles flag 8, 4 hard rounds under every grid)."""
    if dim == 3:
        pts, keep = torch.as_tensor(fo.noisy_torus(100_000, seed=13), device=DEV), 2
    else:
        pts, keep = fa.generate_figure_eight_points_2d(200_000, noise_std=0.02, seed=3).to(DEV), 16
    lms = fa.generate_landmarks(pts, 200, start_idx=0)
    _, simplices = core._build_complex(lms, dim)
    verts = lms[torch.as_tensor(simplices[dim], device=DEV)]
    c = verts.mean(dim=1) - pts.mean(dim=0)
    verts = verts[torch.argsort((c * c).sum(dim=1))[:keep]].contiguous()
    weights, _, fi = core.generate_grid(30, dim, DEV, torch.float32)
    faces = core._FaceTable(fi, weights.shape[0], DEV)
    index = core.PointIndex(pts)
    ref, _ = core._sweep_dimension_cell(index, verts, weights, faces, None)
    tree, _ = core._sweep_dimension_bvh(index, verts, weights, faces, None)
    torch.cuda.synchronize()
    assert torch.equal(ref.view(torch.int32), tree.view(torch.int32)), "the default cell sweep differs from the tree sweep"
    return index, verts, weights, faces, ref.cpu().numpy()


@pytest.mark.parametrize("variant", ["wide", "grid_1", "grid_3", "wide_grid_1"])
@pytest.mark.parametrize("dim", [2, 3])
def test_hard_tiles_end_to_end(dim, variant):
    """Tiles over a budget of one leaf go to the team launch - a workgroup of 16 waves per tile, ``bvh_grid / 4`` of
    them, which was none for a grid below 4 - and the values are the default's, bit for bit."""
    index, verts, weights, faces, ref = _product(dim)
    stats = torch.zeros(16, dtype=torch.int64, device=DEV)
    with options(finish_budget=1, finish_budget_min=1, **VARIANTS[variant]):
        got, _ = core._sweep_dimension_cell(index, verts, weights, faces, None, stats=stats)
        torch.cuda.synchronize()
    hard = core.LAST_STATS.hard_entries
    print(dim, variant, "hard entries", hard, "finish", stats[9:].tolist())
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), ref.view(np.int32), err_msg=f"{dim}-D {variant}")
    assert hard[1] > 0, "no tile exceeded the budget: the team launch had nothing to do"
