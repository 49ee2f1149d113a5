"""The finish's short-list launch (csrc/flood_finish.hip, finish_single_kernel: one wave per live sample, lanes on the
child boxes of a node and then on the 16 points of four candidate leaves per step) on the GPU.

Every case compares face values BIT FOR BIT with the same call under option "bvh_subs" 1 - the passes behind the new
launch alone, tiles not split - and with the tree sweep (method "bvh"), and within helpers' tolerance with a kd-tree;
and every case asserts that the launch it is about did the work: no focus round (stats[6] == 0) with leaves evaluated,
or samples left over where the case is about those.  Most cases call flooder_finish_faces_f32 on a hand-built list of
flagged tiles whose samples all start unsettled from +inf: the finish then computes the face values on its own.
Runs on a real MI355X only (-m gpu)."""
import numpy as np
import pytest
import torch

import flooder_amd as fa
import index_reference as ir
from flooder_amd import _native, core
from helpers import assert_close_filtration, get_options, set_options
from variant_cases import Setup, all_tiles, finish, single_tiles   # the harness, shared with test_gpu_finish_variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    _native.load()
    return torch.device("cuda:0")


def check_whole_simplices(su, verts, what, want_left=False):
    """Every tile of every simplex of `verts` flagged: the new launch against the passes alone (bvh_subs 1), the tree
    sweep and the kd-tree.  Returns (counters, left over)."""
    S = verts.shape[0]
    assert 0 < S * su.tiles <= single_tiles(), (what, S, su.tiles)
    got, stats, left = finish(su, verts, all_tiles(S, su.tiles), 16)
    ref, stats_ref, left_ref = finish(su, verts, all_tiles(S, su.tiles), 1)
    print(what, "S", S, "R", su.R, "stats", stats.tolist(), "left", left, "| bvh_subs 1:", stats_ref.tolist())
    assert left_ref == 0 and stats_ref[6] > 0, f"{what}: bvh_subs 1 did not run the passes alone"
    np.testing.assert_array_equal(got, ref, err_msg=f"{what}: differs from the passes alone (bvh_subs 1)")
    tree, _ = core._sweep_dimension_bvh(su.index, verts, su.weights, su.faces, None)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, tree.view(torch.int32).cpu().numpy(), err_msg=f"{what}: differs from the tree sweep")
    assert_close_filtration(got.view(np.float32).max(axis=1), su.kdtree_top(verts), su.pts.cpu().numpy(), what)
    if want_left:
        assert left > 0, f"{what}: no sample went over the budget of the short-list launch"
    else:
        assert stats[0] > 0 and stats[5] > 0, f"{what}: the short-list launch evaluated nothing"
        assert stats[6] == 0 or left > 0, f"{what}: focus rounds without a sample left over: {stats.tolist()}"
    return stats, left


def gaussian(n, dim, seed):
    return torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))


def innermost(su, count):
    """the `count` top simplices whose centroid is nearest the middle of the cloud (short searches)"""
    c = su.verts.mean(dim=1) - su.pts.mean(dim=0)
    return su.verts[torch.argsort((c * c).sum(dim=1))[:count]].contiguous()


@pytest.mark.parametrize("n,dim", [(900, 2), (900, 3), (5_000, 2), (5_000, 3), (70_000, 2), (70_000, 3), (70_003, 3)])
def test_tree_depths_and_partly_filled_tiles(dev, n, dim):
    """One, two and three levels of the box tree; last leaf partly filled (900, 5 000, 70 003) and full (70 000); 20
    points per edge in 2-D / 10 in 3-D: R = 210 / 220, the last of four tiles has rows beyond R."""
    su = Setup(gaussian(n, dim, 100 + n % 97 + dim), dev, 40, 20 if dim == 2 else 10)
    assert su.R % 64 != 0 and (n % 16 == 0) == (n == 70_000)
    assert len(ir.make_levels(n)[0]) == (1 if n < 1024 else (2 if n < 65536 else 3))
    verts = su.verts[:single_tiles() // su.tiles].contiguous()
    check_whole_simplices(su, verts, f"depth n={n} dim={dim}")


@pytest.mark.parametrize("dim", [2, 3])
def test_one_simplex_and_one_tile(dev, dim):
    su = Setup(gaussian(5_000, dim, 7 + dim), dev, 40, 20 if dim == 2 else 10)
    check_whole_simplices(su, su.verts[3:4].contiguous(), f"one simplex dim={dim}")
    # a list of ONE tile - the last, partly filled one of simplex 5 - of a call over eight simplices
    verts = su.verts[:8].contiguous()
    one = [5 * su.tiles + su.tiles - 1]
    got, stats, left = finish(su, verts, one, 16)
    ref, stats_ref, _ = finish(su, verts, one, 1)
    print("one tile", dim, stats.tolist(), left, stats_ref.tolist())
    np.testing.assert_array_equal(got, ref)
    assert got.any() and stats[0] > 0 and (stats[6] == 0 or left > 0) and stats_ref[6] > 0


def test_list_length_threshold(dev):
    """Exactly FINISH_SINGLE_TILES tiles: the short-list launch does all the work (no focus round); one tile more: it
    does not touch the list (focus rounds, nothing left over, no sample counted by it)."""
    su = Setup(gaussian(20_000, 3, 5), dev, 60, 17)   # (R = 969: 16 tiles per simplex)
    T = single_tiles()
    n_s = T // su.tiles + 1
    assert su.verts.shape[0] >= n_s and su.tiles == 16 and T % su.tiles == 0
    verts = innermost(su, n_s)
    tiles = all_tiles(n_s, su.tiles)
    ref, stats_ref, _ = finish(su, verts, tiles[:T + 1], 1)
    longer, stats_l, left_l = finish(su, verts, tiles[:T + 1], 16)
    print("T + 1:", stats_l.tolist(), left_l, "| bvh_subs 1:", stats_ref.tolist())
    np.testing.assert_array_equal(longer, ref)
    assert stats_l[6] > 0 and left_l == 0
    ref, stats_ref, _ = finish(su, verts, tiles[:T], 1)
    short, stats_s, left_s = finish(su, verts, tiles[:T], 16)
    print("T:", stats_s.tolist(), left_s, "| bvh_subs 1:", stats_ref.tolist())
    np.testing.assert_array_equal(short, ref)
    assert stats_s[6] == 0 and stats_s[0] > 0 and left_s == 0, stats_s.tolist()


@pytest.mark.parametrize("dim,doubled", [(3, True), (2, False)])
def test_ties_and_zeros(dev, dim, doubled):
    """Integer lattice cloud (many points at exactly the same distance from a sample; weights i / 8 keep the samples
    exact), every point stored twice in 3-D, landmarks that are cloud points: the vertex samples have d2 = 0."""
    ax = torch.arange(24 if dim == 3 else 100, dtype=torch.float32)
    pts = torch.stack(torch.meshgrid(*([ax] * dim), indexing="ij"), -1).reshape(-1, dim)
    pts = pts[torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(3))]
    if doubled:
        pts = torch.cat([pts, pts])
    su = Setup(pts.contiguous(), dev, 40, 9)
    verts = su.verts[:single_tiles() // su.tiles].contiguous()
    check_whole_simplices(su, verts, f"lattice dim={dim}")
    got, _, _ = finish(su, verts, all_tiles(verts.shape[0], su.tiles), 16)
    assert (got == 0).sum() >= verts.shape[0] * (dim + 1), "the vertex faces of landmarks in the cloud must be exact zeros"


def test_budget_bail_out(dev):
    """Points on a sphere, one small simplex around its centre: every leaf is almost as near as the nearest one.  The
    samples go over the batch budget, are counted as left over, and the passes behind the launch finish them: same
    bits."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(20_000, 3, generator=g)
    pts = (x / x.norm(dim=1, keepdim=True)).contiguous()
    verts = 0.01 * torch.tensor([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, -1.0, -1.0]]])
    su = Setup(pts, dev, 0, 10, verts=verts)
    # on the CPU first: leaves whose box bound is below the true distance of the middle sample - what any exact search
    # has to evaluate - against four times the budget (a batch is four leaves)
    rows = su.index.pts[:su.index.n, :3].cpu().numpy()
    lo, hi = ir.leaf_boxes(rows)
    p = su.verts[0].mean(dim=0).cpu().numpy()
    gap = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    true_d2 = ((rows - p) ** 2).sum(axis=1).min()
    must = int(((gap * gap).sum(axis=1) < true_d2).sum())
    budget = int(_native.load().flooder_finish_single_batches())
    assert must > 4 * 4 * budget, (must, budget)
    stats, left = check_whole_simplices(su, su.verts, "sphere", want_left=True)
    assert stats[6] > 0   # (the passes behind the launch did run)


def test_through_the_product_path(dev):
    """flood_complex on a Gaussian cloud with the cell sweep told to give up early (one cell size, the smallest
    exhaustive cap), so that it flags tiles: against the CPU branch, against bvh_subs 1 and the tree sweep bit for bit;
    the counters of the top dimension's sweep show the short-list launch at work."""
    lib = _native.load()
    pts = gaussian(30_000, 3, 17).to(dev)
    lms = fa.generate_landmarks(pts, 40, start_idx=0)
    keep = get_options(lib, b"cell_tries", b"cell_exh_dense", b"bvh_subs")
    try:
        set_options(lib, {b"cell_tries": 1, b"cell_exh_dense": 512})
        got = fa.flood_complex(pts, lms, points_per_edge=30, method="cell")
        _, simplices = core._build_complex(lms, 3)
        verts = lms[torch.as_tensor(simplices[3], device=dev)].contiguous()
        weights, _, face_idxs = core.generate_grid(30, 3, dev, torch.float32)
        stats = torch.zeros(16, dtype=torch.int64, device=dev)
        core._sweep_dimension_cell(core.PointIndex(pts), verts, weights, core._FaceTable(face_idxs, weights.shape[0], dev), None,
                                   stats=stats)
        torch.cuda.synchronize()
        stats, left = stats.cpu().numpy(), core.LAST_STATS.finish_single_left
        set_options(lib, {b"bvh_subs": 1})
        alone = fa.flood_complex(pts, lms, points_per_edge=30, method="cell")
    finally:
        set_options(lib, keep)
    tree = fa.flood_complex(pts, lms, points_per_edge=30, method="bvh")
    cpu = fa.flood_complex(pts.cpu(), lms.cpu(), points_per_edge=30)
    print("product path: cell sweep", stats[:9].tolist(), "finish", stats[9:].tolist(), "left", left)
    assert got == alone, "face values differ from the passes alone (bvh_subs 1)"
    assert got == tree, "face values differ from the tree sweep"
    keys = sorted(cpu)
    assert keys == sorted(got)
    assert_close_filtration([got[k] for k in keys], [cpu[k] for k in keys], pts.cpu().numpy(), "product path against the CPU branch")
    assert 0 < stats[2] <= single_tiles(), f"tiles flagged by the cell sweep: {stats[2]}"
    assert stats[9] > 0 and (stats[15] == 0 or left > 0), stats[9:].tolist()
