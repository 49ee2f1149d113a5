"""Simplices of 6 to 9 vertices on the device: what ``flood_complex(points, landmarks)`` sweeps in 5-D to 8-D when
``max_dimension`` is left at its default.

Kernel level: the tree sweep, the sorted sweep, the k-nearest sweep and its profile on integer inputs where float32
arithmetic is exact, word for word against a float64 brute force over all points, with ``k1`` = 6, 7, 8 and 9 vertices.
End to end: the default call on the clouds of ``top_simplices_cases`` (63 to 511 faces per simplex: no fused face masks,
the block kernel of the face epilogue) against the oracle, the kd-tree and the CPU path; every method, random weights,
float64 input, the robust filtration, shards, and exact witnesses and gradients.  Runs on a real MI355X only (-m gpu)."""

import ctypes
import functools
import math
import os
import types

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import grad_reference as gr
import knn_grad_reference as kr
import top_simplices_cases as cases
from helpers import GOLDEN, _kdtree_reference, assert_close_filtration, assert_tree_matches_kdtree, smallest32

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INF_BITS = 0x7F800000
UNWRITTEN = -1


def _stream():
    return _native.current_stream_ptr(DEV)


# ------------------------------------------------------------------------------------------------ kernel level
# (dim = simplex dimension, n points, every point doubled, points_per_edge, simplices).  n = 40: one level of the box
# tree; 1025: two; 70 001: three; none a multiple of 16.  grad_reference.assert_exact_inputs passes at these
# (dim, points_per_edge) with the coordinate range of test_knn_sweep_exact_kth_and_dtm; the lattices have 1287, 210, 330
# and 495 rows.
KERNEL_CASES = [
    (5, 40, False, 9, 30), (5, 1025, True, 9, 12), (5, 70_001, False, 9, 8),
    (6, 40, True, 5, 30), (6, 1025, False, 5, 20), (6, 70_001, True, 5, 12),
    (7, 40, False, 5, 24), (7, 1025, True, 5, 16), (7, 70_001, True, 5, 8),
    (8, 40, True, 5, 20), (8, 1025, False, 5, 12), (8, 70_001, False, 5, 8),
]
KERNEL_IDS = [f"{c[0]}d-{c[1]}{'-dup' if c[2] else ''}" for c in KERNEL_CASES]
KNN_KS = (1, 2, 5, 32)
PROFILE_COLUMNS = ((1, 0), (5, 0), (5, 1), (32, 1))       # (k, statistic): 0 the k-th distance, 1 the DTM


def _levels(n):
    leaves, lv = (n + 15) // 16, 1
    while leaves > 64:
        leaves, lv = (leaves + 63) // 64, lv + 1
    return lv


def test_kernel_cases_cover_what_they_must():
    assert {c[0] + 1 for c in KERNEL_CASES} == {6, 7, 8, 9}                      # k1
    assert sum(c[2] for c in KERNEL_CASES) * 2 == len(KERNEL_CASES)
    for dim in (5, 6, 7, 8):
        mine = [c for c in KERNEL_CASES if c[0] == dim]
        assert {_levels(c[1]) for c in mine} == {1, 2, 3}
        assert {c[2] for c in mine} == {True, False}
    assert all(c[1] % 16 != 0 and 8 <= c[4] <= 30 for c in KERNEL_CASES)
    assert {gr.lattice(ppe, d).shape[0] for d, _, _, ppe, _ in KERNEL_CASES} == {1287, 210, 330, 495}


@functools.lru_cache(maxsize=None)
def _kernel_case(dim, n, dup, ppe, n_s):
    """Inputs on the device, the index, and the reference (computed once, shared by the four kernel tests)."""
    d = dim
    rng = np.random.default_rng(100 * dim + n % 97 + ppe)
    step = ppe - 1
    r = min(511, int(2047 / (step * math.sqrt(dim))))
    if dup:
        base = rng.integers(-r, r + 1, size=((n + 1) // 2, dim))
        P = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        P = rng.integers(-r, r + 1, size=(n, dim))
    V = rng.integers(-r, r + 1, size=(n_s, d + 1, dim))
    V[: n_s // 4] = P[rng.integers(0, n, size=(n_s // 4, d + 1))]              # simplices on points of the cloud
    V[n_s // 4: n_s // 2] //= 4                                                # small ones near the centre
    W = gr.lattice(ppe, d)
    gr.assert_exact_inputs(P, V.reshape(-1, dim), ppe)
    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    assert index.pts.shape[0] % 16 == 0 and index.pts.shape[0] > n
    samples = torch.einsum("rk,skd->srd", W.to(DEV), torch.as_tensor(V, dtype=torch.float64, device=DEV))
    small = smallest32(tp.double(), samples.reshape(-1, dim))                # (S * R, min(32, n)) float64, ascending
    assert small.max() * step * step < 2 ** 24
    asc = small.astype(np.float32)
    assert np.array_equal(asc.astype(np.float64), small)                      # exact in float32
    if dup:    # the copies are there: the two smallest of most samples are equal
        assert (asc[:, 0] == asc[:, 1]).mean() > 0.5
    c = types.SimpleNamespace(dim=dim, n=n, k1=d + 1, R=W.shape[0], n_s=n_s, index=index, asc=asc)
    c.verts = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    c.weights = W.to(torch.float32).to(DEV).contiguous()
    c.common = dict(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=d + 1, nodes=index.nodes, verts=c.verts,
                    weights=c.weights, R=c.R, n_simplices=n_s)
    return c


def _brute(c, k, stat):
    """The words of column (k, stat): the k-th smallest d2, or the float32 replay of the ascending sum over k."""
    if stat == 0:
        return c.asc[:, k - 1].view(np.uint32)
    return kr.dtm_words(c.asc, k).view(np.uint32)


def _same(got, want, what):
    bad = np.argwhere(got != want).ravel()
    assert bad.size == 0, (what, bad.size, [(int(i), hex(got[i]), hex(want[i])) for i in bad[:5]])


def _queue():
    return torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dim,n,dup,ppe,n_s", KERNEL_CASES, ids=KERNEL_IDS)
def test_tree_sweep_words(dim, n, dup, ppe, n_s):
    c = _kernel_case(dim, n, dup, ppe, n_s)
    out, queue = torch.full((n_s, c.R), UNWRITTEN, dtype=torch.int32, device=DEV), _queue()
    _native.check(_native.load().flooder_sweep_bvh_f32(
        _native.ptr(c.index.pts), c.index.n, dim, _native.ptr(c.index.nodes), _native.ptr(c.verts), _native.ptr(c.weights),
        c.k1, c.R, n_s, _native.ptr(queue), _native.ptr(out), None, _stream()), "flooder_sweep_bvh_f32")
    _same(out.cpu().numpy().view(np.uint32).reshape(-1), _brute(c, 1, 0), "flooder_sweep_bvh_f32")


@pytest.mark.parametrize("dim,n,dup,ppe,n_s", KERNEL_CASES, ids=KERNEL_IDS)
def test_sorted_sweep_words(dim, n, dup, ppe, n_s):
    """Keys by ``flooder_sample_keys_f32``, order by ``flooder_index_sort``, minima by ``flooder_sorted_minima``: the
    (S, R) words come back in sample order and are the brute force's."""
    c = _kernel_case(dim, n, dup, ppe, n_s)
    lib, st = _native.load(), _stream()
    n_samples = n_s * c.R
    keys, keys_sorted, order = (torch.empty(n_samples, dtype=torch.int32, device=DEV) for _ in range(3))
    tmp_bytes = int(lib.flooder_index_sort_bytes(n_samples))
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=DEV)
    _native.check(lib.flooder_sample_keys_f32(_native.ptr(c.verts), _native.ptr(c.weights), c.k1, c.R, n_s, dim,
                                              _native.ptr(c.index.box), _native.ptr(keys), st), "flooder_sample_keys_f32")
    _native.check(lib.flooder_index_sort(_native.ptr(keys), n_samples, int(lib.flooder_sample_key_bits(dim)),
                                         _native.ptr(keys_sorted), _native.ptr(order), _native.ptr(tmp), tmp_bytes, st),
                  "flooder_index_sort")
    torch.cuda.synchronize()
    assert np.array_equal(np.sort(order.cpu().numpy()), np.arange(n_samples)), "the sample order is no permutation"
    ks = keys_sorted.cpu().numpy().view(np.uint32)
    assert (ks[1:] >= ks[:-1]).all() and ks[0] != ks[-1], "the keys do not tell the samples apart"
    d2, queue = torch.full((n_s, c.R), INF_BITS, dtype=torch.int32, device=DEV), _queue()
    blk = _native.SortedSweep(**c.common, sample_order=order, queue=queue, out_d2=d2)
    _native.check(lib.flooder_sorted_minima(ctypes.byref(blk), st), "flooder_sorted_minima")
    _same(d2.cpu().numpy().view(np.uint32).reshape(-1), _brute(c, 1, 0), "flooder_sorted_minima")


@pytest.mark.parametrize("dim,n,dup,ppe,n_s", KERNEL_CASES, ids=KERNEL_IDS)
def test_knn_sweep_words(dim, n, dup, ppe, n_s):
    c = _kernel_case(dim, n, dup, ppe, n_s)
    lib = _native.load()
    for k in KNN_KS:
        for stat in (0, 1):
            out = torch.full((n_s, c.R), UNWRITTEN, dtype=torch.int32, device=DEV)
            stats, queue = torch.zeros(4, dtype=torch.int64, device=DEV), _queue()
            blk = _native.KnnSweep(k=k, stat=stat, queue=queue, out_bits=out, stats=stats, **c.common)
            _native.check(lib.flooder_sweep_knn_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_f32")
            _same(out.cpu().numpy().view(np.uint32).reshape(-1), _brute(c, k, stat), ("flooder_sweep_knn_f32", k, stat))
            s = stats.cpu().numpy()
            assert s[0] > 0 and s[1] >= s[0] and s[2] >= n_s * ((c.R + 63) // 64)


@pytest.mark.parametrize("dim,n,dup,ppe,n_s", KERNEL_CASES, ids=KERNEL_IDS)
def test_knn_profile_words(dim, n, dup, ppe, n_s):
    c = _kernel_case(dim, n, dup, ppe, n_s)
    words, guard = len(PROFILE_COLUMNS) * n_s * c.R, 64
    out = torch.full((words + guard,), UNWRITTEN, dtype=torch.int32, device=DEV)
    stats, queue = torch.zeros(4, dtype=torch.int64, device=DEV), _queue()
    blk = _native.KnnProfile(PROFILE_COLUMNS, queue=queue, out_bits=out, stats=stats, **c.common)
    _native.check(_native.load().flooder_sweep_knn_profile_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_profile_f32")
    got = out.cpu().numpy()
    assert (got[words:] == UNWRITTEN).all(), "guard words behind the last plane were written"
    planes = got[:words].view(np.uint32).reshape(len(PROFILE_COLUMNS), n_s * c.R)
    for col, (k, stat) in enumerate(PROFILE_COLUMNS):
        _same(planes[col], _brute(c, k, stat), ("flooder_sweep_knn_profile_f32", k, stat))


# ------------------------------------------------------------------------------------------------ end to end
GRID = ("A", "B", "C", "D")


@functools.lru_cache(maxsize=None)
def _device(name, double=False):
    P, L, _ = cases.config(name)
    tp, tl = torch.as_tensor(P, device=DEV), torch.as_tensor(L, device=DEV)
    return (tp.double(), tl.double()) if double else (tp, tl)


def _call(name, **kw):
    tp, tl = _device(name)
    kw.setdefault("points_per_edge", cases.config(name)[2])
    return fa.flood_complex(tp, tl, **kw)


@functools.lru_cache(maxsize=None)
def _default(name):
    """The default call, and the (simplices, samples per simplex) of its one dimension pass."""
    fc = _call(name)
    return fc, (core.LAST_STATS.top_simplices, core.LAST_STATS.samples_per_simplex)


def _against(got, ref, P, what):
    assert set(got) == set(ref), f"{what}: key sets differ"
    keys = sorted(ref)
    return assert_close_filtration([got[k] for k in keys], [ref[k] for k in keys], P, what, strict=True)


def test_configurations_take_the_paths_they_are_meant_to():
    for name in GRID + ("E",):
        dim, _, _, ppe = cases.CONFIGS[name]
        _, (S, R) = _default(name)
        assert R == cases.rows_per_simplex(ppe, dim) and S > 500
        weights, _, _, faces, plan, _ = core._grid_tables(ppe, dim, DEV, torch.float32)
        assert faces.n_faces == cases.n_faces(dim) > 32 and plan.memb_all is None and plan.late_rows is None
        assert plan.wit is None
        # A to D stay below the sorted sweep's threshold (forced on and off below), E is above it by itself
        assert core.bvh_sorts_samples(dim, S, R) == (name == "E"), (name, S, R)


@pytest.mark.parametrize("name", GRID + ("E",))
def test_default_call_against_cpu_path_and_oracle(name):
    P, _, _ = cases.config(name)
    fc, (S, R) = _default(name)
    assert set(fc) == set(cases.cpu_dict(name)), "key sets differ from the CPU path's"
    worst = _against(fc, cases.oracle(name), P, name)
    print(f"{name}: {len(fc)} simplices, {S} top simplices of {R} samples, worst abs err {worst:.3e}")


@pytest.mark.parametrize("name", GRID + ("E",))
def test_every_dimension_against_the_kdtree(name):
    """Each face table of the tree with the lattice of its own dimension (``assert_tree_matches_kdtree``)."""
    dim = cases.CONFIGS[name][0]
    P, L, ppe = cases.config(name)
    st = _call(name, return_simplex_tree=True)
    n = assert_tree_matches_kdtree(st, P, L, ppe, dim, name, strict=True)
    assert n == len(_default(name)[0]) - L.shape[0]


@pytest.mark.parametrize("name", GRID)
def test_methods_give_equal_dicts(name, monkeypatch):
    """The default, the tree sweep per simplex and over sorted samples, the fused-faces option (which must fall back
    above 32 faces, not fail) and the bounding-ball formulation."""
    dim = cases.CONFIGS[name][0]
    base, (S, R) = _default(name)
    monkeypatch.setattr(core, "BVH_SORTED_MIN_SAMPLES", 0)
    for sort in (True, False):
        monkeypatch.setattr(core, "BVH_SORTED_SAMPLES", sort)
        assert core.bvh_sorts_samples(dim, S, R) == sort
        assert _call(name, method="bvh") == base, f"bvh, sorted samples {sort}"
    monkeypatch.setattr(core, "BVH_SORTED_SAMPLES", True)
    monkeypatch.setattr(core, "SORTED_FUSED_FACES", True)
    assert _call(name, method="bvh") == base, "bvh, fused faces asked for"
    monkeypatch.undo()
    assert _call(name, method="ball") == base, "ball"


def _rand_golden(name, num_rand):
    z = np.load(os.path.join(GOLDEN, f"top_rand_{name}_{num_rand}.npz"))
    keys = [tuple(int(v) for v in row if v >= 0) for row in z["simplices"]]
    return dict(zip(keys, z["filtration"].tolist())), int(z["weight_seed"])


@pytest.mark.parametrize("name,num_rand", [("A", 40), ("A", 1100), ("D", 40), ("D", 1100)])
def test_random_weights(name, num_rand):
    """One face of all rows: 40 rows go to the small kernel of the face epilogue, 1100 to the whole-block branch.
    ``"bvh"`` equals ``"ball"``, and both lie inside the gate of ``flood_complex_oracle`` under the same seed - its
    recorded result (``oracle/make_top_simplices_goldens.py``: two minutes of kd-tree queries for D at 1100)."""
    P, _, _ = cases.config(name)
    ref, seed = _rand_golden(name, num_rand)
    got = {}
    for method in ("bvh", "ball"):
        torch.manual_seed(seed)
        got[method] = _call(name, points_per_edge=None, num_rand=num_rand, method=method)
    assert got["bvh"] == got["ball"]
    worst = _against(got["bvh"], ref, P, f"{name} num_rand={num_rand}")
    print(f"{name} num_rand={num_rand}: {len(ref)} simplices, worst abs err {worst:.3e}")


@pytest.mark.parametrize("name", ["A", "D"])
def test_float64_input(name):
    """As ``test_float64_input_gpu``: the float64 device kernels against the float64 CPU path, to double precision."""
    P, L, ppe = cases.config(name)
    tp, tl = _device(name, True)
    with pytest.warns(RuntimeWarning):
        fc = fa.flood_complex(tp, tl, points_per_edge=ppe)
    with pytest.warns(RuntimeWarning):
        cpu = fa.flood_complex(torch.as_tensor(P).double(), torch.as_tensor(L).double(), points_per_edge=ppe)
    assert set(fc) == set(cpu)
    keys = sorted(cpu)
    got, ref = np.array([fc[k] for k in keys]), np.array([cpu[k] for k in keys])
    scale = float(np.abs(P).max())
    assert np.abs(got - ref).max() <= 1e-12 * scale + 1e-11 * np.abs(ref).max(), np.abs(got - ref).max()


@pytest.mark.parametrize("name", ["B", "D"])
def test_one_neighbor_is_the_default_call(name):
    base, _ = _default(name)
    for stat in ("kth", "dtm"):
        assert _call(name, neighbors=1, neighbor_stat=stat) == base


@pytest.mark.parametrize("name,k", [("B", 2), ("B", 8), ("D", 2), ("D", 8)])
def test_robust_filtration_against_the_kdtree(name, k):
    """``neighbors=k``, both statistics, every simplex of every dimension against ``cKDTree.query(k=k)`` over all
    points with the lattice of the simplex's own dimension."""
    P, L, ppe = cases.config(name)
    ref = None
    for stat in ("kth", "dtm"):
        fc = _call(name, neighbors=k, neighbor_stat=stat)
        assert set(fc) == set(_default(name)[0])
        if ref is None:
            ref = _kdtree_reference(fc, P, L, k, ppe=ppe)
        keys = sorted(fc)
        for d in sorted({len(key) - 1 for key in keys}):
            kd = [key for key in keys if len(key) - 1 == d]
            assert_close_filtration([fc[key] for key in kd], [ref[stat][key] for key in kd], P,
                                    f"{name} k={k} {stat} dimension {d}", strict=True)


def test_profile_columns_are_the_single_calls():
    tp, tl = _device("B")
    ppe = cases.config("B")[2]
    prof = fa.flood_profile(tp, tl, points_per_edge=ppe, neighbors=(1, 2, 8), neighbor_stat=("kth", "dtm"))
    assert len(prof.columns) == 6
    for k, stat in prof.columns:
        assert prof[(k, stat)] == _call("B", neighbors=k, neighbor_stat=stat), (k, stat)


def _simplex_shards(name, **kw):
    bufs = []
    for r in range(3):
        _call(name, simplex_shard=(r, 3), face_reduce_hook=lambda buf, c=bufs: c.append(buf.clone()), **kw)
    assert len(bufs) == 3 and not torch.equal(bufs[0], bufs[1])
    merged = torch.minimum(torch.minimum(bufs[0], bufs[1]), bufs[2])
    assert bool(torch.isfinite(merged).all())
    return bufs, _call(name, simplex_shard=(0, 3), face_reduce_hook=lambda buf: buf.copy_(merged), **kw)


def test_simplex_shards_min_reduce():
    """Three ranks, every third simplex each: the MIN of their (S, F) buffers is the whole call."""
    base, _ = _default("B")
    bufs, out = _simplex_shards("B")
    assert not bool(torch.isfinite(bufs[0]).all()), "a rank that holds every simplex is no shard"
    assert out == base


def test_tile_shards_min_reduce(monkeypatch):
    """The sorted sweep forced on: a rank takes a share of the TILES of the sorted sample order and hands the hook the
    negated maxima over its own samples - still combined with MIN."""
    dim = cases.CONFIGS["B"][0]
    base, (S, R) = _default("B")
    monkeypatch.setattr(core, "BVH_SORTED_SAMPLES", True)
    monkeypatch.setattr(core, "BVH_SORTED_MIN_SAMPLES", 0)
    assert core.shards_sorted_tiles(dim, S, R, "bvh")
    bufs, out = _simplex_shards("B", method="bvh")
    assert all(bool((b <= 0).all()) for b in bufs), "tile shards hand over negated values"
    assert out == base


def test_point_shards_min_reduce():
    """Three shards of the cloud, MIN of the (S, R) words through ``reduce_hook``: the whole call."""
    P, _, ppe = cases.config("B")
    base, _ = _default("B")
    tp, tl = _device("B")
    axis = int(np.argmax(P.max(0) - P.min(0)))
    captured = []
    for r in range(3):
        fa.flood_complex(tp[r::3].contiguous(), tl, points_per_edge=ppe, sort_axis=axis,
                         reduce_hook=lambda buf, c=captured: c.append(buf.clone()))
    assert len(captured) == 3 and not torch.equal(captured[0], captured[1])
    merged = torch.minimum(torch.minimum(captured[0], captured[1]), captured[2])
    out = fa.flood_complex(tp[0::3].contiguous(), tl, points_per_edge=ppe, sort_axis=axis,
                           reduce_hook=lambda buf: buf.copy_(merged))
    assert out == base


# ------------------------------------------------------------------------------------------------ witnesses, gradients
EXACT_HI = 64      # integer coordinates in [0, 64), quarters: differences < 2**8 units, squares < 2**16, 8 axes < 2**19


@functools.lru_cache(maxsize=None)
def _exact_cloud(dim):
    """2000 integer points (every point twice) and 12 integer landmarks off the cloud, float32 on the device."""
    g = torch.Generator().manual_seed(50 + dim)
    base = torch.randint(0, EXACT_HI, (1000, dim), generator=g).to(torch.float32)
    pts = torch.cat([base, base])[torch.randperm(2000, generator=g)]
    taken = {tuple(r) for r in pts.to(torch.int64).tolist()}
    rows = []
    for r in torch.randint(0, EXACT_HI, (600, dim), generator=g).tolist():
        if tuple(r) not in taken:
            taken.add(tuple(r))
            rows.append(r)
    lms = torch.tensor(rows[:12], dtype=torch.float32)
    gr.assert_exact_inputs(pts, lms, 5)
    return pts.to(DEV), lms.to(DEV)


def _coefficients(F):
    gen = torch.Generator().manual_seed(7)
    return [((torch.rand(v.shape[0], generator=gen) + 0.5) * (2 * torch.randint(0, 2, (v.shape[0],), generator=gen) - 1)
             ).to(DEV) for v in F.values]


def _check_gradient(F, tp, tl, reference, what):
    """Points' and landmarks' gradient of a random linear functional of all values: every row within the float32 bound
    the reference derives for that row, rows nothing points at exactly zero."""
    coef = _coefficients(F)
    loss = sum((c * v).sum() for c, v in zip(coef, F.values))
    rp, rl, info = reference(F, tp.detach(), tl.detach(), coef)
    gp, gl = torch.autograd.grad(loss, (tp, tl))
    for name, got, ref, bound, scale in (("points", gp, rp, info["bound_points"], info["scale_points"]),
                                         ("landmarks", gl, rl, info["bound_landmarks"], info["scale_landmarks"])):
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        err = (got.double() - ref).abs().max(dim=1).values
        hit = scale > 0
        assert int(hit.sum()) > 0 and float(ref.abs().sum()) > 0, name
        ratio = float((err[hit] / bound[hit]).max())
        print(f"{what} {name}: {int(hit.sum())} rows, worst error / bound {ratio:.3f}")
        assert not got[~hit].any(), name
        assert torch.all(err <= bound), (what, name, ratio)


@pytest.mark.parametrize("dim", [5, 8])
def test_exact_witnesses_and_gradients(dim):
    """``flood_filtration`` with 6- and 9-vertex simplices at 5 points per edge (126 and 495 rows, 63 and 511 faces):
    value bits, witness sample and witness point of every simplex of every dimension against the brute force, the
    gradient against the float64 closed form."""
    pts, lms = _exact_cloud(dim)
    tp, tl = pts.clone().requires_grad_(True), lms.clone().requires_grad_(True)
    F = fa.flood_filtration(tp, tl, points_per_edge=5)
    assert len(F.simplices) == dim + 1 and F.simplices[dim].shape[0] > 0 and F.faces_not_found == 0
    faces = gr.reference_faces(F.simplices, pts, lms, 5)
    pts_tie, arg_tie, n_simp = gr.tie_shares(faces)
    print(f"{dim}-D: {n_simp} simplices, {F.simplices[dim].shape[0]} of {dim + 1} vertices, more than one nearest point "
          f"on {pts_tie:.1%}, more than one sample at the maximum on {arg_tie:.1%}")
    assert pts_tie >= 0.9          # every point is there twice: the smallest id has to be picked almost everywhere
    gr.check_exact_witnesses(F, faces, pts, smallest_id=True)
    _check_gradient(F, tp, tl, gr.reference_gradient, f"{dim}-D")


@pytest.mark.parametrize("dim,stat", [(5, "kth"), (5, "dtm"), (8, "kth"), (8, "dtm")])
def test_exact_knn_witnesses_and_gradients(dim, stat):
    """The same with ``neighbors=5``: the five nearest points by (d2, id) of the witness sample."""
    pts, lms = _exact_cloud(dim)
    tp, tl = pts.clone().requires_grad_(True), lms.clone().requires_grad_(True)
    F = fa.flood_filtration(tp, tl, points_per_edge=5, neighbors=5, neighbor_stat=stat)
    assert F.simplices[dim].shape[0] > 0 and F.faces_not_found == 0
    faces = kr.exact_knn_faces(F.simplices, pts, lms, 5, 5, stat)
    assert kr.tie_share(faces) >= 0.9          # five of points that come in pairs: the sixth ties with the fifth
    kr.check_exact_knn_witnesses(F, faces, pts)
    _check_gradient(F, tp, tl, kr.reference_gradient_knn, f"{dim}-D k=5 {stat}")
