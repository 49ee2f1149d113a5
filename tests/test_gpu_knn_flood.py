"""Robust filtration on the device: ``flooder_sweep_knn_f32`` bit for bit on inputs where float32 arithmetic is exact,
``flood_complex(neighbors=k)`` against the kd-tree over all points, and what must not change (k = 1, determinism,
simplex shards)."""

import ctypes
import math

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from flooder_amd.synthetic import generate_figure_eight_points_2d, generate_noisy_torus_points_3d

import grad_reference as gr
from helpers import _kdtree_reference, assert_close_filtration, smallest32

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KS = (1, 2, 3, 5, 8, 16, 17, 32)


def _stream():
    return _native.current_stream_ptr(DEV)


# ------------------------------------------------------------------------------------------------ 7 / 8. kernel level
def _levels(n):
    leaves, lv = (n + 15) // 16, 1
    while leaves > 64:
        leaves, lv = (leaves + 63) // 64, lv + 1
    return lv


# (dim, n points, every point doubled, points_per_edge, simplex dimension, simplices, tree levels).  n = 40 / 1000: one
# level; 1025 / 30 001: two; 70 001: three; 4 300 001: four.  No n is a multiple of 16: the last leaf is padded.
KERNEL_CASES = [
    (2, 40, False, 5, 2, 40, 1), (2, 1025, True, 9, 2, 40, 2), (2, 70_001, False, 17, 2, 40, 3), (2, 4_300_001, True, 5, 1, 24, 4),
    (3, 1000, True, 17, 2, 40, 1), (3, 30_001, False, 9, 3, 30, 2), (3, 70_001, True, 5, 3, 40, 3), (3, 4_300_001, False, 5, 3, 8, 4),
    (4, 40, True, 9, 3, 30, 1), (4, 30_001, True, 5, 4, 30, 2), (4, 70_001, False, 17, 2, 40, 3), (4, 4_300_001, False, 9, 2, 8, 4),
    (6, 1000, False, 5, 3, 40, 1), (6, 1025, False, 17, 2, 40, 2), (6, 70_001, True, 9, 2, 40, 3), (6, 4_300_001, True, 5, 3, 8, 4),
    (8, 33, False, 9, 2, 40, 1), (8, 30_001, True, 17, 1, 60, 2), (8, 70_001, False, 5, 3, 40, 3), (8, 4_300_001, True, 5, 2, 8, 4),
]


def test_kernel_cases_cover_what_they_must():
    assert {c[0] for c in KERNEL_CASES} == {2, 3, 4, 6, 8}
    assert {c[3] for c in KERNEL_CASES} == {5, 9, 17}
    for dim in (2, 3, 4, 6, 8):
        assert {c[6] for c in KERNEL_CASES if c[0] == dim} == {1, 2, 3, 4}
        assert {c[2] for c in KERNEL_CASES if c[0] == dim} == {True, False}
    assert {c[6] for c in KERNEL_CASES} == {1, 2, 3, 4}
    assert all(c[1] % 16 != 0 and _levels(c[1]) == c[6] for c in KERNEL_CASES)


@pytest.mark.parametrize("dim,n,dup,ppe,d,n_s,levels", KERNEL_CASES)
def test_knn_sweep_exact_kth_and_dtm(dim, n, dup, ppe, d, n_s, levels):
    """Every k of KS, both statistics, on one cloud: the ``kth`` words equal the k-th smallest d2 of the float64 brute
    force over all points (``np.partition``), the ``dtm`` words the float32 replay of the ascending sum over k; at
    k = 1 the words are ``flooder_sweep_bvh_f32``'s."""
    rng = np.random.default_rng(100 * dim + n % 97 + ppe)
    step = ppe - 1
    # integer coordinates in [-r, r], r <= 511, as wide as keeps every d2 below 2**24 units of step**-2
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
    R = W.shape[0]

    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    assert index.pts.shape[0] % 16 == 0 and index.pts.shape[0] > n and bool(torch.isinf(index.pts[n:, :dim]).all())
    samples = torch.einsum("rk,skd->srd", W.to(DEV), torch.as_tensor(V, dtype=torch.float64, device=DEV))
    small = smallest32(tp.double(), samples.reshape(-1, dim))                # (S*R, 32) float64
    assert small.max() * step * step < 2 ** 24
    if dup:    # the copies are there: the two smallest of most samples are equal
        assert (np.sort(small, axis=1)[:, 0] == np.sort(small, axis=1)[:, 1]).mean() > 0.5

    lib = _native.load()
    t_v = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    t_w = W.to(torch.float32).to(DEV).contiguous()

    def sweep(k, stat):
        out = torch.full((n_s, R), -1, dtype=torch.int32, device=DEV)
        queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
        stats = torch.zeros(4, dtype=torch.int64, device=DEV)
        blk = _native.KnnSweep(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=d + 1, nodes=index.nodes, verts=t_v,
                               weights=t_w, R=R, k=k, n_simplices=n_s, stat=stat, queue=queue, out_bits=out, stats=stats)
        _native.check(lib.flooder_sweep_knn_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_f32")
        st = stats.cpu().numpy()
        assert st[0] > 0 and st[1] >= st[0] and st[2] >= n_s * ((R + 63) // 64)     # leaves evaluated / tested, node tests
        return out.cpu().numpy().view(np.uint32).reshape(-1)

    for k in KS:
        if k > n:
            continue
        want = np.partition(small, k - 1, axis=1)[:, k - 1].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), np.partition(small, k - 1, axis=1)[:, k - 1])   # exact in float32
        got = sweep(k, 0)
        assert np.array_equal(got, want.view(np.uint32)), (k, np.argwhere(got != want.view(np.uint32))[:5].ravel())
        asc = np.sort(small, axis=1)[:, :k].astype(np.float32)
        acc = asc[:, 0].copy()
        for i in range(1, k):
            acc = (acc + asc[:, i]).astype(np.float32)
        want_dtm = (acc / np.float32(k)).astype(np.float32)
        got = sweep(k, 1)
        assert np.array_equal(got, want_dtm.view(np.uint32)), (k, "dtm", np.argwhere(got != want_dtm.view(np.uint32))[:5].ravel())
        if k == 1:
            out = torch.full((n_s, R), -1, dtype=torch.int32, device=DEV)
            queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
            _native.check(lib.flooder_sweep_bvh_f32(_native.ptr(index.pts), index.n, dim, _native.ptr(index.nodes),
                                                    _native.ptr(t_v), _native.ptr(t_w), d + 1, R, n_s, _native.ptr(queue),
                                                    _native.ptr(out), None, _stream()), "flooder_sweep_bvh_f32")
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(-1), sweep(1, 0))
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(-1), sweep(1, 1))


def test_knn_sweep_refuses_more_neighbours_than_points():
    tp = torch.rand(20, 3, device=DEV)
    index = core.PointIndex(tp)
    out = torch.zeros((1, 1), dtype=torch.int32, device=DEV)
    queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
    blk = _native.KnnSweep(pts_sorted=index.pts, n_pts=index.n, dim=3, k1=1, nodes=index.nodes, verts=tp[:1].contiguous(),
                           weights=torch.ones((1, 1), device=DEV), R=1, k=21, n_simplices=1, queue=queue, out_bits=out)
    assert _native.load().flooder_sweep_knn_f32(ctypes.byref(blk), _stream()) != 0


# ------------------------------------------------------------------------------------------------ 9. end to end
def _e2e_cloud(name):
    if name == "torus":
        return generate_noisy_torus_points_3d(200_000, seed=3).to(torch.float32), 300, dict(points_per_edge=20)
    if name == "eight":
        return generate_figure_eight_points_2d(50_000, seed=4).to(torch.float32), 200, dict(points_per_edge=30)
    if name == "gauss6":
        g = torch.Generator().manual_seed(6)
        return torch.randn(200_000, 6, generator=g), 150, dict(points_per_edge=10, max_dimension=2)
    g = torch.Generator().manual_seed(8)
    return torch.randn(100_000, 3, generator=g), 200, dict(points_per_edge=None, num_rand=300)


@pytest.mark.parametrize("name", ["torus", "eight", "gauss6", "num_rand"])
def test_end_to_end_against_the_kdtree(name):
    pts, n_lms, kw = _e2e_cloud(name)
    tp = pts.to(DEV)
    lms = fa.generate_landmarks(tp, n_lms, start_idx=0)
    P, L = pts.numpy(), lms.cpu().numpy()
    torch.manual_seed(21)
    cpu = fa.flood_complex(pts, lms.cpu(), neighbors=2, **kw)               # the CPU path: its key set
    weights = None
    for k in (2, 8, 32):
        ref = None
        for stat in ("kth", "dtm"):
            torch.manual_seed(21)
            fc = fa.flood_complex(tp, lms, neighbors=k, neighbor_stat=stat, **kw)
            assert set(fc) == set(cpu), f"{name} k={k} {stat}: key sets differ"
            if ref is None:
                if kw.get("num_rand"):
                    torch.manual_seed(21)      # the draws of the call, dimension by dimension
                    weights = {d: core.generate_uniform_weights(kw["num_rand"], d, "cpu", torch.float32)
                               for d in sorted({len(key) - 1 for key in fc})}
                ref = _kdtree_reference(fc, P, L, k, ppe=kw.get("points_per_edge"), weights_by_dim=weights,
                                        top=kw.get("max_dimension"))
            keys = sorted(fc)
            for d in sorted({len(key) - 1 for key in keys}):
                kd = [key for key in keys if len(key) - 1 == d]
                worst = assert_close_filtration([fc[key] for key in kd], [ref[stat][key] for key in kd], P,
                                                f"{name} k={k} {stat} dimension {d}", strict=True)
                print(f"{name} k={k} {stat} dimension {d}: {len(kd)} simplices, worst abs err {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 10. k = 1 unchanged
@pytest.mark.parametrize("method", ["cell", "bvh", None])
def test_one_neighbor_is_the_default_call_on_the_device(method):
    pts = generate_noisy_torus_points_3d(100_000, seed=1).to(torch.float32).to(DEV)
    lms = fa.generate_landmarks(pts, 200, start_idx=0)
    base = fa.flood_complex(pts, lms, points_per_edge=12, method=method)
    for stat in ("kth", "dtm"):
        assert fa.flood_complex(pts, lms, points_per_edge=12, method=method, neighbors=1, neighbor_stat=stat) == base
    g = torch.Generator().manual_seed(2)
    pts6 = torch.randn(50_000, 6, generator=g).to(DEV)
    if method != "cell":
        lms6 = fa.generate_landmarks(pts6, 60, start_idx=0)
        base = fa.flood_complex(pts6, lms6, points_per_edge=6, max_dimension=2, method=method)
        assert fa.flood_complex(pts6, lms6, points_per_edge=6, max_dimension=2, method=method, neighbors=1,
                                neighbor_stat="dtm") == base


def test_device_refusals():
    pts = torch.rand(500, 3, device=DEV)
    with pytest.raises(ValueError, match="float32"):
        fa.flood_complex(pts.double(), 20, neighbors=2)
    with pytest.raises(ValueError, match="dimension 2 to 8"):
        fa.flood_complex(torch.rand(500, 1, device=DEV), 20, neighbors=2)
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match="nearest point only"):
            fa.flood_complex(pts, 20, neighbors=2, method=method)
    with pytest.raises(ValueError, match="reduce_hook"):
        fa.flood_complex(pts, 20, neighbors=2, reduce_hook=lambda t: None)
    with pytest.raises(ValueError, match="shard_blocks"):
        fa.flood_complex(pts, 20, neighbors=2, simplex_shard=(0, 2), shard_blocks=True)


# ------------------------------------------------------------------------------------------------ 11. determinism
def test_two_runs_give_equal_dicts():
    pts = generate_noisy_torus_points_3d(200_000, seed=5).to(torch.float32).to(DEV)
    lms = fa.generate_landmarks(pts, 300, start_idx=0)
    for stat in ("kth", "dtm"):
        a = fa.flood_complex(pts, lms, points_per_edge=20, neighbors=8, neighbor_stat=stat)
        b = fa.flood_complex(pts, lms, points_per_edge=20, neighbors=8, neighbor_stat=stat)
        assert a == b


# ------------------------------------------------------------------------------------------------ 12. full size
def test_cfg2_full_size_k8():
    """cfg 2 (1 M Gaussian points in 3-D, 1000 landmarks, 30 points per edge) with the 8-distance: a seeded pick of
    1500 tetrahedra plus the 100 with the largest values against the kd-tree over all points - all of them would be
    32 M queries with k = 8, minutes on 16 host cores, so a pick it is."""
    from scipy.spatial import cKDTree

    torch.manual_seed(42)
    pts = torch.randn(1_000_000, 3)
    tp = pts.to(DEV)
    lms = fa.generate_landmarks(tp, 1000, start_idx=0)
    st = fa.flood_complex(tp, lms, points_per_edge=30, neighbors=8, neighbor_stat="kth", return_simplex_tree=True)
    tets = np.asarray(st.simplices_of_dimension(3))
    vals = np.asarray(st.filtrations_of_dimension(3), dtype=np.float64)
    rng = np.random.default_rng(12)
    pick = np.unique(np.concatenate([np.argsort(-vals)[:100], rng.choice(len(tets), size=1500, replace=False)]))
    assert len(pick) >= 1500
    P, L = pts.numpy(), lms.cpu().numpy()
    tree = cKDTree(P.astype(np.float64))
    w = core.generate_grid(30, 3, "cpu", torch.float32)[0].numpy()
    ref = np.empty(len(pick))
    for b in range(0, len(pick), 400):
        samples = np.matmul(w[None], L[tets[pick[b:b + 400]]]).astype(np.float32).reshape(-1, 3)
        dist, _ = tree.query(samples.astype(np.float64), k=8, workers=-1)
        ref[b:b + 400] = dist[:, -1].reshape(-1, w.shape[0]).max(axis=1)
    worst = assert_close_filtration(vals[pick], ref, P, "cfg2 k=8 tetrahedra", strict=True)
    print(f"cfg2 k=8: {len(pick)} of {len(tets)} tetrahedra, worst abs err {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 13. sharding
def test_simplex_shards_reproduce_the_unsharded_values():
    pts = generate_noisy_torus_points_3d(100_000, seed=9).to(torch.float32).to(DEV)
    lms = fa.generate_landmarks(pts, 200, start_idx=0)
    g = torch.Generator().manual_seed(2)
    pts6 = torch.randn(100_000, 6, generator=g).to(DEV)
    lms6 = fa.generate_landmarks(pts6, 80, start_idx=0)
    for p, l, kw in ((pts, lms, dict(points_per_edge=16)), (pts6, lms6, dict(points_per_edge=8, max_dimension=2))):
        for stat in ("kth", "dtm"):
            whole = fa.flood_complex(p, l, neighbors=8, neighbor_stat=stat, **kw)
            parts = []

            def emulate_min(face):     # the MIN all-reduce of two ranks, in process: rank 0 deposits, rank 1 combines
                parts.append(face.clone())
                if len(parts) == 2:
                    face.copy_(torch.minimum(parts[0], parts[1]))

            fa.flood_complex(p, l, neighbors=8, neighbor_stat=stat, simplex_shard=(0, 2), face_reduce_hook=emulate_min, **kw)
            both = fa.flood_complex(p, l, neighbors=8, neighbor_stat=stat, simplex_shard=(1, 2),
                                    face_reduce_hook=emulate_min, **kw)
            assert len(parts) == 2 and both == whole
