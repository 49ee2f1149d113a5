"""Neighbour profile on the device: every plane of ``flooder_sweep_knn_profile_f32`` word for word against
``flooder_sweep_knn_f32`` with that (k, stat) and against a float64 brute force on inputs where float32 arithmetic is
exact, the refusals of the entry point, and ``flood_profile`` against one ``flood_complex`` call per column."""

import ctypes
import math

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from flooder_amd.synthetic import generate_figure_eight_points_2d, generate_noisy_torus_points_3d

import grad_reference as gr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64                    # words behind the last plane
SENTINEL = 0x5EA1ED


def _stream():
    return _native.current_stream_ptr(DEV)


def _smallest32(P: torch.Tensor, Q: torch.Tensor, chunk_elems: int = 1 << 26) -> np.ndarray:
    """float64 brute force on the device: per row of Q the 32 smallest squared distances to ALL rows of P (d2 added
    axis by axis in float64 - exact on these inputs), ascending."""
    n, dim = P.shape
    per = max(1, chunk_elems // n)
    out = []
    for a in range(0, Q.shape[0], per):
        q = Q[a:a + per]
        d2 = (q[:, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for c in range(1, dim):
            d2 += (q[:, c:c + 1] - P[:, c].unsqueeze(0)) ** 2
        out.append(torch.topk(d2, min(32, n), dim=1, largest=False, sorted=True).values.cpu())
    return torch.cat(out).numpy()


# (dim, n points, every point doubled, points_per_edge, simplex dimension, simplices): trees of one to three levels
# (the walk is the single sweep's own code), R = 1 (vertices), R < 64, R > 64 and no multiple of 64, padded last leaves
# (no n is a multiple of 16), k_max = n (20 points).
KERNEL_CASES = [
    (2, 40, False, 5, 2, 40), (2, 1025, True, 9, 2, 40), (2, 70_001, False, 17, 2, 40),
    (3, 20, False, 5, 2, 8), (3, 1000, False, 5, 0, 40), (3, 30_001, False, 9, 3, 30), (3, 70_001, True, 5, 3, 40),
    (4, 40, True, 9, 3, 30),
    (6, 1025, False, 17, 2, 40), (6, 70_001, True, 9, 2, 40),
    (8, 33, False, 9, 2, 40), (8, 30_001, True, 17, 1, 60),
]


def test_kernel_cases_cover_what_they_must():
    rs = {gr.lattice(c[3], c[4]).shape[0] for c in KERNEL_CASES}
    assert 1 in rs and any(1 < r < 64 for r in rs) and any(r > 64 and r % 64 for r in rs)
    assert {c[0] for c in KERNEL_CASES} == {2, 3, 4, 6, 8} and {c[2] for c in KERNEL_CASES} == {True, False}
    assert all(c[1] % 16 for c in KERNEL_CASES) and any(c[1] < 32 for c in KERNEL_CASES)


def _column_sets(n):
    k_top = min(32, n)
    full = [(k, s) for k in range(1, k_top + 1) for s in (0, 1)]
    mixed = [(k, s) for k, s in ((17, 1), (3, 0), (5, 1), (17, 0), (2, 1)) if k <= n]
    return [full, mixed, [(8, 0)]]


@pytest.mark.parametrize("dim,n,dup,ppe,d,n_s", KERNEL_CASES)
def test_every_plane_is_the_single_sweep_and_the_brute_force(dim, n, dup, ppe, d, n_s):
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
    assert index.pts.shape[0] % 16 == 0 and index.pts.shape[0] > n
    samples = torch.einsum("rk,skd->srd", W.to(DEV), torch.as_tensor(V, dtype=torch.float64, device=DEV))
    small = _smallest32(tp.double(), samples.reshape(-1, dim))                # (S*R, min(32, n)) float64, ascending
    assert small.max() * step * step < 2 ** 24
    asc = small.astype(np.float32)
    assert np.array_equal(asc.astype(np.float64), small)                      # exact in float32

    lib = _native.load()
    t_v = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    t_w = W.to(torch.float32).to(DEV).contiguous()
    common = dict(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=d + 1, nodes=index.nodes, verts=t_v, weights=t_w, R=R,
                  n_simplices=n_s)
    single_cache = {}

    def single(k, stat):
        if (k, stat) not in single_cache:
            out = torch.full((n_s, R), -1, dtype=torch.int32, device=DEV)
            queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
            stats = torch.zeros(4, dtype=torch.int64, device=DEV)
            blk = _native.KnnSweep(k=k, stat=stat, queue=queue, out_bits=out, stats=stats, **common)
            _native.check(lib.flooder_sweep_knn_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_f32")
            single_cache[(k, stat)] = (out.cpu().numpy().view(np.uint32).reshape(-1), stats.cpu().numpy())
        return single_cache[(k, stat)]

    def profile(cols):
        words = len(cols) * n_s * R
        out = torch.full((words + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
        stats = torch.zeros(4, dtype=torch.int64, device=DEV)
        blk = _native.KnnProfile(cols, queue=queue, out_bits=out, stats=stats, **common)
        _native.check(lib.flooder_sweep_knn_profile_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_profile_f32")
        got = out.cpu().numpy()
        assert (got[words:] == SENTINEL).all(), "guard words behind the last plane were written"
        return got[:words].view(np.uint32).reshape(len(cols), n_s * R), stats.cpu().numpy()

    def brute(k, stat):
        if stat == 0:
            return asc[:, k - 1].view(np.uint32)
        acc = asc[:, 0].copy()
        for i in range(1, k):
            acc = (acc + asc[:, i]).astype(np.float32)
        return (acc / np.float32(k)).astype(np.float32).view(np.uint32)

    for cols in _column_sets(n):
        assert cols and len(cols) <= 64
        planes, stats = profile(cols)
        k_max = max(k for k, _ in cols)
        for c, (k, stat) in enumerate(cols):
            want, _ = single(k, stat)
            bad = np.argwhere(planes[c] != want)[:5].ravel()
            assert bad.size == 0, (len(cols), c, k, stat, "single sweep", bad)
            bad = np.argwhere(planes[c] != brute(k, stat))[:5].ravel()
            assert bad.size == 0, (len(cols), c, k, stat, "brute force", bad)
        again, stats2 = profile(cols)
        assert np.array_equal(planes, again) and np.array_equal(stats, stats2)
        # the traversal is that of the single sweep at the largest k: same leaves evaluated, leaf tests, node tests
        _, want_stats = single(k_max, 0)
        assert stats[0] > 0 and np.array_equal(stats[:3], want_stats[:3]), (stats, want_stats)
    if n <= 32:
        assert max(k for k, _ in _column_sets(n)[0]) == n       # k_max = n: every point is a neighbour


def test_entry_point_refusals_leave_the_buffer_alone():
    tp = torch.rand(20, 3, device=DEV)
    index = core.PointIndex(tp)
    lib = _native.load()
    verts = tp[:4].reshape(1, 4, 3).contiguous()
    weights = torch.full((5, 4), 0.25, device=DEV)
    common = dict(pts_sorted=index.pts, n_pts=index.n, dim=3, k1=4, nodes=index.nodes, verts=verts, weights=weights, R=5,
                  n_simplices=1)

    def refused(cols, **change):
        out = torch.full((64 * 5 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
        blk = _native.KnnProfile(cols, queue=queue, out_bits=out, **common)
        for name, value in change.items():
            setattr(blk, name, value)
        rc = lib.flooder_sweep_knn_profile_f32(ctypes.byref(blk), _stream())
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), (cols, change)
        return rc != 0

    good = [(2, 0), (5, 1)]
    assert refused(good, n_cols=0) and refused(good, n_cols=65)
    assert refused([(2, 0), (0, 0)]) and refused([(2, 0), (33, 1)])
    assert refused([(2, 0), (3, 2)])
    assert refused([(2, 0), (5, 1), (2, 0)])
    assert refused([(2, 0), (21, 0)])                 # k_max > n_pts = 20
    assert refused(good, abi=2)
    # ... and the same block without a fault is accepted (k_max = n_pts included)
    out = torch.full((2 * 5 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
    blk = _native.KnnProfile([(2, 0), (20, 1)], queue=queue, out_bits=out, **common)
    assert lib.flooder_sweep_knn_profile_f32(ctypes.byref(blk), _stream()) == 0
    got = out.cpu().numpy()
    assert (got[:10] != SENTINEL).all() and (got[10:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ end to end
KS = (1, 2, 3, 8, 17, 32)
COLUMNS = ((1, "kth"), (2, "kth"), (3, "dtm"), (8, "kth"), (8, "dtm"), (17, "dtm"), (32, "kth"))


def _e2e_cloud(name):
    if name == "torus":
        return generate_noisy_torus_points_3d(100_000, seed=3).to(torch.float32), 200, dict(points_per_edge=12)
    if name == "eight":
        return generate_figure_eight_points_2d(50_000, seed=4).to(torch.float32), 200, dict(points_per_edge=20)
    if name == "gauss6":
        g = torch.Generator().manual_seed(6)
        return torch.randn(50_000, 6, generator=g), 60, dict(points_per_edge=6, max_dimension=2)
    g = torch.Generator().manual_seed(8)
    return torch.randn(100_000, 3, generator=g), 200, dict(points_per_edge=None, num_rand=200)


_REFERENCE = {}


def _reference(name):
    """(points, landmarks, keywords, {column: flood_complex dict}) of a cloud: computed once, shared, never changed."""
    if name not in _REFERENCE:
        pts, n_lms, kw = _e2e_cloud(name)
        tp = pts.to(DEV)
        lms = fa.generate_landmarks(tp, n_lms, start_idx=0)
        ref = {}
        for k, s in COLUMNS:
            torch.manual_seed(21)
            ref[(k, s)] = fa.flood_complex(tp, lms, neighbors=k, neighbor_stat=s, **kw)
        _REFERENCE[name] = (tp, lms, kw, ref)
    return _REFERENCE[name]


@pytest.mark.parametrize("name", ["torus", "eight", "gauss6", "num_rand"])
def test_every_column_is_the_single_call(name):
    tp, lms, kw, ref = _reference(name)
    torch.manual_seed(21)
    prof = fa.flood_profile(tp, lms, neighbors=KS, neighbor_stat=("kth", "dtm"), **kw)
    assert set(COLUMNS) <= set(prof.columns) and len(prof.columns) == 12
    for col in COLUMNS:
        assert prof[col] == ref[col], (name, col)
    assert len(ref[(32, "kth")]) > 1000 and ref[(32, "kth")] != ref[(8, "kth")] != ref[(8, "dtm")]
    torch.manual_seed(21)
    again = fa.flood_profile(tp, lms, neighbors=KS, neighbor_stat=("kth", "dtm"), **kw)
    for col in prof.columns:
        assert again[col] == prof[col], (name, col, "second run")


def test_integer_landmarks():
    tp, _, kw, ref = _reference("torus")
    prof = fa.flood_profile(tp, 200, start_idx=0, neighbors=KS, neighbor_stat=("kth", "dtm"), **kw)
    for col in COLUMNS:
        assert prof[col] == ref[col], col
    k, s = 8, "dtm"
    assert prof[(k, s)] == fa.flood_complex(tp, 200, start_idx=0, neighbors=k, neighbor_stat=s, **kw)


def test_with_the_index_of_the_landmark_selection():
    tp, _, kw, ref = _reference("torus")
    lms, index = fa.generate_landmarks(tp, 200, start_idx=0, return_index=True)
    if index is None:
        index = core.PointIndex(tp)
    prof = fa.flood_profile(tp, lms, neighbors=KS, neighbor_stat=("kth", "dtm"), index=index, **kw)
    for col in COLUMNS:
        assert prof[col] == ref[col], col
    assert prof[(17, "dtm")] == fa.flood_complex(tp, lms, neighbors=17, neighbor_stat="dtm", index=index, **kw)


def test_simplex_trees_hold_equal_arrays():
    tp, lms, kw, _ = _reference("torus")
    prof = fa.flood_profile(tp, lms, neighbors=(1, 3, 32), neighbor_stat=("kth", "dtm"), return_simplex_tree=True, **kw)
    for k, s in ((1, "kth"), (3, "dtm"), (32, "kth")):
        want = fa.flood_complex(tp, lms, neighbors=k, neighbor_stat=s, return_simplex_tree=True, **kw)
        got = prof[(k, s)]
        for d in range(4):
            assert np.array_equal(got.simplices_of_dimension(d), want.simplices_of_dimension(d))
            assert np.array_equal(got.filtrations_of_dimension(d), want.filtrations_of_dimension(d)), (k, s, d)


def test_three_simplex_groups_give_the_same_values(monkeypatch):
    tp, lms, kw, ref = _reference("torus")
    lib = _native.load()
    real = lib.flooder_sweep_knn_profile_f32
    launches = []

    def counted(blk, st):
        launches.append(int(blk._obj.n_simplices))
        return real(blk, st)

    monkeypatch.setattr(lib, "flooder_sweep_knn_profile_f32", counted)
    n_tets = sum(1 for key in ref[(1, "kth")] if len(key) == 4)
    R = core._grid_tables(kw["points_per_edge"], 3, DEV, torch.float32)[0].shape[0]
    monkeypatch.setattr(core, "PROFILE_WORKSPACE_BYTES", 4 * 12 * R * -(-n_tets // 3))
    prof = fa.flood_profile(tp, lms, neighbors=KS, neighbor_stat=("kth", "dtm"), **kw)
    assert len(launches) == 3 and sum(launches) == n_tets and max(launches) == -(-n_tets // 3)
    for col in COLUMNS:
        assert prof[col] == ref[col], col
