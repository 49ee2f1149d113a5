"""The k-nearest sweep over sorted tiles on the device: ``flooder_sweep_knn_sorted_f32`` bit for bit on inputs where
float32 arithmetic is exact (against the float64 brute force and against ``flooder_sweep_knn_f32``), the order as a
performance input only, ``neighbor_distance`` on ROCm tensors, and the robust dimension pass routed through the sorted
form against the per-simplex form."""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from flooder_amd.synthetic import generate_annulus_points_2d

import grad_reference as gr
from helpers import smallest32, tolerances

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KS = (1, 2, 3, 8, 17, 32)
STATS = ("kth", "dtm")


def _stream():
    return _native.current_stream_ptr(DEV)


def _levels(n):
    leaves, lv = (n + 15) // 16, 1
    while leaves > 64:
        leaves, lv = (leaves + 63) // 64, lv + 1
    return lv


# name -> (dim, n points, every point doubled, tree levels, simplex form (points_per_edge, simplex dimension, simplices)
# or None, query form (Q,) or None).  The smallest shapes at which the form can go wrong: a partial last tile (360 =
# 5 * 64 + 40; 1050 = 16 * 64 + 26), the query form at one partial tile / exactly one tile / one live lane in the second,
# every depth of the tree, k = n - 1, clamped keys.
CASES = {
    "2d": (2, 40, False, 1, (5, 2, 24), None),
    "3d_q63": (3, 1025, True, 2, None, 63),
    "3d_q64": (3, 1025, True, 2, None, 64),
    "3d_q65": (3, 1025, True, 2, None, 65),
    "4d": (4, 70_001, False, 3, (5, 3, 30), None),
    "6d": (6, 1025, True, 2, (9, 2, 40), None),
    "8d_far": (8, 33, False, 1, None, 200),
    "3d_deep": (3, 4_300_001, False, 4, None, 130),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of a case on the device, its index, its sorted order and the float64 brute force - built once."""
    dim, n, dup, levels, simplex, n_q = CASES[name]
    assert _levels(n) == levels and n % 16 != 0
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng(700 + seed)
    ppe = simplex[0] if simplex else 2            # (queries: lattice step 1)
    step = ppe - 1
    # integer coordinates in [-r, r] as wide as keeps every d2 below 2**24 units of step**-2 (far queries: 4 r away)
    r = min(511, int(2047 / (step * math.sqrt(dim)))) // (4 if name == "8d_far" else 1)
    if dup:
        base = rng.integers(-r, r + 1, size=((n + 1) // 2, dim))
        P = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        P = rng.integers(-r, r + 1, size=(n, dim))
    if simplex:
        _, d, n_s = simplex
        V = rng.integers(-r, r + 1, size=(n_s, d + 1, dim))
        V[: n_s // 4] = P[rng.integers(0, n, size=(n_s // 4, d + 1))]          # simplices on points of the cloud
        V[n_s // 4: n_s // 2] //= 4                                            # small ones near the centre
        W = gr.lattice(ppe, d)
    else:
        V = rng.integers(-r, r + 1, size=(n_q, 1, dim))
        if name == "8d_far":
            V[: n_q // 2, 0] = P[rng.integers(0, n, size=n_q // 2)]            # half the queries are cloud points
            V[n_q // 2: n_q // 2 + n_q // 4] += 3 * r                           # a quarter far outside the cloud's box
            assert (V[n_q // 2: n_q // 2 + n_q // 4, 0] > P.max(axis=0)).all()
        else:
            V[: n_q // 4, 0] = P[rng.integers(0, n, size=n_q // 4)]
        W = torch.ones((1, 1), dtype=torch.float64)
    gr.assert_exact_inputs(P, V.reshape(-1, dim), ppe)
    n_s, k1, R = V.shape[0], V.shape[1], W.shape[0]
    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    samples = torch.einsum("rk,skd->srd", W.to(DEV), torch.as_tensor(V, dtype=torch.float64, device=DEV))
    small = smallest32(tp.double(), samples.reshape(-1, dim))                  # (S * R, min(32, n)) float64, ascending
    assert small.max() * step * step < 2 ** 24
    if dup:    # the copies are there: the two smallest of most samples are equal
        assert (small[:, 0] == small[:, 1]).mean() > 0.5
    t_v = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    t_w = W.to(torch.float32).to(DEV).contiguous()
    lib = _native.load()
    order = core._sorted_sample_order(lib, _stream(), index, t_v, t_w, None, None, int(lib.flooder_sample_key_bits(dim)))
    assert sorted(order.cpu().tolist()) == list(range(n_s * R))
    return dict(dim=dim, n=n, points=tp, index=index, verts=t_v, weights=t_w, k1=k1, R=R, n_s=n_s, small=small, order=order)


def _sweep(c, k, stat, order=None, check_stats=True):
    """The words of ``flooder_sweep_knn_sorted_f32`` (``order``: a tensor) or ``flooder_sweep_knn_f32`` (None)."""
    lib = _native.load()
    n_s, R = c["n_s"], c["R"]
    out = torch.full((n_s, R), -1, dtype=torch.int32, device=DEV)
    queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    args = dict(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                verts=c["verts"], weights=c["weights"], R=R, k=k, n_simplices=n_s, stat=stat, queue=queue, out_bits=out,
                stats=stats)
    if order is not None:
        blk = _native.KnnSorted(sample_order=order, **args)
        _native.check(lib.flooder_sweep_knn_sorted_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_sorted_f32")
        tiles = (n_s * R + 63) // 64
    else:
        blk = _native.KnnSweep(**args)
        _native.check(lib.flooder_sweep_knn_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_f32")
        tiles = n_s * ((R + 63) // 64)
    if check_stats:
        st = stats.cpu().numpy()
        assert st[0] > 0 and st[1] >= st[0] and st[2] >= tiles, (st, tiles)   # leaves evaluated / tested, node tests
    return out.cpu().numpy().view(np.uint32).reshape(-1)


def _expected(small, k, stat):
    """kth: the k-th smallest of the float64 brute force (exact in float32); dtm: the float32 replay of the ascending
    sum, divided by (float)k."""
    if stat == 0:
        want = small[:, k - 1].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), small[:, k - 1])
        return want.view(np.uint32)
    asc = small[:, :k].astype(np.float32)
    acc = asc[:, 0].copy()
    for i in range(1, k):
        acc = (acc + asc[:, i]).astype(np.float32)
    return (acc / np.float32(k)).astype(np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ kernel level
def test_cases_cover_what_they_must():
    assert {c[0] for c in CASES.values()} == {2, 3, 4, 6, 8} and {c[3] for c in CASES.values()} == {1, 2, 3, 4}
    assert (24 * 15) % 64 != 0 and (30 * 35) % 64 != 0 and CASES["8d_far"][1] - 1 == 32


@pytest.mark.parametrize("name", list(CASES))
def test_sorted_sweep_exact_and_equal_to_the_per_simplex_sweep(name):
    c = _case(name)
    for k in KS:
        if k > c["n"]:
            continue
        for stat in (0, 1):
            want = _expected(c["small"], k, stat)
            got = _sweep(c, k, stat, c["order"])
            assert np.array_equal(got, want), (name, k, STATS[stat], np.argwhere(got != want)[:5].ravel())
            assert np.array_equal(got, _sweep(c, k, stat)), (name, k, STATS[stat], "per-simplex sweep differs")


def test_the_order_is_a_performance_input_only():
    c = _case("4d")
    N = c["n_s"] * c["R"]
    identity = torch.arange(N, dtype=torch.int32, device=DEV)
    shuffled = torch.as_tensor(np.random.default_rng(5).permutation(N).astype(np.int32), device=DEV)
    for k in (2, 17):
        for stat in (0, 1):
            want = _sweep(c, k, stat, c["order"])
            assert np.array_equal(_sweep(c, k, stat, identity), want)
            assert np.array_equal(_sweep(c, k, stat, shuffled), want)


def test_two_runs_give_identical_words():
    for name in ("4d", "3d_q65"):
        c = _case(name)
        for stat in (0, 1):
            assert np.array_equal(_sweep(c, 8, stat, c["order"]), _sweep(c, 8, stat, c["order"]))


# ------------------------------------------------------------------------------------------------- public, on ROCm
@pytest.mark.parametrize("name", ["3d_q65", "8d_far"])
def test_squared_neighbor_distance_is_the_kernels_words(name):
    c = _case(name)
    queries = c["verts"][:, 0, :].contiguous()
    for k in (1, 8, 32):
        for stat in (0, 1):
            got = fa.neighbor_distance(c["points"], queries, k, STATS[stat], squared=True)
            assert got.dtype == torch.float32 and got.shape == (c["n_s"],) and got.device == c["points"].device
            assert np.array_equal(got.cpu().numpy().view(np.uint32), _sweep(c, k, stat, c["order"]))
            assert np.array_equal(fa.neighbor_distance(c["points"], queries, k, STATS[stat], squared=True,
                                                       index=c["index"]).cpu().numpy().view(np.uint32),
                                  got.cpu().numpy().view(np.uint32))


def _complex_cloud(name):
    if name == "annulus":
        return generate_annulus_points_2d(20_000, seed=7).to(torch.float32).to(DEV), 200, dict(points_per_edge=6)
    g = torch.Generator().manual_seed(4)
    return torch.randn(20_000, 4, generator=g).to(DEV), 40, dict(points_per_edge=6, max_dimension=2)


@pytest.mark.parametrize("name", ["annulus", "gauss4"])
def test_vertex_values_of_flood_complex_bit_for_bit(name):
    tp, n_lms, kw = _complex_cloud(name)
    lms = fa.generate_landmarks(tp, n_lms, start_idx=0)
    for k in (2, 17):
        for stat in STATS:
            fc = fa.flood_complex(tp, lms, neighbors=k, neighbor_stat=stat, **kw)
            want = np.array([fc[(i,)] for i in range(n_lms)], dtype=np.float64)
            got = fa.neighbor_distance(tp, lms, k, stat).cpu().numpy().astype(np.float64)
            assert np.array_equal(got, want), (name, k, stat, np.abs(got - want).max())


def test_own_points_against_the_kdtree(monkeypatch):
    from scipy.spatial import cKDTree

    g = torch.Generator().manual_seed(11)
    base = torch.randn(3500, 3, generator=g)
    pts = torch.cat([base, base[:1500]])[torch.randperm(5000, generator=g)]
    tp = pts.to(DEV)
    P = pts.numpy().astype(np.float64)
    rtol, atol = tolerances(P)
    whole = {}
    for k in (1, 2, 9, 32):
        dist, _ = cKDTree(P).query(P, k=k, workers=-1)
        dist = dist.reshape(5000, k)
        for stat in STATS:
            want = dist[:, -1] if stat == "kth" else np.sqrt(np.square(dist).sum(axis=1) / k)
            whole[k, stat] = fa.neighbor_distance(tp, None, k, stat)
            got = whole[k, stat].cpu().numpy().astype(np.float64)
            assert (np.abs(got - want) <= atol + rtol * want).all(), (k, stat, np.abs(got - want).max())
    assert bool((whole[1, "kth"] == 0).all())
    # groups of queries bounded by the workspace: the same words
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", 24 * 1000)
    for key, want in whole.items():
        assert torch.equal(fa.neighbor_distance(tp, None, *key), want), key


def test_device_refusals():
    with pytest.raises(ValueError, match="float32"):
        fa.neighbor_distance(torch.rand(100, 3, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="dimension 2 to 8"):
        fa.neighbor_distance(torch.rand(100, 1, device=DEV))
    with pytest.raises(ValueError, match="dimension 2 to 8"):
        fa.neighbor_distance(torch.rand(100, 9, device=DEV))
    with pytest.raises(RuntimeError, match=r"queries\.device"):
        fa.neighbor_distance(torch.rand(100, 3, device=DEV), torch.rand(5, 3))
    assert fa.neighbor_distance(torch.rand(100, 3, device=DEV), torch.empty((0, 3), device=DEV), 2).shape == (0,)


# ---------------------------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("dim", [4, 6])
def test_dimension_pass_sorted_and_per_simplex_agree(dim, monkeypatch):
    g = torch.Generator().manual_seed(dim)
    tp = torch.randn(20_000, dim, generator=g).to(DEV)
    lms = fa.generate_landmarks(tp, 60, start_idx=0)
    kw = dict(points_per_edge=6, max_dimension=2)
    monkeypatch.setattr(core, "BVH_SORTED_MIN_SAMPLES", 1)
    sorted_calls = []
    sort_stage = core._sorted_sample_order
    monkeypatch.setattr(core, "_sorted_sample_order", lambda *a, **k: sorted_calls.append(1) or sort_stage(*a, **k))
    for k in (2, 17):
        for stat in STATS:
            got = {}
            for form in (True, False):
                monkeypatch.setattr(core, "KNN_SORTED_SAMPLES", form)
                del sorted_calls[:]
                got[form] = (fa.flood_complex(tp, lms, neighbors=k, neighbor_stat=stat, **kw),
                             fa.flood_filtration(tp, lms, neighbors=k, neighbor_stat=stat, **kw))
                assert len(sorted_calls) == (2 if form else 0)      # the one grid pass of each call, or none
            assert got[True][0] == got[False][0], (dim, k, stat)
            Fs, Fp = got[True][1], got[False][1]
            assert Fs.faces_not_found == 0 and Fp.faces_not_found == 0
            for d in range(3):
                assert torch.equal(Fs.values[d], Fp.values[d]), (dim, k, stat, d)
                assert torch.equal(Fs.witness_neighbors[d], Fp.witness_neighbors[d]), (dim, k, stat, d)
                assert torch.equal(Fs.witness_weights[d], Fp.witness_weights[d]), (dim, k, stat, d)
