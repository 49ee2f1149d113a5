"""``flooder_amd.neighbor_distance`` on CPU tensors against a numpy brute force, its argument rules, its agreement with
the vertex values of ``flood_complex(neighbors=k)``, and what ``flooder_sweep_knn_sorted_f32`` refuses before a pointer is
looked at (no device needed; the non-null "pointers" are the number 4096)."""

import ctypes

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native

from helpers import tolerances

KS = (1, 2, 5, 32)
STATS = ("kth", "dtm")


def _brute(P, Q, k, stat):
    """float64: all squared distances sorted ascending -> the squared statistic (duplicates are separate columns)."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    d2 = np.sort(((Q[:, None, :] - P[None, :, :]) ** 2).sum(axis=2), axis=1)[:, :k]
    return d2[:, -1] if stat == "kth" else d2.sum(axis=1) / k


def _cloud(dim, dtype, seed=0):
    """300 points of which 100 are copies of others, 70 queries: 20 of them cloud points, the rest around the cloud."""
    g = torch.Generator().manual_seed(1000 * dim + seed)
    base = torch.randn(200, dim, generator=g, dtype=torch.float64)
    pts = torch.cat([base, base[:100]])[torch.randperm(300, generator=g)].to(dtype)
    qs = torch.cat([pts[:20], 1.5 * torch.randn(50, dim, generator=g, dtype=torch.float64).to(dtype)])
    return pts, qs


def _assert_close(got, want, points, what):
    rtol, atol = tolerances(points)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    assert (err <= atol + rtol * np.abs(want)).all(), (what, float(err.max()))


# ----------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dim", [1, 2, 3, 6])
def test_values_against_the_brute_force(dim, dtype):
    pts, qs = _cloud(dim, dtype)
    for k in KS:
        for stat in STATS:
            want2 = _brute(pts.numpy(), qs.numpy(), k, stat)
            got = fa.neighbor_distance(pts, qs, k, stat)
            got2 = fa.neighbor_distance(pts, qs, k, stat, squared=True)
            assert got.dtype == dtype and got.shape == (70,) and got2.dtype == dtype and got2.shape == (70,)
            _assert_close(got.numpy(), np.sqrt(want2), pts.numpy(), (dim, k, stat))
            # (squared: the tolerance of the distance carried through the square, d^2 (1 + e)^2 + 2 d a + a^2)
            rtol, atol = tolerances(pts.numpy())
            d = np.sqrt(want2)
            assert (np.abs(got2.numpy().astype(np.float64) - want2) <= 3 * rtol * want2 + 3 * d * atol + atol * atol).all()


def test_duplicates_count_twice():
    pts, _ = _cloud(3, torch.float64)
    P = pts.numpy()
    _, inverse, counts = np.unique(P, axis=0, return_inverse=True, return_counts=True)
    doubled = counts[inverse.ravel()] == 2
    assert len(counts) == 200 and doubled.sum() == 200
    d2 = fa.neighbor_distance(pts, None, 2, "kth").numpy()
    assert (d2[doubled] == 0).all() and (d2[~doubled] > 0).all()          # the copy is the second neighbour
    dtm = fa.neighbor_distance(pts, None, 3, "dtm", squared=True).numpy()
    assert np.allclose(dtm[doubled], fa.neighbor_distance(pts, None, 3, "kth", squared=True).numpy()[doubled] / 3, rtol=1e-12)


# ----------------------------------------------------------------------------------------------------- queries=None
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_queries_none_is_the_cloud_in_input_order(dtype):
    pts, _ = _cloud(3, dtype, seed=1)
    assert (fa.neighbor_distance(pts) == 0).all() and fa.neighbor_distance(pts).shape == (300,)
    for k in (1, 2, 5):
        for stat in STATS:
            own = fa.neighbor_distance(pts, None, k, stat)
            assert torch.equal(own, fa.neighbor_distance(pts, pts.clone(), k, stat))
            _assert_close(own.numpy(), np.sqrt(_brute(pts.numpy(), pts.numpy(), k, stat)), pts.numpy(), (k, stat))


def test_no_queries_give_an_empty_tensor():
    pts, _ = _cloud(2, torch.float32)
    out = fa.neighbor_distance(pts, torch.empty((0, 2)), 3, "dtm")
    assert out.shape == (0,) and out.dtype == torch.float32


# ------------------------------------------------------------------------------------------ agreement with the complex
@pytest.mark.parametrize("dim,dtype", [(2, torch.float32), (3, torch.float64), (4, torch.float32)])
def test_vertex_values_of_flood_complex(dim, dtype):
    g = torch.Generator().manual_seed(dim)
    pts = torch.randn(2000, dim, generator=g, dtype=torch.float64).to(dtype)
    lms = fa.generate_landmarks(pts, 25, start_idx=0)
    for k in (1, 2, 5):
        for stat in STATS:
            fc = fa.flood_complex(pts, lms, points_per_edge=4, max_dimension=1, neighbors=k, neighbor_stat=stat)
            want = np.array([fc[(i,)] for i in range(25)])
            _assert_close(fa.neighbor_distance(pts, lms, k, stat).numpy(), want, pts.numpy(), (dim, k, stat))


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    pts = torch.rand(10, 3)
    with pytest.raises(ValueError, match=r"neighbors must be in 1\.\.32"):
        fa.neighbor_distance(pts, None, 0)
    with pytest.raises(ValueError, match=r"neighbors must be in 1\.\.32"):
        fa.neighbor_distance(pts, None, 33)
    with pytest.raises(ValueError, match="exceeds the number of points"):
        fa.neighbor_distance(pts, None, 11)
    with pytest.raises(TypeError, match="integer"):
        fa.neighbor_distance(pts, None, 2.0)
    with pytest.raises(TypeError, match="integer"):
        fa.neighbor_distance(pts, None, True)
    with pytest.raises(ValueError, match="neighbor_stat"):
        fa.neighbor_distance(pts, None, 2, "mean")
    for bad in (torch.rand(5, 2), torch.rand(5), torch.rand(5, 3, 1)):
        with pytest.raises(RuntimeError, match="queries must be"):
            fa.neighbor_distance(pts, bad)
    with pytest.raises(RuntimeError, match=r"queries\.dtype"):
        fa.neighbor_distance(pts, torch.rand(5, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"queries\.device"):
        fa.neighbor_distance(pts, torch.empty((5, 3), device="meta"))
    with pytest.raises(ValueError, match="index="):
        fa.neighbor_distance(pts, None, 2, index=object())
    with pytest.raises(RuntimeError, match="non-empty"):
        fa.neighbor_distance(torch.empty((0, 3)))


def test_is_a_public_name():
    assert "neighbor_distance" in fa.__all__ and fa.neighbor_distance is fa.neighbors.neighbor_distance


# ---------------------------------------------------------------------------------------------- ABI without a device
P = 4096   # a pointer that is not NULL (never dereferenced: every call below is refused, or has nothing to do)
POINTERS = "pts_sorted nodes verts weights queue out_bits sample_order".split()
GOOD = dict(n_pts=1000, dim=3, k1=4, R=35, k=8, n_simplices=10, stat=1, **{name: P for name in POINTERS})


def _rc(**change):
    blk = _native.KnnSorted(**{**GOOD, **change})
    return _native.load().flooder_sweep_knn_sorted_f32(ctypes.byref(blk), None)


def test_sorted_entry_refuses_before_a_pointer_is_looked_at():
    assert "flooder_sweep_knn_sorted_f32" in _native.SIGNATURES
    assert len(_native.SIGNATURES["flooder_sweep_knn_sorted_f32"][1]) == 2
    lib = _native.load()
    for name in POINTERS:
        assert _rc(**{name: None}) == -1, name
        assert lib.flooder_last_error(), name
    assert _rc(sample_order=None) == -1 and b"sample_order" in lib.flooder_last_error()
    bad = [dict(k=0), dict(k=33), dict(dim=1), dict(dim=9), dict(stat=2), dict(n_pts=7), dict(k1=0), dict(k1=10),
           dict(n_simplices=1 << 22, R=1024),              # 2^32 samples
           dict(n_simplices=(1 << 32) - 2, R=1),           # the sorted sweeps' own limit
           dict(R=-1), dict(n_simplices=-1)]
    for change in bad:
        assert _rc(**change) == -1, change
        assert lib.flooder_last_error().startswith(b"flooder_sweep_knn_sorted_f32"), change
    assert _rc(n_simplices=(1 << 32) - 3, R=1, pts_sorted=None) == -1      # (below the limit: refused for the pointer)
    # nothing to do: accepted before any pointer is looked at
    null = {name: None for name in POINTERS}
    assert _rc(n_simplices=0, **null) == 0
    assert _rc(R=0, **null) == 0
    assert lib.flooder_sweep_knn_sorted_f32(None, None) == -1


def test_block_layout_extends_the_per_simplex_block():
    a, b = _native.KnnSweep._fields_, _native.KnnSorted._fields_
    assert b[:len(a)] == a and [name for name, _ in b[len(a):]] == ["sample_order"]
    assert ctypes.sizeof(_native.KnnSorted) == ctypes.sizeof(_native.KnnSweep) + 8
