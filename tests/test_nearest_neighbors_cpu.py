"""``flooder_amd.nearest_neighbors`` on CPU tensors against a float64 brute force, its agreement with
``neighbor_distance`` and its refusals; ``neighbor_distance`` as a differentiable function (``gradcheck`` of the closed
form of DESIGN.md section 9.4 on the kd-tree's ids); the export and the layout of ``flooder_knn_ids_t`` (no device
needed)."""

import ctypes
import os

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native

from helpers import ROOT, header_numbers, tolerances

KS = (1, 2, 8, 32)
STATS = ("kth", "dtm")


def _cloud(dim, dtype, seed=0, n=300, n_q=70):
    """Points in general position (no two squared distances of a query tie) and queries around the cloud."""
    g = torch.Generator().manual_seed(1000 * dim + seed)
    pts = torch.randn(n, dim, generator=g, dtype=torch.float64).to(dtype)
    qs = (1.5 * torch.randn(n_q, dim, generator=g, dtype=torch.float64)).to(dtype)
    return pts, qs


def _brute(P, Q, k):
    """float64: (ids, d2) of the k smallest (d2, id) per query."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    d2 = ((Q[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    ids = np.lexsort((np.broadcast_to(np.arange(P.shape[0]), d2.shape), d2), axis=1)[:, :k]
    return ids, np.take_along_axis(d2, ids, axis=1)


# ------------------------------------------------------------------------------------------------------ brute force
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dim", [2, 3, 6])
def test_ids_and_distances_against_the_brute_force(dim, dtype):
    pts, qs = _cloud(dim, dtype)
    rtol, atol = tolerances(pts.numpy())
    for own in (False, True):
        Q = pts if own else qs
        for k in KS:
            want_ids, want_d2 = _brute(pts.numpy(), Q.numpy(), k)
            # general position: the k + 1 smallest d2 of a query are apart by far more than the rounding of a
            # float64 squared distance (the kd-tree and the brute force both work in float64 on these very numbers)
            gaps = np.diff(_brute(pts.numpy(), Q.numpy(), k + 1)[1], axis=1)
            assert (gaps > 1e-12 * want_d2.max()).all()
            ids, dist = fa.nearest_neighbors(pts, None if own else qs, k)
            assert ids.dtype == torch.int64 and ids.shape == (Q.shape[0], k)
            assert dist.dtype == dtype and dist.shape == (Q.shape[0], k)
            assert np.array_equal(ids.numpy(), want_ids), (dim, k, own)
            want = np.sqrt(want_d2)
            assert (np.abs(dist.numpy().astype(np.float64) - want) <= atol + rtol * want).all(), (dim, k, own)
            if own:
                assert np.array_equal(ids[:, 0].numpy(), np.arange(pts.shape[0])) and bool((dist[:, 0] == 0).all())
            _, sq = fa.nearest_neighbors(pts, None if own else qs, k, squared=True)
            assert sq.dtype == dtype
            assert (np.abs(sq.numpy().astype(np.float64) - want_d2) <= 3 * rtol * want_d2 + 3 * want * atol + atol * atol).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_consistent_with_neighbor_distance(dtype):
    pts, qs = _cloud(3, dtype, seed=2)
    eps = 1e-12 if dtype is torch.float64 else 1e-6
    for k in KS:
        _, dist = fa.nearest_neighbors(pts, qs, k)
        assert torch.equal(dist[:, k - 1], fa.neighbor_distance(pts, qs, k, "kth"))
        dtm = fa.neighbor_distance(pts, qs, k, "dtm").double()
        rms = dist.double().square().mean(dim=1).sqrt()
        assert bool(((rms - dtm).abs() <= eps * dtm).all()), k


def test_no_queries_give_empty_tensors():
    pts, _ = _cloud(2, torch.float32)
    ids, dist = fa.nearest_neighbors(pts, torch.empty((0, 2)), 3)
    assert ids.shape == (0, 3) and ids.dtype == torch.int64 and dist.shape == (0, 3) and dist.dtype == torch.float32


# --------------------------------------------------------------------------------------------------------- refusals
def _refusal(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except Exception as exc:  # noqa: BLE001
        return type(exc), str(exc)
    return None


def test_every_refusal_of_neighbor_distance_with_the_same_message():
    pts = torch.rand(10, 3)
    calls = [((pts, None, 0), {}), ((pts, None, 33), {}), ((pts, None, 11), {}), ((pts, None, 2.0), {}),
             ((pts, None, True), {}), ((pts, torch.rand(5, 2)), {}), ((pts, torch.rand(5)), {}),
             ((pts, torch.rand(5, 3, 1)), {}), ((pts, torch.rand(5, 3, dtype=torch.float64)), {}),
             ((pts, torch.empty((5, 3), device="meta")), {}), ((pts, None, 2), dict(index=object())),
             ((torch.empty((0, 3)),), {}), ((torch.rand(10, 3).half(),), {}), (([[0.0, 1.0]],), {})]
    for args, kw in calls:
        want = _refusal(fa.neighbor_distance, *args, **kw)
        assert want is not None, (args, kw)
        assert _refusal(fa.nearest_neighbors, *args, **kw) == want, (args, kw)


# -------------------------------------------------------------------------------------------------------- gradients
def _grad_inputs(dim, own, seed):
    """40 to 80 points in general position; queries off the cloud (f > 0), or the cloud itself with k >= 2."""
    g = torch.Generator().manual_seed(50 + 7 * dim + seed)
    n = 40 + 20 * (dim - 2) + 20 * seed
    pts = torch.randn(n, dim, generator=g, dtype=torch.float64)
    qs = None if own else 1.3 * torch.randn(9, dim, generator=g, dtype=torch.float64) + 0.05
    return pts, qs


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_gradcheck(dim, own, stat, squared):
    pts, qs = _grad_inputs(dim, own, int(squared))
    assert 40 <= pts.shape[0] <= 80
    for k in (2, 5):      # (own points: k >= 2, so that f > 0)
        _, d = fa.nearest_neighbors(pts, qs, k + 1)
        assert bool((d[:, 1 if own else 0] > 1e-3).all())                      # f > 0: the closed form applies
        # the neighbour set and its last member stay what they are under gradcheck's perturbation (1e-6 per coordinate)
        assert bool((d[:, k] - d[:, k - 1] > 1e-5).all()) and bool((d[:, k - 1] - d[:, k - 2] > 1e-5).all())
        p = pts.clone().requires_grad_(True)
        if own:
            fn = lambda x: fa.neighbor_distance(x, None, k, stat, squared=squared)   # noqa: E731
            assert torch.autograd.gradcheck(fn, (p,))
        else:
            q = qs.clone().requires_grad_(True)
            fn = lambda x, y: fa.neighbor_distance(x, y, k, stat, squared=squared)   # noqa: E731
            assert torch.autograd.gradcheck(fn, (p, q))
            # one side only
            out = fa.neighbor_distance(pts, q, k, stat, squared=squared)
            (gq,) = torch.autograd.grad(out.sum(), q)
            out = fa.neighbor_distance(p, q, k, stat, squared=squared)
            gp2, gq2 = torch.autograd.grad(out.sum(), (p, q))
            assert torch.equal(gq, gq2) and bool((gp2.sum(dim=0) + gq2.sum(dim=0)).abs().max() < 1e-9)


def test_a_query_on_a_cloud_point_has_value_and_gradient_zero():
    pts, _ = _grad_inputs(3, False, 0)
    for stat in STATS:
        p = pts.clone().requires_grad_(True)
        q = pts[:5].clone().requires_grad_(True)
        out = fa.neighbor_distance(p, q, 1, stat)
        assert out.grad_fn is not None and bool((out == 0).all())
        out.sum().backward()
        assert bool((p.grad == 0).all()) and bool((q.grad == 0).all())


def test_values_with_grad_are_the_values_without_and_no_grad_means_no_graph():
    pts, qs = _grad_inputs(2, False, 1)
    for stat in STATS:
        plain = fa.neighbor_distance(pts, qs, 3, stat)
        assert plain.grad_fn is None and not plain.requires_grad
        with_grad = fa.neighbor_distance(pts.clone().requires_grad_(True), qs, 3, stat)
        assert with_grad.grad_fn is not None and torch.equal(with_grad.detach(), plain)
        with torch.no_grad():
            assert fa.neighbor_distance(pts.clone().requires_grad_(True), qs, 3, stat).grad_fn is None


# ---------------------------------------------------------------------------------------------- exports and binding
def test_is_a_public_name_and_bound():
    assert "nearest_neighbors" in fa.__all__ and fa.nearest_neighbors is fa.neighbors.nearest_neighbors
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "flooder_knn_ids_sorted_f32(" in header
    res, args = _native.SIGNATURES["flooder_knn_ids_sorted_f32"]
    assert res is ctypes.c_int and len(args) == 2 and args[0]._type_ is _native.KnnIds
    assert hasattr(_native.load(), "flooder_knn_ids_sorted_f32")
    a, b = _native.KnnSorted._fields_, _native.KnnIds._fields_
    assert b[:len(a)] == a and [name for name, _ in b[len(a):]] == ["order", "out_ids", "out_d2"]


def test_block_has_the_layout_of_the_header(tmp_path):
    """``flooder_knn_ids_t`` is ``flooder_knn_sorted_t`` and a tail in C as well (size and offsets of each against its
    class: test_host.py, test_parameter_block_has_the_layout_of_the_header)."""
    out = header_numbers(tmp_path, {"flooder_knn_sorted_t": _native.KnnSorted, "flooder_knn_ids_t": _native.KnnIds})
    for fname, _ in _native.KnnSorted._fields_:
        assert out["flooder_knn_ids_t", fname] == out["flooder_knn_sorted_t", fname], fname
    assert out["flooder_knn_ids_t", "order"] >= out["flooder_knn_sorted_t", "sizeof"]
