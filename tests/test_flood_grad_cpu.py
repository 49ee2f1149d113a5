"""flood_filtration on CPU tensors: values, exact witnesses, gradients against brute-force autograd, diagrams."""

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd.core import generate_grid

from helpers import tolerances


def _cloud(n, dim, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, dim, generator=g, dtype=torch.float64).to(dtype)


def _grid(ppe, d):
    return torch.ones((1, 1), dtype=torch.float64) if d == 0 else generate_grid(ppe, d, "cpu", torch.float64)[0]


def _witness_values(F, points, landmarks):
    """|p* - x*| in float64 from the witnesses, per dimension."""
    P, L = points.detach().double(), landmarks.detach().double()
    out = []
    for d, simp in enumerate(F.simplices):
        p = (F.witness_weights[d].double().unsqueeze(2) * L[simp.long()]).sum(1)
        out.append((p - P[F.witness_point[d]]).norm(dim=1))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("num_rand", [None, 25])
def test_values_equal_flood_complex(dtype, dim, num_rand):
    pts = _cloud(2500, dim, dtype)
    torch.manual_seed(7)
    F = fa.flood_filtration(pts, 30, points_per_edge=7, num_rand=num_rand)
    torch.manual_seed(7)
    with pytest.warns(RuntimeWarning) if dtype is torch.float64 else _nothing():
        fc = fa.flood_complex(pts, 30, points_per_edge=7, num_rand=num_rand)
    assert F.to_dict() == fc
    for d, simp in enumerate(F.simplices):
        want = torch.tensor([fc[tuple(r)] for r in simp.tolist()], dtype=dtype)
        assert torch.equal(F.values[d].detach(), want)
        assert F.values[d].dtype == dtype and F.values[d].device == pts.device
        assert (F.witness_point[d] >= 0).all()


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("num_rand", [None, 25])
def test_witness_realises_value_and_is_nearest(dtype, num_rand):
    pts = _cloud(2000, 3, dtype, seed=1)
    torch.manual_seed(3)
    F = fa.flood_filtration(pts, 25, points_per_edge=6, num_rand=num_rand)
    lms = pts[F.landmark_ids]
    P = pts.double()
    rtol, atol = tolerances(pts.numpy())
    for d, wv in enumerate(_witness_values(F, pts, lms)):
        v = F.tree.filtrations_of_dimension(d)
        tol = atol + rtol * np.abs(v)
        assert np.all(np.abs(wv.numpy() - v) <= tol), d
        # no point of the cloud is closer to p* than x* (brute force)
        p = (F.witness_weights[d].double().unsqueeze(2) * lms.double()[F.simplices[d].long()]).sum(1)
        nn = torch.cdist(p, P).min(dim=1).values
        assert torch.all(wv - nn <= torch.as_tensor(tol)), d
        # the weights are a convex combination over the simplex's own vertices
        w = F.witness_weights[d].double()
        assert torch.all(w >= 0) and torch.allclose(w.sum(1), torch.ones(w.shape[0], dtype=torch.float64), atol=1e-6)


def test_witness_weights_are_sample_rows():
    ppe = 6
    pts = _cloud(1500, 2, torch.float64, seed=2)
    F = fa.flood_filtration(pts, 20, points_per_edge=ppe)
    for d, w in enumerate(F.witness_weights):
        grid = _grid(ppe, d).numpy()
        for row in w.numpy():
            assert np.abs(grid - row).max(axis=1).min() == 0.0


def test_deterministic_witnesses():
    pts = _cloud(1500, 3, torch.float32, seed=4)
    a = fa.flood_filtration(pts, 20, points_per_edge=5)
    b = fa.flood_filtration(pts, 20, points_per_edge=5)
    for d in range(len(a.simplices)):
        assert torch.equal(a.witness_point[d], b.witness_point[d])
        assert torch.equal(a.witness_weights[d], b.witness_weights[d])


def _brute_values(points, landmarks, simplices, ppe):
    """float64 autograd: samples = W @ V, cdist, min over points, max over samples, per simplex."""
    out, gaps = [], []
    for d, simp in enumerate(simplices):
        W = _grid(ppe, d)
        V = landmarks[simp.long()]                                  # (n, d+1, dim)
        samples = W.unsqueeze(0) @ V                                 # (n, R, dim)
        dist = torch.cdist(samples.reshape(-1, points.shape[1]), points).reshape(samples.shape[0], W.shape[0], -1)
        top2 = torch.topk(dist.detach(), 2, dim=2, largest=False).values     # nearest two points per sample
        mn = dist.min(dim=2).values                                  # (n, R)
        val, arg = mn.max(dim=1)
        s2 = torch.topk(mn.detach(), min(2, W.shape[0]), dim=1).values
        gap_max = (s2[:, 0] - s2[:, 1]) if W.shape[0] > 1 else torch.full_like(val, np.inf)
        t2 = top2[torch.arange(samples.shape[0]), arg]
        gap_min = t2[:, 1] - t2[:, 0]
        out.append(val)
        rel = torch.clamp(val.detach(), min=1e-12)
        gaps.append((gap_max > 1e-6 * rel) & (gap_min > 1e-6 * rel))
    return out, gaps


def test_gradients_match_brute_force():
    ppe = 6
    pts = _cloud(400, 2, torch.float64, seed=5).requires_grad_(True)
    lms = _cloud(18, 2, torch.float64, seed=6).mul_(0.8).requires_grad_(True)
    F = fa.flood_filtration(pts, lms, points_per_edge=ppe)
    ref, good = _brute_values(pts, lms, F.simplices, ppe)
    n_good = sum(int(g.sum()) for g in good)
    assert n_good >= 0.95 * sum(g.numel() for g in good)
    gen = torch.Generator().manual_seed(0)
    coef = [torch.rand(g.shape[0], generator=gen, dtype=torch.float64) * g for g in good]
    for d in range(len(ref)):
        assert torch.allclose(F.values[d].detach(), ref[d].detach(), rtol=1e-12, atol=1e-12)
    loss = sum((c * v).sum() for c, v in zip(coef, F.values))
    gp, gl = torch.autograd.grad(loss, (pts, lms))
    loss_ref = sum((c * v).sum() for c, v in zip(coef, ref))
    rp, rl = torch.autograd.grad(loss_ref, (pts, lms))
    assert torch.allclose(gp, rp, rtol=1e-9, atol=1e-9)
    assert torch.allclose(gl, rl, rtol=1e-9, atol=1e-9)


def test_diagrams_match_tree_and_h1_gradient():
    ppe = 6
    pts = _cloud(400, 2, torch.float64, seed=8).requires_grad_(True)
    lms = _cloud(18, 2, torch.float64, seed=9).mul_(0.8).requires_grad_(True)
    F = fa.flood_filtration(pts, lms, points_per_edge=ppe)
    dg = F.diagrams()
    F.tree.compute_persistence()
    for d in range(2):
        want = F.tree.persistence_intervals_in_dimension(d)
        got = dg[d].detach().numpy() if d in dg else np.zeros((0, 2))
        assert np.array_equal(got, want), d
    assert 1 in dg and dg[1].shape[0] > 0
    # H1 total persistence against the brute force values at the same simplices
    from flooder_amd.persistence import persistence_pairs_simplices

    pairs = persistence_pairs_simplices(F.tree)[1]
    ref, _ = _brute_values(pts, lms, F.simplices, ppe)
    h1 = dg[1]
    loss = (h1[:, 1] - h1[:, 0]).sum()
    loss_ref = sum(ref[dd][dr] - ref[bd][br] for bd, br, dd, dr in pairs.tolist())
    gp, gl = torch.autograd.grad(loss, (pts, lms))
    rp, rl = torch.autograd.grad(loss_ref, (pts, lms))
    assert torch.allclose(gp, rp, rtol=1e-9, atol=1e-9) and torch.allclose(gl, rl, rtol=1e-9, atol=1e-9)


def test_essential_class_differentiable_in_birth_only():
    pts = _cloud(300, 2, torch.float64, seed=10).requires_grad_(True)
    F = fa.flood_filtration(pts, 12, points_per_edge=5)
    h0 = F.diagrams()[0]
    assert torch.isinf(h0[:, 1]).sum() == 1
    ess = h0[torch.isinf(h0[:, 1])][0, 0]
    (g,) = torch.autograd.grad(ess, pts)
    assert torch.isfinite(g).all()


def test_integer_landmarks_route_gradient_into_points():
    pts = _cloud(800, 2, torch.float64, seed=11).requires_grad_(True)
    F = fa.flood_filtration(pts, 15, points_per_edge=5)
    ids = fa.core.fps_indices(pts.detach(), 15, 0)
    assert torch.equal(F.landmark_ids, ids)
    loss = sum((v * (1 + d)).sum() for d, v in enumerate(F.values))
    (g,) = torch.autograd.grad(loss, pts)
    assert g[ids].abs().sum() > 0
    # the same landmarks passed as a tensor: the points' gradient = its own part + the landmarks' part at `ids`
    pts2 = pts.detach().clone().requires_grad_(True)
    lms2 = pts.detach()[ids].clone().requires_grad_(True)
    F2 = fa.flood_filtration(pts2, lms2, points_per_edge=5)
    assert F2.to_dict() == F.to_dict()
    loss2 = sum((v * (1 + d)).sum() for d, v in enumerate(F2.values))
    gp2, gl2 = torch.autograd.grad(loss2, (pts2, lms2))
    assert torch.allclose(g, gp2.index_add(0, ids, gl2), rtol=1e-12, atol=1e-12)


def test_landmark_tensor_gets_its_own_gradient():
    pts = _cloud(500, 2, torch.float64, seed=12)
    lms = _cloud(10, 2, torch.float64, seed=13).requires_grad_(True)
    F = fa.flood_filtration(pts, lms, points_per_edge=5)
    loss = sum(v.sum() for v in F.values)
    (gl,) = torch.autograd.grad(loss, lms)
    assert gl.shape == lms.shape and gl.abs().sum() > 0


def test_result_is_freed_after_use():
    """The autograd node keeps the witness tensors, not the result object: nothing holds F once the caller drops it."""
    import gc
    import weakref

    pts = _cloud(600, 2, torch.float64, seed=14).requires_grad_(True)
    for run_backward in (True, False):
        F = fa.flood_filtration(pts, 15, points_per_edge=5)
        ref = weakref.ref(F)
        loss = sum(v.sum() for v in F.values)
        if run_backward:
            loss.backward()
        del F, loss
        gc.collect()
        assert ref() is None


def test_unsupported_arguments_raise():
    pts = _cloud(200, 2, torch.float32)
    with pytest.raises(ValueError):
        fa.flood_filtration(pts, 10, method="ball")
    with pytest.raises(ValueError):
        fa.flood_filtration(pts, 10, method="nope")
    with pytest.raises(TypeError):
        fa.flood_filtration(pts.half(), 10)
    with pytest.raises(TypeError):
        fa.flood_filtration(pts, 10, reduce_hook=lambda t: None)
    with pytest.raises(TypeError):
        fa.flood_filtration(pts, 10, simplex_shard=(0, 2))
