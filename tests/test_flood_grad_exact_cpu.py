"""The exact reference of the device tests (tests/grad_reference.py) held against the CPU path, without a GPU.

On integer clouds with a dyadic lattice float32 arithmetic is exact, so the kd-tree path of ``flood_filtration`` and the
float64 brute force must agree bit for bit on values, witness samples and witness distances (everything but the
smallest-id rule among equidistant points, which the kd-tree does not follow); and ``reference_gradient`` must equal
float64 autograd through the brute-force formula where no ties exist.  The reference, not the device, is the fixed point
of tests/test_gpu_flood_grad.py."""

import pytest
import torch

import flooder_amd as fa

import grad_reference as gr


def _integer_cloud(n, dim, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hi, (n, dim), generator=g).to(torch.float32)


# the two clouds of the device test's dense cases, shrunk (same density of points per lattice cell):
#   2-D  [0, 64)^2, points_per_edge 9: differences < 2^6 * 8 = 2^9 eighths, squares < 2^18, two axes < 2^19
#   3-D  [0, 16)^3, points_per_edge 5: differences < 2^4 * 4 = 2^6 quarters, squares < 2^12, three axes < 2^14
CASES = [("dense2d", 6000, 2, 64, 9, 40), ("dense3d", 2500, 3, 16, 5, 30)]


@pytest.mark.parametrize("name,n,dim,hi,ppe,n_l", CASES, ids=[c[0] for c in CASES])
def test_cpu_path_passes_the_exact_checks(name, n, dim, hi, ppe, n_l):
    pts = _integer_cloud(n, dim, hi, seed=3)
    F = fa.flood_filtration(pts, n_l, points_per_edge=ppe)
    lms = pts[F.landmark_ids]
    gr.assert_exact_inputs(pts, lms, ppe)
    faces = gr.reference_faces(F.simplices, pts, lms, ppe)
    pts_tie, arg_tie, n_simp = gr.tie_shares(faces)
    assert n_simp == sum(s.shape[0] for s in F.simplices) > 100
    assert pts_tie >= 0.25 and arg_tie >= 0.05, (pts_tie, arg_tie)
    gr.check_exact_witnesses(F, faces, pts, smallest_id=False)


def test_nearest_points_agrees_with_the_full_sets():
    pts = _integer_cloud(500, 3, 6, seed=1)
    q = _integer_cloud(64, 3, 12, seed=2) / 2 - 1.0
    dmin, first, count = gr.nearest_points(pts, q, chunk_bytes=1 << 16)
    sets = gr.nearest_sets(pts, q)
    assert int(count.max()) > 1
    for i, ids in enumerate(sets):
        assert int(first[i]) == int(ids.min()) and int(count[i]) == ids.numel()
        assert float(dmin[i]) == float(((pts[ids[0]].double() - q[i].double()) ** 2).sum())


def test_lattice_is_generate_grid():
    for ppe, d in [(2, 1), (3, 2), (5, 3), (9, 2), (17, 1)]:
        assert torch.equal(gr.lattice(ppe, d), fa.core.generate_grid(ppe, d, "cpu", torch.float64)[0])


def test_reference_gradient_equals_float64_autograd():
    """A tie-free float64 cloud: the closed form with the CPU path's witnesses against autograd through
    max-over-samples of min-over-points of the distance, every simplex of every dimension, points and landmarks."""
    ppe = 5   # (dyadic weights: core.generate_grid divides in float32, so only those are the same numbers in float64)
    g = torch.Generator().manual_seed(21)
    pts = torch.randn(500, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    lms = (0.8 * torch.randn(14, 3, generator=g, dtype=torch.float64)).requires_grad_(True)
    F = fa.flood_filtration(pts, lms, points_per_edge=ppe)
    coef = [torch.rand(s.shape[0], generator=g, dtype=torch.float64) - 0.3 for s in F.simplices]
    vals = []
    for d, simp in enumerate(F.simplices):
        W = gr.lattice(ppe, d)
        samples = W.unsqueeze(0) @ lms[simp.long()]
        dist = (samples.unsqueeze(2) - pts.reshape(1, 1, -1, 3)).norm(dim=3)      # (n, R, N), no matmul shortcut
        vals.append(dist.min(dim=2).values.max(dim=1).values)
        assert torch.allclose(vals[-1].detach(), F.values[d].detach(), rtol=1e-12, atol=1e-12)
    rp, rl = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, vals)), (pts, lms))
    gp, gl, info = gr.reference_gradient(F, pts, lms, coef)
    assert torch.allclose(gp, rp, rtol=1e-12, atol=1e-12) and torch.allclose(gl, rl, rtol=1e-12, atol=1e-12)
    assert rp.abs().sum() > 0 and rl.abs().sum() > 0
    # the bound is a float32 bound: positive on every row that receives something, zero elsewhere
    assert torch.equal(info["bound_points"] > 0, info["scale_points"] > 0)
    assert torch.equal(info["bound_landmarks"] > 0, info["scale_landmarks"] > 0)
