"""``flood_filtration(neighbors=k)`` on the MI355X: exact witnesses of the robust filtration on integer clouds (value
bits, witness sample, the k nearest points by (d2, id)), the values of ``flood_complex`` and float64 checks of the
witnesses on float clouds, gradients that repeat bit for bit and match the float64 closed form within a derived
float32 bound, and the device against the CPU path."""

import numpy as np
import pytest
import torch

import flooder_amd as fa

import grad_reference as gr
import knn_grad_reference as kr
from helpers import tolerances

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- exact inputs
def _integer_cloud(n, dim, hi, twice, seed):
    """n random integer points of [0, hi)^dim as float32; ``twice``: every point present twice, the copies anywhere."""
    g = torch.Generator().manual_seed(seed)
    if not twice:
        return torch.randint(0, hi, (n, dim), generator=g).to(torch.float32)
    base = torch.randint(0, hi, (n // 2, dim), generator=g).to(torch.float32)
    return torch.cat([base, base])[torch.randperm(2 * (n // 2), generator=g)]


# Exactness (grad_reference.assert_exact_inputs re-checks each; the unit is the lattice step): as twice3d, dense2d and
# twice5d of test_gpu_flood_grad.py - every d2 below 2^22 units.
# name, dim, points, hi, points_per_edge, landmarks, every point twice, max_dimension, (k, statistic) ...
EXACT_CASES = [
    ("twice3d", 3, 24_000, 256, 5, 40, True, None, ((3, "kth"), (5, "dtm"))),
    ("dense2d", 2, 40_000, 128, 9, 50, False, None, ((2, "dtm"), (8, "kth"))),
    ("twice5d", 5, 20_000, 64, 9, 40, True, 2, ((17, "dtm"),)),
]


@pytest.mark.parametrize("name,dim,n,hi,ppe,n_l,twice,max_dim,stats", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_knn_witnesses_on_integer_clouds(name, dim, n, hi, ppe, n_l, twice, max_dim, stats):
    """Integer clouds, dyadic lattice: float32 is exact and the brute force of knn_grad_reference.py is THE answer (the
    DTM sum replayed in float32).  Every simplex of every dimension: value bits, witness sample (the smallest row at
    the maximum), witness_neighbors (the k smallest by (d2, id), in order); nothing unfound; two runs agree."""
    pts = _integer_cloud(n, dim, hi, twice, seed=17)
    tp = pts.to(DEV)
    for k, stat in stats:
        runs = [fa.flood_filtration(tp, n_l, max_dimension=max_dim, points_per_edge=ppe, neighbors=k, neighbor_stat=stat)
                for _ in range(2)]
        F = runs[0]
        lms = tp[F.landmark_ids]
        gr.assert_exact_inputs(pts, lms.cpu(), ppe)
        # the reference alone first: the case has ties to decide
        faces = kr.exact_knn_faces(F.simplices, tp, lms, ppe, k, stat)
        share = kr.tie_share(faces)
        n_simp = sum(s.shape[0] for s in F.simplices)
        print(f"{name} k={k} {stat}: {n_simp} simplices, more than k points within the k-th distance on {share:.1%}")
        assert n_simp > 100
        if twice and k % 2 == 1:
            assert share >= 0.9
        assert F.faces_not_found == 0
        kr.check_exact_knn_witnesses(F, faces, tp)
        for d in range(len(F.simplices)):
            assert torch.equal(F.simplices[d], runs[1].simplices[d])
            assert torch.equal(F.values[d], runs[1].values[d])
            assert torch.equal(F.witness_neighbors[d], runs[1].witness_neighbors[d])
            assert torch.equal(F.witness_point[d], runs[1].witness_point[d])
            assert torch.equal(F.witness_weights[d], runs[1].witness_weights[d])


# ---------------------------------------------------------------------------------------------- float clouds
def _cloud(kind, n):
    torch.manual_seed(42)
    if kind == "eight2d":
        return fa.generate_figure_eight_points_2d(n, noise_std=0.01, seed=42).to(torch.float32)
    if kind == "gauss3d":
        return torch.randn(n, 3)
    if kind == "gauss6d":
        return torch.randn(n, 6)
    raise ValueError(kind)


SIZES = {"eight2d": (20_000, 100, 12, None), "gauss3d": (50_000, 100, 8, None), "gauss6d": (30_000, 60, 6, 2)}
FLOAT_CASES = [("eight2d", 2, "dtm"), ("eight2d", 32, "kth"), ("gauss3d", 8, "dtm"), ("gauss3d", 2, "kth"),
               ("gauss6d", 32, "dtm"), ("gauss6d", 8, "kth")]
LANDMARK_TENSOR = ("gauss3d", "gauss6d")    # the cases that pass the landmarks as a tensor requiring grad


def _check_witnesses(F, tp, lms, n_check=500, seed=0):
    """float64, 500 random simplices per dimension: every reported neighbour is within the gate of being at most as far
    as the true k-th nearest point (brute force over the cloud), and the statistic of the reported ids is the value."""
    pts64, lms64 = tp.double(), lms.double()
    rtol, atol = tolerances(tp.cpu().numpy())
    g = torch.Generator().manual_seed(seed)
    k = F.neighbors
    for d, simp in enumerate(F.simplices):
        n = simp.shape[0]
        if n == 0:
            continue
        nb = F.witness_neighbors[d]
        assert nb.shape == (n, k) and bool((nb >= 0).all()) and torch.equal(nb[:, -1], F.witness_point[d])
        pick = torch.randperm(n, generator=g)[:n_check].to(DEV)
        w = F.witness_weights[d][pick].double()
        assert torch.all(w >= 0)
        p = (w.unsqueeze(2) * lms64[simp.to(DEV)[pick]]).sum(1)
        dist = (p.unsqueeze(1) - pts64[nb[pick]]).norm(dim=2)                       # (m, k)
        true_k = torch.cat([torch.topk(torch.cdist(p[i:i + 128], pts64), k, dim=1, largest=False).values[:, -1]
                            for i in range(0, p.shape[0], 128)])
        v = F.values[d].detach()[pick].double()
        tol = atol + rtol * v.abs()
        assert torch.all(dist.max(dim=1).values - true_k <= tol), d
        assert bool((nb[pick].sort(dim=1).values.diff(dim=1) > 0).all()), d            # k different points
        stat = dist[:, -1] if F.neighbor_stat == "kth" else dist.pow(2).mean(dim=1).sqrt()
        assert torch.all((stat - v).abs() <= tol), d


# The 1 % cap of the gradient check rests on how small a positive value gets against the coordinates.  CPU path, these
# clouds at these sizes, values of dimension >= 1, c = largest |coordinate| (profiles/knn_grad_tests.txt):
#   eight2d 20 k / 100 / 12: 455 values, no zeros, smallest f / c 2.20e-3 (k = 2, dtm), 9.83e-3 (k = 32, kth)
#   gauss3d 50 k / 100 / 8: 2073 values, no zeros, smallest f / c 1.85e-2 (k = 8, dtm), 1.46e-2 (k = 2, kth)
#   gauss6d 30 k / 60 / 6, max_dimension 2: 8153 values, no zeros, smallest f / c 2.05e-1 (k = 32, dtm), 1.86e-1 (k = 8, kth)
# and the bound exceeds 1 % of the row's scale on 0.16 % of the rows of the first case, on none elsewhere.
def gradient_check(F, tp, tl, coef, loss, what):
    """Rows of the points' (and landmarks') gradient against knn_grad_reference.reference_gradient_knn."""
    lms = tl.detach() if tl is not None else tp.detach()[F.landmark_ids]
    rp, rl, info = kr.reference_gradient_knn(F, tp.detach(), lms, coef)
    if tl is not None:
        gp, gl = torch.autograd.grad(loss, (tp, tl))
        rows = [("points", gp, rp, info["bound_points"], info["scale_points"]),
                ("landmarks", gl, rl, info["bound_landmarks"], info["scale_landmarks"])]
    else:
        (gp,) = torch.autograd.grad(loss, tp)
        rows = [("points", gp) + gr.fold_landmarks(rp, rl, info, F.landmark_ids)]
    for name, got, ref, bound, scale in rows:
        assert got.dtype == tp.dtype and torch.isfinite(got).all()
        err = (got.double() - ref).abs().max(dim=1).values
        hit = scale > 0
        assert int(hit.sum()) > 0.5 * min(lms.shape[0], got.shape[0])
        over = float((bound[hit] > 0.01 * scale[hit]).double().mean())
        ratio = float((err[hit] / bound[hit]).max())
        print(f"{what} {name}: {int(hit.sum())} rows, worst error / bound {ratio:.3f}, "
              f"bound above 1 % of the row's scale on {over:.3%} of the rows")
        assert over < 0.01, name
        assert not got[~hit].any(), name            # a row nothing points at stays exactly zero
        assert torch.all(err <= bound), (name, ratio)
    return gp


def _coefficients(F, dev):
    gen = torch.Generator().manual_seed(7)
    return [((torch.rand(v.shape[0], generator=gen) + 0.5) * (2 * torch.randint(0, 2, (v.shape[0],), generator=gen) - 1)
             ).to(dev) for v in F.values]


def run_float_case(kind, k, stat, dev):
    n, n_l, ppe, max_dim = SIZES[kind]
    tp = _cloud(kind, n).to(dev).requires_grad_(True)
    kw = dict(max_dimension=max_dim, points_per_edge=ppe, neighbors=k, neighbor_stat=stat)
    if kind in LANDMARK_TENSOR:
        tl = tp.detach()[fa.core.fps_indices(tp.detach(), n_l, 0)].clone().requires_grad_(True)
        arg = tl
    else:
        tl, arg = None, n_l
    F = fa.flood_filtration(tp, arg, **kw)
    coef = _coefficients(F, dev)
    g1 = gradient_check(F, tp, tl, coef, sum((c * v).sum() for c, v in zip(coef, F.values)), f"{kind} k={k} {stat}")
    return tp, tl, arg, kw, F, coef, g1


@pytest.mark.parametrize("kind,k,stat", FLOAT_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in FLOAT_CASES])
def test_values_witnesses_and_gradients_on_float_clouds(kind, k, stat):
    tp, tl, arg, kw, F, coef, g1 = run_float_case(kind, k, stat, DEV)
    assert F.faces_not_found == 0
    assert F.to_dict() == fa.flood_complex(tp.detach(), arg if tl is None else tl.detach(), **kw)
    _check_witnesses(F, tp.detach(), tl.detach() if tl is not None else tp.detach()[F.landmark_ids])
    # forward and backward twice: bit-identical witnesses and gradient
    F2 = fa.flood_filtration(tp, arg, **kw)
    (g2,) = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, F2.values)), tp)
    for d in range(len(F.simplices)):
        assert torch.equal(F.values[d], F2.values[d])
        assert torch.equal(F.witness_neighbors[d], F2.witness_neighbors[d])
        assert torch.equal(F.witness_weights[d], F2.witness_weights[d])
    assert torch.equal(g1, g2)
    assert g1.abs().sum() > 0


def test_gradients_match_cpu_path_dtm():
    """The construction of test_gradients_match_cpu_path for (k = 8, dtm): the device witnesses give the gradient the
    host path gives on the simplices whose witnesses agree - the same sample, the same SET of neighbours - which are at
    least 95 %."""
    pts = _cloud("eight2d", 20_000)
    lms = pts[fa.core.fps_indices(pts, 60, 0)].clone()
    kw = dict(points_per_edge=12, neighbors=8, neighbor_stat="dtm")
    Fc = fa.flood_filtration(pts.requires_grad_(True), lms.requires_grad_(True), **kw)
    tp = pts.detach().to(DEV).requires_grad_(True)
    tl = lms.detach().to(DEV).requires_grad_(True)
    Fg = fa.flood_filtration(tp, tl, **kw)
    same, total = [], 0
    for d in range(3):
        assert torch.allclose(Fg.values[d].detach().cpu(), Fc.values[d].detach(), rtol=1e-5, atol=1e-7)
        same.append((Fg.witness_neighbors[d].cpu().sort(dim=1).values == Fc.witness_neighbors[d].sort(dim=1).values).all(dim=1)
                    & (Fg.witness_weights[d].cpu() == Fc.witness_weights[d]).all(dim=1))
        total += same[-1].numel()
    assert sum(int(s.sum()) for s in same) >= 0.95 * total
    loss_c = sum((s.float() * v).sum() for s, v in zip(same, Fc.values))
    loss_g = sum((s.float().to(DEV) * v).sum() for s, v in zip(same, Fg.values))
    gpc, glc = torch.autograd.grad(loss_c, (pts, lms))
    gpg, glg = torch.autograd.grad(loss_g, (tp, tl))
    assert torch.allclose(gpg.cpu(), gpc, rtol=1e-4, atol=1e-4)
    assert torch.allclose(glg.cpu(), glc, rtol=1e-4, atol=1e-4)


def test_refused_on_device():
    tp = torch.randn(1000, 3, device=DEV)
    with pytest.raises(ValueError, match="nearest point only"):
        fa.flood_filtration(tp, 20, neighbors=2, method="cell")
    with pytest.raises(ValueError, match="float32"):
        fa.flood_filtration(tp.double(), 20, neighbors=2)
    with pytest.raises(TypeError):
        fa.flood_filtration(tp.double(), 20, neighbors=1, neighbor_stat="dtm")
