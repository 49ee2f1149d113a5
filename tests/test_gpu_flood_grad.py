"""flood_filtration on the MI355X: values bit-equal to flood_complex, exact witnesses (csrc/flood_grad.hip), gradients
that repeat bit for bit."""

import itertools

import numpy as np
import pytest
import torch

import flooder_amd as fa

from flooder_amd import core

from helpers import tolerances

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _cloud(kind, n):
    torch.manual_seed(42)
    if kind == "eight2d":
        return fa.generate_figure_eight_points_2d(n, noise_std=0.01, seed=42).to(torch.float32)
    if kind == "gauss3d":
        return torch.randn(n, 3)
    if kind == "torus3d":
        return fa.generate_noisy_torus_points_3d(n, seed=42).to(torch.float32)
    if kind == "cheese3d":
        return fa.generate_swiss_cheese_points(n, k=6, seed=42)[0].to(torch.float32)
    if kind == "gauss6d":
        return torch.randn(n, 6)
    raise ValueError(kind)


CASES = [  # kind, points, landmarks, points_per_edge, max_dimension, method
    ("eight2d", 50_000, 300, 30, None, None),
    ("gauss3d", 200_000, 400, 20, None, None),
    ("torus3d", 300_000, 500, 16, None, None),
    ("cheese3d", 100_000, 300, 16, None, None),
    ("gauss6d", 100_000, 150, 8, 2, "bvh"),
]


def _nearest64(p, pts64, chunk=256):
    out = []
    for i in range(0, p.shape[0], chunk):
        out.append(torch.cdist(p[i:i + chunk], pts64).min(dim=1).values)
    return torch.cat(out)


def _check_witnesses(F, tp, n_check=2000, seed=0):
    """float64: |p* - x*| equals the value within the gate, and no point is closer to p* (brute force over the cloud)."""
    pts64 = tp.double()
    lms64 = tp[F.landmark_ids].double()
    rtol, atol = tolerances(tp.cpu().numpy())
    g = torch.Generator().manual_seed(seed)
    for d, simp in enumerate(F.simplices):
        n = simp.shape[0]
        if n == 0:
            continue
        assert (F.witness_point[d] >= 0).all()
        pick = torch.randperm(n, generator=g)[:n_check].to(DEV)
        w = F.witness_weights[d][pick].double()
        assert torch.all(w >= 0)
        p = (w.unsqueeze(2) * lms64[simp.to(DEV)[pick]]).sum(1)
        wv = (p - pts64[F.witness_point[d][pick]]).norm(dim=1)
        v = F.values[d].detach()[pick].double()
        tol = atol + rtol * v.abs()
        assert torch.all((wv - v).abs() <= tol), d
        assert torch.all(wv - _nearest64(p, pts64) <= tol), d


@pytest.mark.parametrize("kind,n,n_l,ppe,max_dim,method", CASES, ids=[c[0] for c in CASES])
def test_values_witnesses_and_repeatable_gradients(kind, n, n_l, ppe, max_dim, method):
    tp = _cloud(kind, n).to(DEV).requires_grad_(True)
    F = fa.flood_filtration(tp, n_l, max_dimension=max_dim, points_per_edge=ppe, method=method)
    assert F.faces_not_found == 0
    fc = fa.flood_complex(tp.detach(), n_l, max_dimension=max_dim, points_per_edge=ppe)   # the default method
    assert F.to_dict() == fc
    for d, simp in enumerate(F.simplices):
        want = torch.tensor([fc[tuple(r)] for r in simp.tolist()], dtype=torch.float32)
        assert torch.equal(F.values[d].detach().cpu(), want), d
    _check_witnesses(F, tp.detach())
    # forward and backward twice: bit-identical witnesses and gradients
    coef = [torch.linspace(0.5, 1.5, v.shape[0], device=DEV) for v in F.values]
    (g1,) = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, F.values)), tp)
    F2 = fa.flood_filtration(tp, n_l, max_dimension=max_dim, points_per_edge=ppe, method=method)
    (g2,) = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, F2.values)), tp)
    for d in range(len(F.simplices)):
        assert torch.equal(F.witness_point[d], F2.witness_point[d])
        assert torch.equal(F.witness_weights[d], F2.witness_weights[d])
    assert torch.equal(g1, g2)
    assert torch.isfinite(g1).all() and g1.abs().sum() > 0


def test_gradients_match_cpu_path():
    """The device witnesses give the gradient the host path gives (float32 both, same cloud and landmarks) on the
    simplices whose witnesses agree - all but near-ties of two samples or two points (at least 95 %)."""
    pts = _cloud("eight2d", 20_000)
    lms = pts[fa.core.fps_indices(pts, 60, 0)].clone()
    Fc = fa.flood_filtration(pts.requires_grad_(True), lms.requires_grad_(True), points_per_edge=12)
    tp = pts.detach().to(DEV).requires_grad_(True)
    tl = lms.detach().to(DEV).requires_grad_(True)
    Fg = fa.flood_filtration(tp, tl, points_per_edge=12)
    same, total = [], 0
    for d in range(3):
        assert torch.allclose(Fg.values[d].detach().cpu(), Fc.values[d].detach(), rtol=1e-5, atol=1e-7)
        same.append((Fg.witness_point[d].cpu() == Fc.witness_point[d])
                    & (Fg.witness_weights[d].cpu() == Fc.witness_weights[d]).all(dim=1))
        total += same[-1].numel()
    assert sum(int(s.sum()) for s in same) >= 0.95 * total
    loss_c = sum((s.float() * v).sum() for s, v in zip(same, Fc.values))
    loss_g = sum((s.float().to(DEV) * v).sum() for s, v in zip(same, Fg.values))
    gpc, glc = torch.autograd.grad(loss_c, (pts, lms))
    gpg, glg = torch.autograd.grad(loss_g, (tp, tl))
    assert torch.allclose(gpg.cpu(), gpc, rtol=1e-4, atol=1e-4)
    assert torch.allclose(glg.cpu(), glc, rtol=1e-4, atol=1e-4)


def test_num_rand_values_equal_flood_complex():
    tp = _cloud("gauss3d", 100_000).to(DEV)
    torch.manual_seed(5)
    F = fa.flood_filtration(tp, 200, num_rand=64)
    torch.manual_seed(5)
    fc = fa.flood_complex(tp, 200, num_rand=64)
    assert F.to_dict() == fc
    assert F.faces_not_found == 0
    _check_witnesses(F, tp, n_check=500)


def test_diagrams_on_device():
    tp = _cloud("eight2d", 50_000).to(DEV).requires_grad_(True)
    F = fa.flood_filtration(tp, 200, points_per_edge=20)
    dg = F.diagrams()
    F.tree.compute_persistence()
    for d in (0, 1):
        assert np.array_equal(dg[d].detach().cpu().numpy(), F.tree.persistence_intervals_in_dimension(d))
    h1 = dg[1]
    (g,) = torch.autograd.grad((h1[:, 1] - h1[:, 0]).sum(), tp)
    assert torch.isfinite(g).all() and g.abs().sum() > 0


def test_refused_on_device():
    tp = torch.randn(1000, 3, device=DEV)
    with pytest.raises(TypeError):
        fa.flood_filtration(tp.double(), 20)
    with pytest.raises(ValueError):
        fa.flood_filtration(tp, 20, method="ball")
    with pytest.raises(ValueError):
        fa.flood_filtration(torch.randn(1000, 6, device=DEV), 20, method="cell")


def test_cfg2_size_witnesses_are_nearest_neighbours():
    """1 M Gaussian points, 1 k landmarks, points_per_edge 30: the values of flood_complex, and for 2000 random simplices
    of each dimension the witness point is a float64 brute-force nearest neighbour of p* over all points."""
    torch.manual_seed(42)
    tp = torch.randn(1_000_000, 3).to(DEV)
    lms, index = fa.generate_landmarks(tp, 1000, start_idx=0, return_index=True)
    F = fa.flood_filtration(tp, lms, points_per_edge=30, index=index)
    assert F.faces_not_found == 0
    fc = fa.flood_complex(tp, lms, points_per_edge=30, index=index)
    assert F.to_dict() == fc
    pts64 = tp.double()
    rtol, atol = tolerances(tp.cpu().numpy())
    g = torch.Generator().manual_seed(1)
    for d, simp in enumerate(F.simplices):
        pick = torch.randperm(simp.shape[0], generator=g)[:2000].to(DEV)
        p = (F.witness_weights[d][pick].double().unsqueeze(2) * lms.double()[simp.to(DEV)[pick]]).sum(1)
        wv = (p - pts64[F.witness_point[d][pick]]).norm(dim=1)
        v = F.values[d].detach()[pick].double()
        tol = atol + rtol * v.abs()
        assert torch.all((wv - v).abs() <= tol), d
        assert torch.all(wv - _nearest64(p, pts64, chunk=64) <= tol), d
    _check_argmax_bits(F, index, lms, 30, n_cells=2000)


def _check_argmax_bits(F, index, lms, ppe, n_cells):
    """Bit-exact argmax: for n_cells random top cells, the (S, R) minimum d2 bits of the unfused sweep (captured with a
    reduce_hook); the witness sample of each of their faces is a sample row of that face whose d2 is the face maximum."""
    tree = F.tree
    top = tree._cells.shape[1] - 1
    cells = tree._cells[np.random.default_rng(0).permutation(tree._cells.shape[0])[:n_cells]]
    weights, _, _, faces, plan, v_idx_np = core._grid_tables(ppe, top, DEV, torch.float32)
    sv = lms.to(torch.float32)[torch.as_tensor(cells, device=DEV)].contiguous()
    got = []
    core._sweep_dimension_cell(index, sv, weights, faces, got.append, plan=plan)
    d2 = got[0].cpu().numpy().view(np.uint32)                 # (n_cells, R), columns in the swept (w_perm) order
    w_perm = plan.w_perm.cpu().numpy()
    col_of = {w_perm[c].tobytes(): c for c in range(w_perm.shape[0])}
    ptr, rows = faces.ptr.cpu().numpy(), plan.rows_perm.cpu().numpy()
    cell_row = {tuple(c): i for i, c in enumerate(tree._cells.tolist())}
    f = 0
    for v_idx in v_idx_np:
        nf, k = v_idx.shape
        index_k = tree.cell_face_index(k - 1)
        combos = list(itertools.combinations(range(top + 1), k))
        ww = F.witness_weights[k - 1].cpu().numpy()
        for pos in v_idx:
            j = combos.index(tuple(int(x) for x in pos))
            face_rows = index_k[[cell_row[tuple(c)] for c in cells.tolist()], j]
            emb = np.zeros((cells.shape[0], top + 1), dtype=np.float32)
            emb[:, pos] = ww[face_rows]
            cols = np.array([col_of[e.tobytes()] for e in emb])
            fmax = d2[:, rows[ptr[f]:ptr[f + 1]]].max(axis=1)
            assert np.array_equal(d2[np.arange(cells.shape[0]), cols], fmax), (k, j)
            assert np.all(np.isin(cols, rows[ptr[f]:ptr[f + 1]])), (k, j)
            f += 1
