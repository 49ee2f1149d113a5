"""flood_filtration on the MI355X: values bit-equal to flood_complex, exact witnesses (csrc/flood_grad.hip), gradients
that repeat bit for bit."""

import itertools

import numpy as np
import pytest
import torch

import flooder_amd as fa

from flooder_amd import core

import grad_reference as gr
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


def _check_witnesses(F, tp, n_check=2000, seed=0, lms=None):
    """float64: |p* - x*| equals the value within the gate, and no point is closer to p* (brute force over the cloud)."""
    pts64 = tp.double()
    lms64 = (tp[F.landmark_ids] if lms is None else lms).double()
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


# ---------------------------------------------------------------------------------------------- exact tie rules
def _integer_cloud(n, dim, hi, twice, seed):
    """n random integer points of [0, hi)^dim as float32; ``twice``: every point present twice, the copies anywhere."""
    g = torch.Generator().manual_seed(seed)
    if not twice:
        return torch.randint(0, hi, (n, dim), generator=g).to(torch.float32)
    base = torch.randint(0, hi, (n // 2, dim), generator=g).to(torch.float32)
    return torch.cat([base, base])[torch.randperm(2 * (n // 2), generator=g)]


def _integer_landmarks(pts, n_l, hi, seed):
    """n_l distinct integer positions of the box, none of them a point of the cloud."""
    g = torch.Generator().manual_seed(seed)
    taken = {tuple(r) for r in pts.to(torch.int64).tolist()}
    rows = []
    for r in torch.randint(0, hi, (50 * n_l, pts.shape[1]), generator=g).tolist():
        if tuple(r) not in taken:
            taken.add(tuple(r))
            rows.append(r)
    assert len(rows) >= n_l
    return torch.tensor(rows[:n_l], dtype=torch.float32)


# Exactness (grad_reference.assert_exact_inputs re-checks each): the unit is the lattice step 1/(points_per_edge - 1).
#   dense2d  [0, 128)^2, eighths:  differences < 2^10 units, squares < 2^20, two axes   < 2^21
#   dense3d  [0, 32)^3,  quarters: differences < 2^7,        squares < 2^14, three axes < 2^16
#   tensor3d [0, 64)^3,  eighths:  differences < 2^9,        squares < 2^18, three axes < 2^20
#   twice3d  [0, 256)^3, quarters: differences < 2^10,       squares < 2^20, three axes < 2^22
#   twice5d  [0, 64)^5,  eighths:  differences < 2^9,        squares < 2^18, five axes  < 2^21
# name, dim, points, hi, points_per_edge, landmarks, landmarks as an integer tensor off the cloud, every point twice,
# max_dimension, methods, dense (more than one sample at the maximum on at least 5 % of the simplices)
EXACT_CASES = [
    ("dense2d", 2, 40_000, 128, 9, 50, False, False, None, ("cell", "bvh"), True),
    ("dense3d", 3, 20_000, 32, 5, 40, False, False, None, ("cell", "bvh"), True),
    ("tensor3d", 3, 50_000, 64, 9, 40, True, False, None, ("cell", "bvh"), False),
    ("twice3d", 3, 24_000, 256, 5, 40, False, True, None, ("cell", "bvh"), False),
    ("twice5d", 5, 20_000, 64, 9, 40, False, True, 2, ("bvh",), False),
]


@pytest.mark.parametrize("name,dim,n,hi,ppe,n_l,off_cloud,twice,max_dim,methods,dense", EXACT_CASES,
                         ids=[c[0] for c in EXACT_CASES])
def test_exact_witnesses_on_integer_clouds(name, dim, n, hi, ppe, n_l, off_cloud, twice, max_dim, methods, dense):
    """Integer clouds, dyadic lattice: float32 is exact and the float64 brute force of grad_reference.py is THE answer.
    Every simplex of every dimension: value bits, witness sample (smallest row at the maximum), witness point (smallest
    id among the nearest points of that sample); "cell" == "bvh"; two runs agree."""
    pts = _integer_cloud(n, dim, hi, twice, seed=17)
    tp = pts.to(DEV)
    arg = _integer_landmarks(pts, n_l, hi, seed=18).to(DEV) if off_cloud else n_l
    runs = [fa.flood_filtration(tp, arg, max_dimension=max_dim, points_per_edge=ppe, method=m)
            for m in methods + methods[:1]]
    F = runs[0]
    lms = arg if off_cloud else tp[F.landmark_ids]
    bound = gr.assert_exact_inputs(pts, lms.cpu(), ppe)
    # the reference alone first: the case has ties to decide
    faces = gr.reference_faces(F.simplices, tp, lms, ppe)
    pts_tie, arg_tie, n_simp = gr.tie_shares(faces)
    print(f"{name}: {n_simp} simplices, largest d2 {bound} units, more than one nearest point on {pts_tie:.1%}, "
          f"more than one sample at the maximum on {arg_tie:.1%}")
    assert n_simp == sum(s.shape[0] for s in F.simplices) and n_simp > 100
    assert pts_tie >= 0.25
    assert not dense or arg_tie >= 0.05
    assert F.faces_not_found == 0
    gr.check_exact_witnesses(F, faces, tp, smallest_id=True)
    for other in runs[1:]:
        for d in range(len(F.simplices)):
            assert torch.equal(F.simplices[d], other.simplices[d])
            assert torch.equal(F.values[d], other.values[d])
            assert torch.equal(F.witness_point[d], other.witness_point[d])
            assert torch.equal(F.witness_weights[d], other.witness_weights[d])


@pytest.mark.parametrize("method", ["cell", "bvh"])
def test_points_per_edge_two_is_all_zeros(method):
    """Only the vertices are sampled and the landmarks are cloud points: every value is 0, every witness a point at
    distance 0 - the smallest id among the copies of a doubled cloud -, the gradient exactly zero."""
    pts = _integer_cloud(20_000, 3, 256, True, seed=19)
    tp = pts.to(DEV).requires_grad_(True)
    F = fa.flood_filtration(tp, 40, points_per_edge=2, method=method)
    lms = tp.detach()[F.landmark_ids]
    gr.assert_exact_inputs(pts, lms.cpu(), 2)
    faces = gr.reference_faces(F.simplices, tp.detach(), lms, 2)
    assert all(float(E.dmax.max()) == 0.0 for E in faces)
    gr.check_exact_witnesses(F, faces, tp.detach(), smallest_id=True)
    for d, v in enumerate(F.values):
        assert v.shape[0] > 0 and not v.detach().any(), d
        assert (F.witness_point[d] >= 0).all()
        # the smallest id of the landmark's position: never the later copy
        assert (F.witness_point[d] <= F.landmark_ids.to(DEV)[F.simplices[d].to(DEV)].max(dim=1).values).all()
    (g,) = torch.autograd.grad(sum((torch.linspace(0.5, 1.5, v.shape[0], device=DEV) * v).sum() for v in F.values), tp)
    assert not g.any()


# ---------------------------------------------------------------------------------------------- gradients, float64
# The 1 % cap below rests on how small a positive value gets against the coordinates.  CPU path, the clouds of CASES
# at the same sizes, dimensions >= 1, c = largest |coordinate|:
#   eight2d 50 k / 300 / 30: 1441 values, no zeros, smallest f / c 1.27e-3, none below 1e-3
#   gauss3d 200 k / 400 / 20: 9515 values, no zeros, smallest f / c 7.5e-3
#   torus3d 300 k / 500 / 16: 12 147 values, no zeros, smallest f / c 4.5e-3
#   cheese3d 100 k / 300 / 16: 7251 values, no zeros, smallest f / c 1.13e-2
#   gauss6d 100 k / 150 / 8, max_dimension 2: 36 544 values, no zeros, smallest f / c 6.7e-2
# so one contribution's bound relative to |g| is at most 2 (2 sqrt(2) 5 2^-24 / 1.27e-3 + 5 2^-24) = 1.4e-3 on the
# worst cloud, seven times inside the line.
LANDMARK_TENSOR = ("gauss3d", "gauss6d")    # the cases that pass the landmarks as a tensor requiring grad


@pytest.mark.parametrize("kind,n,n_l,ppe,max_dim,method", CASES, ids=[c[0] for c in CASES])
def test_gradients_match_float64_closed_form(kind, n, n_l, ppe, max_dim, method):
    """Points' and landmarks' gradient of a random linear functional of ALL values against the float64 closed form
    (grad_reference.reference_gradient: float32 inputs, the device's witnesses - checked on their own above), every row
    within the derived float32 bound of that row; the bound itself stays below 1 % of the row's sum |g| |w| on all but
    1 % of the rows, so it cannot hide a dropped or misplaced contribution."""
    tp = _cloud(kind, n).to(DEV).requires_grad_(True)
    if kind in LANDMARK_TENSOR:
        tl = fa.generate_landmarks(tp.detach(), n_l, start_idx=0).detach().clone().requires_grad_(True)
        F = fa.flood_filtration(tp, tl, max_dimension=max_dim, points_per_edge=ppe, method=method)
    else:
        tl = None
        F = fa.flood_filtration(tp, n_l, max_dimension=max_dim, points_per_edge=ppe, method=method)
    gen = torch.Generator().manual_seed(7)
    coef = [((torch.rand(v.shape[0], generator=gen) + 0.5) * (2 * torch.randint(0, 2, (v.shape[0],), generator=gen) - 1)
             ).to(DEV) for v in F.values]
    loss = sum((c * v).sum() for c, v in zip(coef, F.values))
    lms = tl.detach() if tl is not None else tp.detach()[F.landmark_ids]
    rp, rl, info = gr.reference_gradient(F, tp.detach(), lms, coef)
    if tl is not None:
        gp, gl = torch.autograd.grad(loss, (tp, tl))
        rows = [("points", gp, rp, info["bound_points"], info["scale_points"]),
                ("landmarks", gl, rl, info["bound_landmarks"], info["scale_landmarks"])]
    else:
        (gp,) = torch.autograd.grad(loss, tp)
        rows = [("points", gp) + gr.fold_landmarks(rp, rl, info, F.landmark_ids)]
    for what, got, ref, bound, scale in rows:
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        err = (got.double() - ref).abs().max(dim=1).values
        hit = scale > 0
        assert int(hit.sum()) > 0.5 * min(n_l, got.shape[0])
        over = float((bound[hit] > 0.01 * scale[hit]).double().mean())
        ratio = float((err[hit] / bound[hit]).max())
        print(f"{kind} {what}: {int(hit.sum())} rows, worst error / bound {ratio:.3f}, "
              f"bound above 1 % of the row's scale on {over:.3%} of the rows")
        assert over < 0.01, what
        assert not got[~hit].any(), what            # a row nothing points at stays exactly zero
        assert torch.all(err <= bound), (what, ratio)


# ---------------------------------------------------------------------------------------------- small shapes
def _outcome(fn):
    try:
        return "ok", fn()
    except Exception as exc:   # noqa: BLE001  (the TYPE is what is compared)
        return "raise", type(exc)


def _small_cloud(n, dim, seed):
    return torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))


SMALL = [  # name, points, dim, landmarks (the first rows of the cloud), keywords, must give a result
    ("one_point", 1, 2, 1, dict(points_per_edge=5), False),
    ("one_triangle", 3, 2, 3, dict(points_per_edge=5), True),
    ("one_tetrahedron", 4, 3, 4, dict(points_per_edge=5), True),
    ("seventeen_points", 17, 2, 6, dict(points_per_edge=5), True),
    ("num_rand_every_dimension", 2000, 3, 12, dict(num_rand=8, max_dimension=1), True),
    ("two_landmarks_3d", 1000, 3, 2, dict(points_per_edge=5), False),
    ("three_landmarks_3d", 1000, 3, 3, dict(points_per_edge=5), False),
]


@pytest.mark.parametrize("name,n,dim,n_l,kw,must", SMALL, ids=[c[0] for c in SMALL])
def test_small_shapes(name, n, dim, n_l, kw, must):
    """Small inputs through flood_filtration on the device: what flood_complex does with them (a result or an exception
    type), and a result equals the CPU path's values and has valid witnesses (fewer landmarks than dim + 1: no cell,
    every value NaN on both paths, no witness)."""
    pts = _small_cloud(n, dim, seed=n + dim)
    lms = pts[:n_l].clone()
    tp, tl = pts.to(DEV), lms.to(DEV)
    torch.manual_seed(3)
    how_c, fc = _outcome(lambda: fa.flood_complex(tp, tl, **kw))
    torch.manual_seed(3)
    how_f, F = _outcome(lambda: fa.flood_filtration(tp, tl, **kw))
    assert how_f == how_c, (F, fc)
    if how_c == "raise":
        assert not must and F is fc, (F, fc)
        return
    # (without a top cell nothing is swept and flood_complex leaves NaN: NaN must meet NaN, simplex by simplex)
    got = F.to_dict()
    assert got.keys() == fc.keys() and F.faces_not_found == 0
    assert all(got[k] == fc[k] or (np.isnan(got[k]) and np.isnan(fc[k])) for k in fc), (got, fc)
    torch.manual_seed(3)
    Fc = fa.flood_filtration(pts, lms, **kw)
    rtol, atol = tolerances(pts.numpy())
    assert len(F.simplices) == len(Fc.simplices)
    finite = True
    for d in range(len(F.simplices)):
        assert torch.equal(F.simplices[d], Fc.simplices[d])
        assert torch.allclose(F.values[d].detach().cpu(), Fc.values[d].detach(), rtol=rtol, atol=atol, equal_nan=True), d
        nan = torch.isnan(F.values[d].detach())
        assert torch.equal(F.witness_point[d] < 0, nan), d        # no value, no witness - and only then
        finite = finite and not bool(nan.any())
    assert finite or not must
    if finite:
        _check_witnesses(F, tp, lms=tl)
