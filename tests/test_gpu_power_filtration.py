"""power_filtration, power_nearest and the differentiable power_distance on the MI355X: values bit-equal to
flood_complex(point_weights=w), exact witnesses (flooder_witness_power) against a float64 brute force, gradients
against the float64 closed form within a derived float32 bound, runs that repeat bit for bit."""

import math

import numpy as np
import pytest
import torch

import flooder_amd as fa

import grad_reference as gr
import power_grad_reference as pgr
import power_reference as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- exact tie rules
def _integer_cloud(n, dim, hi, twice, seed):
    """n random integer points of [0, hi)^dim as float32 with integer weights 0..3; ``twice``: every point present
    twice, the copies anywhere in the cloud and of the SAME weight."""
    g = torch.Generator().manual_seed(seed)
    m = n // 2 if twice else n
    pts = torch.randint(0, hi, (m, dim), generator=g).to(torch.float32)
    w = torch.randint(0, 4, (m,), generator=g).to(torch.float32)
    if not twice:
        return pts, w
    perm = torch.randperm(2 * m, generator=g)
    return torch.cat([pts, pts])[perm], torch.cat([w, w])[perm]


# The constructions of test_gpu_flood_grad.EXACT_CASES (the unit is the lattice step 1 / (points_per_edge - 1)); the
# weights add at most (3 * 8)^2 = 576 units to its bounds, assert_exact_power_inputs re-checks each.
# name, dim, points, hi, points_per_edge, landmarks, every point twice, max_dimension
EXACT_CASES = [
    ("dense2d", 2, 40_000, 128, 9, 50, False, None),
    ("twice3d", 3, 24_000, 256, 5, 40, True, None),
    ("twice5d", 5, 20_000, 64, 9, 40, True, 2),
]


@pytest.mark.parametrize("name,dim,n,hi,ppe,n_l,twice,max_dim", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_witnesses_on_integer_clouds(name, dim, n, hi, ppe, n_l, twice, max_dim):
    """Integer clouds, integer weights, dyadic lattice: float32 is exact and the float64 brute force is THE answer.
    Every simplex of every dimension: value bits, witness sample (smallest row at the maximum), witness point (smallest
    id at the power minimum of that sample); two runs agree in every tensor."""
    pts, w = _integer_cloud(n, dim, hi, twice, seed=17)
    tp, tw = pts.to(DEV), w.to(DEV)
    runs = [fa.power_filtration(tp, n_l, tw, max_dimension=max_dim, points_per_edge=ppe) for _ in range(2)]
    F = runs[0]
    lms = tp[F.landmark_ids]
    bound = pgr.assert_exact_power_inputs(pts, lms.cpu(), w, ppe)
    faces = pgr.reference_power_faces(F.simplices, tp, tw, lms, ppe)
    pts_tie, arg_tie, n_simp = gr.tie_shares(faces)
    print(f"{name}: {n_simp} simplices, largest word {bound} units, more than one point at the power minimum on "
          f"{pts_tie:.1%}, more than one sample at the maximum on {arg_tie:.1%}")
    assert n_simp == sum(s.shape[0] for s in F.simplices) and n_simp > 100
    assert not twice or pts_tie >= 0.25
    assert F.faces_not_found == 0
    assert F.point_weights is tw
    pgr.check_exact_power_witnesses(F, faces, tp, tw)
    other = runs[1]
    for d in range(len(F.simplices)):
        assert torch.equal(F.simplices[d], other.simplices[d])
        assert torch.equal(F.values[d], other.values[d])
        assert torch.equal(F.witness_point[d], other.witness_point[d])
        assert torch.equal(F.witness_weights[d], other.witness_weights[d])
        assert torch.equal(F.witness_neighbors[d], F.witness_point[d].unsqueeze(1))


# ---------------------------------------------------------------------------------------------- generic clouds
GENERIC = [(2, None), (3, None), (6, 2)]       # dimension, max_dimension: 5000 points, 30 landmarks, 6 points per edge


def _generic(dim, seed=0):
    g = torch.Generator().manual_seed(seed + dim)
    pts = torch.randn(5000, dim, generator=g)
    w = (torch.rand(5000, generator=g) - 0.5) * 4.0 * pr.median_nn_distance(pts.numpy())   # signed, the spacing's scale
    return pts.to(DEV), w.to(torch.float32).to(DEV)


@pytest.mark.parametrize("dim,max_dim", GENERIC)
def test_values_equal_flood_complex(dim, max_dim):
    tp, tw = _generic(dim)
    F = fa.power_filtration(tp, 30, tw, max_dimension=max_dim, points_per_edge=6)
    fc = fa.flood_complex(tp, 30, max_dimension=max_dim, points_per_edge=6, point_weights=tw)
    assert F.to_dict() == fc and F.faces_not_found == 0
    for d, simp in enumerate(F.simplices):
        want = torch.tensor([fc[tuple(r)] for r in simp.tolist()], dtype=torch.float32)
        assert torch.equal(F.values[d].detach().cpu(), want), d
        assert (F.witness_point[d] >= 0).all()
    # the vertex witnesses are the power-nearest points of the landmarks, their values the power distances
    ids, dist = fa.power_nearest(tp, tw, tp[F.landmark_ids])
    own = F.tree.filtrations_of_dimension(0)
    assert torch.equal(F.witness_point[0], ids)
    assert np.array_equal(dist.cpu().numpy().astype(np.float64), own)


@pytest.mark.parametrize("dim,max_dim", GENERIC)
def test_zero_weights_are_flood_filtration(dim, max_dim):
    tp, _ = _generic(dim)
    a = tp.clone().requires_grad_(True)
    b = tp.clone().requires_grad_(True)
    zero = torch.zeros(tp.shape[0], device=DEV, requires_grad=True)
    Fp = fa.power_filtration(a, 30, zero, max_dimension=max_dim, points_per_edge=6)
    Ff = fa.flood_filtration(b, 30, max_dimension=max_dim, points_per_edge=6, method="bvh")
    coef = [torch.linspace(0.5, 1.5, v.shape[0], device=DEV) for v in Ff.values]
    for d in range(len(Ff.simplices)):
        assert torch.equal(Fp.values[d], Ff.values[d]), d
        assert torch.equal(Fp.witness_point[d], Ff.witness_point[d]), d
        assert torch.equal(Fp.witness_weights[d], Ff.witness_weights[d]), d
    ga, gz = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, Fp.values)), (a, zero))
    (gb,) = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, Ff.values)), b)
    assert torch.equal(ga, gb) and ga.abs().sum() > 0
    assert not gz.any()


@pytest.mark.parametrize("dim,max_dim", GENERIC)
def test_gradients_match_float64_closed_form(dim, max_dim):
    """Points', landmarks' and weights' gradient of a random linear functional of ALL values against the float64 closed
    form at the device's witnesses (power_grad_reference.reference_power_gradient), every row within the derived
    float32 bound of that row; the bound itself stays below 1 % of the row's scale on all but 1 % of the rows (checked on
    the reference's numbers alone); a row nothing points at is exactly zero; a second run repeats every bit."""
    tp, tw = _generic(dim)
    tp.requires_grad_(True), tw.requires_grad_(True)
    tensor_landmarks = dim != 2
    if tensor_landmarks:
        tl = fa.generate_landmarks(tp.detach(), 30, start_idx=0).detach().clone().requires_grad_(True)
        inputs = (tp, tl, tw)
    else:
        tl, inputs = 30, (tp, tw)

    def run():
        F = fa.power_filtration(tp, tl, tw, max_dimension=max_dim, points_per_edge=6)
        gen = torch.Generator().manual_seed(7)
        coef = [((torch.rand(v.shape[0], generator=gen) + 0.5)
                 * (2 * torch.randint(0, 2, (v.shape[0],), generator=gen) - 1)).to(DEV) for v in F.values]
        return F, coef, torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, F.values)), inputs)

    F, coef, got = run()
    _, _, again = run()
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    lms = tl.detach() if tensor_landmarks else tp.detach()[F.landmark_ids]
    rp, rl, rw, info = pgr.reference_power_gradient(F, tp.detach(), lms, tw.detach(), coef)
    if tensor_landmarks:
        rows = [("points", got[0], rp, info["bound_points"], info["scale_points"]),
                ("landmarks", got[1], rl, info["bound_landmarks"], info["scale_landmarks"])]
    else:
        rows = [("points", got[0]) + gr.fold_landmarks(rp, rl, info, F.landmark_ids)]
    rows.append(("weights", got[-1].unsqueeze(1), rw.unsqueeze(1), info["bound_weights"], info["scale_weights"]))
    for what, g, ref, bound, scale in rows:
        assert g.dtype == torch.float32 and torch.isfinite(g).all()
        err = (g.double() - ref).abs().max(dim=1).values
        hit = scale > 0
        assert int(hit.sum()) >= 15, what
        over = float((bound[hit] > 0.01 * scale[hit]).double().mean())
        ratio = float((err[hit] / bound[hit]).max())
        print(f"{dim}-D {what}: {int(hit.sum())} rows, worst error / bound {ratio:.3f}, "
              f"bound above 1 % of the row's scale on {over:.3%} of the rows")
        assert over < 0.01, what
        assert not g[~hit].any(), what              # a row nothing points at stays exactly zero
        assert torch.all(err <= bound), (what, ratio)
    assert got[-1].abs().sum() > 0 and (got[-1] < 0).any() and (got[-1] > 0).any()    # the caller's sign


# ---------------------------------------------------------------------------------------------- queries
def test_power_nearest_ids_on_an_integer_cloud():
    """Integer cloud, half-integer queries, integer weights: the ids are the brute force's smallest id at the minimum,
    the distances the roots of its words, bit for bit - with and without ties (a doubled cloud)."""
    for twice in (False, True):
        pts, w = _integer_cloud(30_000, 3, 64, twice, seed=23)
        g = torch.Generator().manual_seed(24)
        q = torch.randint(-8, 2 * 72, (20_000, 3), generator=g).to(torch.float32) / 2
        pgr.assert_exact_power_inputs(pts, pts, w, 3, queries=q)
        tp, tw, tq = pts.to(DEV), w.to(DEV), q.to(DEV)
        ids, dist = fa.power_nearest(tp, tw, tq)
        word, first, count, euclid = pgr.power_nearest_points(tp, tw, tq)
        print(f"twice {twice}: more than one point at the minimum on {float((count > 1).double().mean()):.1%}, "
              f"no Euclidean nearest point on {float((~euclid).double().mean()):.1%} of the queries")
        assert float((count > 1).double().mean()) > (0.9 if twice else 0.02) and float((~euclid).double().mean()) > 0.02
        assert ids.dtype is torch.int64 and torch.equal(ids, first)
        assert torch.equal(dist, word.sqrt().to(torch.float32))
        assert torch.equal(dist, fa.power_distance(tp, tw, tq))
        assert torch.equal(fa.power_distance(tp, tw, tq, squared=True), word.to(torch.float32))
    ids, dist = fa.power_nearest(tp, tw, tq[:0])
    assert ids.shape == (0,) and ids.dtype is torch.int64 and ids.device == tp.device and dist.shape == (0,)


def _closed_form(P, W, Q, ids, coef, squared, own):
    """float64 gradients of sum(coef * value) at the given witnesses and the per-row sums of |terms| and term counts."""
    diff = Q - P[ids]
    ws = W[ids]
    f = ((diff * diff).sum(1) + ws * ws).sqrt()
    k = coef * 2.0 if squared else torch.where(f > 0, coef / f.clamp(min=1e-300), torch.zeros_like(f))
    gq = diff * k.unsqueeze(1)
    n = P.shape[0]
    gp = torch.zeros_like(P).index_add_(0, ids, -gq)
    ap = torch.zeros_like(P).index_add_(0, ids, gq.abs())
    mp = torch.zeros(n, dtype=torch.float64, device=P.device).index_add_(0, ids, torch.ones_like(f))
    if own:
        gp, ap, mp = gp + gq, ap + gq.abs(), mp + 1
    gw = torch.zeros_like(W).index_add_(0, ids, ws * k)
    aw = torch.zeros_like(W).index_add_(0, ids, (ws * k).abs())
    return gq, gp, ap, mp, gw, aw


@pytest.mark.parametrize("dim", [2, 3, 6])
def test_power_distance_backward_matches_float64_closed_form(dim):
    """Queries, points and weights, ``queries=None`` included, plain and squared.  The bound of a float32 evaluation,
    eps = 2**-24: one term g (q - x*) / f rounds the difference, the quotient and the product once each and carries f's
    own error, (dim + 1) / 2 roundings of the sweep's fma chain halved by the root plus the root's: at most
    (dim / 2 + 5) eps |term| (g w* / f likewise); the in-order sum of a row's m terms adds (m - 1) eps sum |terms|; twice
    the sum of the two for what first order drops."""
    tp, tw = _generic(dim, seed=3)
    g = torch.Generator().manual_seed(9)
    tq = (torch.randn(3000, dim, generator=g) * 1.2).to(DEV)
    eps = 2.0 ** -24
    for q in (tq, None):
        own = q is None
        n_q = tp.shape[0] if own else q.shape[0]
        coef = ((torch.rand(n_q, generator=g) + 0.5) * (2 * torch.randint(0, 2, (n_q,), generator=g) - 1)).to(DEV)
        for squared in (False, True):
            a, b = tp.clone().requires_grad_(True), tw.clone().requires_grad_(True)
            c = None if own else q.clone().requires_grad_(True)
            out = fa.power_distance(a, b, c, squared=squared)
            # the forward with grad is the forward without: the parent's path, bit for bit
            plain = fa.power_distance(tp, tw, q, squared=squared)
            assert plain.grad_fn is None and out.grad_fn is not None and torch.equal(out.detach(), plain)
            got = torch.autograd.grad((coef * out).sum(), [a, b] + ([] if own else [c]))
            again = torch.autograd.grad((coef * fa.power_distance(a, b, c, squared=squared)).sum(),
                                        [a, b] + ([] if own else [c]))
            assert all(torch.equal(x, y) for x, y in zip(got, again))
            ids = fa.power_nearest(tp, tw, q)[0]
            Q64 = tp.double() if own else q.double()
            gq, gp, ap, mp, gw, aw = _closed_form(tp.double(), tw.double(), Q64, ids, coef.double(), squared, own)
            per = (dim / 2 + 5) * eps
            bound_p = 2 * (per + (mp - 1).clamp(min=0).unsqueeze(1) * eps) * ap
            assert torch.all((got[0].double() - gp).abs() <= bound_p), ("points", own, squared)
            assert not got[0][ap == 0].any()
            bound_w = 2 * (per + (mp - 1 - (1 if own else 0)).clamp(min=0) * eps) * aw
            assert torch.all((got[1].double() - gw).abs() <= bound_w), ("weights", own, squared)
            assert not got[1][aw == 0].any() and got[1].abs().sum() > 0
            if not own:
                assert torch.all((got[2].double() - gq).abs() <= 2 * per * gq.abs()), ("queries", squared)


def test_no_grad_runs_the_parent_path():
    """Nothing requires grad, or grad mode is off: no autograd node, and the bits of the call with grad."""
    tp, tw = _generic(3, seed=5)
    lms = tp[:50].clone()
    want = fa.power_distance(tp, tw, lms)
    assert want.grad_fn is None
    with torch.no_grad():
        off = fa.power_distance(tp.clone().requires_grad_(True), tw, lms)
    assert off.grad_fn is None and torch.equal(off, want)
    on = fa.power_distance(tp, tw.clone().requires_grad_(True), lms)
    assert on.grad_fn is not None and torch.equal(on.detach(), want)
    fc = fa.flood_complex(tp, lms, points_per_edge=4, point_weights=tw)
    assert torch.equal(want.cpu(), torch.tensor([fc[(i,)] for i in range(50)], dtype=torch.float32))


def test_refused_on_device():
    tp = torch.randn(1000, 3, device=DEV)
    tw = torch.rand(1000, device=DEV)
    with pytest.raises(ValueError, match="needs float32"):
        fa.power_filtration(tp.double(), 20, tw.double())
    with pytest.raises(ValueError, match="ambient dimension 2 to 8"):
        fa.power_filtration(torch.randn(1000, 9, device=DEV), 20, tw)
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match="point_weights needs the tree sweep"):
            fa.power_filtration(tp, 20, tw, method=method)
    with pytest.raises(ValueError, match=r"point_weights\.device"):
        fa.power_filtration(tp, 20, tw.cpu())
    with pytest.raises(ValueError):
        fa.power_nearest(tp.double(), tw.double())
    with pytest.raises(ValueError, match="ambient dimension 2 to 8"):
        fa.power_nearest(torch.randn(1000, 9, device=DEV), tw)
