"""``power_filtration``, ``power_nearest`` and the differentiable ``power_distance`` on CPU tensors: the values of
``flood_complex(point_weights=w)``, witnesses against a brute force, gradients against central finite differences,
the chain through ``neighbor_distance``, zero weights, the refusals, the signatures and the new C symbol."""

import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import power_reference as pr
from helpers import tolerances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(n, dim, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(n, dim, generator=g, dtype=torch.float64).to(dtype)
    # signed weights on the scale of the spacing (the weight enters squared)
    w = (torch.rand(n, generator=g, dtype=torch.float64) - 0.5) * 4.0 * pr.median_nn_distance(pts.numpy())
    return pts, w.to(dtype)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dim", [2, 3, 5])
def test_values_equal_flood_complex(dim, dtype):
    pts, w = _cloud(1200, dim, dtype, seed=dim)
    kw = dict(max_dimension=min(dim, 3), points_per_edge=5)
    F = fa.power_filtration(pts, 14, w, **kw)
    fc = fa.flood_complex(pts, 14, point_weights=w, **kw)
    assert F.to_dict() == fc
    assert F.point_weights is w and F.neighbors == 1
    for d, simp in enumerate(F.simplices):
        want = torch.tensor([fc[tuple(r)] for r in simp.tolist()], dtype=dtype)
        assert torch.equal(F.values[d].detach(), want)
        assert F.values[d].dtype == dtype
        assert (F.witness_point[d] >= 0).all()
        assert torch.equal(F.witness_neighbors[d], F.witness_point[d].unsqueeze(1))
    torch.manual_seed(4)
    Fr = fa.power_filtration(pts, 14, w, max_dimension=2, points_per_edge=None, num_rand=20)
    torch.manual_seed(4)
    assert Fr.to_dict() == fa.flood_complex(pts, 14, max_dimension=2, points_per_edge=None, num_rand=20, point_weights=w)
    assert fa.flood_filtration(pts, 14, **kw).point_weights is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_witness_realises_value_and_is_power_nearest(dtype):
    pts, w = _cloud(1500, 3, dtype, seed=1)
    F = fa.power_filtration(pts, 20, w, points_per_edge=6)
    lms = pts[F.landmark_ids].double()
    rtol, atol = tolerances(pts.numpy())
    for d, simp in enumerate(F.simplices):
        p = (F.witness_weights[d].double().unsqueeze(2) * lms[simp.long()]).sum(1)
        jp = F.witness_point[d]
        wv = ((p - pts.double()[jp]).pow(2).sum(1) + w.double()[jp] ** 2).sqrt()
        v = F.tree.filtrations_of_dimension(d)
        tol = torch.as_tensor(atol + rtol * np.abs(v))
        assert torch.all((wv - torch.as_tensor(v)).abs() <= tol), d
        best = pr.brute_power(pts, w, p)[0].sqrt()            # no point gives a smaller power distance
        assert torch.all(wv - best <= tol), d
        lam = F.witness_weights[d].double()
        assert torch.all(lam >= 0) and torch.allclose(lam.sum(1), torch.ones(lam.shape[0], dtype=torch.float64), atol=1e-6)


# ------------------------------------------------------------------------------------------------ finite differences
def _five_point(fn, x, at, h=1e-5):
    """d fn / d x.flat[at] by the fourth-order central difference (f(-2h) - 8 f(-h) + 8 f(h) - f(2h)) / 12h."""
    out = 0.0
    for step, c in ((-2, 1.0), (-1, -8.0), (1, 8.0), (2, -1.0)):
        y = x.clone()
        y.view(-1)[at] += step * h
        out = out + c * fn(y)
    return out / (12 * h)


def _brute_gaps(points, landmarks, w, simplices, ppe, rel=1e-3):
    """Per dimension: is the value's witness isolated - the runner-up sample and the runner-up point of the witness
    sample both further than ``rel`` of the value away (a finite difference must not cross a tie)?"""
    good = []
    for d, simp in enumerate(simplices):
        W = torch.ones((1, 1), dtype=torch.float64) if d == 0 else core.generate_grid(ppe, d, "cpu", torch.float64)[0]
        samples = W.unsqueeze(0) @ landmarks[simp.long()]
        word = (torch.cdist(samples.reshape(-1, points.shape[1]), points) ** 2 + w ** 2).sqrt()
        word = word.reshape(samples.shape[0], W.shape[0], -1)
        mn = word.min(dim=2).values
        val, arg = mn.max(dim=1)
        s2 = torch.topk(mn, min(2, W.shape[0]), dim=1).values
        gap_max = (s2[:, 0] - s2[:, 1]) if W.shape[0] > 1 else torch.full_like(val, np.inf)
        t2 = torch.topk(word[torch.arange(samples.shape[0]), arg], 2, dim=1, largest=False).values
        good.append((gap_max > rel * val) & (t2[:, 1] - t2[:, 0] > rel * val))
    return good


def test_gradients_match_finite_differences():
    """Points, landmark tensor and weights against the fourth-order central difference of the values themselves
    (float64, step 1e-5: truncation h^4 f^(5) / 30 and rounding 1.5 eps |f| / h are both below 1e-10 here), on the
    simplices whose witness is isolated, with the tolerances of test_flood_grad_cpu.py."""
    ppe = 5
    pts, w = _cloud(60, 2, torch.float64, seed=5)
    lms = _cloud(8, 2, torch.float64, seed=6)[0] * 0.8
    pts.requires_grad_(True), lms.requires_grad_(True), w.requires_grad_(True)
    F = fa.power_filtration(pts, lms, w, points_per_edge=ppe)
    good = _brute_gaps(pts.detach(), lms.detach(), w.detach(), F.simplices, ppe)
    assert sum(int(g.sum()) for g in good) >= 0.9 * sum(g.numel() for g in good)
    gen = torch.Generator().manual_seed(0)
    coef = torch.cat([(torch.rand(g.shape[0], generator=gen, dtype=torch.float64) + 0.5) * g for g in good])
    gp, gl, gw = torch.autograd.grad((coef * torch.cat(F.values)).sum(), (pts, lms, w))
    assert gw.abs().sum() > 0 and gp.abs().sum() > 0

    def loss(x=pts.detach(), L=lms.detach(), ww=w.detach()):
        with torch.no_grad():
            return float((coef * torch.cat(fa.power_filtration(x, L, ww, points_per_edge=ppe).values)).sum())

    rng = np.random.default_rng(0)
    rows = np.union1d(torch.nonzero(gp.abs().sum(1) + gw.abs()).reshape(-1).numpy(), rng.choice(60, 6, replace=False))
    for r in rows:
        for c in range(2):
            fd = _five_point(lambda y: loss(x=y), pts.detach(), int(r) * 2 + c)
            assert abs(fd - float(gp[r, c])) <= 1e-9 + 1e-9 * abs(fd), ("points", r, c, fd, float(gp[r, c]))
        fd = _five_point(lambda y: loss(ww=y), w.detach(), int(r))
        assert abs(fd - float(gw[r])) <= 1e-9 + 1e-9 * abs(fd), ("weights", r, fd, float(gw[r]))
    for at in range(lms.numel()):
        fd = _five_point(lambda y: loss(L=y), lms.detach(), at)
        assert abs(fd - float(gl.view(-1)[at])) <= 1e-9 + 1e-9 * abs(fd), ("landmarks", at, fd, float(gl.view(-1)[at]))


def test_chain_through_neighbor_distance():
    """w = the distance to the measure of the cloud at its own points: the weights' gradient flows on into the points."""
    ppe, k = 5, 8
    pts = _cloud(80, 2, torch.float64, seed=7)[0].requires_grad_(True)
    lms = (_cloud(8, 2, torch.float64, seed=8)[0] * 0.8)

    def values(x, detach=False):
        w = fa.neighbor_distance(x, neighbors=k, neighbor_stat="dtm")
        return torch.cat(fa.power_filtration(x, lms, w.detach() if detach else w, points_per_edge=ppe).values)

    coef = torch.linspace(0.5, 1.5, values(pts.detach()).shape[0], dtype=torch.float64)
    (g_full,) = torch.autograd.grad((coef * values(pts)).sum(), pts)
    (g_cut,) = torch.autograd.grad((coef * values(pts, detach=True)).sum(), pts)
    assert (g_full - g_cut).abs().max() > 1e-3
    rows = torch.topk((g_full - g_cut).abs().sum(1), 4).indices.tolist()
    for r in rows:
        for c in range(2):
            fd = _five_point(lambda y: float((coef * values(y)).sum()), pts.detach(), r * 2 + c)
            assert abs(fd - float(g_full[r, c])) <= 1e-9 + 1e-9 * abs(fd), (r, c, fd, float(g_full[r, c]))


# ------------------------------------------------------------------------------------------------ zero weights, signs
def test_zero_weights_are_the_plain_filtration_and_signs_do_not_matter():
    pts, w = _cloud(900, 3, torch.float64, seed=9)
    a = pts.clone().requires_grad_(True)
    b = pts.clone().requires_grad_(True)
    zero = torch.zeros(900, dtype=torch.float64, requires_grad=True)
    Fp = fa.power_filtration(a, 15, zero, points_per_edge=5)
    Ff = fa.flood_filtration(b, 15, points_per_edge=5)
    for d in range(len(Ff.simplices)):
        assert torch.equal(Fp.values[d], Ff.values[d]) and torch.equal(Fp.witness_weights[d], Ff.witness_weights[d])
        # (the lifted and the plain kd-tree may name different copies of equidistant points: none in a generic cloud)
        assert torch.equal(Fp.witness_point[d], Ff.witness_point[d])
    coef = [torch.linspace(0.5, 1.5, v.shape[0], dtype=torch.float64) for v in Ff.values]
    ga, gz = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, Fp.values)), (a, zero))
    (gb,) = torch.autograd.grad(sum((c * v).sum() for c, v in zip(coef, Ff.values)), b)
    assert torch.equal(ga, gb) and not gz.any()
    neg = fa.power_filtration(pts, 15, w, points_per_edge=5)
    pos = fa.power_filtration(pts, 15, w.abs(), points_per_edge=5)
    assert (w < 0).any() and neg.to_dict() == pos.to_dict()
    for d in range(len(neg.simplices)):
        assert torch.equal(neg.witness_point[d], pos.witness_point[d])
    # ... but the gradient carries the caller's sign: d f / d w = w / f
    ws = w.clone().requires_grad_(True)
    wa = w.abs().requires_grad_(True)
    (gs,) = torch.autograd.grad(sum(v.sum() for v in fa.power_filtration(pts, 15, ws, points_per_edge=5).values), ws)
    (gabs,) = torch.autograd.grad(sum(v.sum() for v in fa.power_filtration(pts, 15, wa, points_per_edge=5).values), wa)
    assert torch.equal(gs, gabs * torch.sign(w)) and (gs < 0).any()


def test_diagrams():
    pts, w = _cloud(400, 2, torch.float64, seed=10)
    pts.requires_grad_(True), w.requires_grad_(True)
    F = fa.power_filtration(pts, 18, w, points_per_edge=6)
    dg = F.diagrams()
    F.tree.compute_persistence()
    for d in range(2):
        assert np.array_equal(dg[d].detach().numpy(), F.tree.persistence_intervals_in_dimension(d)), d
    assert dg[1].shape[0] > 0
    gp, gw = torch.autograd.grad((dg[1][:, 1] - dg[1][:, 0]).sum(), (pts, w))
    assert torch.isfinite(gp).all() and gp.abs().sum() > 0 and torch.isfinite(gw).all() and gw.abs().sum() > 0


def test_integer_landmarks_route_gradient_into_points():
    pts, w = _cloud(500, 2, torch.float64, seed=11)
    pts.requires_grad_(True)
    F = fa.power_filtration(pts, 12, w, points_per_edge=5)
    ids = fa.core.fps_indices(pts.detach(), 12, 0)
    assert torch.equal(F.landmark_ids, ids)
    (g,) = torch.autograd.grad(sum(v.sum() for v in F.values), pts)
    p2 = pts.detach().clone().requires_grad_(True)
    l2 = pts.detach()[ids].clone().requires_grad_(True)
    F2 = fa.power_filtration(p2, l2, w, points_per_edge=5)
    assert F2.to_dict() == F.to_dict()
    gp2, gl2 = torch.autograd.grad(sum(v.sum() for v in F2.values), (p2, l2))
    assert torch.allclose(g, gp2.index_add(0, ids, gl2), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ queries
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_power_nearest_and_differentiable_power_distance(dtype):
    pts, w = _cloud(300, 3, dtype, seed=12)
    g = torch.Generator().manual_seed(5)
    queries = (torch.randn(50, 3, generator=g, dtype=torch.float64) * 1.2).to(dtype)
    for q in (queries, None):
        qq = pts if q is None else q
        ids, dist = fa.power_nearest(pts, w, q)
        plain = fa.power_distance(pts, w, q)
        assert ids.dtype is torch.int64 and ids.shape == (qq.shape[0],) and torch.equal(dist, plain)
        ref, arg, _ = pr.brute_power(pts, w, qq)
        at = ((qq.double() - pts.double()[ids]) ** 2).sum(1) + w.double()[ids] ** 2
        assert torch.allclose(at, ref, rtol=1e-12, atol=0)                 # a point at the minimum
        for squared in (False, True):
            # float64 autograd of the brute-force minimum at the same argmin is the closed form
            P = pts.double().clone().requires_grad_(True)
            Wt = w.double().clone().requires_grad_(True)
            Q = None if q is None else q.double().clone().requires_grad_(True)
            QQ = P if Q is None else Q
            val2 = ((QQ - P[ids]) ** 2).sum(1) + Wt[ids] ** 2
            # (a point that is its own power-nearest point at w = 0 has f = 0: the gradient is 0 there, not NaN)
            val = val2 if squared else torch.where(val2 > 0, val2.clamp(min=1e-300).sqrt(), val2)
            coef = torch.linspace(0.5, 1.5, qq.shape[0], dtype=torch.float64)
            want = torch.autograd.grad((coef * val).sum(), [P, Wt] + ([] if Q is None else [Q]))
            a, b = pts.clone().requires_grad_(True), w.clone().requires_grad_(True)
            c = None if q is None else q.clone().requires_grad_(True)
            out = fa.power_distance(a, b, c, squared=squared)
            assert out.grad_fn is not None and torch.equal(out.detach(), fa.power_distance(pts, w, q, squared=squared))
            got = torch.autograd.grad((coef.to(dtype) * out).sum(), [a, b] + ([] if c is None else [c]))
            tol = dict(rtol=1e-9, atol=1e-9) if dtype is torch.float64 else dict(rtol=2e-4, atol=2e-5)
            for x, y in zip(got, want):
                assert x.dtype is dtype and torch.allclose(x.double(), y, **tol)
    # only the weights require grad; no grad at all: the plain tensor
    b = w.clone().requires_grad_(True)
    (gw,) = torch.autograd.grad(fa.power_distance(pts, b, queries).sum(), b)
    assert gw.abs().sum() > 0
    assert fa.power_distance(pts, w, queries).grad_fn is None
    with torch.no_grad():
        assert fa.power_distance(pts, b, queries).grad_fn is None
    # no queries
    ids, dist = fa.power_nearest(pts, w, pts[:0])
    assert ids.shape == (0,) and ids.dtype is torch.int64 and dist.shape == (0,) and dist.dtype is dtype
    assert fa.power_distance(pts.clone().requires_grad_(True), w, pts[:0]).shape == (0,)
    # the vertex witnesses of the filtration are the power-nearest points of the landmarks
    lms = pts[:10].clone()
    F = fa.power_filtration(pts, lms, w, points_per_edge=4)
    assert torch.equal(F.witness_point[0], fa.power_nearest(pts, w, lms)[0])


# ------------------------------------------------------------------------------------------------ signatures, refusals
def test_signatures():
    assert "power_filtration" in fa.__all__ and "power_nearest" in fa.__all__
    assert list(inspect.signature(fa.power_filtration).parameters) == [
        "points", "landmarks", "point_weights", "max_dimension", "points_per_edge", "num_rand", "start_idx", "method",
        "index"]
    sig = inspect.signature(fa.power_filtration).parameters
    assert sig["method"].kind is inspect.Parameter.KEYWORD_ONLY and sig["index"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["points_per_edge"].default == 30 and sig["start_idx"].default == 0
    assert list(inspect.signature(fa.power_nearest).parameters) == ["points", "point_weights", "queries", "index"]
    assert inspect.signature(fa.power_nearest).parameters["index"].kind is inspect.Parameter.KEYWORD_ONLY
    # unchanged
    assert list(inspect.signature(fa.flood_filtration).parameters) == [
        "points", "landmarks", "max_dimension", "points_per_edge", "num_rand", "start_idx", "method", "index",
        "neighbors", "neighbor_stat"]
    assert list(inspect.signature(fa.power_distance).parameters) == ["points", "point_weights", "queries", "squared",
                                                                    "index"]
    from flooder_amd import grad

    assert list(inspect.signature(grad.witness_backward).parameters) == [
        "simplices", "witness_point", "witness_weights", "points", "landmarks", "grad", "witness_neighbors"]
    assert "keep" in inspect.signature(core._sweep_dimension_power).parameters


def test_refusals():
    pts, w = _cloud(200, 3, torch.float32)
    for bad, match in ((w[:-1], r"point_weights must be a \(200,\) tensor"), (w.unsqueeze(1), "one weight per point"),
                       (w.numpy(), "one weight per point"), (w.double(), r"point_weights\.dtype"),
                       (w.to("meta"), r"point_weights\.device")):
        with pytest.raises(ValueError, match=match):
            fa.power_filtration(pts, 10, bad)
        with pytest.raises(ValueError, match=match):
            fa.power_nearest(pts, bad)
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match="point_weights needs the tree sweep.*unweighted nearest point only"):
            fa.power_filtration(pts, 10, w, method=method)
    with pytest.raises(ValueError, match="method must be"):
        fa.power_filtration(pts, 10, w, method="nope")
    for value in (float("nan"), float("inf")):
        bad = w.clone()
        bad[7] = value
        with pytest.raises(ValueError, match="point_weights must be finite"):
            fa.power_filtration(pts, 10, bad)
        with pytest.raises(ValueError, match="point_weights must be finite"):
            fa.power_nearest(pts, bad)
    with pytest.raises(RuntimeError, match="non-empty"):
        fa.power_filtration(pts[:0], 10, w[:0])
    with pytest.raises(TypeError):
        fa.power_filtration(pts.half(), 10, w.half())
    with pytest.raises(TypeError):
        fa.power_filtration(pts, 10, w, neighbors=2)
    for method in (None, "auto", "bvh"):
        assert fa.power_filtration(pts, 10, w, points_per_edge=4, method=method).to_dict() == \
            fa.flood_complex(pts, 10, points_per_edge=4, point_weights=w)


def test_witness_power_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "int flooder_witness_power(const flooder_witness_search_t* p, const float* w_sorted, const float* node_w, " \
           "void* stream);" in header
    res, args = _native.SIGNATURES["flooder_witness_power"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_native.WitnessSearch), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "flooder_witness_power")
    # refused before a pointer is read: a foreign block, a block that is too long
    lib = _native.load()
    blk = _native.WitnessSearch()
    blk.abi = 2
    assert lib.flooder_witness_power(ctypes.byref(blk), None, None, None) == -1
    blk = _native.WitnessSearch()
    blk.size = ctypes.sizeof(blk) + 8
    assert lib.flooder_witness_power(ctypes.byref(blk), None, None, None) == -1
    assert lib.flooder_witness_power(ctypes.byref(_native.WitnessSearch(n_queries=5, dim=3)), None, None, None) == -1
    assert lib.flooder_last_error().decode() == "flooder_witness_power: bad argument"
    assert lib.flooder_witness_power(ctypes.byref(_native.WitnessSearch(n_queries=0)), None, None, None) == 0
