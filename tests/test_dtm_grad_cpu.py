"""``distance_to_measure(differentiable=True)`` and ``dtm_filtration`` on CPU tensors: gradcheck, the float64 closed form
on the returned ids for k in the hundreds, ``neighbor_distance``'s gradients up to k = 32, the detached default, the
composition ``dtm_filtration`` stands for, a finite-difference check, and the two new C symbols."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, build, core

import dtm_grad_reference as ref
from test_knn_wide_cpu import _cloud
from test_power_grad_cpu import _five_point

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ gradcheck
@pytest.mark.parametrize("squared", [False, True], ids=["root", "squared"])
@pytest.mark.parametrize("stat", ["dtm", "kth"])
@pytest.mark.parametrize("own", [True, False], ids=["own", "queries"])
def test_gradcheck(own, stat, squared):
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(40, 3, generator=g, dtype=torch.float64, requires_grad=True)
    qs = None if own else torch.randn(5, 3, generator=g, dtype=torch.float64, requires_grad=True)

    def fn(*xs):
        return fa.distance_to_measure(xs[0], None if own else xs[1], neighbors=7, neighbor_stat=stat, squared=squared,
                                      differentiable=True)

    assert torch.autograd.gradcheck(fn, (pts,) if own else (pts, qs), eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ k in the hundreds
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [40, 200])
@pytest.mark.parametrize("stat", ["dtm", "kth"])
def test_gradient_is_the_closed_form_on_the_returned_ids(stat, k, dtype):
    """Own points (a third of them duplicates: f = 0 at k = 1 only, ties everywhere) and separate queries; within the
    bound of the device test, whose derivation covers a float32 sum in any order (float64: 2^-53 in place of 2^-24
    would do; the float32 bound is simply not reached)."""
    pts, qs = _cloud(3, 600, dtype)
    gen = torch.Generator().manual_seed(k)
    for own in (True, False):
        p = pts.clone().requires_grad_(True)
        q = None if own else qs.clone().requires_grad_(True)
        val, ids, dist = fa.distance_to_measure(p, q, neighbors=k, neighbor_stat=stat, return_neighbors=True,
                                                differentiable=True)
        assert val.requires_grad and not dist.requires_grad and ids.dtype == torch.int64
        go = torch.rand(val.shape[0], generator=gen, dtype=torch.float64).to(dtype) + 0.5
        grads = torch.autograd.grad((val * go).sum(), (p,) if own else (p, q))
        gq, gp, abs_q, abs_p, n_q, n_p = ref.closed_form(pts.numpy(), (pts if own else qs).numpy(), ids.numpy(),
                                                         go.numpy(), stat, False, own)
        assert grads[0].dtype == dtype and grads[0].shape == pts.shape
        ref.within_bound(grads[0].numpy(), gp, n_p, abs_p, f"points {stat} k={k} own={own}")
        if not own:
            ref.within_bound(grads[1].numpy(), gq, n_q, abs_q, f"queries {stat} k={k}")


@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("stat", ["dtm", "kth"])
def test_gradients_are_those_of_neighbor_distance_up_to_32(stat, k):
    pts, qs = _cloud(3, 600, torch.float64, seed=1)
    for squared in (False, True):
        got, want = [], []
        for fn, kw, out in ((fa.distance_to_measure, dict(differentiable=True), got), (fa.neighbor_distance, {}, want)):
            p, q = pts.clone().requires_grad_(True), qs.clone().requires_grad_(True)
            a = fn(p, neighbors=k, neighbor_stat=stat, squared=squared, **kw)
            b = fn(p, q, neighbors=k, neighbor_stat=stat, squared=squared, **kw)
            w = torch.linspace(0.5, 1.5, 600, dtype=torch.float64)
            out.extend([a.detach(), b.detach(), *torch.autograd.grad((w * a).sum() + (w[:60] * b).sum(), (p, q))])
        for x, y in zip(got, want):
            assert torch.allclose(x, y, rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------------------------ opt-in
def test_the_keyword_changes_nothing_without_a_grad_input_and_the_default_stays_detached():
    pts, qs = _cloud(3, 600, torch.float32)
    plain = fa.distance_to_measure(pts, qs, mass=0.1)
    same = fa.distance_to_measure(pts, qs, mass=0.1, differentiable=True)
    assert torch.equal(plain, same) and not same.requires_grad and same.grad_fn is None
    p = pts.clone().requires_grad_(True)
    assert not fa.distance_to_measure(p, qs, mass=0.1).requires_grad                      # the default: detached
    assert not fa.distance_to_measure(p, mass=0.1, differentiable=False).requires_grad
    with torch.no_grad():
        assert not fa.distance_to_measure(p, mass=0.1, differentiable=True).requires_grad
    got = fa.distance_to_measure(p, qs, mass=0.1, differentiable=True)
    assert got.requires_grad and torch.equal(got.detach(), plain)                          # the value's bits
    val, ids, dist = fa.distance_to_measure(p, qs, mass=0.1, differentiable=True, return_neighbors=True)
    v0, i0, d0 = fa.distance_to_measure(pts, qs, mass=0.1, return_neighbors=True)
    assert torch.equal(val.detach(), v0) and torch.equal(ids, i0) and torch.equal(dist, d0) and not dist.requires_grad
    # only the queries require grad: nothing flows into the points
    q = qs.clone().requires_grad_(True)
    out = fa.distance_to_measure(pts, q, mass=0.1, differentiable=True)
    (gq,) = torch.autograd.grad(out.sum(), q)
    assert gq.shape == qs.shape and gq.abs().sum() > 0
    sig = inspect.signature(fa.distance_to_measure).parameters["differentiable"]
    assert sig.kind is inspect.Parameter.KEYWORD_ONLY and sig.default is False
    assert fa.distance_to_measure(p, qs[:0], neighbors=1, differentiable=True).shape == (0,)      # no queries


# ------------------------------------------------------------------------------------------------ dtm_filtration
def _annulus(n, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=g, dtype=torch.float64) * 2 * np.pi
    r = 1.0 + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    return torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_dtm_filtration_is_the_manual_composition(dtype):
    pts = _annulus(500, dtype)
    kw = dict(max_dimension=2, points_per_edge=5)
    a = pts.clone().requires_grad_(True)
    F = fa.dtm_filtration(a, 16, 0.05, **kw)
    w0 = fa.distance_to_measure(pts, mass=0.05)
    assert F.to_dict() == fa.flood_complex(pts, 16, point_weights=w0, **kw)
    assert F.point_weights.requires_grad and torch.equal(F.point_weights.detach(), w0)
    b = pts.clone().requires_grad_(True)
    w = fa.distance_to_measure(b, mass=0.05, differentiable=True)
    G = fa.power_filtration(b, 16, w, **kw)
    coef = [torch.linspace(0.5, 1.5, v.shape[0], dtype=dtype) for v in F.values]
    sum((c * v).sum() for c, v in zip(coef, F.values)).backward()
    sum((c * v).sum() for c, v in zip(coef, G.values)).backward()
    for d in range(len(F.values)):
        assert torch.equal(F.values[d], G.values[d])
    assert torch.equal(a.grad, b.grad) and torch.isfinite(a.grad).all()
    # the weights' gradient reaches more rows than the witnesses alone
    c = pts.clone().requires_grad_(True)
    H = fa.power_filtration(c, 16, w0, **kw)
    sum((cf * v).sum() for cf, v in zip(coef, H.values)).backward()
    assert int((a.grad.abs().sum(1) > 0).sum()) > int((c.grad.abs().sum(1) > 0).sum())
    # neighbors= and "kth" pass through; the argument checks are those of the two functions
    K = fa.dtm_filtration(pts, 16, neighbors=25, neighbor_stat="kth", **kw)
    assert K.to_dict() == fa.flood_complex(pts, 16, point_weights=fa.distance_to_measure(pts, neighbors=25,
                                                                                       neighbor_stat="kth"), **kw)
    with pytest.raises(ValueError, match="distance_to_measure needs exactly one of mass and neighbors"):
        fa.dtm_filtration(pts, 16)
    with pytest.raises(ValueError, match="method"):
        fa.dtm_filtration(pts, 16, 0.05, method="cell")
    assert "dtm_filtration" in fa.__all__ and fa.dtm_filtration is fa.grad.dtm_filtration
    assert "dtm_filtration" in fa.grad.__all__


def test_dtm_filtration_matches_finite_differences():
    """One scalar loss of a 200-point 2-D cloud, 12 fixed landmarks, points_per_edge 5, float64, against the
    fourth-order central difference (step 1e-5) on the rows where the weights' share of the gradient is largest - as
    test_power_grad_cpu.py checks the chain through ``neighbor_distance``."""
    pts = _annulus(200, torch.float64, seed=2).requires_grad_(True)
    lms = _annulus(12, torch.float64, seed=3) * 0.9

    def values(x, detach=False):
        F = fa.dtm_filtration(x, lms, 0.06, points_per_edge=5)
        if detach:
            F = fa.power_filtration(x, lms, F.point_weights.detach(), points_per_edge=5)
        return torch.cat(F.values)

    coef = torch.linspace(0.5, 1.5, values(pts.detach()).shape[0], dtype=torch.float64)
    (g_full,) = torch.autograd.grad((coef * values(pts)).sum(), pts)
    (g_cut,) = torch.autograd.grad((coef * values(pts, detach=True)).sum(), pts)
    assert (g_full - g_cut).abs().max() > 1e-3
    rows = torch.topk((g_full - g_cut).abs().sum(1), 4).indices.tolist()
    for r in rows:
        for c in range(2):
            fd = _five_point(lambda y: float((coef * values(y)).sum()), pts.detach(), r * 2 + c)
            assert abs(fd - float(g_full[r, c])) <= 1e-9 + 1e-9 * abs(fd), (r, c, fd, float(g_full[r, c]))


# ------------------------------------------------------------------------------------------------ the C entries
def test_header_bindings_and_sources_agree():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "flood_dtm_grad.hip" in build.HIP_SOURCES
    for name in ("flooder_dtm_grad_queries_f32", "flooder_dtm_grad_points_f32"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) <= 12
        decl = re.search(rf"^int {name}\((.*?)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args)
    assert core.DTM_GRAD_WORKSPACE_BYTES > 0
