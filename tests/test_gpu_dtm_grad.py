"""``distance_to_measure(differentiable=True)`` and ``dtm_filtration`` on ROCm tensors: exact end to end on integer
clouds, within a derived bound of the float64 closed form on float clouds, bit-identical run to run and whatever the
groups of the forward and of the backward, the forward's bits, ``neighbor_distance``'s gradients at k = 8 and 32, and
the annulus of the README through ``dtm_filtration``."""

import functools
import math

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import dtm_grad_reference as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _bits(t):
    return t.detach().view(torch.int32)


# ------------------------------------------------------------------------------------------------ exact end to end
@pytest.mark.parametrize("n,dim,hi,k,twice", [(3000, 2, 128, 64, False), (4000, 3, 64, 128, True), (2048, 8, 8, 1024, False)])
def test_integer_clouds_are_exact_end_to_end(n, dim, hi, k, twice):
    """``squared=True`` and k a power of two: the coefficient grad_out * 2 / k is exact, every term and partial sum is
    an integer multiple of 2 / k below 2^24 of them (asserted by the reference), so ``points.grad`` is the int64
    brute force times 2 / k, bit for bit."""
    P = ref.integer_cloud(n, dim, hi, seed=n + dim, twice=twice)
    want_ids = ref.knn_ids(P, P, k)
    go = np.random.default_rng(k).integers(1, 5, size=n, dtype=np.int64)
    x = torch.as_tensor(P).to(torch.float32).to(DEV).requires_grad_(True)
    val, ids, dist = fa.distance_to_measure(x, neighbors=k, squared=True, differentiable=True, return_neighbors=True)
    assert torch.equal(ids.cpu(), torch.as_tensor(want_ids)) and not dist.requires_grad
    (val * torch.as_tensor(go).to(torch.float32).to(DEV)).sum().backward()
    _, gp, largest = ref.integer_grads(P, P, want_ids, go, own=True)
    print(f"largest sum of |terms| of a word, in units of 2 / k: {largest}")
    assert torch.equal(x.grad.cpu(), torch.as_tensor(gp * (2.0 / k)).to(torch.float32))


# ------------------------------------------------------------------------------------------------ float clouds
@functools.lru_cache(maxsize=None)
def _float_cloud(n, dim):
    g = torch.Generator().manual_seed(n + dim)
    return torch.randn(n, dim, generator=g), 1.2 * torch.randn(1000, dim, generator=g)


def _grads(pts, qs, k, stat, squared, own, go, fn=fa.distance_to_measure, **kw):
    """(value, ids, points.grad, queries.grad or None) of one forward and backward on the device."""
    x = pts.to(DEV).requires_grad_(True)
    q = None if own else qs.to(DEV).requires_grad_(True)
    out = fn(x, q, neighbors=k, neighbor_stat=stat, squared=squared, **kw)
    val = out[0] if isinstance(out, tuple) else out
    (val * go.to(DEV)).sum().backward()
    return val.detach(), (out[1] if isinstance(out, tuple) else None), x.grad, (None if own else q.grad)


@pytest.mark.parametrize("own", [True, False], ids=["own", "queries"])
@pytest.mark.parametrize("squared", [False, True], ids=["root", "squared"])
@pytest.mark.parametrize("stat", ["dtm", "kth"])
@pytest.mark.parametrize("n,dim,k", [(20_000, 3, 300), (30_000, 6, 100)])
def test_float_clouds_within_the_derived_bound(n, dim, k, stat, squared, own):
    """Per component |g - g64| <= (n + 64) * 2^-24 * sum |c_i| over the n float64 contributions c_i of that word on the
    ids the call returned.  Derivation: a contribution is coef * (q - x), computed with one rounding for the difference
    and one for the product (grad_points fuses the product into the running sum: one rounding fewer); the coefficient
    grad_out / (f m) carries at most 44 * 2^-24 relative - the forward's 78 * 2^-24 on the squared value, halved by the
    root, plus the root's, the product's and the division's rounding -; that is below 64 * 2^-24 * |c_i| per term;
    the n - 1 additions of a word (n with the own-points addition), in any order, add at most n * 2^-24 times the sum
    of the |c_i| to first order.  A float32 sequential replay of the 3-D case on the host stayed at 0.04 of the bound."""
    pts, qs = _float_cloud(n, dim)
    go = torch.rand(n if own else 1000, generator=torch.Generator().manual_seed(k)) + 0.5
    val, ids, gx, gq = _grads(pts, qs, k, stat, squared, own, go, differentiable=True, return_neighbors=True)
    assert bool(torch.isfinite(gx).all()) and ids.dtype == torch.int64 and ids.shape == (go.shape[0], k)
    wq, wp, abs_q, abs_p, n_q, n_p = ref.closed_form(pts.numpy(), (pts if own else qs).numpy(), ids.cpu().numpy(),
                                                     go.numpy(), stat, squared, own)
    ref.within_bound(gx.cpu().numpy(), wp, n_p, abs_p, f"points n={n} k={k} {stat} squared={squared} own={own}")
    if not own:
        ref.within_bound(gq.cpu().numpy(), wq, n_q, abs_q, f"queries n={n} k={k} {stat} squared={squared}")
        assert int((gx.abs().sum(1) > 0).sum()) < n         # 1000 queries do not reach every point


@pytest.mark.parametrize("k", [8, 32])
@pytest.mark.parametrize("stat", ["dtm", "kth"])
def test_gradients_are_within_the_bound_of_neighbor_distance(stat, k):
    pts, qs = _float_cloud(20_000, 3)
    for own in (True, False):
        go = torch.rand(20_000 if own else 1000, generator=torch.Generator().manual_seed(k)) + 0.5
        val, ids, gx, gq = _grads(pts, qs, k, stat, False, own, go, differentiable=True, return_neighbors=True)
        val0, _, gx0, gq0 = _grads(pts, qs, k, stat, False, own, go, fn=fa.neighbor_distance)
        assert torch.equal(_bits(val), _bits(val0))
        _, _, abs_q, abs_p, n_q, n_p = ref.closed_form(pts.numpy(), (pts if own else qs).numpy(), ids.cpu().numpy(),
                                                       go.numpy(), stat, False, own)
        ref.within_bound(gx.cpu().numpy(), gx0.cpu().double().numpy(), n_p, abs_p, f"points k={k} {stat} own={own}")
        if not own:
            ref.within_bound(gq.cpu().numpy(), gq0.cpu().double().numpy(), n_q, abs_q, f"queries k={k} {stat}")


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("stat", ["dtm", "kth"])
def test_bit_identical_run_to_run_and_whatever_the_groups(stat, monkeypatch):
    pts, qs = _float_cloud(20_000, 3)
    k = 300
    go = torch.rand(20_000, generator=torch.Generator().manual_seed(1)) + 0.5
    plain = fa.distance_to_measure(pts.to(DEV), neighbors=k, neighbor_stat=stat)
    val, _, gx, _ = _grads(pts, qs, k, stat, False, True, go, differentiable=True)
    assert torch.equal(_bits(val), _bits(plain))                      # the forward's bits with grad
    again = _grads(pts, qs, k, stat, False, True, go, differentiable=True)
    assert torch.equal(_bits(again[2]), _bits(gx))
    _, _, gx_q, gq = _grads(pts, qs, k, stat, False, False, go[:1000], differentiable=True)
    # at least three groups in the forward (28 + 4 k bytes per query) and in the backward (64 m bytes per query)
    lib = _native.load()
    sort, entry, seen = core._sorted_sample_order, lib.flooder_dtm_grad_points_f32, {"forward": 0, "backward": 0}

    def counted_sort(*args):
        seen["forward"] += 1
        return sort(*args)

    def counted_entry(*args):
        seen["backward"] += 1
        return entry(*args)

    monkeypatch.setattr(core, "_sorted_sample_order", counted_sort)
    monkeypatch.setattr(lib, "flooder_dtm_grad_points_f32", counted_entry)
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", (28 + 4 * k) * 7000)
    monkeypatch.setattr(core, "DTM_GRAD_WORKSPACE_BYTES", 64 * (k if stat == "dtm" else 1) * 6000)
    grouped = _grads(pts, qs, k, stat, False, True, go, differentiable=True)
    assert seen == {"forward": 3, "backward": 4}
    assert torch.equal(_bits(grouped[0]), _bits(val)) and torch.equal(_bits(grouped[2]), _bits(gx))
    monkeypatch.setattr(core, "DTM_GRAD_WORKSPACE_BYTES", 64 * (k if stat == "dtm" else 1) * 300)
    grouped_q = _grads(pts, qs, k, stat, False, False, go[:1000], differentiable=True)
    assert seen["backward"] == 4 + 4
    assert torch.equal(_bits(grouped_q[2]), _bits(gx_q)) and torch.equal(_bits(grouped_q[3]), _bits(gq))


# ------------------------------------------------------------------------------------------------ dtm_filtration
def test_dtm_filtration_on_the_annulus_of_the_readme():
    clean = fa.generate_annulus_points_2d(20000, radius=1.0, width=0.2, seed=0).float()
    g = torch.Generator().manual_seed(1)
    r, t = 0.7 * torch.sqrt(torch.rand(100, generator=g.manual_seed(1))), 2 * math.pi * torch.rand(100, generator=g)
    dirty = torch.cat([clean, torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1)]).to(DEV)
    kw = dict(points_per_edge=20)

    def run(how):
        x = dirty.clone().requires_grad_(True)
        if how == "entry":
            F = fa.dtm_filtration(x, 200, 0.006, **kw)
        else:
            w = fa.distance_to_measure(x, mass=0.006, differentiable=True)
            F = fa.power_filtration(x, 200, w.detach() if how == "detached" else w, **kw)
        h1 = F.diagrams()[1]
        (-(h1[:, 1] - h1[:, 0]).max()).backward()
        return F, x.grad

    F, grad = run("entry")
    assert F.to_dict() == fa.flood_complex(dirty, 200, point_weights=fa.distance_to_measure(dirty, mass=0.006), **kw)
    assert F.point_weights.requires_grad
    assert torch.equal(_bits(F.point_weights), _bits(fa.distance_to_measure(dirty, mass=0.006)))
    G, manual = run("manual")
    for a, b in zip(F.values, G.values):
        assert torch.equal(_bits(a), _bits(b))
    assert bool(torch.isfinite(grad).all()) and torch.equal(_bits(grad), _bits(manual))
    assert torch.equal(_bits(run("entry")[1]), _bits(grad))           # a second run: the same bits
    rows, rows_cut = (int((x.abs().sum(1) > 0).sum()) for x in (grad, run("detached")[1]))
    print(f"x.grad is non-zero on {rows} rows, with detached weights on {rows_cut}")
    assert rows > rows_cut > 0
