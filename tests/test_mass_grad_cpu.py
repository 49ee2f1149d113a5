"""The backward of ``distance_to_weighted_measure(differentiable=True)``, ``voxel_measure(differentiable=True)`` and
``dtm_filtration(cell_size=...)`` on CPU tensors, the refusals, the CLI flag and the wiring of the two
``flooder_mass_grad_*_f32`` entries (no GPU).  The oracle is ``mass_grad_reference.oracle``: float64 autograd of the rule
itself on the ids and counts the call returned."""

import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, build, cli

import mass_grad_reference as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-10


def _cloud(dim, kind, seed):
    g = torch.Generator().manual_seed(seed)
    sites = torch.rand(300, dim, dtype=torch.float64, generator=g)
    if kind == "integer":
        mu = torch.randint(0, 4, (300,), generator=g).to(torch.float64)
    else:
        mu = torch.rand(300, dtype=torch.float64, generator=g) * 3.0
    queries = torch.rand(70, dim, dtype=torch.float64, generator=g)
    return sites, mu, queries, g


def _run(sites, mu, queries, grad_out, mass, stat, squared, **kw):
    """One differentiable call and its backward -> (value, ids, count, grads of sites, masses, queries or None)."""
    y, m = sites.clone().requires_grad_(True), mu.clone().requires_grad_(True)
    q = None if queries is None else queries.clone().requires_grad_(True)
    value, ids, _, count = fa.distance_to_weighted_measure(y, m, q, mass=mass, neighbor_stat=stat, squared=squared,
                                                           return_neighbors=True, differentiable=True, **kw)
    assert value.grad_fn is not None and not ids.requires_grad and not count.requires_grad
    plain = fa.distance_to_weighted_measure(sites, mu, queries, mass=mass, neighbor_stat=stat, squared=squared, **kw)
    assert torch.equal(value.detach(), plain)
    value.backward(grad_out)
    return value.detach(), ids, count, y.grad, m.grad, None if q is None else q.grad


@pytest.mark.parametrize("dim", [3, 10])
@pytest.mark.parametrize("kind", ["integer", "real"])
@pytest.mark.parametrize("stat", ["dtm", "kth"])
@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("own", [False, True])
def test_three_gradients_against_float64_autograd(dim, kind, stat, squared, own):
    sites, mu, queries, g = _cloud(dim, kind, 10 * dim + (kind == "real"))
    queries = None if own else queries
    Q = 300 if own else 70
    grad_out = torch.rand(Q, dtype=torch.float64, generator=g) + 0.5
    mass = 0.05
    value, ids, count, gy, gm, gq = _run(sites, mu, queries, grad_out, mass, stat, squared)
    reached = torch.isfinite(value)
    assert bool(reached.all()) and int(count.max()) > 5
    want_y, want_m, want_q = mref.oracle(sites, mu, queries, ids, count, reached, grad_out, mass, stat, squared, own)
    mref.relative_close(gy, want_y, REL, "sites")
    if stat == "kth":
        assert not np.any(want_m) and not bool(gm.any())
    else:
        mref.relative_close(gm, want_m, REL, "masses")
    if own:
        assert gq is None
    else:
        mref.relative_close(gq, want_q, REL, "queries")


@pytest.mark.parametrize("stat", ["dtm", "kth"])
@pytest.mark.parametrize("squared", [False, True])
def test_rows_that_are_not_reached_add_nothing(stat, squared):
    sites, mu, queries, g = _cloud(3, "integer", 5)
    mass = 0.21                                  # tau = 0.21 * sum(mu), about what 64 sites of mean mass 1.5 hold
    grad_out = torch.ones(70, dtype=torch.float64)
    value, ids, count, gy, gm, gq = _run(sites, mu, queries, grad_out, mass, stat, squared, max_neighbors=64)
    reached = torch.isfinite(value)
    assert 0 < int(reached.sum()) < 70, "the case must leave some, not all, rows unreached"
    for t in (gy, gm, gq):
        assert bool(torch.isfinite(t).all())
    assert not bool(gq[~reached].any())
    want_y, want_m, want_q = mref.oracle(sites, mu, queries, ids, count, reached, grad_out, mass, stat, squared)
    mref.relative_close(gy, want_y, REL, "sites")
    mref.relative_close(gq, want_q, REL, "queries")
    if stat == "dtm":
        mref.relative_close(gm, want_m, REL, "masses")
    # ... whatever their incoming gradient is
    wild = torch.where(reached, grad_out, torch.full_like(grad_out, float("inf")))
    again = _run(sites, mu, queries, wild, mass, stat, squared, max_neighbors=64)
    for a, b in zip((gy, gm, gq), again[3:]):
        assert torch.equal(a, b)
    # every row unreached: zero gradients, no NaN
    none = _run(sites, mu, queries, grad_out, 1.0, stat, squared, max_neighbors=64)
    assert not bool(torch.isfinite(none[0]).any())
    for t in none[3:]:
        assert not bool(t.any())


@pytest.mark.parametrize("stat", ["dtm", "kth"])
def test_a_value_of_zero_has_gradient_zero(stat):
    g = torch.Generator().manual_seed(2)
    half = torch.rand(60, 3, dtype=torch.float64, generator=g)
    sites = torch.cat([half, half])                       # every site twice
    mu = torch.ones(120, dtype=torch.float64)
    value, ids, count, gy, gm, gq = _run(sites, mu, None, torch.ones(120, dtype=torch.float64), 2 / 120, stat, False)
    assert not bool(value.any())                          # the site and its copy hold the mass 2: f = 0 everywhere
    for t in (gy, gm):
        assert bool(torch.isfinite(t).all()) and not bool(t.any())
    # ... and a mixed case: three sites of mass, f > 0, next to f = 0 rows of another call stays finite
    value, ids, count, gy, gm, gq = _run(sites, mu, None, torch.ones(120, dtype=torch.float64), 3 / 120, stat, False)
    assert bool((value > 0).all()) and bool(torch.isfinite(gy).all()) and bool(gy.any())


def test_float32_cpu_tensors_and_the_default_call():
    sites, mu, queries, g = _cloud(3, "integer", 9)
    y, m, q = (t.to(torch.float32) for t in (sites, mu, queries))
    value, ids, count, gy, gm, gq = _run(y, m, q, torch.ones(70), 0.05, "dtm", False)
    assert gy.dtype == gm.dtype == gq.dtype == torch.float32
    want_y, want_m, want_q = mref.oracle(y, m, q, ids, count, torch.isfinite(value), np.ones(70), 0.05, "dtm", False)
    mref.relative_close(gy, want_y, 1e-5, "sites")
    mref.relative_close(gm, want_m, 1e-5, "masses")
    mref.relative_close(gq, want_q, 1e-5, "queries")
    # without the keyword, and with it but without an input that requires grad, nothing changes
    y.requires_grad_(True)
    assert fa.distance_to_weighted_measure(y, m, q, mass=0.05).grad_fn is None
    assert fa.distance_to_weighted_measure(y.detach(), m, q, mass=0.05, differentiable=True).grad_fn is None
    with torch.no_grad():
        assert fa.distance_to_weighted_measure(y, m, q, mass=0.05, differentiable=True).grad_fn is None
    only_m = m.clone().requires_grad_(True)
    v = fa.distance_to_weighted_measure(y.detach(), only_m, q, mass=0.05, differentiable=True)
    v.sum().backward()
    assert bool(only_m.grad.any())


def test_voxel_measure_gradient_is_that_of_a_segment_mean():
    g = torch.Generator().manual_seed(4)
    pts = torch.rand(2000, 3, dtype=torch.float64, generator=g)
    plain_sites, plain_mu = fa.voxel_measure(pts, 0.13)
    x = pts.clone().requires_grad_(True)
    sites, mu = fa.voxel_measure(x, 0.13, differentiable=True)
    assert sites.grad_fn is not None and not mu.requires_grad
    assert torch.equal(sites.detach(), plain_sites) and torch.equal(mu, plain_mu)
    weight = torch.rand(sites.shape, dtype=torch.float64, generator=g)
    (sites * weight).sum().backward()
    # a plain torch segment mean over the same cells
    cell = torch.floor((pts - pts.min(dim=0).values) * (1.0 / 0.13)).to(torch.int64)
    _, inverse, counts = torch.unique(cell, dim=0, return_inverse=True, return_counts=True)
    z = pts.clone().requires_grad_(True)
    mean = torch.zeros(sites.shape, dtype=torch.float64).index_add(0, inverse.reshape(-1), z) / counts.unsqueeze(1)
    assert float((mean.detach() - plain_sites).abs().max()) < 1e-12
    (mean * weight).sum().backward()
    assert torch.equal(x.grad, z.grad)
    # the default call stays detached
    assert fa.voxel_measure(x, 0.13)[0].grad_fn is None
    assert fa.voxel_measure(pts, 0.13, differentiable=True)[0].grad_fn is None


def _dirty_annulus(n=3000):
    g = torch.Generator()
    clean = fa.generate_annulus_points_2d(n, radius=1.0, width=0.2, seed=0).float()
    r, t = 0.7 * torch.sqrt(torch.rand(100, generator=g.manual_seed(1))), 2 * math.pi * torch.rand(100, generator=g)
    return torch.cat([clean, torch.stack([r * torch.cos(t), r * torch.sin(t)], dim=1)])


def test_dtm_filtration_over_a_coreset():
    dirty = _dirty_annulus()
    mass, cell = 0.02, 0.05                                  # 62 points of 3100: a few tens of sites per point
    x = dirty.clone().requires_grad_(True)
    F = fa.dtm_filtration(x, 60, mass, points_per_edge=6, cell_size=cell)
    sites, mu = fa.voxel_measure(dirty, cell)
    w = fa.distance_to_weighted_measure(sites, mu, dirty, mass)
    assert bool(torch.isfinite(w).all()) and torch.equal(F.point_weights.detach(), w)
    assert F.to_dict() == fa.flood_complex(dirty, 60, points_per_edge=6, point_weights=w)
    sum(v.sum() for v in F.values).backward()
    assert bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
    # the weight gradient reaches the cloud through both roles: as queries and through the centroids
    y = dirty.clone().requires_grad_(True)
    s2, m2 = fa.voxel_measure(y, cell, differentiable=True)
    fa.distance_to_weighted_measure(s2, m2, dirty, mass, differentiable=True).sum().backward()
    assert bool(y.grad.any())


def test_refusals():
    dirty = _dirty_annulus(1000)
    with pytest.raises(ValueError, match="a coreset is addressed by mass"):
        fa.dtm_filtration(dirty, 30, cell_size=0.1, neighbors=20)
    with pytest.raises(ValueError, match="a coreset is addressed by mass"):
        fa.dtm_filtration(dirty, 30, 0.02, cell_size=0.1, neighbors=20)
    with pytest.raises(ValueError, match="max_neighbors.*needs cell_size"):
        fa.dtm_filtration(dirty, 30, 0.02, max_neighbors=64)
    with pytest.raises(ValueError, match="needs mass"):
        fa.dtm_filtration(dirty, 30, cell_size=0.1)
    # a point that is not reached: the number of them and the two remedies
    with pytest.raises(ValueError, match=r"\d+ of 1100 points were not reached.*coarsen cell_size or lower mass"):
        fa.dtm_filtration(dirty, 30, 0.5, cell_size=0.01, max_neighbors=64)
    with pytest.raises(TypeError):
        fa.dtm_filtration(dirty, 30, 0.02, None, 30, None, 0, 0.1)      # cell_size is keyword-only


def test_cli_flag(tmp_path):
    dirty = _dirty_annulus(600)
    np.save(tmp_path / "cloud.npy", dirty.numpy())
    common = ["--input-file", str(tmp_path / "cloud.npy"), "--device", "cpu", "--num-landmarks", "20",
              "--points-per-edge", "5"]
    out = tmp_path / "out.pkl"
    assert cli.main(common + ["--output-file", str(out), "--dtm-weights", "0.05", "--dtm-cell-size", "0.1"]) == 0
    got = pickle.load(open(out, "rb"))["diagrams"]
    sites, mu = fa.voxel_measure(dirty, 0.1)
    w = fa.distance_to_weighted_measure(sites, mu, dirty, 0.05)
    st = fa.flood_complex(dirty, 20, points_per_edge=5, point_weights=w, return_simplex_tree=True)
    st.compute_persistence()
    want = [st.persistence_intervals_in_dimension(i) for i in range(2)]
    assert len(got) == len(want) and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))
    with pytest.raises(SystemExit):
        cli.main(common + ["--dtm-cell-size", "0.1"])                   # only with --dtm-weights
    np.save(tmp_path / "large.npy", _dirty_annulus(2400).numpy())          # 2500 sites of one point: 1024 hold 41 %
    with pytest.raises(ValueError, match="were not reached"):
        cli.main(["--input-file", str(tmp_path / "large.npy"), *common[2:], "--dtm-weights", "0.9", "--dtm-cell-size",
                  "0.0001"])
    text = cli.build_parser().format_help()
    assert "--dtm-cell-size" in text and "unless --dtm-cell-size is given" in " ".join(text.split())


def test_wiring():
    assert "flood_mass_grad.hip" in build.HIP_SOURCES and "flood_dtm_grad.hip" in build.HIP_SOURCES
    assert os.path.exists(os.path.join(ROOT, "flooder_amd", "csrc", "flood_mass_grad.hip"))
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    for name, n_args in (("flooder_mass_grad_queries_f32", 12), ("flooder_mass_grad_points_f32", 12),
                         ("flooder_mass_grad_masses_f32", 12)):
        decl = re.search(rf"^int {name}\(([^;]*)\);", header, re.M)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        res, args = _native.SIGNATURES[name]
        assert len(args) == n_args and res is _native.c_int
    import inspect

    assert inspect.signature(fa.distance_to_weighted_measure).parameters["differentiable"].default is False
    assert inspect.signature(fa.voxel_measure).parameters["differentiable"].default is False
    sig = inspect.signature(fa.dtm_filtration)
    for name in ("cell_size", "max_neighbors"):
        assert sig.parameters[name].default is None and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
