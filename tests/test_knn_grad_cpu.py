"""``flood_filtration(neighbors=k, neighbor_stat=...)`` on the CPU path: the values and refusals of ``flood_complex``,
the witnesses against a float64 brute force, the backward against torch autograd through the reported witnesses, the
envelope claim (witnesses may be frozen) against central differences of ``flood_complex``, and the ABI of
``flooder_witness_knn``."""

import ctypes
import os

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from flooder_amd.grad import flood_filtration

import grad_reference as gr
import knn_grad_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.filterwarnings("ignore:float64 inputs")


def _cloud(dim, n, dtype, seed=0):
    g = torch.Generator().manual_seed(100 * dim + seed)
    return torch.rand(n, dim, generator=g, dtype=torch.float64).to(dtype)


# ------------------------------------------------------------------------------------------------ values, validation
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("stat", ["kth", "dtm"])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_values_are_flood_complex_and_neighbors_have_their_shape(k, stat, dim, dtype):
    pts = _cloud(dim, 300, dtype)
    kw = dict(points_per_edge=5, start_idx=0, neighbors=k, neighbor_stat=stat)
    F = flood_filtration(pts, 12, **kw)
    assert F.to_dict() == fa.flood_complex(pts, 12, **kw)
    assert (F.neighbors, F.neighbor_stat) == (k, stat)
    for d, simp in enumerate(F.simplices):
        nb = F.witness_neighbors[d]
        assert nb.shape == (simp.shape[0], k) and nb.dtype == torch.int64
        assert torch.equal(nb[:, -1], F.witness_point[d])
        assert bool(((nb >= 0) & (nb < 300)).all())
        if k == 1:
            assert torch.equal(nb, F.witness_point[d][:, None])
        else:    # k different points, ascending by (distance, id)
            assert all(len(set(row)) == k for row in nb.tolist())
            p = (F.witness_weights[d].double().unsqueeze(2) * pts.double()[F.landmark_ids][simp.long()]).sum(dim=1)
            dist = (p.unsqueeze(1) - pts.double()[nb]).norm(dim=2)
            assert bool((dist[:, 1:] >= dist[:, :-1] * (1 - 1e-6)).all())


@pytest.mark.parametrize("stat", ["kth", "dtm"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_one_neighbor_is_the_call_without_the_argument(stat, dtype):
    for dim in (2, 3):
        x = _cloud(dim, 300, dtype).requires_grad_(True)
        y = x.detach().clone().requires_grad_(True)
        A = flood_filtration(x, 12, points_per_edge=5)
        B = flood_filtration(y, 12, points_per_edge=5, neighbors=1, neighbor_stat=stat)
        g = torch.Generator().manual_seed(3)
        for d in range(len(A.values)):
            assert torch.equal(A.values[d], B.values[d])
            assert torch.equal(A.witness_point[d], B.witness_point[d])
            assert torch.equal(A.witness_weights[d], B.witness_weights[d])
            assert torch.equal(B.witness_neighbors[d], B.witness_point[d][:, None])
        coef = [torch.randn(v.shape[0], generator=g, dtype=torch.float64).to(dtype) for v in A.values]
        sum((c * v).sum() for c, v in zip(coef, A.values)).backward()
        sum((c * v).sum() for c, v in zip(coef, B.values)).backward()
        assert torch.equal(x.grad, y.grad)


def test_refusals_are_flood_complex_s_and_come_before_any_work(monkeypatch):
    pts = _cloud(3, 40, torch.float32)

    def no_work(*a, **kw):
        raise AssertionError("work done before the arguments were validated")

    import flooder_amd.grad as grad_mod

    monkeypatch.setattr(core, "generate_landmarks", no_work)
    monkeypatch.setattr(core, "_build_complex", no_work)
    monkeypatch.setattr(core, "fps_indices", no_work)
    monkeypatch.setattr(grad_mod, "delaunay_cells", no_work)
    bad_calls = ([dict(neighbors=b) for b in (0, -1, 33, 41, 2.0, "2", None, True)]
                 + [dict(neighbors=k, neighbor_stat="mean") for k in (1, 2)]
                 + [dict(neighbors=2, method="cell"), dict(neighbors=2, neighbor_stat="dtm", method="cell")])
    for kw in bad_calls:
        with pytest.raises((ValueError, TypeError)) as want:
            fa.flood_complex(pts, 10, **kw)
        with pytest.raises(type(want.value)) as got:
            flood_filtration(pts, 10, **kw)
        assert str(got.value) == str(want.value), kw
    with pytest.raises(ValueError, match="number of points") as got:
        flood_filtration(pts[:20], 10, neighbors=21)
    with pytest.raises(ValueError) as want:
        fa.flood_complex(pts[:20], 10, neighbors=21)
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match="nearest point only"):
        flood_filtration(pts, 10, neighbors=2, method="cell")
    with pytest.raises(ValueError):                       # (no exact witnesses: refused at every k)
        flood_filtration(pts, 10, neighbors=2, method="ball")


# ------------------------------------------------------------------------------------------------ brute force
BRUTE = {2: 300, 3: 400}


@pytest.mark.parametrize("k,stat", [(2, "kth"), (2, "dtm"), (5, "kth"), (5, "dtm"), (32, "kth"), (32, "dtm")])
@pytest.mark.parametrize("dim", [2, 3])
def test_witnesses_against_brute_force(dim, k, stat):
    """General position (no exact ties): the witness row is the argmax of the float64 brute-force statistic over the
    simplex's own lattice, the neighbours are the brute-force k nearest of that sample, in order."""
    pts = _cloud(dim, BRUTE[dim], torch.float64, seed=1)
    F = flood_filtration(pts, 12, points_per_edge=5, start_idx=0, neighbors=k, neighbor_stat=stat)
    L = pts[F.landmark_ids]
    for d, simp in enumerate(F.simplices):
        W = gr.lattice(5, d)
        samples = torch.einsum("rk,skd->srd", W, L[simp.long()])
        S, R, _ = samples.shape
        dist = torch.cdist(samples.reshape(-1, dim), pts, compute_mode="donot_use_mm_for_euclid_dist")
        small, ids = torch.topk(dist, k, dim=1, largest=False, sorted=True)
        val = (small[:, -1] if stat == "kth" else small.pow(2).mean(dim=1).sqrt()).reshape(S, R)
        row = gr.lattice_row(W, F.witness_weights[d])
        assert torch.equal(row, val.argmax(dim=1)), f"dimension {d}"
        assert torch.equal(F.witness_neighbors[d], ids.reshape(S, R, k)[torch.arange(S), row]), f"dimension {d}"
        assert torch.allclose(F.values[d], val.max(dim=1).values, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ gradient formula
@pytest.mark.parametrize("k,stat", [(1, "kth"), (2, "dtm"), (5, "kth"), (8, "dtm"), (32, "kth"), (32, "dtm")])
@pytest.mark.parametrize("dim,integer_landmarks", [(2, False), (3, True)])
def test_backward_is_autograd_through_the_witnesses(dim, integer_landmarks, k, stat):
    """Every value rebuilt in torch float64 from the reported witnesses and differentiated by autograd: the same formula
    in the same precision - only the order of at most a few hundred additions per row differs, so 1e-12 of the row's
    sum |g| |w| scale."""
    x = _cloud(dim, BRUTE[dim], torch.float64, seed=2).requires_grad_(True)
    if integer_landmarks:
        lm = 12
    else:
        lm = (x.detach()[::25][:12] + 0.01).clone().requires_grad_(True)     # landmarks off the cloud
    F = flood_filtration(x, lm, points_per_edge=5, start_idx=0, neighbors=k, neighbor_stat=stat)
    g = torch.Generator().manual_seed(5)
    coef = [torch.randn(v.shape[0], generator=g, dtype=torch.float64) for v in F.values]
    sum((c * v).sum() for c, v in zip(coef, F.values)).backward()
    x2 = x.detach().clone().requires_grad_(True)
    l2 = x2.index_select(0, F.landmark_ids) if integer_landmarks else lm.detach().clone().requires_grad_(True)
    vals = kr.values_from_witnesses(F, x2, l2)
    for d in range(len(vals)):
        assert torch.allclose(vals[d], F.values[d].detach(), rtol=1e-12, atol=1e-15)
    sum((c * v).sum() for c, v in zip(coef, vals)).backward()
    # the scale of a row: sum |g| |w| over its contributions (w = 1 for a point, 1 / k per point of a dtm value is
    # bounded by that too)
    scale_p = torch.zeros(x.shape[0], dtype=torch.float64)
    scale_l = torch.zeros(F.landmark_ids.shape[0] if integer_landmarks else lm.shape[0], dtype=torch.float64)
    for d, simp in enumerate(F.simplices):
        nb = F.witness_neighbors[d] if stat == "dtm" else F.witness_point[d][:, None]
        scale_p.index_add_(0, nb.reshape(-1), coef[d].abs().repeat_interleave(nb.shape[1]))
        scale_l.index_add_(0, simp.long().reshape(-1), (coef[d].abs().unsqueeze(1) * F.witness_weights[d].abs()).reshape(-1))
    if integer_landmarks:
        scale_p.index_add_(0, F.landmark_ids, scale_l)
    err = (x.grad - x2.grad).abs().max(dim=1).values
    assert bool((err <= 1e-12 * scale_p).all()), float((err / scale_p.clamp(min=1e-300)).max())
    assert float(x.grad.abs().sum()) > 0
    if not integer_landmarks:
        err = (lm.grad - l2.grad).abs().max(dim=1).values
        assert bool((err <= 1e-12 * scale_l).all()), float((err / scale_l.clamp(min=1e-300)).max())
        assert float(lm.grad.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ envelope
ENVELOPE_H = 1e-7


def envelope_discrepancy(filtration, k, stat, dim=2):
    """|central difference of sum_s c_s flood_complex(x +- h v)[s] - <grad from ``filtration``, v>| / |<grad, v>| on a
    fixed cloud, direction and functional (float64, CPU path; landmarks = fixed rows of the moving cloud)."""
    x = _cloud(dim, BRUTE[dim], torch.float64, seed=4)
    rows = core.fps_indices(x, 12, 0)
    g = torch.Generator().manual_seed(11)
    v = torch.randn(x.shape, generator=g, dtype=torch.float64)
    extra = {} if k == 1 else dict(neighbors=k, neighbor_stat=stat)
    xg = x.clone().requires_grad_(True)
    F = filtration(xg, xg[rows], points_per_edge=5, **extra)
    keys = sorted(F.to_dict())
    c = dict(zip(keys, torch.randn(len(keys), generator=g, dtype=torch.float64).tolist()))
    loss = 0
    for d, simp in enumerate(F.simplices):
        cd = torch.tensor([c[tuple(s)] for s in simp.tolist()], dtype=torch.float64)
        loss = loss + (cd * F.values[d]).sum()
    loss.backward()
    slope = float((xg.grad * v).sum())

    def total(xp):
        fc = fa.flood_complex(xp, xp[rows], points_per_edge=5, **extra)
        assert sorted(fc) == keys
        return sum(c[key] * fc[key] for key in keys)

    fd = (total(x + ENVELOPE_H * v) - total(x - ENVELOPE_H * v)) / (2 * ENVELOPE_H)
    return abs(fd - slope) / abs(slope)


# Measured with this very function (same cloud, h = 1e-7, v, functional; relative to |<grad, v>|):
#   k = 1, flood_filtration of the parent commit (no neighbors argument):   2.213e-10
#   k > 1, this commit:  (2, kth) 3.43e-10   (2, dtm) 6.14e-10   (8, kth) 1.63e-11   (8, dtm) 4.12e-10
#                        (32, kth) 4.99e-10  (32, dtm) 1.17e-09                  (profiles/knn_grad_tests.txt)
# The k > 1 cases are allowed ten times the k = 1 figure: a DTM value sums up to 32 terms and the perturbed clouds
# cross correspondingly more kinks (a change of witness sample or of a neighbour set), each worth O(h) of the slope.
ENVELOPE_K1 = 2.213e-10


@pytest.mark.parametrize("k,stat", [(2, "kth"), (2, "dtm"), (8, "kth"), (8, "dtm"), (32, "kth"), (32, "dtm")])
def test_envelope_against_central_differences(k, stat):
    got = envelope_discrepancy(flood_filtration, k, stat)
    print(f"envelope k={k} {stat}: relative discrepancy {got:.3e} (k = 1 on the parent commit: {ENVELOPE_K1:.3e})")
    assert got <= 10 * ENVELOPE_K1


# ------------------------------------------------------------------------------------------------ ABI
def test_witness_knn_block_has_the_layout_of_the_header():
    """(size and offsets against the header: test_host.py, test_parameter_block_has_the_layout_of_the_header)"""
    cls = _native.WitnessKnn
    for needed in ("size", "abi", "pts_sorted", "n_pts", "dim", "k1", "nodes", "order", "verts", "weights", "R",
                   "n_simplices", "n_queries", "q_simplex", "q_row", "not_found", "k", "stat", "q_stat", "out_ids", "out_d2"):
        assert hasattr(cls, needed), needed
    blk = cls(n_pts=7, R=3, k=5, stat=1)
    assert blk.size == ctypes.sizeof(cls) and blk.abi == 1 and (blk.n_pts, blk.R, blk.k, blk.stat) == (7, 3, 5, 1)
    assert not blk.out_d2
    with pytest.raises(TypeError):
        cls(no_such_field=1)


def test_witness_knn_is_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "flooder_witness_knn(" in header
    assert len(_native.SIGNATURES["flooder_witness_knn"][1]) == 2
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "flooder_witness_knn")
    assert hasattr(_native.load(), "flooder_witness_knn")


def test_witness_knn_refuses_foreign_blocks_and_bad_ranges():
    """Every refusal returns before a pointer is looked at or a kernel is launched (no device needed)."""
    lib = _native.load()
    call = lambda blk: lib.flooder_witness_knn(ctypes.byref(blk), None)
    good = dict(n_pts=100, dim=3, k1=4, R=10, n_simplices=5, n_queries=0, k=8, stat=0)
    assert call(_native.WitnessKnn(**good)) == 0                   # no queries: accepted, nothing launched
    blk = _native.WitnessKnn(**good)
    blk.abi = 2
    assert call(blk) != 0
    blk = _native.WitnessKnn(**good)
    blk.size = ctypes.sizeof(blk) + 8
    assert call(blk) != 0
    blk = _native.WitnessKnn(**good)
    blk.size = 4
    assert call(blk) != 0
    for k in (0, -1, 33):
        assert call(_native.WitnessKnn(**{**good, "k": k})) != 0
        assert b"k must be in 1..32" in lib.flooder_last_error()
    assert call(_native.WitnessKnn(**{**good, "n_pts": 7})) != 0
    assert b"fewer points than k" in lib.flooder_last_error()
    for dim in (0, 1, 9):
        assert call(_native.WitnessKnn(**{**good, "dim": dim})) != 0
        assert b"dim must be in 2..8" in lib.flooder_last_error()
    for stat in (-1, 2):
        assert call(_native.WitnessKnn(**{**good, "stat": stat})) != 0
        assert b"stat must be" in lib.flooder_last_error()
    assert call(_native.WitnessKnn(**{**good, "n_pts": 1 << 31})) != 0
    assert call(_native.WitnessKnn(**{**good, "n_queries": 3})) != 0       # null pointers with work to do
    assert b"null pointer" in lib.flooder_last_error()
    assert call(_native.WitnessKnn(**{**good, "n_queries": -1})) != 0
