"""``distance_to_weighted_measure`` and ``voxel_measure`` on ROCm tensors: the values of the torus coreset against the
CPU float64 path within the float32 gate of the sibling tests, equal counts, the unit-mass identity with
``distance_to_measure`` bit for bit, the coreset on the device against the coreset on the host, the README's recipe end
to end, groups of queries, and the float64 refusal."""

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import core

import knn_mass_reference as km
from helpers import assert_close_filtration

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32) if t.dtype is torch.float32 else t


def test_torus_coreset_against_the_cpu_float64_path():
    t = km.torus_coreset()
    sites, mu, qs, m = t["sites"], t["masses"], t["queries"], t["mass"]
    for stat in ("dtm", "kth"):
        want, w_ids, w_dist, w_count = fa.distance_to_weighted_measure(sites.double(), mu.double(), qs.double(), mass=m,
                                                                       neighbor_stat=stat, return_neighbors=True)
        got, ids, dist, count = fa.distance_to_weighted_measure(sites.to(DEV), mu.to(DEV), qs.to(DEV), mass=m,
                                                                neighbor_stat=stat, return_neighbors=True)
        assert got.dtype is torch.float32 and got.device.type == "cuda" and ids.dtype is torch.int64
        assert ids.shape == dist.shape == (qs.shape[0], 1024) and count.dtype is torch.int64
        assert bool(torch.isfinite(got).all())
        err = assert_close_filtration(got.cpu().numpy(), want.numpy(), sites.numpy(), stat)
        print(f"{stat}: worst abs err {err:.3g}, neighbours median {int(count.median())} max {int(count.max())}")
        assert torch.equal(count.cpu(), w_count)
        # ... and within the derived bound of the squared "dtm" word plus a float32 rounding of every coordinate
        # difference (2 * 2^-24 relative on a squared distance, 3 more for its two fmas and the root's square)
        if stat == "dtm":
            sq = fa.distance_to_weighted_measure(sites.to(DEV), mu.to(DEV), qs.to(DEV), mass=m, squared=True)
            rel = (sq.cpu().double() - want ** 2).abs() / (want ** 2)
            assert float(rel.max()) <= float((km.dtm_bound(count.cpu().numpy()) + 5 * 2.0 ** -24).max())
        plain = fa.distance_to_weighted_measure(sites.to(DEV), mu.to(DEV), qs.to(DEV), mass=m, neighbor_stat=stat)
        assert torch.equal(_bits(plain), _bits(got))
        listed = torch.arange(1024, device=DEV).unsqueeze(0) < count.unsqueeze(1)
        assert bool((ids[~listed] == -1).all()) and bool(torch.isinf(dist[~listed]).all()) and bool((ids[listed] >= 0).all())


def test_unit_masses_are_distance_to_measure_bit_for_bit():
    g = torch.Generator().manual_seed(4)
    pts, qs = torch.randn(3000, 3, generator=g).to(DEV), (1.5 * torch.randn(500, 3, generator=g)).to(DEV)
    ones = torch.ones(3000, device=DEV)
    for k in (1, 40, 65, 1000):
        for stat in ("dtm", "kth"):
            want, w_ids, w_dist = fa.distance_to_measure(pts, qs, neighbors=k, neighbor_stat=stat, return_neighbors=True)
            got, ids, dist, count = fa.distance_to_weighted_measure(pts, ones, qs, mass=k / 3000, neighbor_stat=stat,
                                                                    return_neighbors=True)
            assert torch.equal(_bits(got), _bits(want)) and bool((count == k).all()), (k, stat)
            assert torch.equal(ids[:, :k], w_ids) and torch.equal(_bits(dist[:, :k].contiguous()), _bits(w_dist))
    # not reached: +inf, documented and not raised
    v, ids, _, count = fa.distance_to_weighted_measure(pts, ones, qs, mass=65 / 3000, max_neighbors=64, return_neighbors=True)
    assert ids.shape == (500, 64) and bool(torch.isinf(v).all()) and bool((count == 64).all()) and bool((ids >= 0).all())
    # the sites themselves as queries; no queries
    own = fa.distance_to_weighted_measure(pts, ones, mass=7 / 3000)
    assert torch.equal(_bits(own), _bits(fa.distance_to_measure(pts, neighbors=7)))
    e = fa.distance_to_weighted_measure(pts, ones, qs[:0], mass=0.5, return_neighbors=True)
    assert [tuple(x.shape) for x in e] == [(0,), (0, 1024), (0, 1024), (0,)] and e[0].device.type == "cuda"


def test_voxel_measure_on_the_device_is_the_host_result():
    pts = km.torus_coreset()["points"]
    for cell in (0.1, 0.37):
        sites, mu = fa.voxel_measure(pts, cell)
        d_sites, d_mu = fa.voxel_measure(pts.to(DEV), cell)
        assert d_sites.device.type == "cuda" and d_sites.dtype is torch.float32 and d_mu.dtype is torch.float32
        assert torch.equal(d_mu.cpu(), mu) and d_sites.shape == sites.shape            # counts and order exact
        ulp = np.spacing(np.abs(sites.numpy()))
        assert np.all(np.abs(d_sites.cpu().numpy().astype(np.float64) - sites.numpy().astype(np.float64)) <= ulp)
        again = fa.voxel_measure(pts.to(DEV), cell)
        assert torch.equal(again[0], d_sites) and torch.equal(again[1], d_mu)


def test_recipe_end_to_end():
    pts = km.torus_coreset()["points"].to(DEV)
    sites, mu = fa.voxel_measure(pts, 0.1)
    w = fa.distance_to_weighted_measure(sites, mu, queries=pts, mass=0.02)
    assert w.shape == (pts.shape[0],) and bool(torch.isfinite(w).all())
    lms = fa.generate_landmarks(pts, 40, start_idx=0)
    fc = fa.flood_complex(pts, lms, point_weights=w)
    at = fa.power_distance(pts, w, lms)
    assert np.array_equal(np.array([fc[(i,)] for i in range(lms.shape[0])]), at.cpu().numpy().astype(np.float64))
    assert len(fc) > lms.shape[0]


def test_groups_give_the_words_of_one_group(monkeypatch):
    t = km.torus_coreset()
    sites, mu, qs = t["sites"].to(DEV), t["masses"].to(DEV), t["queries"][:700].to(DEV)
    whole = fa.distance_to_weighted_measure(sites, mu, qs, mass=0.01, return_neighbors=True, max_neighbors=256, squared=True)
    value = fa.distance_to_weighted_measure(sites, mu, qs, mass=0.01, max_neighbors=256, squared=True)
    seen, sort = [], core._sorted_sample_order

    def counted(lib, st, index, verts, *rest):
        seen.append(verts.shape[0])
        return sort(lib, st, index, verts, *rest)

    monkeypatch.setattr(core, "_sorted_sample_order", counted)
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", (32 + 8 * 256) * 200)
    grouped = fa.distance_to_weighted_measure(sites, mu, qs, mass=0.01, return_neighbors=True, max_neighbors=256, squared=True)
    assert seen == [200, 200, 200, 100]
    for got, want in zip(grouped, whole):
        assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))
    del seen[:]
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", 32 * 200)
    assert torch.equal(_bits(fa.distance_to_weighted_measure(sites, mu, qs, mass=0.01, max_neighbors=256, squared=True)),
                       _bits(value))
    assert seen == [200, 200, 200, 100]
    assert torch.equal(_bits(value), _bits(whole[0]))


def test_refusals_on_the_device():
    pts, mu = torch.rand(100, 3, device=DEV), torch.ones(100, device=DEV)
    with pytest.raises(ValueError, match="distance_to_weighted_measure on ROCm tensors needs float32: the k-nearest sweep "
                                         "has no float64 kernel"):
        fa.distance_to_weighted_measure(pts.double(), mu.double(), mass=0.5)
    with pytest.raises(ValueError, match="ambient dimension 2 to 8"):
        fa.distance_to_weighted_measure(torch.rand(100, 9, device=DEV), mu, mass=0.5)
    with pytest.raises(ValueError, match=r"point_masses\.device"):
        fa.distance_to_weighted_measure(pts, mu.cpu(), mass=0.5)
    with pytest.raises(RuntimeError, match=r"queries\.device"):
        fa.distance_to_weighted_measure(pts, mu, pts.cpu(), mass=0.5)
