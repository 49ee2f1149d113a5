"""The robust filtration by mass on the MI355X: ``distance_to_measure`` bit for bit against ``neighbor_distance`` and
``nearest_neighbors`` up to k = 32, ``flood_complex(neighbor_mass=m)`` at k = 40 and 300 bit for bit against the brute
force on an exact lattice cloud and within the parity gate against the CPU path on float clouds, its vertex values
against ``distance_to_measure``, simplex shards, and what the device path refuses."""

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import core, distributed

import grad_reference as gr
import knn_grad_reference as kr
import knn_wide_reference as kw
from helpers import assert_close_filtration

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
STATS = ("kth", "dtm")


def _float_cloud(dim):
    g = torch.Generator().manual_seed(11 * dim)
    n = 4000 if dim == 3 else 3000
    base = torch.randn(n - 500, dim, generator=g)
    pts = torch.cat([base, base[:500]])[torch.randperm(n, generator=g)]          # 500 points twice
    qs = torch.cat([pts[:100], 1.5 * torch.randn(600, dim, generator=g)])
    return pts.to(DEV), qs.to(DEV)


@pytest.mark.parametrize("dim", [3, 6])
def test_up_to_32_the_words_of_the_register_family(dim):
    tp, tq = _float_cloud(dim)
    index = core.PointIndex(tp)
    for k in (1, 7, 32):
        ids, dist = fa.nearest_neighbors(tp, tq, k, index=index)
        ids2, dist2 = fa.nearest_neighbors(tp, tq, k, squared=True, index=index)
        for stat in STATS:
            for squared in (False, True):
                want = fa.neighbor_distance(tp, tq, k, stat, squared=squared, index=index)
                got = fa.distance_to_measure(tp, tq, neighbors=k, neighbor_stat=stat, squared=squared, index=index)
                assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32)), (k, stat)
                value, w_ids, w_dist = fa.distance_to_measure(tp, tq, neighbors=k, neighbor_stat=stat, squared=squared,
                                                              return_neighbors=True, index=index)
                assert torch.equal(value, got) and w_ids.dtype == torch.int64 and torch.equal(w_ids, ids)
                assert torch.equal(w_dist.view(torch.int32), (dist2 if squared else dist).view(torch.int32))
    # by mass, the cloud's own points, no queries
    n = tp.shape[0]
    own = fa.distance_to_measure(tp, None, 7 / n)
    assert torch.equal(own, fa.neighbor_distance(tp, None, 7, "dtm"))
    empty = fa.distance_to_measure(tp, tq[:0], 0.01, return_neighbors=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, core.mass_neighbors(0.01, n)) and empty[1].dtype == torch.int64


def test_wide_values_against_the_cpu_path():
    tp, tq = _float_cloud(3)
    for k in (40, 300, 1024):
        for stat in STATS:
            got, ids, dist = fa.distance_to_measure(tp, tq, neighbors=k, neighbor_stat=stat, return_neighbors=True)
            want = fa.distance_to_measure(tp.cpu(), tq.cpu(), neighbors=k, neighbor_stat=stat)
            assert_close_filtration(got.cpu().numpy(), want.numpy(), tp.cpu().numpy(), (k, stat))
            # the neighbours realise the distances, ascending by (distance, id)
            d = (tq.double().unsqueeze(1) - tp.double()[ids]).norm(dim=2)
            assert_close_filtration(dist.cpu().numpy(), d.cpu().numpy(), tp.cpu().numpy(), (k, "neighbours"))
            _, ids2, d2 = fa.distance_to_measure(tp, tq, neighbors=k, neighbor_stat=stat, squared=True,
                                                 return_neighbors=True)
            assert torch.equal(ids2, ids) and bool((dist[:, 1:] >= dist[:, :-1]).all())
            assert bool(((d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (ids[:, 1:] > ids[:, :-1]))).all())


def _integer_cloud(n, dim, hi, seed):
    """n integer points of [0, hi)^dim as float32, every point present twice, the copies anywhere."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, hi, (n // 2, dim), generator=g).to(torch.float32)
    return torch.cat([base, base])[torch.randperm(2 * (n // 2), generator=g)]


@pytest.mark.parametrize("stat", STATS)
def test_exact_lattice_cloud_bit_for_bit(stat):
    """Integer cloud, dyadic lattice: float32 is exact and the brute force is THE answer - with the statistic in the wide
    kernel's own arithmetic (the strided sum replayed in numpy); k = 40 also through ``exact_knn_faces`` (up to 64 the
    strided sum is the sequential one)."""
    n, ppe = 3000, 5
    pts = _integer_cloud(n, 3, 64, seed=23)
    tp = pts.to(DEV)
    lms = fa.generate_landmarks(tp, 30, start_idx=0)
    gr.assert_exact_inputs(pts, lms.cpu(), ppe)
    for k in (40, 300):
        mass = k / n
        assert core.mass_neighbors(mass, n) == k
        fc = fa.flood_complex(tp, lms, points_per_edge=ppe, neighbor_mass=mass, neighbor_stat=stat)
        assert fc == fa.flood_complex(tp, lms, points_per_edge=ppe, neighbor_mass=mass, neighbor_stat=stat)   # run twice
        ref = kw.exact_flood_reference(fc, tp, lms, ppe, k, stat)
        assert len(fc) > 200
        bad = [key for key in fc if np.float32(fc[key]) != ref[key] or float(np.float32(fc[key])) != fc[key]]
        assert not bad, (k, stat, len(bad), bad[:5], [(fc[key], float(ref[key])) for key in bad[:5]])
        if k <= 64:
            by_dim = {}
            for key in sorted(fc):
                by_dim.setdefault(len(key) - 1, []).append(key)
            simplices = [torch.as_tensor(by_dim[d], device=DEV) for d in sorted(by_dim)]
            for d, E in enumerate(kr.exact_knn_faces(simplices, tp, lms, ppe, k, stat)):
                want = E.smax.double().sqrt().to(torch.float32).cpu().numpy()
                assert np.array_equal(np.array([fc[key] for key in by_dim[d]], dtype=np.float32), want), (k, stat, d)
        # the vertex values are distance_to_measure at the landmarks, bit for bit
        at_lms = fa.distance_to_measure(tp, lms, mass, neighbor_stat=stat).cpu().numpy()
        assert np.array_equal(np.array([fc[(i,)] for i in range(lms.shape[0])], dtype=np.float32), at_lms)


@pytest.mark.parametrize("dim", [3, 6])
def test_float_cloud_against_the_cpu_path(dim):
    tp, _ = _float_cloud(dim)
    lms = fa.generate_landmarks(tp, 14, start_idx=0)
    n = tp.shape[0]
    for k, stat in ((40, "dtm"), (300, "dtm"), (300, "kth")):
        kwargs = dict(points_per_edge=5, max_dimension=2, neighbor_mass=k / n, neighbor_stat=stat)
        fc = fa.flood_complex(tp, lms, **kwargs)
        ref = fa.flood_complex(tp.cpu(), lms.cpu(), **kwargs)
        assert set(fc) == set(ref)
        keys = sorted(fc)
        assert_close_filtration([fc[key] for key in keys], [ref[key] for key in keys], tp.cpu().numpy(), (dim, k, stat))
        at_lms = fa.distance_to_measure(tp, lms, k / n, neighbor_stat=stat).cpu().numpy()
        assert np.array_equal(np.array([fc[(i,)] for i in range(14)], dtype=np.float32), at_lms), (dim, k, stat)


def test_simplex_shards_reduce_to_the_whole_dict():
    tp, _ = _float_cloud(3)
    lms = fa.generate_landmarks(tp, 14, start_idx=0)
    kwargs = dict(points_per_edge=5, neighbor_mass=0.05)
    assert core.mass_neighbors(0.05, tp.shape[0]) == 200
    whole = fa.flood_complex(tp, lms, **kwargs)
    halves = []
    for rank in (0, 1):       # one buffer per dimension pass: this rank's rows, +inf elsewhere
        got = []
        fa.flood_complex(tp, lms, simplex_shard=(rank, 2), face_reduce_hook=lambda face, got=got: got.append(face.clone()),
                         **kwargs)
        halves.append(got)
    merged = iter([torch.minimum(a, b) for a, b in zip(*halves)])
    both = fa.flood_complex(tp, lms, simplex_shard=(1, 2), face_reduce_hook=lambda face: face.copy_(next(merged)), **kwargs)
    assert both == whole
    assert distributed.flood_complex_sharded(tp, lms, **kwargs) == whole


def test_device_refusals():
    tp, _ = _float_cloud(3)
    lms = tp[:10].clone()
    with pytest.raises(ValueError, match="neighbor_mass on ROCm tensors needs float32"):
        fa.flood_complex(tp.double(), lms.double(), points_per_edge=3, neighbor_mass=0.05)
    with pytest.raises(ValueError, match="distance_to_measure on ROCm tensors needs float32"):
        fa.distance_to_measure(tp.double(), None, 0.05)
    nine = torch.randn(500, 9, device=DEV)
    with pytest.raises(ValueError, match="neighbor_mass on ROCm tensors needs ambient dimension 2 to 8"):
        fa.flood_complex(nine, nine[:12].clone(), points_per_edge=3, neighbor_mass=0.2)
    with pytest.raises(ValueError, match="distance_to_measure on ROCm tensors needs ambient dimension 2 to 8"):
        fa.distance_to_measure(nine, None, 0.2)
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match=f"neighbor_mass needs the tree sweep: method '{method}'"):
            fa.flood_complex(tp, lms, points_per_edge=3, neighbor_mass=0.05, method=method)
    with pytest.raises(ValueError, match=r"above KNN_WIDE_MAX = 1024 .*largest mass that fits this cloud is 0\.256"):
        fa.flood_complex(tp, lms, points_per_edge=3, neighbor_mass=0.5)
    with pytest.raises(ValueError, match=r"above KNN_WIDE_MAX = 1024"):
        fa.distance_to_measure(tp, None, 0.5)
    hook = lambda t: None   # noqa: E731
    for name in ("reduce_hook", "neighbor_reduce_hook"):
        with pytest.raises(ValueError, match="neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook"):
            fa.flood_complex(tp, lms, points_per_edge=3, neighbor_mass=0.05, **{name: hook})
    with pytest.raises(ValueError, match="neighbor_mass cannot be combined with shard_blocks=True"):
        fa.flood_complex(tp, lms, points_per_edge=3, neighbor_mass=0.05, shard_blocks=True, simplex_shard=(0, 2))
