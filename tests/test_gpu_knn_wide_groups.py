"""``distance_to_measure`` on ROCm tensors in GROUPS of queries: with ``core.SORTED_WORKSPACE_BYTES`` below what all
queries need, the query driver sorts and sweeps them group by group (``flooder_knn_wide_f32`` with ``sample_order``), and
the values, the ids and the d2 words are those of the single group, bit for bit - with neighbours ((28 + 8 k) bytes per
query) and without (28).  At k = 32 the grouped wide result is that of the register family.  The register forms have
this test in ``test_gpu_knn_sorted`` and ``test_gpu_knn_ids``.

3-D, 3000 points, 700 queries that are no cloud points, groups of 200: four groups, the last one short."""

import functools

import pytest
import torch

import flooder_amd as fa
from flooder_amd import core

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
Q, GROUP = 700, 200


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(33)
    return torch.randn(3000, 3, generator=g).to(DEV), (1.5 * torch.randn(Q, 3, generator=g)).to(DEV)


def _count_groups(monkeypatch):
    """-> a list that gets one entry per group the driver sorts."""
    seen, sort = [], core._sorted_sample_order

    def counted(lib, st, index, verts, *rest):
        seen.append(verts.shape[0])
        return sort(lib, st, index, verts, *rest)

    monkeypatch.setattr(core, "_sorted_sample_order", counted)
    return seen


def _bits(t):
    return t if t.dtype is torch.int64 else t.view(torch.int32)


@pytest.mark.parametrize("k", [33, 200])
def test_groups_give_the_words_of_one_group(k, monkeypatch):
    pts, qs = _inputs()
    whole = fa.distance_to_measure(pts, qs, neighbors=k, return_neighbors=True, squared=True)
    value = fa.distance_to_measure(pts, qs, neighbors=k, squared=True)
    assert whole[1].shape == whole[2].shape == (Q, k) and torch.equal(_bits(value), _bits(whole[0]))
    seen = _count_groups(monkeypatch)
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", (28 + 8 * k) * GROUP)
    grouped = fa.distance_to_measure(pts, qs, neighbors=k, return_neighbors=True, squared=True)
    assert seen == [200, 200, 200, 100]
    for got, want in zip(grouped, whole):           # values, ids, d2 words
        assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))
    del seen[:]
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", 28 * GROUP)
    assert torch.equal(_bits(fa.distance_to_measure(pts, qs, neighbors=k, squared=True)), _bits(value))
    assert seen == [200, 200, 200, 100]


def test_grouped_wide_sweep_at_32_is_the_register_family(monkeypatch):
    pts, qs = _inputs()
    ids, dist = fa.nearest_neighbors(pts, qs, 32, squared=True)
    dtm = fa.neighbor_distance(pts, qs, 32, "dtm", squared=True)
    seen = _count_groups(monkeypatch)
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", (28 + 8 * 32) * GROUP)
    value, wide_ids, wide_dist = fa.distance_to_measure(pts, qs, neighbors=32, return_neighbors=True, squared=True)
    assert seen == [200, 200, 200, 100]
    assert torch.equal(wide_ids, ids) and torch.equal(_bits(wide_dist), _bits(dist)) and torch.equal(_bits(value), _bits(dtm))
