"""The k-nearest sweep, its profile and the float64 sweep under option "bvh_grid": one persistent workgroup (its four
waves drain every shard of the work queue through the stealing loop) and 65536 (far more waves than items: most find
nothing).  Word for word against the float64 brute force, on the exact cases of ``variant_cases`` and on the inputs of
``test_gpu_f64_sweep``.  Runs on a real MI355X only (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import f64_reference as fr
import grad_reference as gr
import knn_grad_reference as kr
import test_gpu_f64_sweep as f64_sweep
import variant_cases as vc
from variant_cases import UNWRITTEN, kernel_case, options, same_words

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GRIDS = vc.SET_BY["test_gpu_grid_variants"]["bvh_grid"]
# one two-level and one three-level cloud per dimension: a single tile per simplex and nine
KNN_CASES = [(dim, n, 65 if n == 1025 else 513) for dim in (2, 3, 6) for n in (1025, 70_001)]
KNN_IDS = [f"{dim}d-{n}-R{R}" for dim, n, R in KNN_CASES]
KNN_KS = (2, 32)
PROFILE_COLUMNS = ((1, 0), (5, 0), (5, 1), (32, 1))       # (k, statistic): 0 the k-th distance, 1 the DTM


def _stream():
    return _native.current_stream_ptr(DEV)


def _queue():
    return torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)


def _brute(c, k, stat):
    """The words of column (k, stat): the k-th smallest d2, or the float32 replay of the ascending sum over k."""
    if stat == 0:
        return np.ascontiguousarray(c.asc[:, k - 1]).view(np.uint32)
    return kr.dtm_words(c.asc, k).view(np.uint32)


@pytest.mark.parametrize("dim,n,R", KNN_CASES, ids=KNN_IDS)
@pytest.mark.parametrize("grid", GRIDS)
def test_knn_sweep_words(dim, n, R, grid):
    c = kernel_case(dim, n, R)
    lib, words = _native.load(), c.n_s * R
    with options(bvh_grid=grid):
        for k in KNN_KS:
            for stat in (0, 1):
                out = vc.guarded(words, UNWRITTEN, DEV)
                stats = torch.zeros(4, dtype=torch.int64, device=DEV)
                blk = _native.KnnSweep(k=k, stat=stat, queue=_queue(), out_bits=out, stats=stats, **c.common)
                _native.check(lib.flooder_sweep_knn_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_f32")
                what = ("flooder_sweep_knn_f32", "bvh_grid", grid, k, stat)
                same_words(vc.read_guarded(out, words, what), _brute(c, k, stat), what)
                s = stats.cpu().numpy()
                assert s[0] > 0 and s[1] >= s[0] and s[2] >= c.n_s * ((R + 63) // 64), (what, s.tolist())


@pytest.mark.parametrize("dim,n,R", KNN_CASES, ids=KNN_IDS)
@pytest.mark.parametrize("grid", GRIDS)
def test_knn_profile_words(dim, n, R, grid):
    c = kernel_case(dim, n, R)
    words = len(PROFILE_COLUMNS) * c.n_s * R
    out = vc.guarded(words, UNWRITTEN, DEV)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    blk = _native.KnnProfile(PROFILE_COLUMNS, queue=_queue(), out_bits=out, stats=stats, **c.common)
    with options(bvh_grid=grid):
        _native.check(_native.load().flooder_sweep_knn_profile_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_profile_f32")
    planes = vc.read_guarded(out, words, ("profile", grid)).reshape(len(PROFILE_COLUMNS), c.n_s * R)
    for col, (k, stat) in enumerate(PROFILE_COLUMNS):
        same_words(planes[col], _brute(c, k, stat), ("flooder_sweep_knn_profile_f32", "bvh_grid", grid, k, stat))


F64_CASES = [c for c in f64_sweep.SWEEP_CASES if c[6] < 4]      # (the clouds of 4.3 M points take seconds to index)


@pytest.mark.parametrize("dim,n,dup,ppe,d,n_s,levels,e", F64_CASES)
def test_f64_sweep_words(dim, n, dup, ppe, d, n_s, levels, e):
    """``test_sweep_words_equal_the_brute_force`` under the two grids: its inputs, its reference, its guarded call."""
    P, V, _ = fr.exact_case(dim, n, dup, d, n_s, 2 ** e, f64_sweep._seed(dim, n, ppe))
    W = gr.lattice(ppe, d)
    fr.assert_exact_inputs_f64(P, V, ppe)
    index, rows, tv, tw, ref, _, _ = f64_sweep._prepare(P, V, W, ppe)
    want = ref.view(np.int64)
    for grid in GRIDS:
        with options(bvh_grid=grid):
            got = f64_sweep._sweep(rows, index, tv, tw, n_s)
        assert np.array_equal(got, want), (grid, np.argwhere(got != want)[:5].tolist())
