"""The sorted-sample sweep (csrc/flood_sorted.hip) under its options, word for word against the float64 brute force on
the exact 3-D and 6-D cases of ``variant_cases``: "sorted_ks" 2 (sweep_sorted_kernel<DIM, 2, false>: tiles of 128
samples, and with them the tile shares of the sharded form), "sorted_batch_pct" and "sorted_blocks"; and end to end on
a 6-D golden input, whole and in three tile shards.  Runs on a real MI355X only (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import variant_cases as vc
from helpers import get_options, load_e2e
from variant_cases import INF_BITS, UNWRITTEN, kernel_case, options, same_words

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MINE = vc.SET_BY["test_gpu_sorted_variants"]
SORTED_CASES = [(dim, n, R) for dim, n, R in vc.CASE_R if dim in (3, 6)]
SORTED_IDS = [f"{dim}d-{n}-R{R}" for dim, n, R in SORTED_CASES]


def _stream():
    return _native.current_stream_ptr(DEV)


def _order(c):
    """The sample order as ``test_sorted_sweep_words`` builds it: keys by flooder_sample_keys_f32, sorted by
    flooder_index_sort; checked to be a permutation."""
    if getattr(c, "order", None) is not None:
        return c.order
    lib, st = _native.load(), _stream()
    n_samples = c.n_s * c.R
    keys, keys_sorted, order = (torch.empty(n_samples, dtype=torch.int32, device=DEV) for _ in range(3))
    tmp_bytes = int(lib.flooder_index_sort_bytes(n_samples))
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=DEV)
    _native.check(lib.flooder_sample_keys_f32(_native.ptr(c.verts), _native.ptr(c.weights), c.k1, c.R, c.n_s, c.dim,
                                              _native.ptr(c.index.box), _native.ptr(keys), st), "flooder_sample_keys_f32")
    _native.check(lib.flooder_index_sort(_native.ptr(keys), n_samples, int(lib.flooder_sample_key_bits(c.dim)),
                                         _native.ptr(keys_sorted), _native.ptr(order), _native.ptr(tmp), tmp_bytes, st),
                  "flooder_index_sort")
    torch.cuda.synchronize()
    assert np.array_equal(np.sort(order.cpu().numpy()), np.arange(n_samples)), "the sample order is no permutation"
    ks = keys_sorted.cpu().numpy().view(np.uint32)
    assert (ks[1:] >= ks[:-1]).all() and ks[0] != ks[-1], "the keys do not tell the samples apart"
    c.order = order
    return order


def _minima(c, what):
    words = c.n_s * c.R
    d2 = vc.guarded(words, INF_BITS, DEV)
    queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
    blk = _native.SortedSweep(**c.common, sample_order=_order(c), queue=queue, out_d2=d2)
    _native.check(_native.load().flooder_sorted_minima(ctypes.byref(blk), _stream()), "flooder_sorted_minima")
    same_words(vc.read_guarded(d2, words, what), c.want, what)


@pytest.mark.parametrize("dim,n,R", SORTED_CASES, ids=SORTED_IDS)
def test_sorted_minima_words_under_every_option(dim, n, R):
    """One or two samples per lane, batches of one leaf, of the default's width and of every leaf whose bound is below
    a thousand times the nearest one, all workgroups a CU holds or one."""
    c = kernel_case(dim, n, R)
    lib = _native.load()
    default = get_options(lib, b"sorted_ks", b"sorted_batch_pct", b"sorted_blocks")
    for ks in sorted({default[b"sorted_ks"], *MINE["sorted_ks"]}):
        for pct in sorted({default[b"sorted_batch_pct"], *MINE["sorted_batch_pct"]}):
            for blocks in sorted({default[b"sorted_blocks"], *MINE["sorted_blocks"]}):
                with options(sorted_ks=ks, sorted_batch_pct=pct, sorted_blocks=blocks):
                    assert int(lib.flooder_sorted_tile_samples()) == 64 * ks
                    _minima(c, ("flooder_sorted_minima", "sorted_ks", ks, "sorted_batch_pct", pct, "sorted_blocks", blocks))


@pytest.mark.parametrize("dim,n,R", SORTED_CASES, ids=SORTED_IDS)
@pytest.mark.parametrize("ks", [1, 2])
def test_sorted_shards_of_three_ranks(dim, n, R, ks):
    """flooder_sweep_bvh_sorted_shard_f32, world 3: rank r writes the samples of tiles [T r / 3, T (r + 1) / 3) of the
    sorted order - tiles of flooder_sorted_tile_samples() samples, T of them - and no other word; what it writes is
    exact; the three sets are disjoint and together all samples."""
    c = kernel_case(dim, n, R)
    lib, words, world = _native.load(), c.n_s * R, 3
    order = _order(c).cpu().numpy().astype(np.int64)
    written = np.zeros(words, dtype=np.int32)
    with options(sorted_ks=ks):
        per_tile = int(lib.flooder_sorted_tile_samples())
        assert per_tile == 64 * ks
        n_tiles = (words + per_tile - 1) // per_tile
        for rank in range(world):
            out = vc.guarded(words, UNWRITTEN, DEV)
            queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
            _native.check(lib.flooder_sweep_bvh_sorted_shard_f32(
                _native.ptr(c.index.pts), c.index.n, dim, _native.ptr(c.index.nodes), _native.ptr(c.verts),
                _native.ptr(c.weights), c.k1, R, c.n_s, _native.ptr(_order(c)), rank, world, _native.ptr(queue),
                _native.ptr(out), None, _stream()), "flooder_sweep_bvh_sorted_shard_f32")
            got = vc.read_guarded(out, words, ("shard", rank))
            mine = np.zeros(words, dtype=bool)
            mine[order[n_tiles * rank // world * per_tile: n_tiles * (rank + 1) // world * per_tile]] = True
            assert np.array_equal(got.view(np.int32) != UNWRITTEN, mine), f"rank {rank} did not write exactly its tiles' samples"
            same_words(got[mine], c.want[mine], ("shard", rank, "sorted_ks", ks))
            written += mine
    assert (written == 1).all(), "the ranks' samples are not a partition of all samples"


# ------------------------------------------------------------------------------------------------ end to end
def _golden():
    z, kw, _ = load_e2e("gauss6d_maxdim2")
    return z, kw, torch.as_tensor(z["points"], device=DEV), torch.as_tensor(z["landmarks"], device=DEV)


def test_sorted_ks_2_end_to_end(monkeypatch):
    z, kw, pts, lms = _golden()
    torch.manual_seed(int(z["weight_seed"]))
    base = fa.flood_complex(pts, lms, **kw)
    monkeypatch.setattr(core, "BVH_SORTED_MIN_SAMPLES", 0)
    with options(sorted_ks=2):
        torch.manual_seed(int(z["weight_seed"]))
        got = fa.flood_complex(pts, lms, method="bvh", **kw)
        assert core.bvh_sorts_samples(pts.shape[1], core.LAST_STATS.top_simplices, core.LAST_STATS.samples_per_simplex)
    assert got == base


def test_sorted_ks_2_tile_shards_min_reduce(monkeypatch):
    """As ``test_tile_shards_min_reduce``: three ranks take a third of the 128-sample tiles each and hand the hook the
    negated maxima over their own samples; the MIN of the three buffers is the whole call."""
    z, kw, pts, lms = _golden()
    torch.manual_seed(int(z["weight_seed"]))
    base = fa.flood_complex(pts, lms, **kw)
    monkeypatch.setattr(core, "BVH_SORTED_SAMPLES", True)
    monkeypatch.setattr(core, "BVH_SORTED_MIN_SAMPLES", 0)

    def call(**more):
        torch.manual_seed(int(z["weight_seed"]))
        return fa.flood_complex(pts, lms, method="bvh", **kw, **more)

    with options(sorted_ks=2):
        bufs = {}
        for r in range(3):
            call(simplex_shard=(r, 3), face_reduce_hook=lambda buf, r=r: bufs.setdefault(r, []).append(buf.clone()))
        passes = len(bufs[0])
        assert passes > 0 and all(len(bufs[r]) == passes for r in range(3))
        merged = [torch.minimum(torch.minimum(bufs[0][i], bufs[1][i]), bufs[2][i]) for i in range(passes)]
        assert all(bool(torch.isfinite(m).all()) for m in merged)
        assert all(bool((bufs[r][-1] <= 0).all()) for r in range(3)), "tile shards hand over negated values"
        assert any(not torch.equal(bufs[0][i], bufs[1][i]) for i in range(passes))
        turn = iter(merged)
        out = call(simplex_shard=(0, 3), face_reduce_hook=lambda buf: buf.copy_(next(turn)))
    assert out == base
