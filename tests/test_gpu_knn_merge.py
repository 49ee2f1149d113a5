"""``flooder_knn_merge_f32`` alone against numpy: the k-th smallest of the W * k words of a cell and the float32 replay
of the ascending mean, word for word; the order of the lists does not matter; guard words stay; refusals."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64                    # words behind out_bits
SENTINEL = 0x5EA1ED
INF = np.float32(np.inf)

WS = (1, 2, 3, 8)
KS = (1, 2, 3, 5, 8, 16, 17, 32)
NS = (1, 63, 64, 65, 1000)


def _lists(W, k, n, rng, shift):
    """(W, k, n) float32, ascending over axis 1.  Cell c of wave c // 64: every third wave holds rank-disjoint lists
    (list w lies above list w - 1: the wave leaves every further list at its first plane); elsewhere the cell's kind is
    (c + shift) % 6 - random, heavy ties, the same list on every rank, 1 .. k - 1 trailing +inf pads, one rank all +inf,
    many zeros."""
    v = rng.random((W, k, n), dtype=np.float32) * np.float32(4.0)
    cells = np.arange(n)
    kind = (cells + shift) % 6
    kind[(cells // 64) % 3 == 2] = 6
    ties = rng.integers(0, 4, size=(W, k, n)).astype(np.float32) * np.float32(0.5)
    v = np.where(kind == 1, ties, v)
    v = np.where(kind == 5, np.where(rng.random((W, k, n)) < 0.6, np.float32(0), v), v)
    v = np.where(kind == 6, v + np.float32(4.0) * np.arange(W, dtype=np.float32)[:, None, None], v)
    v = np.where(kind == 2, v[:1], v)
    v = np.sort(v, axis=1)
    if k > 1:   # lists that end in 1 .. k - 1 pads (a shard with fewer than k points), another count on every rank
        pads = 1 + (cells[None, :] + 3 * np.arange(W)[:, None]) % (k - 1)                 # (W, n)
        padded = np.arange(k)[None, :, None] >= (k - pads)[:, None, :]
        v = np.where((kind == 3) & padded, INF, v)
    v = np.where((kind == 4) & (np.arange(W)[:, None, None] == (cells % W)), INF, v)      # one rank's list all +inf
    assert (v[:, 1:] >= v[:, :-1]).all()
    return np.ascontiguousarray(v.astype(np.float32))


def _expected(lists, k, stat):
    W, _, n = lists.shape
    asc = np.sort(lists.transpose(2, 0, 1).reshape(n, W * k), axis=1)[:, :k]
    if stat == 0:
        return asc[:, k - 1].view(np.uint32)
    acc = asc[:, 0].copy()
    with np.errstate(over="ignore"):
        for i in range(1, k):   # ascending, smallest first, one float32 rounding per addition
            acc = (acc + asc[:, i]).astype(np.float32)
        return (acc / np.float32(k)).astype(np.float32).view(np.uint32)


def _merge(lists_dev, k, stat, n):
    lib = _native.load()
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    blk = _native.KnnMerge(lists=lists_dev, n_cells=n, n_lists=lists_dev.shape[0], k=k, stat=stat, out_bits=out)
    _native.check(lib.flooder_knn_merge_f32(ctypes.byref(blk), _native.current_stream_ptr(DEV)), "flooder_knn_merge_f32")
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all(), "guard words behind out_bits were written"
    return got[:n].view(np.uint32)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("W", WS)
def test_merge_is_the_k_best_of_the_union_word_for_word(W, k):
    rng = np.random.default_rng(1000 * W + k)
    for n in NS:
        for shift in (range(6) if n < 6 else (0,)):
            lists = _lists(W, k, n, rng, shift)
            dev = torch.as_tensor(lists.view(np.int32), device=DEV)
            perm = torch.as_tensor(rng.permutation(W), device=DEV)
            for stat in (0, 1):
                want = _expected(lists, k, stat)
                got = _merge(dev, k, stat, n)
                assert np.array_equal(got, want), (W, k, n, stat, np.flatnonzero(got != want)[:8])
                # a permutation of the ranks changes nothing
                assert np.array_equal(_merge(dev[perm].contiguous(), k, stat, n), want), (W, k, n, stat, "permuted")


def test_generated_lists_hold_every_kind():
    rng = np.random.default_rng(5)
    v = _lists(3, 8, 1000, rng, 0)
    assert np.isinf(v).all(axis=1).any() and (np.isinf(v).sum(axis=1) == 7).any() and (np.isinf(v).sum(axis=1) == 1).any()
    assert (v[0] == v[1]).all(axis=0).any() and (v == 0).any()
    assert (v[1, 0, 128:192] >= v[0, -1, 128:192]).all()          # a wave of rank-disjoint lists
    assert len(np.unique(v[:, :, 1])) < 8                         # heavy ties


def test_plane_offsets_past_2_to_the_31_words():
    """W * k * n > 2**31 words: the plane offsets are 64-bit.  Lists by formula, checked on cells at both ends and in
    the middle against the same numpy model."""
    W, k = 2, 32
    n = (1 << 25) + 77
    assert W * k * n > 1 << 31
    cells = torch.arange(n, device=DEV, dtype=torch.int32)
    a = (cells % 97).to(torch.float32)
    b = (cells % 5).to(torch.float32) * 0.25
    lists = torch.empty((W, k, n), dtype=torch.int32, device=DEV)
    for w in range(W):
        for j in range(k):
            lists[w, j] = (a + float(j) + (b if w else 0.0)).view(torch.int32)
    pick = torch.cat([torch.arange(0, 1000), torch.arange(n // 2 - 500, n // 2 + 500), torch.arange(n - 1000, n)]).to(DEV)
    sub = lists[:, :, pick].cpu().numpy().view(np.float32)
    lib = _native.load()
    for stat in (0, 1):
        out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        blk = _native.KnnMerge(lists=lists, n_cells=n, n_lists=W, k=k, stat=stat, out_bits=out)
        _native.check(lib.flooder_knn_merge_f32(ctypes.byref(blk), _native.current_stream_ptr(DEV)), "flooder_knn_merge_f32")
        assert bool((out[n:] == SENTINEL).all())
        assert np.array_equal(out[pick].cpu().numpy().view(np.uint32), _expected(sub, k, stat)), stat


def test_foreign_blocks_and_parameters_out_of_range_are_refused():
    lib = _native.load()
    lists = torch.zeros((2, 4, 8), dtype=torch.int32, device=DEV)
    out = torch.full((8 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    good = dict(lists=lists, n_cells=8, n_lists=2, k=4, stat=0, out_bits=out)
    st = _native.current_stream_ptr(DEV)

    def rc(**change):
        fields = {**good, **{f: v for f, v in change.items() if f not in ("size", "abi")}}
        blk = _native.KnnMerge(**fields)
        if "size" in change:
            blk.size = change["size"]
        if "abi" in change:
            blk.abi = change["abi"]
        return lib.flooder_knn_merge_f32(ctypes.byref(blk), st)

    assert rc() == 0
    size = ctypes.sizeof(_native.KnnMerge)
    for change in (dict(size=size + 8), dict(size=4), dict(abi=2), dict(k=0), dict(k=33), dict(stat=2), dict(n_lists=0),
                   dict(n_cells=-1), dict(lists=None), dict(out_bits=None)):
        assert rc(**change) == -1, change
        assert b"flooder_knn_merge_f32" in lib.flooder_last_error()
    assert rc(n_cells=0, lists=None, out_bits=None) == 0       # nothing to do
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:8] == 0).all() and (got[8:] == SENTINEL).all()
