"""``flooder_knn_wide_f32`` on its own, bit for bit against an integer brute force over all points: the k smallest
(d2 word, original id) keys in order, their d2 words and the statistic words of both statistics (the strided sum
replayed in numpy from the header's rule) for k from 1 to 1024 - on clouds where equidistant points at the k-th place
are the rule (integer coordinates, half-integer positions, doubled points), from one point to three tree levels, with a
padded last leaf, k = n (at 1, 17, 65 and 1024 points: k = n = 1025 is above the cap and refused), positions far outside
the cloud (everything passes the threshold for a long time: the buffer overflows and is merged again and again) and a
grid-stride loop that wraps.  For k <= 32 the words are also those of
``flooder_knn_ids_sorted_f32`` and ``flooder_sweep_knn_sorted_f32`` on the same inputs."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import grad_reference as gr
import knn_wide_reference as kw

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HI = {2: 256, 3: 64, 5: 16, 8: 8}      # coordinate ranges (test_gpu_knn_grad_kernel's)
KS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 512, 1000, 1023, 1024)
K_IS_N = (1, 17, 65)                    # (k = n = 1025 is above the entry's cap of 1024: refused, asserted below)
GUARD = 64                              # words behind every output buffer that must stay untouched
SUBSETS = (("ids",), ("d2",), ("ids", "d2"), ("ids", "bits"), ("d2", "bits"))

# (n points, dim, every point doubled, cells, the k to run): 1 = one point, 17 = a padded last leaf, 65 = one more than a
# wave, 1025 = two levels, 65 537 = three; every point doubled in half of the cases
CASES = ([(n, dim, (i + j) % 2 == 1 and n > 1, 300, KS)
          for i, n in enumerate((1, 17, 65, 1025, 65_537)) for j, dim in enumerate((2, 3, 5, 8))]
         # more cells than the 16 384 waves of the grid
         + [(1025, 3, True, 20_000, (5,))]
         # k = n on two tree levels and the top rung (1025 points cannot have it: the cap is 1024)
         + [(1024, 3, True, 300, (1024,))])


def make_case(n, dim, dup, n_cells):
    """(P (n, dim) int, hi, verts (n_s, k1, dim) f64, W (R, k1) f64, pos (n_s * R, dim) f64 in cell order): positions
    inside the cloud (40 %), on its corners (20 %) and far outside (40 %), integers or half-integers."""
    rng = np.random.default_rng(n * 10 + dim + (7 if n_cells > 10_000 else 0))
    hi = HI[dim]
    if dup:            # every point twice, the copies anywhere in the cloud; n is odd: the one point without a copy
        base = rng.integers(0, hi, size=((n + 1) // 2, dim))   # lies outside the box, behind every other point for a
        if n % 2:                                              # position inside it - the pairs stay aligned up to k = n - 2
            base[-1] = 2 * hi
        P = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        P = rng.integers(0, hi, size=(n, dim))
    k1 = 2 if dim in (2, 5) else 1
    W = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]]) if k1 == 2 else np.array([[1.0]])
    n_s = n_cells // W.shape[0]
    kind = rng.random((n_s, k1, 1))
    verts = np.where(kind < 0.4, rng.integers(0, hi, size=(n_s, k1, dim)),
                     np.where(kind < 0.6, rng.choice([0, hi - 1], size=(n_s, k1, dim)),
                              rng.integers(-511, 512, size=(n_s, k1, dim)))).astype(np.float64)
    if k1 == 1:
        verts = verts + rng.choice([0.0, 0.5], size=verts.shape) * (np.abs(verts) < 511)   # half-integer positions
    pos = np.einsum("rk,skd->srd", W, verts).reshape(-1, dim)
    return P, hi, verts, W, pos


def wide(c, k, stat, want, sample_order=None):
    """One launch writing the outputs named in ``want`` -> {name: uint32 / int32 array}, each buffer followed by a guard
    band that is checked here."""
    N = c["N"]
    shapes = {"ids": N * k, "d2": N * k, "bits": N}
    bufs = {name: torch.full((shapes[name] + GUARD,), -7, dtype=torch.int32, device=DEV) for name in want}
    blk = _native.KnnWide(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                          verts=c["verts"], weights=c["weights"], R=c["R"], k=k, n_simplices=c["n_s"], stat=stat,
                          order=c["index"].order32, sample_order=sample_order, out_bits=bufs.get("bits"),
                          out_ids=bufs.get("ids"), out_d2=bufs.get("d2"))
    _native.check(_native.load().flooder_knn_wide_f32(ctypes.byref(blk), _native.current_stream_ptr(DEV)),
                  "flooder_knn_wide_f32")
    out = {}
    for name, t in bufs.items():
        assert bool((t[shapes[name]:] == -7).all()), f"{name}: the guard band was written"
        a = t[:shapes[name]].cpu().numpy()
        out[name] = a.reshape(N, k) if name == "ids" else (a.view(np.uint32).reshape(N, k) if name == "d2"
                                                           else a.view(np.uint32))
    return out


def register_family(c, k, stat, order):
    """(ids, d2 words, statistic words) of ``flooder_knn_ids_sorted_f32`` and the statistic words of
    ``flooder_sweep_knn_sorted_f32`` on the same inputs (k <= 32)."""
    lib, st, N = _native.load(), _native.current_stream_ptr(DEV), c["N"]
    ids = torch.full((N, k), -1, dtype=torch.int32, device=DEV)
    d2 = torch.full((N, k), -1, dtype=torch.int32, device=DEV)
    bits, bits2 = (torch.full((N,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    common = dict(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                  verts=c["verts"], weights=c["weights"], R=c["R"], k=k, n_simplices=c["n_s"], stat=stat,
                  sample_order=order)
    blk = _native.KnnIds(queue=torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV), out_bits=bits,
                         order=c["index"].order32, out_ids=ids, out_d2=d2, **common)
    _native.check(lib.flooder_knn_ids_sorted_f32(ctypes.byref(blk), st), "flooder_knn_ids_sorted_f32")
    blk = _native.KnnSorted(queue=torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV), out_bits=bits2, **common)
    _native.check(lib.flooder_sweep_knn_sorted_f32(ctypes.byref(blk), st), "flooder_sweep_knn_sorted_f32")
    u32 = lambda t: t.cpu().numpy().view(np.uint32)    # noqa: E731
    return ids.cpu().numpy(), u32(d2), u32(bits), u32(bits2)


@pytest.mark.parametrize("n,dim,dup,n_cells,ks", CASES)
def test_knn_wide_bitwise(n, dim, dup, n_cells, ks):
    P, hi, verts, W, pos = make_case(n, dim, dup, n_cells)
    # exactness: in half units every difference is an integer and the largest d2 (quarters) stays below 2**24
    gr.assert_exact_inputs(P, P, 3, queries=pos)
    assert np.array_equal(pos * 2, np.round(pos * 2)) and np.abs(pos).max() < 512

    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    assert np.array_equal(np.sort(index.order32.long().cpu().numpy()), np.arange(n))
    assert index.pts.shape[0] % 16 == 0 and bool(torch.isinf(index.pts[n:, :dim]).all())   # the padded last leaf
    c = dict(n=n, dim=dim, index=index, k1=W.shape[1], R=W.shape[0], n_s=verts.shape[0], N=pos.shape[0],
             verts=torch.as_tensor(verts, dtype=torch.float32, device=DEV).contiguous(),
             weights=torch.as_tensor(W, dtype=torch.float32, device=DEV).contiguous())
    ks = tuple(sorted({k for k in ks if k <= n} | ({n} if n in K_IS_N and len(ks) > 1 else set())))
    assert ks

    d2f, ids, d2q = kw.smallest_keys(P, pos, max(ks), DEV)
    inside = torch.as_tensor(((pos >= 0) & (pos <= hi - 1)).all(axis=1), device=DEV)
    for k in ks:   # the tie rule is really exercised - from the reference alone
        if dup and n >= 1024 and k % 2 == 1 and k < d2q.shape[1]:
            share = float((d2q[:, k] == d2q[:, k - 1])[inside].float().mean())
            assert share >= 0.9, (n, k, share)

    lib = _native.load()
    if n == 1025 and len(ks) > 1:   # k = n here is one more than FLOODER_KNN_WIDE_MAX
        with pytest.raises(RuntimeError, match=r"flooder_knn_wide_f32: k must be in 1\.\.1024"):
            wide(c, n, 0, ("bits",))
    sorted_order = core._sorted_sample_order(lib, _native.current_stream_ptr(DEV), index, c["verts"], c["weights"], None,
                                             None, int(lib.flooder_sample_key_bits(dim)))
    rng = np.random.default_rng(n + dim)
    random_order = torch.as_tensor(rng.permutation(c["N"]).astype(np.int32), device=DEV)
    for i, k in enumerate(ks):
        want = {"ids": ids[:, :k].astype(np.int32), "d2": np.ascontiguousarray(d2f[:, :k]).view(np.uint32)}
        # all three outputs: stat 0 in cell order, stat 1 in the sorted order; the statistic alone in a random order
        runs = [(0, ("ids", "d2", "bits"), None), (1, ("ids", "d2", "bits"), sorted_order), (1, ("bits",), random_order),
                (0, ("ids", "d2", "bits"), None),                     # ... the first launch again: the same bits
                (i % 2, SUBSETS[i % len(SUBSETS)], random_order if i % 3 == 0 else None)]   # ... alone and in pairs
        if len(ks) == 1:   # (the wrapping case runs one k: every subset there)
            runs += [(1, sub, None) for sub in SUBSETS]
        first = None
        for stat, names, order in runs:
            got = wide(c, k, stat, names, order)
            want["bits"] = kw.statistic_words(d2f, k, stat)
            for name in names:
                assert np.array_equal(got[name], want[name]), (k, stat, names, name,
                                                               np.argwhere(got[name] != want[name])[:5].tolist())
            if first is None:
                first = got
            elif (stat, names, order) == runs[0]:   # run twice: identical bits
                assert all(np.array_equal(got[name], first[name]) for name in names), k
        if k <= core.KNN_MAX:   # the register family on the same inputs: the same words
            for stat in (0, 1):
                r_ids, r_d2, r_bits, r_bits2 = register_family(c, k, stat, sorted_order)
                bits = kw.statistic_words(d2f, k, stat)
                assert np.array_equal(r_ids, want["ids"]) and np.array_equal(r_d2, want["d2"]), (k, stat)
                assert np.array_equal(r_bits, bits) and np.array_equal(r_bits2, bits), (k, stat)


def test_cases_cover_what_they_must():
    assert {c[0] for c in CASES} >= {1, 17, 65, 1025, 65_537} and {c[1] for c in CASES} == {2, 3, 5, 8}
    assert sum(c[2] for c in CASES) * 2 >= len(CASES) - 4            # doubled in half of the cases that can be (n > 1)
    assert any(c[3] > 4 * 256 * 16 for c in CASES)                   # the grid-stride loop wraps
    assert {31, 32, 33, 63, 64, 65, 127, 129, 512, 1000, 1023, 1024} <= set(KS)
