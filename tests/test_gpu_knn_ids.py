"""``flooder_knn_ids_sorted_f32`` on the device, word for word: the k smallest (d2 word, original id) keys of every
sample against a brute-force key sort and against ``flooder_witness_knn``, its statistic words against
``flooder_sweep_knn_sorted_f32``, the order as a performance input only; ``nearest_neighbors`` and the backward of
``neighbor_distance`` on ROCm tensors; what the entry point refuses.

The inputs are the exact ones of ``test_gpu_knn_sorted`` (integer coordinates, float32 arithmetic exact, half the clouds
with every point doubled so that equidistant points at the k-th place are the rule) - that module's cached cases are
used as they are - plus one cloud with k = n_pts, where no list is full before the tree is exhausted."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import grad_reference as gr
import knn_grad_reference as kr
import test_gpu_knn_sorted as tks
from helpers import smallest32, tolerances

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KS = (1, 2, 3, 8, 17, 32)
STATS = ("kth", "dtm")
K_IS_N = "3d_k_is_n"
# the cases of test_gpu_knn_sorted at one to three tree levels (name -> lattice step**-2, the unit of their d2) and the
# cloud of 20 points swept at k = 20
NAMES = {"2d": 16, "3d_q63": 1, "3d_q64": 1, "3d_q65": 1, "4d": 16, "6d": 64, "8d_far": 1, K_IS_N: 1}


def _k_is_n_case():
    """3-D, 20 points (ten, each twice: a padded last leaf of 12 rows that must not leak in), 70 queries: one full
    tile and six live lanes in the second."""
    rng = np.random.default_rng(77)
    base = rng.integers(-40, 41, size=(10, 3))
    P = np.concatenate([base, base])[rng.permutation(20)]
    V = rng.integers(-60, 61, size=(70, 1, 3))
    V[:10, 0] = P[rng.integers(0, 20, size=10)]
    gr.assert_exact_inputs(P, V.reshape(-1, 3), 2)
    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    t_v = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    t_w = torch.ones((1, 1), dtype=torch.float32, device=DEV)
    lib = _native.load()
    order = core._sorted_sample_order(lib, tks._stream(), index, t_v, t_w, None, None, int(lib.flooder_sample_key_bits(3)))
    small = smallest32(tp.double(), t_v.reshape(-1, 3).double())
    return dict(dim=3, n=20, points=tp, index=index, verts=t_v, weights=t_w, k1=1, R=1, n_s=70, small=small, order=order)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case and its brute-force key sort: (d2 (N, m) float64 - exact, equal to the float32 word -, ids (N, m)), m =
    min(33, n) smallest keys of every sample, one more than the largest k so that ties at the k-th place can be read."""
    c = _k_is_n_case() if name == K_IS_N else tks._case(name)
    samples = torch.einsum("rk,skd->srd", c["weights"].double(), c["verts"].double()).reshape(-1, c["dim"])
    m = min(33, c["n"])
    d2, ids = kr.smallest_keys_f64(c["points"], samples, m, NAMES[name])
    d2, ids = d2.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(d2[:, :min(32, m)], c["small"][:, :m])           # the value tests' brute force, with ids
    assert np.array_equal(d2.astype(np.float32).astype(np.float64), d2)
    return c, d2, ids


def _ks(name):
    return (20,) if name == K_IS_N else tuple(k for k in KS if k <= _case(name)[0]["n"])


def _ids_sweep(c, k, stat, order, with_d2=True, with_bits=True):
    """(out_ids (N, k) int32, out_d2 (N, k) uint32 or None, out_bits (N,) uint32 or None), every buffer prefilled
    with -1."""
    lib = _native.load()
    N = c["n_s"] * c["R"]
    ids = torch.full((N, k), -1, dtype=torch.int32, device=DEV)
    d2 = torch.full((N, k), -1, dtype=torch.int32, device=DEV) if with_d2 else None
    bits = torch.full((N,), -1, dtype=torch.int32, device=DEV) if with_bits else None
    queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    blk = _native.KnnIds(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                         verts=c["verts"], weights=c["weights"], R=c["R"], k=k, n_simplices=c["n_s"], stat=stat,
                         queue=queue, out_bits=bits, stats=stats, sample_order=order, order=c["index"].order32,
                         out_ids=ids, out_d2=d2)
    _native.check(lib.flooder_knn_ids_sorted_f32(ctypes.byref(blk), tks._stream()), "flooder_knn_ids_sorted_f32")
    st = stats.cpu().numpy()
    assert st[0] > 0 and st[1] >= st[0] and st[2] >= (N + 63) // 64, st
    u32 = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)    # noqa: E731
    return ids.cpu().numpy(), u32(d2), u32(bits)


def _witness(c, k, stat, q_stat):
    """``flooder_witness_knn`` for every (simplex, sample) of the case, in cell order."""
    lib = _native.load()
    S, R = c["n_s"], c["R"]
    N = S * R
    q_s = torch.arange(S, dtype=torch.int32, device=DEV).repeat_interleave(R).contiguous()
    q_r = torch.arange(R, dtype=torch.int32, device=DEV).repeat(S).contiguous()
    out_ids = torch.full((N, k), -7, dtype=torch.int64, device=DEV)
    out_d2 = torch.full((N, k), 7, dtype=torch.int32, device=DEV)
    not_found = torch.zeros(1, dtype=torch.int32, device=DEV)
    blk = _native.WitnessKnn(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                             order=c["index"].order32, verts=c["verts"], weights=c["weights"], R=R, k=k, n_simplices=S,
                             n_queries=N, q_simplex=q_s, q_row=q_r,
                             q_stat=torch.as_tensor(q_stat.view(np.int32), device=DEV), out_ids=out_ids, out_d2=out_d2,
                             not_found=not_found, stat=stat)
    _native.check(lib.flooder_witness_knn(ctypes.byref(blk), tks._stream()), "flooder_witness_knn")
    return out_ids.cpu().numpy(), out_d2.cpu().numpy().view(np.uint32), int(not_found.item())


# ------------------------------------------------------------------------------------------------------ kernel level
def test_cases_cover_what_they_must():
    shapes = {name: tks.CASES[name] for name in NAMES if name != K_IS_N}
    assert {s[0] for s in shapes.values()} == {2, 3, 4, 6, 8} and {s[3] for s in shapes.values()} == {1, 2, 3}
    assert sum(s[2] for s in shapes.values()) * 2 >= len(shapes)               # every point doubled in half of them
    assert {s[5] for s in shapes.values() if s[5]} >= {63, 64, 65}
    assert all(s[1] % 16 for s in shapes.values())                             # a padded last leaf everywhere


@pytest.mark.parametrize("name", list(NAMES))
def test_keys_word_for_word(name):
    """Against the brute-force key sort, ``flooder_witness_knn`` and the value sweep's statistic words."""
    c, d2, ids = _case(name)
    dup = name == K_IS_N or tks.CASES[name][2]
    tied = 0
    for k in _ks(name):
        want_ids = ids[:, :k].astype(np.int32)
        want_d2 = d2[:, :k].astype(np.float32).view(np.uint32)
        if k < d2.shape[1]:       # ties at the k-th place: more than k points within the k-th distance
            share = float((d2[:, k] == d2[:, k - 1]).mean())
            tied += share > 0
            if dup and k % 2 == 1 and name != "8d_far":
                assert share > 0.5, (name, k, share)
        for stat in (0, 1):
            got_ids, got_d2, got_bits = _ids_sweep(c, k, stat, c["order"], with_d2=stat == 0 or k % 2 == 1)
            assert np.array_equal(got_ids, want_ids), (name, k, stat, np.argwhere(got_ids != want_ids)[:5].tolist())
            if got_d2 is not None:
                assert np.array_equal(got_d2, want_d2), (name, k, stat, np.argwhere(got_d2 != want_d2)[:5].tolist())
            words = tks._sweep(c, k, stat, c["order"])
            assert np.array_equal(got_bits, words), (name, k, STATS[stat])
            assert np.array_equal(words, tks._expected(d2[:, :max(k, 1)], k, stat))
            w_ids, w_d2, missing = _witness(c, k, stat, words)
            assert missing == 0
            assert np.array_equal(got_ids.astype(np.int64), w_ids) and np.array_equal(want_d2, w_d2), (name, k, stat)
    if name in ("4d", "6d", "3d_q65"):
        assert tied > 0, name
    if name == K_IS_N:     # k = n: every point is reported, each id once
        assert np.array_equal(np.sort(ids[:, :20], axis=1), np.broadcast_to(np.arange(20), (70, 20)))


def test_no_output_is_optional_but_the_ids():
    c, d2, ids = _case("3d_q65")
    got_ids, got_d2, got_bits = _ids_sweep(c, 8, 1, c["order"], with_d2=False, with_bits=False)
    assert got_d2 is None and got_bits is None and np.array_equal(got_ids, ids[:, :8].astype(np.int32))


def test_the_order_is_a_performance_input_only():
    c, _, _ = _case("4d")
    N = c["n_s"] * c["R"]
    identity = torch.arange(N, dtype=torch.int32, device=DEV)
    shuffled = torch.as_tensor(np.random.default_rng(5).permutation(N).astype(np.int32), device=DEV)
    for k in (2, 17):
        for stat in (0, 1):
            want = _ids_sweep(c, k, stat, c["order"])
            for order in (identity, shuffled):
                got = _ids_sweep(c, k, stat, order)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (k, stat)


# ------------------------------------------------------------------------------------------------- public, on ROCm
@pytest.mark.parametrize("name", ["3d_q65", "8d_far"])
def test_nearest_neighbors_is_the_kernels_keys(name):
    c, d2, ids = _case(name)
    queries = c["verts"][:, 0, :].contiguous()
    for k in (1, 8, 32):
        got_ids, got_dist = fa.nearest_neighbors(c["points"], queries, k)
        assert got_ids.dtype == torch.int64 and got_ids.shape == (c["n_s"], k) and got_ids.device == c["points"].device
        assert got_dist.dtype == torch.float32 and got_dist.shape == (c["n_s"], k)
        assert np.array_equal(got_ids.cpu().numpy(), ids[:, :k])
        # (the float32 root is correctly rounded, and so is the float64 root rounded to float32)
        assert np.array_equal(got_dist.cpu().numpy(), np.sqrt(d2[:, :k]).astype(np.float32))
        sq_ids, sq = fa.nearest_neighbors(c["points"], queries, k, squared=True, index=c["index"])
        assert torch.equal(sq_ids, got_ids) and np.array_equal(sq.cpu().numpy().astype(np.float64), d2[:, :k])
        assert torch.equal(got_dist[:, k - 1], fa.neighbor_distance(c["points"], queries, k, "kth"))


def test_own_points_and_groups_of_queries(monkeypatch):
    c, _, _ = _case("3d_q65")
    tp = c["points"]
    ids, dist = fa.nearest_neighbors(tp, None, 3)
    P = tp.cpu().numpy().astype(np.int64)
    want_d2, want_ids = kr.smallest_keys_int(torch.as_tensor(P, device=DEV), torch.as_tensor(P, device=DEV), 3)
    assert torch.equal(ids, want_ids) and torch.equal(dist.double().square().round().long(), want_d2)
    assert bool((dist[:, 0] == 0).all()) and bool((ids[:, 0] <= torch.arange(tp.shape[0], device=DEV)).all())
    monkeypatch.setattr(core, "SORTED_WORKSPACE_BYTES", 48 * 300)      # four groups
    ids2, dist2 = fa.nearest_neighbors(tp, None, 3)
    assert torch.equal(ids2, ids) and torch.equal(dist2, dist)


def _closed_form(P, Q, own, ids, k, stat, squared, coef):
    """float64 gradient of ``(coef * neighbor_distance(...)).sum()`` on the given ids ->
    [(gradient, sum of the magnitudes of the terms of each entry, number of terms of each row)] for the points and,
    unless ``own``, for the queries."""
    P, Q = P.double(), Q.double()
    d2 = (Q.unsqueeze(1) - P[ids]).square().sum(dim=2)                       # (Q, k) ascending
    f2 = d2[:, -1] if stat == "kth" else d2.mean(dim=1)
    use = ids[:, -1:] if stat == "kth" else ids
    m = use.shape[1]
    c = coef.double() * (2.0 if squared else torch.where(f2 > 0, f2.sqrt().reciprocal(), torch.zeros_like(f2))) / m
    contrib = (Q.unsqueeze(1) - P[use]) * c.view(-1, 1, 1)
    flat = contrib.reshape(-1, P.shape[1])
    gq, mq = contrib.sum(dim=1), contrib.abs().sum(dim=1)
    gp = torch.zeros_like(P).index_add_(0, use.reshape(-1), -flat)
    mp = torch.zeros_like(P).index_add_(0, use.reshape(-1), flat.abs())
    tp = torch.zeros(P.shape[0], dtype=torch.float64, device=P.device).index_add_(
        0, use.reshape(-1), torch.ones(flat.shape[0], dtype=torch.float64, device=P.device))
    if own:
        return [(gp + gq, mp + mq, tp + m)]
    return [(gp, mp, tp), (gq, mq, torch.full((Q.shape[0],), float(m), dtype=torch.float64, device=P.device))]


@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("name", ["3d_q65", "8d_far"])
def test_backward_of_neighbor_distance(name, own):
    """The values with grad are the bits of the call without; two backward passes give the same bits; the gradient is
    the float64 closed form on the reported ids.

    Tolerance: the suite's gate, ``helpers.tolerances`` of the points (1e-5 relative, two float32 ulps of the coordinate
    scale absolute) - or, where an entry is a sum of so many terms that float32 addition alone can exceed that gate,
    the rounding bound of that sum.  An entry of a gradient is a float32 sum of T terms (q - x) * c, the difference
    exact on these inputs and c = coef / (f m) (or 2 coef / m) formed with at most k + 8 roundings (the k additions and
    the division of the mean, the root, the product f m, the quotient, the product with the difference; the sum over
    the k neighbours inside a query's own term), so its error is at most (T + k + 8) * 2**-24 * sum |term| to first
    order whatever the order of the additions.  The gate alone cannot be the bound: a point that is the neighbour of
    many queries sums that many terms of either sign (up to 200 on "8d_far", of the size of the coordinates with
    ``squared=True``), and the rounding of a float32 sum grows with the magnitudes added, not with the result.  Both
    bounds come from the inputs and the number format, none from a run; each figure is printed before it is asserted."""
    c, _, _ = _case(name)
    tp = c["points"]
    queries = None if own else c["verts"][:, 0, :].contiguous()
    Q = tp.shape[0] if own else queries.shape[0]
    coef = torch.as_tensor(np.random.default_rng(3).uniform(0.5, 1.5, size=Q), dtype=torch.float32, device=DEV)
    rtol, atol = tolerances(tp.cpu().numpy())
    for k in (1, 8, 32):
        ids, _ = fa.nearest_neighbors(tp, queries, k)
        for stat in STATS:
            for squared in (False, True):
                plain = fa.neighbor_distance(tp, queries, k, stat, squared=squared)
                grads = []
                for _ in range(2):
                    p = tp.clone().requires_grad_(True)
                    q = None if own else queries.clone().requires_grad_(True)
                    out = fa.neighbor_distance(p, q, k, stat, squared=squared)
                    assert out.grad_fn is not None and torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))
                    (coef * out).sum().backward()
                    grads.append([p.grad] if own else [p.grad, q.grad])
                for g0, g1 in zip(*grads):
                    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)), (k, stat, squared)
                wants = _closed_form(tp, tp if own else queries, own, ids, k, stat, squared, coef)
                for got, (want, mag, terms) in zip(grads[0], wants):
                    err = (got.double() - want).abs()
                    bound = torch.maximum(atol + rtol * want.abs(), 1.01 * (terms.unsqueeze(1) + k + 8) * gr.EPS32 * mag)
                    print(name, own, k, stat, squared, "max err", float(err.max()), "max err / bound", float((err / bound).max()))
                    assert bool((err <= bound).all()), (k, stat, squared, float(err.max()))
                if k == 1 and not own:     # a query on a cloud point: value 0, gradient 0
                    zero = plain == 0
                    assert bool(zero.any()) and bool((grads[0][1][zero] == 0).all())


def test_without_grad_there_is_no_graph_and_no_ids_sweep(monkeypatch):
    c, _, _ = _case("3d_q65")
    calls = []
    real = fa.neighbors._knn_ids_hip
    monkeypatch.setattr(fa.neighbors, "_knn_ids_hip", lambda *a, **k: calls.append(1) or real(*a, **k))
    out = fa.neighbor_distance(c["points"], None, 4, "dtm")
    assert out.grad_fn is None and not calls
    with torch.no_grad():
        assert fa.neighbor_distance(c["points"].clone().requires_grad_(True), None, 4, "dtm").grad_fn is None and not calls
    assert fa.neighbor_distance(c["points"].clone().requires_grad_(True), None, 4, "dtm").grad_fn is not None and calls


# ------------------------------------------------------------------------------------------------------------- ABI
P = 4096   # a pointer that is not NULL (never dereferenced: every call below is refused, or has nothing to do)
POINTERS = "pts_sorted nodes verts weights queue sample_order order out_ids".split()
GOOD = dict(n_pts=1000, dim=3, k1=4, R=35, k=8, n_simplices=10, stat=1, **{name: P for name in POINTERS})


def _rc(**change):
    blk = _native.KnnIds(**{**GOOD, **change})
    return _native.load().flooder_knn_ids_sorted_f32(ctypes.byref(blk), None)


def test_entry_refuses_before_a_pointer_is_looked_at():
    lib = _native.load()
    for name in POINTERS:
        assert _rc(**{name: None}) == -1, name
        assert lib.flooder_last_error().startswith(b"flooder_knn_ids_sorted_f32"), name
    assert _rc(order=None) == -1 and b"order is NULL" in lib.flooder_last_error()
    assert _rc(out_ids=None) == -1 and b"out_ids is NULL" in lib.flooder_last_error()
    bad = [dict(k=0), dict(k=33), dict(dim=1), dict(dim=9), dict(stat=2), dict(n_pts=7), dict(n_pts=1 << 31),
           dict(k1=0), dict(k1=10), dict(n_simplices=1 << 22, R=1024), dict(n_simplices=(1 << 32) - 2, R=1),
           dict(R=-1), dict(n_simplices=-1)]
    for change in bad:
        assert _rc(**change) == -1, change
        assert lib.flooder_last_error().startswith(b"flooder_knn_ids_sorted_f32"), change
    null = {name: None for name in POINTERS}
    assert _rc(n_simplices=0, **null) == 0
    assert _rc(R=0, **null) == 0
    assert lib.flooder_knn_ids_sorted_f32(None, None) == -1
