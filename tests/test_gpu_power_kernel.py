"""``flooder_node_min_f32`` and ``flooder_sweep_power_f32`` on their own, through ``_native``.

The words of the power-distance sweep are the minimum of ``fmaf(w, w, d2)`` over ALL points, whatever the tree and the
sample order, so three oracles apply bit for bit: (a) integer inputs, where the float64 brute force is exact in float32;
(b) the lift - ``flooder_sweep_knn_sorted_f32`` at k = 1 over ``PointIndex([x, w])`` against ``(p, 0)`` ends its distance
chain in ``fmaf(-w, -w, d2)``; (c) zero weights give the k = 1 words and a constant weight shifts them by one rounded
addition.  Every output buffer is prefilled with a sentinel and has a guard of 64 words behind it."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import grad_reference as gr
import power_reference as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DIMS = (2, 3, 4, 5, 8)
SIZES = (1, 15, 40, 1000, 1025, 30_001, 70_001)
# (points_per_edge, simplex dimension): k1 = 1..9 vertices; R = 1, below 64, above 64, never a multiple of 64
SHAPES = [(5, 0), (5, 1), (9, 1), (17, 1), (5, 2), (9, 2), (17, 2), (5, 3), (9, 3), (5, 4), (5, 5), (5, 6), (5, 7), (5, 8)]
ORDERS = ("identity", "sorted", "random")


def _stream():
    return _native.current_stream_ptr(DEV)


def _guarded(n, dtype=torch.int32, fill=pr.SENTINEL):
    """(buffer of n words + guard, the view of the n words)."""
    buf = torch.full((n + pr.GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _guard_intact(buf, n, fill=pr.SENTINEL):
    return bool((buf[n:] == fill).all())


def _weights_in_tree_order(index, w):
    """(w_sorted (n_pad,) with +inf pad rows, node_w through ``flooder_node_min_f32`` behind a guard)."""
    n_pad = index.pts.shape[0]
    w_sorted = torch.full((n_pad,), float("inf"), dtype=torch.float32, device=DEV)
    w_sorted[:index.n] = torch.as_tensor(w, dtype=torch.float32, device=DEV).abs()[index.order32.long()]
    n_nodes = index.nodes.shape[0]
    buf, node_w = _guarded(n_nodes, torch.float32, -7.0)
    _native.check(_native.load().flooder_node_min_f32(_native.ptr(w_sorted), index.n, _native.ptr(node_w), _stream()),
                  "flooder_node_min_f32")
    assert _guard_intact(buf, n_nodes, -7.0)
    return w_sorted, node_w


def _block(index, verts, weights, out, order=None, stats=None, **over):
    fields = dict(pts_sorted=index.pts, n_pts=index.n, dim=index.dim, k1=verts.shape[1], nodes=index.nodes, verts=verts,
                  weights=weights, R=weights.shape[0], n_simplices=verts.shape[0], k=1, stat=0,
                  queue=torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV), out_bits=out, stats=stats,
                  sample_order=order)
    fields.update(over)
    return _native.KnnSorted(**fields)


def _power(index, verts, weights, w_sorted, node_w, order=None, count=True):
    """The words of ``flooder_sweep_power_f32``: every cell overwritten, the guard untouched, the counters alive."""
    N = verts.shape[0] * weights.shape[0]
    buf, out = _guarded(N)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV) if count else None
    blk = _block(index, verts, weights, out, order, stats)
    _native.check(_native.load().flooder_sweep_power_f32(ctypes.byref(blk), _native.ptr(w_sorted), _native.ptr(node_w),
                                                         _stream()), "flooder_sweep_power_f32")
    assert _guard_intact(buf, N) and bool((out >= 0).all())
    if count:
        st = stats.cpu().numpy()
        assert st[0] > 0 and st[1] >= st[0] and st[2] >= (N + 63) // 64 and st[3] > 0
    return out.cpu().numpy().view(np.uint32)


def _knn1(index, verts, weights, order):
    """The words of ``flooder_sweep_knn_sorted_f32`` at k = 1."""
    N = verts.shape[0] * weights.shape[0]
    buf, out = _guarded(N)
    blk = _block(index, verts, weights, out, order)
    _native.check(_native.load().flooder_sweep_knn_sorted_f32(ctypes.byref(blk), _stream()), "flooder_sweep_knn_sorted_f32")
    assert _guard_intact(buf, N)
    return out.cpu().numpy().view(np.uint32)


def _order(kind, index, verts, weights, rng):
    N = verts.shape[0] * weights.shape[0]
    if kind == "identity":
        return None
    if kind == "sorted":
        lib = _native.load()
        return core._sorted_sample_order(lib, _stream(), index, verts, weights, None, None,
                                         int(lib.flooder_sample_key_bits(index.dim)))
    return torch.as_tensor(rng.permutation(N).astype(np.int32), device=DEV)


def _identity(N):
    return torch.arange(N, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ node minima
@pytest.mark.parametrize("n", SIZES + (4_300_001,))
def test_node_min_layout_and_padding(n):
    rng = np.random.default_rng(n)
    n_pad = (n + 15) // 16 * 16
    vals = np.full(n_pad, np.inf, dtype=np.float32)
    vals[:n] = rng.uniform(0.0, 100.0, size=n).astype(np.float32)
    n_nodes = int(_native.load().flooder_bvh_node_count(n))
    want = pr.node_min_reference(vals, n)
    assert want.shape == (n_nodes,) and n_nodes % 64 == 0
    buf, out = _guarded(n_nodes, torch.float32, -7.0)
    t = torch.as_tensor(vals, device=DEV)
    for _ in range(2):    # a second call repeats the words
        _native.check(_native.load().flooder_node_min_f32(_native.ptr(t), n, _native.ptr(out), _stream()),
                      "flooder_node_min_f32")
        assert np.array_equal(out.cpu().numpy(), want)
        assert _guard_intact(buf, n_nodes, -7.0)
    assert np.isinf(want[(n + 15) // 16:64]).all() if n <= 1000 else True
    assert _native.load().flooder_node_min_f32(None, n, _native.ptr(out), _stream()) == -1
    assert _native.load().flooder_node_min_f32(_native.ptr(t), 0, _native.ptr(out), _stream()) == -1


# ------------------------------------------------------------------------------------------------ (a) exact lattice
def _lattice_case(dim, n, seed, ppe, d, n_s, r):
    rng = np.random.default_rng(seed)
    base = rng.integers(-r, r + 1, size=((n + 1) // 2, dim))
    P = np.concatenate([base, base])[:n][rng.permutation(n)] if seed % 2 else rng.integers(-r, r + 1, size=(n, dim))
    V = rng.integers(-r, r + 1, size=(n_s, d + 1, dim))
    V[: n_s // 4] = P[rng.integers(0, n, size=(n_s // 4, d + 1))]              # simplices on points of the cloud
    W = gr.lattice(ppe, d)
    gr.assert_exact_inputs(P, V.reshape(-1, dim), ppe)
    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    assert index.pts.shape[0] % 16 == 0 and index.pts.shape[0] > n
    t_v = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    t_w = W.to(torch.float32).to(DEV).contiguous()
    samples = pr.samples_of(torch.as_tensor(V, dtype=torch.float64, device=DEV), W.to(DEV))
    return rng, P, tp, index, t_v, t_w, samples


def _check_family_exact(family, rng, P, tp, index, t_v, t_w, samples, step, orders):
    w = pr.weight_family(family, P, rng, integer=True)
    assert np.array_equal(w, np.round(w)) and (w >= 0).all()
    val, arg, _ = pr.brute_power(tp, torch.as_tensor(w, device=DEV), samples)
    val, arg = val.cpu().numpy(), arg.cpu().numpy()
    assert val.max() * step * step < 2 ** 24                      # the minimum is exact in float32
    want = val.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), val)
    if family == "beacons":
        assert (w[arg] == 0).all() and (w > 0).sum() == max(0, P.shape[0] - 3)     # the far light point wins
    w_sorted, node_w = _weights_in_tree_order(index, w)
    for kind in orders:
        got = _power(index, t_v, t_w, w_sorted, node_w, _order(kind, index, t_v, t_w, rng))
        assert np.array_equal(got, want.view(np.uint32)), (family, kind, np.argwhere(got != want.view(np.uint32))[:5].ravel())
    return w_sorted, node_w, want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", DIMS)
def test_words_are_the_brute_force_minima_on_integer_inputs(dim, n):
    case = DIMS.index(dim) * len(SIZES) + SIZES.index(n)
    ppe, d = SHAPES[case % len(SHAPES)]
    assert pr.tree_levels(n) == (1 if n <= 1000 else 2 if n <= 30_001 else 3) and n % 16 != 0
    rng, P, tp, index, t_v, t_w, samples = _lattice_case(dim, n, 7000 + case, ppe, d, 12, 8 if dim <= 4 else 2)
    for i, family in enumerate(pr.FAMILIES):
        orders = ORDERS if family == "mixed" else (ORDERS[(case + i) % 3],)
        w_sorted, node_w, want = _check_family_exact(family, rng, P, tp, index, t_v, t_w, samples, ppe - 1, orders)
        if family == "mixed":     # a second call repeats the words
            assert np.array_equal(_power(index, t_v, t_w, w_sorted, node_w), want.view(np.uint32))


def test_shapes_cover_what_they_must():
    cases = [SHAPES[c % len(SHAPES)] for c in range(len(DIMS) * len(SIZES))]
    assert {ppe for ppe, _ in cases} == {5, 9, 17} and {d + 1 for _, d in cases} == set(range(1, 10))
    R = {gr.lattice(ppe, d).shape[0] for ppe, d in SHAPES}
    assert 1 in R and any(1 < x < 64 for x in R) and any(x > 64 for x in R) and all(x % 64 for x in R)
    # every padded row width, and dimensions below their padded width
    assert {_native.load().flooder_padded_dim(dim) for dim in DIMS} == {2, 4, 8} and 3 in DIMS and 5 in DIMS


def test_four_level_cloud():
    n, ppe, d = 4_300_001, 5, 3
    assert pr.tree_levels(n) == 4
    rng, P, tp, index, t_v, t_w, samples = _lattice_case(3, n, 4301, ppe, d, 8, 60)
    for family, kind in (("mixed", "sorted"), ("beacons", "identity"), ("heavy", "random")):
        _check_family_exact(family, rng, P, tp, index, t_v, t_w, samples, ppe - 1, (kind,))


# ------------------------------------------------------------------------------------------------ (b) / (c) general position
@functools.lru_cache(maxsize=None)
def _general_case(dim, n):
    g = torch.Generator().manual_seed(31 * dim + n)
    pts = torch.randn(n, dim, generator=g)
    verts = torch.randn(40, 3, dim, generator=g).to(DEV).contiguous()
    weights = gr.lattice(9, 2).to(torch.float32).to(DEV).contiguous()          # R = 45
    tp = pts.to(DEV)
    return pts.numpy().astype(np.float64), tp, core.PointIndex(tp), verts, weights


@pytest.mark.parametrize("n", [1000, 30_001])
@pytest.mark.parametrize("dim", [2, 3, 4, 5, 6, 7])
def test_words_are_those_of_the_lifted_k1_sweep(dim, n):
    P, tp, index, verts, weights = _general_case(dim, n)
    rng = np.random.default_rng(dim * n)
    samples = pr.samples_of(verts, weights)
    N = samples.shape[0]
    for family in ("mixed", "beacons"):
        w = torch.as_tensor(pr.weight_family(family, P, rng), dtype=torch.float32, device=DEV)
        _, arg, near = pr.brute_power(tp, w, samples)
        if family == "mixed":
            share = float((arg != near).double().mean())
            print(f"{dim}-D n={n}: {100 * share:.1f} % of the samples have a power-nearest point that is not their nearest")
            assert share >= 0.20
        else:
            assert bool((w[arg] == 0).all())
        up = core.PointIndex(pr.lifted(tp, w))
        want = _knn1(up, pr.with_zero_column(verts), weights, _identity(N))
        w_sorted, node_w = _weights_in_tree_order(index, w)
        for kind in ORDERS:
            got = _power(index, verts, weights, w_sorted, node_w, _order(kind, index, verts, weights, rng))
            assert np.array_equal(got, want), (family, kind, np.argwhere(got != want)[:5].ravel())


@pytest.mark.parametrize("n", [1000, 30_001])
@pytest.mark.parametrize("dim", DIMS)
def test_zero_and_constant_weights(dim, n):
    P, tp, index, verts, weights = _general_case(dim, n)
    N = verts.shape[0] * weights.shape[0]
    word0 = _knn1(index, verts, weights, _identity(N))
    w_sorted, node_w = _weights_in_tree_order(index, np.zeros(n))
    assert np.array_equal(_power(index, verts, weights, w_sorted, node_w), word0)
    w_sorted, node_w = _weights_in_tree_order(index, np.full(n, -pr.CONSTANT))       # the sign does not matter
    d2 = word0.view(np.float32).astype(np.float64)
    assert ((d2 == 0) | ((d2 >= 2.0 ** -31) & (d2 < 2.0 ** 45))).all()   # d2 + 9/64 needs at most 53 bits: exact in float64
    want = (d2 + pr.CONSTANT ** 2).astype(np.float32)
    assert pr.CONSTANT ** 2 == 0.140625
    assert np.array_equal(_power(index, verts, weights, w_sorted, node_w), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ refusals, empty calls
def test_refusals_and_empty_calls():
    lib = _native.load()
    P, tp, index, verts, weights = _general_case(3, 1000)
    w_sorted, node_w = _weights_in_tree_order(index, np.ones(1000))
    N = verts.shape[0] * weights.shape[0]
    buf, out = _guarded(N)

    def call(w_s=w_sorted, n_w=node_w, **over):
        blk = _block(index, verts, weights, out)
        for key, value in over.items():      # (None: a NULL pointer)
            setattr(blk, key, value)
        return lib.flooder_sweep_power_f32(ctypes.byref(blk), _native.ptr(w_s), _native.ptr(n_w), _stream())

    def refused(match, **kw):
        assert call(**kw) == -1
        msg = lib.flooder_last_error().decode()
        assert msg.startswith("flooder_sweep_power_f32") and match in msg, msg

    assert lib.flooder_sweep_power_f32(None, _native.ptr(w_sorted), _native.ptr(node_w), _stream()) == -1
    refused("abi / size", abi=2)
    refused("abi / size", size=ctypes.sizeof(_native.KnnSorted) + 8)
    refused("abi / size", size=4)
    for k in (0, 2, 32):
        refused("k must be in 1..1", k=k)
    refused("dim must be in 2..8", dim=1)
    refused("dim must be in 2..8", dim=9)
    refused("stat", stat=1)
    refused("stat", stat=2)
    refused("reserved", reserved=1)
    # nothing to do: FLOODER_OK before a pointer is looked at, nothing written
    assert call(n_simplices=0, pts_sorted=None, nodes=None) == 0
    assert call(R=0, verts=None, w_s=None, n_w=None) == 0
    for null in ("pts_sorted", "nodes", "verts", "weights", "queue", "out_bits"):
        refused("null pointer", **{null: None})
    refused("null pointer", w_s=None)
    refused("null pointer", n_w=None)
    refused("null pointer", n_pts=0)
    refused("null pointer", k1=0)
    assert bool((buf == pr.SENTINEL).all())          # none of the calls above has written a word
