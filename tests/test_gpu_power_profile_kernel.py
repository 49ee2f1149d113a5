"""``flooder_node_min_cols_f32`` and ``flooder_sweep_power_profile_f32`` on their own, through ``_native``.

Plane c of the multi-column sweep must be, word for word, what ``flooder_sweep_power_f32`` writes with column c's
weights - for any tree, both sample orders and any tile company - and, on integer inputs with dyadic lattice weights,
the float64 brute force minimum ``min_x |p - x|^2 + w_x^2`` (exact in float32 there).  The column mixes put a zero
column next to heavy ones and a BEACON column (one light point far away among heavy ones) among them: the column that
needs a node every other column culls.  Every output buffer is prefilled with a sentinel and has a guard behind it."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import power_reference as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DIMS = (2, 3, 5, 8)
SIZES = (1, 17, 5000, 70_001)
NCOLS = (1, 2, 3, 5, 8)
ROWS = (1, 63, 64, 65, 130)
MIX = ("zero", "heavy", "beacons", "constant", "mixed", "mixed", "beacons", "heavy")   # the first nc of these
STEP = 16              # lattice weights are multiples of 1 / 16

# (dim, n, n_cols, R): every value of each list, every (dim, n) pair once
CASES = [(dim, n, NCOLS[(4 * i + j) % 5], ROWS[(4 * i + j + 2 * (i % 2)) % 5])
         for i, dim in enumerate(DIMS) for j, n in enumerate(SIZES)]
CASES += [(3, 70_001, 8, 65), (5, 70_001, 8, 130), (2, 5000, 5, 130)]   # eight columns on three tree levels


def test_cases_cover_what_they_must():
    assert {c[2] for c in CASES} == set(NCOLS) and {c[3] for c in CASES} == set(ROWS)
    assert {(c[0], c[1]) for c in CASES} == {(d, n) for d in DIMS for n in SIZES} and len(set(CASES)) == len(CASES)
    assert (3, 70_001, 8, 65) in CASES
    assert [pr.tree_levels(n) for n in SIZES] == [1, 1, 2, 3]
    for n in (5000, 70_001):   # several column counts and tile shapes on the multi-level trees
        assert len({c[2] for c in CASES if c[1] == n}) >= 3 and len({c[3] for c in CASES if c[1] == n}) >= 3


def _stream():
    return _native.current_stream_ptr(DEV)


def _nc(m):
    return 1 if m <= 1 else 2 if m <= 2 else 4 if m <= 4 else 8


def _columns_in_tree_order(index, w_cols_np):
    """(w_cols (n_pad, NC), node_w_cols (nodes, NC)) of the (n, m) weights: pad rows and padding columns +inf."""
    n, m = w_cols_np.shape
    nc = _nc(m)
    w = torch.full((index.pts.shape[0], nc), float("inf"), dtype=torch.float32, device=DEV)
    w[:n, :m] = torch.as_tensor(w_cols_np, dtype=torch.float32, device=DEV).abs()[index.order32.long()]
    n_nodes = index.nodes.shape[0]
    buf = torch.full((n_nodes * nc + pr.GUARD,), -7.0, dtype=torch.float32, device=DEV)
    node_w = buf[:n_nodes * nc].view(n_nodes, nc)
    _native.check(_native.load().flooder_node_min_cols_f32(_native.ptr(w), index.n, nc, _native.ptr(node_w), _stream()),
                  "flooder_node_min_cols_f32")
    assert bool((buf[n_nodes * nc:] == -7.0).all())
    return w, node_w


def _single_weights(index, w_np):
    w = torch.full((index.pts.shape[0],), float("inf"), dtype=torch.float32, device=DEV)
    w[:index.n] = torch.as_tensor(w_np, dtype=torch.float32, device=DEV).abs()[index.order32.long()]
    node_w = torch.empty(index.nodes.shape[0], dtype=torch.float32, device=DEV)
    _native.check(_native.load().flooder_node_min_f32(_native.ptr(w), index.n, _native.ptr(node_w), _stream()),
                  "flooder_node_min_f32")
    return w, node_w


def _geometry(index, verts, weights):
    return dict(pts_sorted=index.pts, n_pts=index.n, dim=index.dim, k1=verts.shape[1], nodes=index.nodes, verts=verts,
                weights=weights, R=weights.shape[0], n_simplices=verts.shape[0])


def _single(index, verts, weights, w_sorted, node_w, order):
    N = verts.shape[0] * weights.shape[0]
    out = torch.full((N,), pr.SENTINEL, dtype=torch.int32, device=DEV)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    blk = _native.KnnSorted(k=1, stat=0, queue=torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV), out_bits=out,
                            stats=stats, sample_order=order, **_geometry(index, verts, weights))
    _native.check(_native.load().flooder_sweep_power_f32(ctypes.byref(blk), _native.ptr(w_sorted), _native.ptr(node_w),
                                                         _stream()), "flooder_sweep_power_f32")
    return out.cpu().numpy().view(np.uint32), stats.cpu().numpy()


def _profile(index, verts, weights, m, w_cols, node_w_cols, order):
    """(planes (m, N) uint32, counters): every word of the m planes overwritten, nothing behind them."""
    N = verts.shape[0] * weights.shape[0]
    buf = torch.full((m * N + pr.GUARD,), pr.SENTINEL, dtype=torch.int32, device=DEV)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    blk = _native.KnnSorted(k=1, stat=0, queue=torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV), out_bits=buf,
                            stats=stats, sample_order=order, **_geometry(index, verts, weights))
    _native.check(_native.load().flooder_sweep_power_profile_f32(ctypes.byref(blk), m, _native.ptr(w_cols),
                                                                 _native.ptr(node_w_cols), _stream()),
                  "flooder_sweep_power_profile_f32")
    assert bool((buf[m * N:] == pr.SENTINEL).all()) and bool((buf[:m * N] >= 0).all())
    st = stats.cpu().numpy()
    assert st[0] > 0 and st[1] >= st[0] and st[2] >= (N + 63) // 64 and st[3] > 0
    return buf[:m * N].cpu().numpy().view(np.uint32).reshape(m, N), st


def _sorted_order(index, verts, weights):
    lib = _native.load()
    return core._sorted_sample_order(lib, _stream(), index, verts, weights, None, None,
                                     int(lib.flooder_sample_key_bits(index.dim)))


# ------------------------------------------------------------------------------------------------ node minima
@pytest.mark.parametrize("nc", NCOLS)
def test_node_min_cols_is_the_single_reference_per_column(nc):
    lib = _native.load()
    for n in SIZES + (1025,):
        rng = np.random.default_rng(10 * n + nc)
        n_pad = (n + 15) // 16 * 16
        vals = np.full((n_pad, nc), np.inf, dtype=np.float32)
        vals[:n] = rng.uniform(0.0, 100.0, size=(n, nc)).astype(np.float32)
        n_nodes = int(lib.flooder_bvh_node_count(n))
        buf = torch.full((n_nodes * nc + pr.GUARD,), -7.0, dtype=torch.float32, device=DEV)
        t = torch.as_tensor(vals, device=DEV)
        for _ in range(2):    # a second call repeats the words
            _native.check(lib.flooder_node_min_cols_f32(_native.ptr(t), n, nc, _native.ptr(buf), _stream()),
                          "flooder_node_min_cols_f32")
            got = buf.cpu().numpy()
            assert (got[n_nodes * nc:] == -7.0).all()
            got = got[:n_nodes * nc].reshape(n_nodes, nc)
            for c in range(nc):
                assert np.array_equal(got[:, c], pr.node_min_reference(np.ascontiguousarray(vals[:, c]), n)), (n, c)
    t = torch.zeros((16, nc), device=DEV)
    out = torch.empty((64, nc), device=DEV)
    assert lib.flooder_node_min_cols_f32(None, 5, nc, _native.ptr(out), _stream()) == -1
    assert lib.flooder_node_min_cols_f32(_native.ptr(t), 5, nc, None, _stream()) == -1
    assert lib.flooder_node_min_cols_f32(_native.ptr(t), 0, nc, _native.ptr(out), _stream()) == -1
    for bad in (0, 9, -1):
        assert lib.flooder_node_min_cols_f32(_native.ptr(t), 5, bad, _native.ptr(out), _stream()) == -1
        assert lib.flooder_last_error().decode().startswith("flooder_node_min_cols_f32")


# ------------------------------------------------------------------------------------------------ the sweep
def _case(dim, n, R, seed):
    """Integer points (half of the cases: every point doubled), integer vertices (a quarter on points of the cloud),
    R rows of weights that are multiples of 1 / 16 - every sample, difference and square is exact in float32."""
    rng = np.random.default_rng(seed)
    r = 8 if dim <= 3 else 2
    if seed % 2:
        base = rng.integers(-r, r + 1, size=((n + 1) // 2, dim))
        P = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        P = rng.integers(-r, r + 1, size=(n, dim))
    n_s = 12
    k1 = 1 if R == 1 else 2
    V = rng.integers(-r, r + 1, size=(n_s, k1, dim))
    V[: n_s // 4] = P[rng.integers(0, n, size=(n_s // 4, k1))]
    if R == 1:
        W = np.ones((1, 1))
    else:
        i = (np.arange(R) * 7) % (STEP + 1)
        W = np.stack([i / STEP, 1.0 - i / STEP], axis=1)
    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    t_v = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    t_w = torch.as_tensor(W, dtype=torch.float32, device=DEV).contiguous()
    samples = pr.samples_of(torch.as_tensor(V, dtype=torch.float64, device=DEV), torch.as_tensor(W, device=DEV))
    return rng, P, tp, index, t_v, t_w, samples


@pytest.mark.parametrize("dim,n,m,R", CASES)
def test_planes_are_the_single_sweeps_and_the_brute_force(dim, n, m, R):
    rng, P, tp, index, t_v, t_w, samples = _case(dim, n, R, 9000 + CASES.index((dim, n, m, R)))
    N = samples.shape[0]
    assert t_w.shape[0] == R and N == 12 * R
    cols = np.stack([pr.weight_family(f, P, rng, integer=True) for f in MIX[:m]], axis=1)        # (n, m)
    assert np.array_equal(cols, np.round(cols)) and (cols >= 0).all()
    want = np.empty((m, N), dtype=np.uint32)
    for c in range(m):
        val, arg, _ = pr.brute_power(tp, torch.as_tensor(cols[:, c], device=DEV), samples)
        val, arg = val.cpu().numpy(), arg.cpu().numpy()
        assert val.max() * STEP * STEP < 2 ** 24                      # the minimum is exact in float32
        w32 = val.astype(np.float32)
        assert np.array_equal(w32.astype(np.float64), val)
        want[c] = w32.view(np.uint32)
        if MIX[c] == "beacons":
            assert (cols[arg, c] == 0).all() and (cols[:, c] > 0).sum() == max(0, n - 3)     # the far light point wins
    w_cols, node_w_cols = _columns_in_tree_order(index, cols)
    assert w_cols.shape[1] == _nc(m) and (m == _nc(m) or bool(torch.isinf(w_cols[:, m:]).all()))
    sorted_order = _sorted_order(index, t_v, t_w)
    random_order = torch.as_tensor(rng.permutation(N).astype(np.int32), device=DEV)
    counters = {}
    for kind, order in (("identity", None), ("sorted", sorted_order), ("random", random_order)):
        got, counters[kind] = _profile(index, t_v, t_w, m, w_cols, node_w_cols, order)
        assert np.array_equal(got, want), (kind, np.argwhere(got != want)[:5])
        again, _ = _profile(index, t_v, t_w, m, w_cols, node_w_cols, order)      # two runs: the same words
        assert np.array_equal(again, got)
    # ... and word for word the single sweep of every column, in both orders of the issue (NULL and sorted)
    leaf_eval = 0
    for c in range(m):
        w_sorted, node_w = _single_weights(index, cols[:, c])
        for order in (None, sorted_order):
            one, st = _single(index, t_v, t_w, w_sorted, node_w, order)
            assert np.array_equal(one, want[c]), (c, MIX[c])
        leaf_eval += int(st[0])
    print(f"{dim}-D n={n} cols={m} R={R}: leaf evaluations profile {int(counters['sorted'][0])} vs the {m} single sweeps "
          f"together {leaf_eval}")


def test_padding_columns_enter_no_test():
    """Three real columns in rows of four: whatever the fourth holds - +inf, zero, NaN - the planes and the walk's
    counters are the same (a padding column of zeros that entered the tests would keep every node alive)."""
    rng, P, tp, index, t_v, t_w, samples = _case(3, 5000, 65, 77)
    cols = np.stack([pr.weight_family(f, P, rng, integer=True) for f in ("heavy", "beacons", "constant")], axis=1)
    w_cols, _ = _columns_in_tree_order(index, cols)
    lib = _native.load()
    ref = None
    for fill in (float("inf"), 0.0, float("nan")):
        w = w_cols.clone()
        w[:, 3] = fill
        node_w = torch.empty((index.nodes.shape[0], 4), dtype=torch.float32, device=DEV)
        _native.check(lib.flooder_node_min_cols_f32(_native.ptr(w), index.n, 4, _native.ptr(node_w), _stream()),
                      "flooder_node_min_cols_f32")
        got, st = _profile(index, t_v, t_w, 3, w, node_w, None)
        if ref is None:
            ref = (got, st)
        assert np.array_equal(got, ref[0]) and np.array_equal(st[:3], ref[1][:3]), fill


def test_refusals_and_empty_calls():
    lib = _native.load()
    rng, P, tp, index, t_v, t_w, samples = _case(3, 5000, 63, 5)
    cols = np.stack([pr.weight_family(f, P, rng, integer=True) for f in MIX[:2]], axis=1)
    w_cols, node_w_cols = _columns_in_tree_order(index, cols)
    N = samples.shape[0]
    buf = torch.full((2 * N + pr.GUARD,), pr.SENTINEL, dtype=torch.int32, device=DEV)

    def call(n_cols=2, w_c=w_cols, n_w=node_w_cols, **over):
        blk = _native.KnnSorted(k=1, stat=0, queue=torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV),
                                out_bits=buf, **_geometry(index, t_v, t_w))
        for key, value in over.items():      # (None: a NULL pointer)
            setattr(blk, key, value)
        return lib.flooder_sweep_power_profile_f32(ctypes.byref(blk), n_cols, _native.ptr(w_c), _native.ptr(n_w), _stream())

    def refused(match, **kw):
        assert call(**kw) == -1
        msg = lib.flooder_last_error().decode()
        assert msg.startswith("flooder_sweep_power_profile_f32") and match in msg, msg

    assert lib.flooder_sweep_power_profile_f32(None, 2, _native.ptr(w_cols), _native.ptr(node_w_cols), _stream()) == -1
    refused("abi / size", abi=2)
    refused("abi / size", size=ctypes.sizeof(_native.KnnSorted) + 8)
    refused("abi / size", size=4)
    refused("n_cols must be in 1..8", n_cols=0)
    refused("n_cols must be in 1..8", n_cols=9)
    for k in (0, 2, 32):
        refused("k must be in 1..1", k=k)
    refused("dim must be in 2..8", dim=1)
    refused("dim must be in 2..8", dim=9)
    refused("stat", stat=1)
    refused("reserved", reserved=1)
    # nothing to do: FLOODER_OK before a pointer is looked at, nothing written
    assert call(n_simplices=0, pts_sorted=None, nodes=None) == 0
    assert call(R=0, verts=None, w_c=None, n_w=None) == 0
    for null in ("pts_sorted", "nodes", "verts", "weights", "queue", "out_bits"):
        refused("null pointer", **{null: None})
    refused("null pointer", w_c=None)
    refused("null pointer", n_w=None)
    refused("null pointer", n_pts=0)
    refused("null pointer", k1=0)
    refused("null pointer", k1=10)
    torch.cuda.synchronize()
    assert bool((buf == pr.SENTINEL).all())          # none of the calls above has written a word
