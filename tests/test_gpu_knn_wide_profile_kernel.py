"""``flooder_knn_wide_profile_f32`` on its own, through ``_native``: ONE walk at k_max = max(col_k) writes a plane of
statistic words per (k, stat) column.  Every plane is compared word for word with a single ``flooder_knn_wide_f32`` call
at that column's (k, stat), and - the inputs are exact: integer points, half-integer positions - with the numpy replay of
the header's rule over an integer brute force (``knn_wide_reference``).  Column sets straddle the list capacities (64,
128, 256, 1024 keys) and the lane count; the planes lie ``plane_stride`` words apart with sentinel words between them
that must stay untouched."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import grad_reference as gr
import knn_wide_reference as kw

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HI = {2: 256, 3: 64, 6: 16}            # coordinate ranges: the largest d2 in quarters stays below 2**24
SENTINEL = -7
GAP = 37                               # sentinel words between two planes (plane_stride = N + GAP)
BOTH = (0, 1)
COLS_200 = [(k, s) for k in (1, 2, 63, 64, 65, 128, 129, 200) for s in BOTH]
COLS_1024 = [(k, s) for k in (1, 64, 65, 1000, 1024) for s in BOTH]

# (n points, dim, every point doubled, R, columns)
CASES = [(3001, 2, False, 1, COLS_200), (3001, 3, True, 65, COLS_200), (3001, 6, False, 1, COLS_200),
         (3001, 3, False, 65, COLS_1024), (3001, 6, True, 1, COLS_1024), (3001, 2, True, 65, COLS_1024),
         # k_max == n_pts: nothing is culled, the walk ends with the tree
         (200, 3, False, 1, [(200, 1), (1, 0), (64, 1), (200, 0), (65, 1)]),
         (1024, 2, True, 65, [(1024, 0), (1024, 1), (513, 1)])]


def make_case(n, dim, dup, R):
    """Integer points (doubled: every point twice), n_s "simplices" of two integer vertices and R rows of weights from
    {(1, 0), (.5, .5), (0, 1)} (R = 1: one vertex, weight 1): half-integer positions inside, on the corners of and far
    outside the cloud."""
    rng = np.random.default_rng(100 * n + 10 * dim + R)
    hi = HI[dim]
    if dup:
        base = rng.integers(0, hi, size=((n + 1) // 2, dim))
        P = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        P = rng.integers(0, hi, size=(n, dim))
    if R == 1:
        k1, W, n_s = 1, np.array([[1.0]]), 320
    else:
        k1, n_s = 2, 5
        W = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])[rng.integers(0, 3, size=R)]
    kind = rng.random((n_s, k1, 1))
    verts = np.where(kind < 0.5, rng.integers(0, hi, size=(n_s, k1, dim)),
                     np.where(kind < 0.7, rng.choice([0, hi - 1], size=(n_s, k1, dim)),
                              rng.integers(-300, 301, size=(n_s, k1, dim)))).astype(np.float64)
    if k1 == 1:
        verts = verts + rng.choice([0.0, 0.5], size=verts.shape)
    pos = np.einsum("rk,skd->srd", W, verts).reshape(-1, dim)
    gr.assert_exact_inputs(P, P, 3, queries=pos)
    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    c = dict(n=n, dim=dim, index=index, k1=k1, R=W.shape[0], n_s=n_s, N=pos.shape[0],
             verts=torch.as_tensor(verts, dtype=torch.float32, device=DEV).contiguous(),
             weights=torch.as_tensor(W, dtype=torch.float32, device=DEV).contiguous())
    return P, pos, c


def _fields(c):
    return dict(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                verts=c["verts"], weights=c["weights"], R=c["R"], n_simplices=c["n_s"], order=c["index"].order32)


def single(c, k, stat, sample_order=None):
    out = torch.full((c["N"],), SENTINEL, dtype=torch.int32, device=DEV)
    blk = _native.KnnWide(k=k, stat=stat, sample_order=sample_order, out_bits=out, **_fields(c))
    _native.check(_native.load().flooder_knn_wide_f32(ctypes.byref(blk), _native.current_stream_ptr(DEV)),
                  "flooder_knn_wide_f32")
    return out.cpu().numpy().view(np.uint32)


def profile(c, cols, sample_order=None, stride=None, lists=False):
    """-> (planes (n_cols, N) uint32, ids, d2 or None): the words between and behind the planes are checked here."""
    N, n_cols = c["N"], len(cols)
    stride = N + GAP if stride is None else stride
    k_max = max(k for k, _ in cols)
    buf = torch.full((n_cols * stride + GAP,), SENTINEL, dtype=torch.int32, device=DEV)
    ids = torch.full((N * k_max + GAP,), SENTINEL, dtype=torch.int32, device=DEV) if lists else None
    d2 = torch.full((N * k_max + GAP,), SENTINEL, dtype=torch.int32, device=DEV) if lists else None
    blk = _native.KnnWide(k=k_max, stat=0, sample_order=sample_order, out_bits=buf, out_ids=ids, out_d2=d2, **_fields(c))
    _native.check(_native.load().flooder_knn_wide_profile_f32(ctypes.byref(blk), *_native.column_arrays(cols), stride,
                                                              _native.current_stream_ptr(DEV)),
                  "flooder_knn_wide_profile_f32")
    host = buf.cpu().numpy()
    planes = host[:n_cols * stride].reshape(n_cols, stride)
    assert (planes[:, N:] == SENTINEL).all() and (host[n_cols * stride:] == SENTINEL).all(), "a word outside the planes was written"
    if lists:
        assert bool((ids[N * k_max:] == SENTINEL).all()) and bool((d2[N * k_max:] == SENTINEL).all())
        return (planes[:, :N].copy().view(np.uint32), ids[:N * k_max].cpu().numpy().reshape(N, k_max),
                d2[:N * k_max].cpu().numpy().view(np.uint32).reshape(N, k_max))
    return planes[:, :N].copy().view(np.uint32), None, None


@pytest.mark.parametrize("n,dim,dup,R,cols", CASES)
def test_planes_are_the_single_calls_and_the_brute_force(n, dim, dup, R, cols):
    P, pos, c = make_case(n, dim, dup, R)
    k_max = max(k for k, _ in cols)
    assert c["R"] == R and c["N"] == c["n_s"] * R and k_max <= n
    d2f, ids, _ = kw.smallest_keys(P, pos, k_max, DEV)
    rng = np.random.default_rng(n + dim)
    permuted = torch.as_tensor(rng.permutation(c["N"]).astype(np.int32), device=DEV)

    got, got_ids, got_d2 = profile(c, cols, None, lists=True)
    for i, (k, stat) in enumerate(cols):
        want = kw.statistic_words(d2f, k, stat)
        assert np.array_equal(got[i], want), (k, stat, np.argwhere(got[i] != want)[:5].ravel())
        assert np.array_equal(got[i], single(c, k, stat, permuted if i % 2 else None)), (k, stat)
    # the lists of the walk are the single entry's: the k_max smallest keys, ascending
    assert np.array_equal(got_ids, ids[:, :k_max].astype(np.int32))
    assert np.array_equal(got_d2, np.ascontiguousarray(d2f[:, :k_max]).view(np.uint32))
    # a permuted order, planes packed (plane_stride == N), the columns reversed: the same words, twice
    rev = cols[::-1]
    for _ in range(2):
        again, _, _ = profile(c, rev, permuted, stride=c["N"])
        assert np.array_equal(again[::-1], got)


def test_one_column_is_the_single_entry():
    P, pos, c = make_case(3001, 3, True, 1)
    for k, stat in ((1, 0), (64, 1), (65, 1), (300, 0), (1024, 1)):
        got, _, _ = profile(c, [(k, stat)])
        assert np.array_equal(got[0], single(c, k, stat))


def test_refusals():
    lib = _native.load()
    P, pos, c = make_case(200, 3, False, 1)
    N = c["N"]
    buf = torch.full((4 * N + GAP,), SENTINEL, dtype=torch.int32, device=DEV)

    def call(cols=((5, 0), (9, 1)), n_cols=None, plane_stride=N, null=(), **over):
        blk = _native.KnnWide(k=max(k for k, _ in cols), stat=0, out_bits=buf, **_fields(c))
        for key, value in over.items():
            setattr(blk, key, value)
        n, col_k, col_stat = _native.column_arrays(cols)
        return lib.flooder_knn_wide_profile_f32(ctypes.byref(blk), n if n_cols is None else n_cols,
                                                None if "col_k" in null else col_k,
                                                None if "col_stat" in null else col_stat, plane_stride,
                                                _native.current_stream_ptr(DEV))

    def refused(match, *args, **kw_):
        assert call(*args, **kw_) == -1
        msg = lib.flooder_last_error().decode()
        assert msg.startswith("flooder_knn_wide_profile_f32") and match in msg, msg

    assert call() == 0
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    n, col_k, col_stat = _native.column_arrays(((5, 0),))
    assert lib.flooder_knn_wide_profile_f32(None, n, col_k, col_stat, N, _native.current_stream_ptr(DEV)) == -1
    refused("abi / size", abi=2)
    refused("abi / size", size=ctypes.sizeof(_native.KnnWide) + 8)
    refused("abi / size", size=4)
    refused("n_cols must be in 1..64", n_cols=0)
    refused("n_cols must be in 1..64", n_cols=65)
    refused("col_k and col_stat must not be NULL", null=("col_k",))
    refused("col_k and col_stat must not be NULL", null=("col_stat",))
    refused("col_k must be in 1..k", ((5, 0), (0, 1)), k=5)
    refused("col_k must be in 1..k", ((5, 0), (9, 1)), k=8)
    refused("col_stat must be 0 (kth) or 1 (dtm)", ((5, 2), (9, 1)))
    refused("col_stat must be 0 (kth) or 1 (dtm)", ((5, 0), (9, -1)))
    refused("listed twice", ((5, 0), (9, 1), (5, 0)))
    refused("k must equal the largest col_k", ((5, 0), (9, 1)), k=10)
    refused("k must be in 1..1024", ((5, 0),), k=1025)
    refused("plane_stride must be at least", plane_stride=N - 1)
    refused("plane_stride must be at least", plane_stride=0)
    # ... and what the single entry refuses
    refused("dim must be in 2..8", dim=9)
    refused("stat must be 0 (kth) or 1 (dtm)", stat=2)
    refused("fewer points than k", ((201, 0),))
    refused("no output", out_bits=None)
    refused("out_ids needs order", out_ids=buf.data_ptr(), order=None)
    # nothing to do: FLOODER_OK before a pointer is looked at (the stride is not judged against no cells)
    assert call(n_simplices=0, pts_sorted=None, nodes=None, plane_stride=0) == 0
    assert call(R=0, verts=None) == 0
    refused("null pointer", pts_sorted=None)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())          # none of the refused or empty calls has written a word
