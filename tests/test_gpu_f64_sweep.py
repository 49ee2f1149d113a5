"""The float64 device route (``csrc/flood_f64.hip``) on coordinates float32 cannot hold: ``flooder_sweep_bvh_f64`` bit
for bit against the float64 brute force over all points on inputs where double arithmetic is exact (and within the
rounding of a squared distance on inputs where it is not), ``flooder_gather_rows_f64`` and ``flooder_face_max_f64`` on
their own, and ``flood_complex`` on ROCm float64 tensors - whole and in point / simplex shards - against the kd-tree
path on clouds a million units away from the origin.  The inputs and what makes them bite: ``f64_reference``."""

import functools

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core

import f64_reference as fr
import grad_reference as gr

gpu = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64      # words behind every output buffer that no kernel may touch


def _stream():
    return _native.current_stream_ptr(DEV)


def _seed(dim, n, ppe):
    return 1000 * dim + n % 997 + ppe


# (dim, n points, every point doubled, points_per_edge, simplex dimension, simplices, tree levels, log2 of the spread of
# the integer part).  n = 1 / 15: one padded leaf; 40 / 1000: one level; 1025 / 30 001: two; 70 001: three; 4 300 001:
# four.  No n is a multiple of 16.  The spread is the widest power of two at which the median nearest-neighbour
# distance of the samples (kd-tree over the float64 cloud, on the host) stays near 0.06, half the float32 ulp at 2**20;
# ``assert_neighbours_below_ulp`` checks the condition itself on every run.
SWEEP_CASES = [
    (2, 40, False, 5, 0, 40, 1, 9), (2, 1025, True, 9, 2, 40, 2, 11), (2, 70_001, False, 17, 2, 40, 3, 14),
    (2, 4_300_001, True, 5, 1, 8, 4, 14),
    (3, 1000, True, 17, 1, 40, 1, 9), (3, 30_001, False, 9, 3, 30, 2, 11), (3, 70_001, True, 5, 3, 40, 3, 11),
    (3, 4_300_001, False, 5, 3, 8, 4, 13),
    (4, 40, True, 9, 4, 20, 1, 7), (4, 30_001, True, 5, 4, 30, 2, 9), (4, 70_001, False, 17, 2, 40, 3, 10),
    (4, 4_300_001, False, 5, 2, 8, 4, 11),
    (5, 1000, False, 5, 5, 30, 1, 8), (5, 1025, False, 17, 3, 20, 2, 8), (5, 70_001, True, 9, 2, 40, 3, 9),
    (5, 4_300_001, True, 5, 3, 8, 4, 10),
    (8, 1000, False, 5, 8, 12, 1, 7), (8, 30_001, True, 17, 1, 60, 2, 7), (8, 70_001, False, 9, 3, 40, 3, 7),
    (8, 4_300_001, True, 5, 2, 8, 4, 8),
    (3, 1, False, 5, 2, 8, 1, 6), (8, 15, False, 9, 1, 8, 1, 6), (2, 15, True, 9, 1, 8, 1, 8), (5, 1, False, 9, 0, 8, 1, 5),
]
DIMS = (2, 3, 4, 5, 8)


def _rows_per_simplex(ppe, d):
    return gr.lattice(ppe, d).shape[0]


def test_sweep_cases_cover_what_they_must():
    assert {c[0] for c in SWEEP_CASES} == set(DIMS)                    # padded widths 2, 4, 8 and DIM < DP (3, 5)
    assert {c[3] for c in SWEEP_CASES} == {5, 9, 17}
    for dim in DIMS:
        mine = [c for c in SWEEP_CASES if c[0] == dim]
        assert {c[6] for c in mine} == {1, 2, 3, 4}
        assert {c[2] for c in mine} == {True, False}
        assert all(c[4] <= dim for c in mine)
    assert all(c[1] % 16 != 0 and fr.tree_levels(c[1]) == c[6] for c in SWEEP_CASES)
    assert {1, 15} <= {c[1] for c in SWEEP_CASES}
    assert {0, 8} <= {c[4] for c in SWEEP_CASES} and max(c[4] + 1 for c in SWEEP_CASES) == 9    # k1 from 1 to 9
    rows = {_rows_per_simplex(c[3], c[4]) for c in SWEEP_CASES}
    assert 1 in rows and any(1 < r < 64 for r in rows) and any(r > 64 for r in rows)
    assert all(r % 64 != 0 for r in rows)
    assert all(c[3] == 5 and c[5] == 8 for c in SWEEP_CASES if c[6] == 4)


@pytest.mark.parametrize("dim", DIMS)
def test_exact_inputs_leave_float32_on_the_host(dim):
    """The smallest case of every dimension, without a device: double arithmetic is exact on it, float32 holds next to
    none of its coordinates, and the samples' true nearest neighbours are closer than a float32 ulp."""
    _, n, dup, ppe, d, n_s, _, e = min((c for c in SWEEP_CASES if c[0] == dim), key=lambda c: c[1])
    P, V, off = fr.exact_case(dim, n, dup, d, n_s, 2 ** e, _seed(dim, n, ppe))
    assert (off > 0).any() and (off < 0).any() and off[0] == 2.0 ** 20 and (np.abs(off) == 2.0 ** 20).all()
    assert fr.assert_exact_inputs_f64(P, V, ppe) < 2 ** 53
    fr.assert_float32_cannot_hold(P)
    samples = torch.einsum("rk,skd->srd", gr.lattice(ppe, d), torch.as_tensor(V))
    d2, _, _ = gr.nearest_points(torch.as_tensor(P), samples.reshape(-1, dim))
    fr.assert_neighbours_below_ulp(d2.numpy())
    with pytest.raises(AssertionError):      # the helper does tell: float32 numbers are no such input
        fr.assert_float32_cannot_hold(P.astype(np.float32))
    with pytest.raises(AssertionError):
        fr.assert_exact_inputs_f64(P + 2.0 ** -11, V, ppe)


# ------------------------------------------------------------------------------------------------ the three exports
def _gather(points: torch.Tensor, index, ld=None, base=None):
    """``flooder_gather_rows_f64`` into a buffer of sentinels with a guard behind it; (n_pad, DP) rows."""
    n, dim = points.shape
    n_pad, dp = index.pts.shape
    buf = torch.full((n_pad * dp + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    src = points.contiguous() if base is None else base
    _native.check(_native.load().flooder_gather_rows_f64(_native.ptr(src), n, dim, dim if ld is None else ld,
                                                         _native.ptr(index.order32), _native.ptr(buf), n_pad, _stream()),
                  "flooder_gather_rows_f64")
    assert bool((buf[n_pad * dp:] == -7.0).all()), "gather wrote behind its output"
    return buf[:n_pad * dp].view(n_pad, dp)


def _check_gathered(rows, points, index):
    n, dim = points.shape
    n_pad, dp = index.pts.shape
    assert n_pad % 16 == 0 and n_pad - 16 < n <= n_pad
    assert torch.equal(rows[:n, :dim], points[index.order32.long()]), "rows are not points[order]"
    assert bool((rows[:n, dim:] == 0).all()), "pad columns of real rows are not 0"
    assert bool((rows[n:] == float("inf")).all()), "padding rows are not +inf in every column"
    assert torch.equal(rows.to(torch.float32).view(torch.int32), index.pts.view(torch.int32)), \
        "rows rounded to float32 are not the rows of the index"


def _sweep(rows, index, verts, weights, n_s):
    """``flooder_sweep_bvh_f64`` into words prefilled with -1 and a guard behind them; (n_s, R) int64 on the host."""
    R, k1 = weights.shape
    buf = torch.full((n_s * R + GUARD,), -1, dtype=torch.int64, device=DEV)
    queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
    _native.check(_native.load().flooder_sweep_bvh_f64(_native.ptr(rows), index.n, index.dim, _native.ptr(index.nodes),
                                                       _native.ptr(verts), _native.ptr(weights), k1, R, n_s,
                                                       _native.ptr(queue), _native.ptr(buf), _stream()),
                  "flooder_sweep_bvh_f64")
    out = buf.cpu().numpy()
    assert (out[n_s * R:] == -1).all(), "the sweep wrote behind row R of the last simplex"
    out = out[:n_s * R].reshape(n_s, R)
    assert out.shape == (n_s, R)
    return out


def _prepare(P, V, W, ppe):
    """Index, gathered rows (checked), device tensors, the brute-force minimum d2 of every sample, and the conditions
    that make the case bite."""
    n, dim = P.shape
    tp = torch.as_tensor(P, device=DEV)
    index = core.PointIndex(tp)
    rows = _gather(tp, index)
    _check_gathered(rows, tp, index)
    fr.assert_float32_cannot_hold(P)
    share = fr.assert_leaves_need_widening(rows, index.nodes, n, dim)
    tv = torch.as_tensor(V, device=DEV).contiguous()
    tw = W.to(DEV).contiguous()
    samples = torch.einsum("rk,skd->srd", tw, tv)
    ref, _, _ = gr.nearest_points(tp, samples.reshape(-1, dim), chunk_bytes=1 << 30)
    ref = ref.cpu().numpy().reshape(V.shape[0], W.shape[0])
    med = fr.assert_neighbours_below_ulp(ref)
    return index, rows, tv, tw, ref, share, med


@gpu
@pytest.mark.parametrize("dim,n,dup,ppe,d,n_s,levels,e", SWEEP_CASES)
def test_sweep_words_equal_the_brute_force(dim, n, dup, ppe, d, n_s, levels, e):
    """Exact inputs: the int64 words ARE the float64 brute-force minima; nothing beyond row R is written; a second call
    gives the same words."""
    P, V, _ = fr.exact_case(dim, n, dup, d, n_s, 2 ** e, _seed(dim, n, ppe))
    W = gr.lattice(ppe, d)
    bound = fr.assert_exact_inputs_f64(P, V, ppe)
    index, rows, tv, tw, ref, share, med = _prepare(P, V, W, ppe)
    print(f"dim {dim} n {n}: d2 below 2**{np.log2(max(bound, 1)):.1f} units, {fr.float32_survivors(P):.2%} of the "
          f"coordinates are float32 numbers, {share:.0%} of the leaves hold a row outside their float32 box, median "
          f"nearest-neighbour distance {med:.4f}")
    want = ref.view(np.int64)
    got = _sweep(rows, index, tv, tw, n_s)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert np.array_equal(_sweep(rows, index, tv, tw, n_s), got)


INEXACT_CASES = [c for c in SWEEP_CASES if c[6] < 4] + [c for c in SWEEP_CASES if c[6] == 4 and c[0] in (3, 8)]


@gpu
@pytest.mark.parametrize("dim,n,dup,ppe,d,n_s,levels,e", INEXACT_CASES)
def test_sweep_within_rounding_on_inexact_points(dim, n, dup, ppe, d, n_s, levels, e):
    """Points with full mantissas (``randn * 1e-3 + offsets``), exact samples: the kernel's d2 and the brute force's
    are both within gamma = gamma_(dim+2) (``f64_reference.gamma``) of the true squared distance of every point, the
    minimum over the points is monotone, so the two minima differ by at most 2 gamma times the true minimum, which is
    at most ref / (1 - gamma).  (Observed: the words coincide.  Doubles next to 2**20 lie on a grid of 2**-32, the
    differences to a sample a few thousandths away have some 25 significant bits, and their squares and sums are exact
    in double after all; the bound is what is guaranteed, not what these offsets provoke.)"""
    _, V, off = fr.exact_case(dim, n, dup, d, n_s, 4, _seed(dim, n, ppe))     # vertices within 4 sigma of the offsets
    P = fr.inexact_cloud(dim, n, off, _seed(dim, n, ppe) + 1)
    W = gr.lattice(ppe, d)
    index, rows, tv, tw, ref, share, med = _prepare(P, V, W, ppe)
    got = _sweep(rows, index, tv, tw, n_s).view(np.float64)
    assert np.isfinite(got).all() and (got >= 0).all()
    g = fr.gamma(dim)
    bound = 2 * g * ref / (1 - g)
    err = np.abs(got - ref)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"dim {dim} n {n}: worst |d2 - brute force| / bound {ratio:.3f}, {(got != ref).mean():.1%} of the words differ, "
          f"median nearest-neighbour distance {med:.5f}")
    assert (err <= bound).all(), ratio
    assert np.array_equal(_sweep(rows, index, tv, tw, n_s).view(np.float64), got)


WEIGHT_CASES = [c for c in SWEEP_CASES if c[6] == 2]      # one two-level cloud per dimension


@gpu
@pytest.mark.parametrize("dim,n,dup,ppe,d,n_s,levels,e", WEIGHT_CASES)
def test_sweep_reads_the_weights_in_double(dim, n, dup, ppe, d, n_s, levels, e):
    """70 rows of barycentric weights with full mantissas (no float32 numbers) on the exact cloud.  The sample is now
    rounded: with c the largest |coordinate| and k1 vertices, a sum of k1 products in any order is within
    gamma_(k1+1) c sum(w) of the true coordinate, on the device and in the reference, so the two samples are at most
    delta = 2 sqrt(dim) gamma_(k1+1) c sum(w) apart, and so are their true nearest-neighbour distances (1-Lipschitz);
    each computed d2 is within gamma = gamma_(dim+2) of its own true value, its root within gamma as well:
    |sqrt(d2) - sqrt(ref)| <= delta + 2 gamma max(sqrt(d2), sqrt(ref)) / (1 - gamma).  About 1e-8 here; weights
    read through float32 move a sample by up to 2**-24 * 2**20 = 0.06."""
    P, V, _ = fr.exact_case(dim, n, dup, d, n_s, 2 ** e, _seed(dim, n, ppe))
    rng = np.random.default_rng(_seed(dim, n, ppe) + 2)
    W = rng.dirichlet(np.ones(d + 1), size=70)
    assert fr.float32_survivors(W) == 0.0 and (W > 0).all()
    index, rows, tv, tw, ref, share, med = _prepare(P, V, torch.as_tensor(W), ppe)
    got = np.sqrt(_sweep(rows, index, tv, tw, n_s).view(np.float64))
    ref = np.sqrt(ref)
    k = d + 2
    c = max(np.abs(P).max(), np.abs(V).max())
    delta = 2 * np.sqrt(dim) * (k * fr.U64 / (1 - k * fr.U64)) * c * W.sum(axis=1).max()
    g = fr.gamma(dim)
    bound = delta + 2 * g * np.maximum(got, ref) / (1 - g)
    err = np.abs(got - ref)
    print(f"dim {dim} n {n}: worst |distance - brute force| {err.max():.3e}, worst ratio to the bound "
          f"{(err / bound).max():.3f} (bound {bound.max():.3e}), median nearest-neighbour distance {med:.4f}")
    assert (err <= bound).all(), float((err / bound).max())


@gpu
def test_sweep_refusals():
    P, V, _ = fr.exact_case(3, 40, False, 2, 4, 2 ** 7, 5)
    W = gr.lattice(5, 2)
    tp = torch.as_tensor(P, device=DEV)
    index = core.PointIndex(tp)
    rows = _gather(tp, index)
    tv, tw = torch.as_tensor(V, device=DEV).contiguous(), W.to(DEV).contiguous()
    wide = torch.zeros((15, 10), dtype=torch.float64, device=DEV)
    out = torch.full((4, 15), -1, dtype=torch.int64, device=DEV)
    queue = torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)
    lib = _native.load()
    good = dict(pts=_native.ptr(rows), n=40, dim=3, nodes=_native.ptr(index.nodes), verts=_native.ptr(tv),
                weights=_native.ptr(tw), k1=3, R=15, ns=4, queue=_native.ptr(queue), out=_native.ptr(out))

    def call(**change):
        a = {**good, **change}
        return lib.flooder_sweep_bvh_f64(a["pts"], a["n"], a["dim"], a["nodes"], a["verts"], a["weights"], a["k1"], a["R"],
                                         a["ns"], a["queue"], a["out"], _stream())

    for name in ("pts", "nodes", "verts", "weights", "queue", "out"):
        assert call(**{name: None}) != 0, name
    assert call(k1=10, weights=_native.ptr(wide)) != 0          # FLOODER_MAX_VERTS is 9
    assert call(n=0) != 0
    assert call(R=0) == 0 and call(ns=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "an empty call wrote to its output"
    assert call() == 0
    assert bool((out != -1).all())
    # the gather's own refusals
    buf = torch.empty_like(rows)
    o = _native.ptr(index.order32)
    assert lib.flooder_gather_rows_f64(None, 40, 3, 3, o, _native.ptr(buf), 48, _stream()) != 0
    assert lib.flooder_gather_rows_f64(_native.ptr(tp), 40, 3, 3, None, _native.ptr(buf), 48, _stream()) != 0
    assert lib.flooder_gather_rows_f64(_native.ptr(tp), 40, 3, 3, o, None, 48, _stream()) != 0
    assert lib.flooder_gather_rows_f64(_native.ptr(tp), 0, 3, 3, o, _native.ptr(buf), 48, _stream()) != 0
    assert lib.flooder_gather_rows_f64(_native.ptr(tp), 40, 3, 2, o, _native.ptr(buf), 48, _stream()) != 0    # ld < dim
    assert lib.flooder_gather_rows_f64(_native.ptr(tp), 40, 3, 3, o, _native.ptr(buf), 39, _stream()) != 0    # n_pad < n


# (dim, n, leading dimension): ld == dim and a strided view of a wider tensor; 4 300 001 rows pad to more than
# 8192 * 256, so the kernel's stride loop takes a second turn
GATHER_CASES = [(2, 40, 2), (2, 1000, 5), (3, 15, 4), (3, 1025, 3), (4, 1, 4), (4, 1025, 6), (5, 30_001, 7), (8, 1000, 8),
                (8, 70_001, 11), (3, 4_300_001, 5), (8, 4_300_001, 8)]


def test_gather_cases_cover_what_they_must():
    assert {c[0] for c in GATHER_CASES} == set(DIMS)
    assert any(c[2] == c[0] for c in GATHER_CASES) and any(c[2] > c[0] for c in GATHER_CASES)
    assert any((c[1] + 15) // 16 * 16 > 8192 * 256 for c in GATHER_CASES)
    assert {1, 15} <= {c[1] for c in GATHER_CASES}


@gpu
@pytest.mark.parametrize("dim,n,ld", GATHER_CASES)
def test_gather_rows(dim, n, ld):
    rng = np.random.default_rng(n + ld)
    wide = np.full((n, ld), 7e7)                              # what a wrong stride would pick up
    wide[:, :dim] = fr.axis_offsets(dim, rng) + rng.integers(-2 ** 12, 2 ** 12 + 1, size=(n, dim)) * fr.GRID
    base = torch.as_tensor(wide, device=DEV)
    view = base[:, :dim]
    assert view.is_contiguous() == (ld == dim)
    index = core.PointIndex(view)
    order = index.order32.long()
    assert torch.equal(torch.sort(order).values, torch.arange(n, device=DEV)), "the index's order is no permutation"
    rows = _gather(view, index, ld=ld, base=base)
    _check_gathered(rows, view, index)


FACE_R = (1, 63, 64, 65, 255, 256, 257, 1000)


def _face_words(rng, S, R):
    """(S, R) non-negative doubles of every size, with +inf, 0 and denormals among them."""
    v = np.abs(rng.standard_normal((S, R))) * 10.0 ** rng.uniform(-300, 300, size=(S, R))
    kind = rng.integers(0, 12, size=(S, R))
    v[kind == 0] = 0.0
    v[kind == 1] = np.inf
    v[kind == 2] = (rng.integers(1, 2 ** 40, size=(S, R)) * 5e-324)[kind == 2]       # denormals
    v[kind == 3] = 2.2250738585072014e-308                                          # the smallest normal
    assert (v >= 0).all() and np.isinf(v).any() == (kind == 1).any()
    return v


def _face_table(rng, R, n_faces):
    """Ranges of length 1, 64, 65 and all of R (cut to R), rows drawn with repetition within and across faces."""
    lens = [1, min(64, R), min(65, R), R]
    rows, ptr = [], [0]
    for f in range(n_faces):
        L = lens[f % 4]
        rows.append(rng.permutation(R) if L == R and f % 8 == 3 else rng.integers(0, R, size=L))
        ptr.append(ptr[-1] + L)
    return np.asarray(ptr, dtype=np.int32), np.concatenate(rows).astype(np.int32)


def _face_max(words, ptr, rows, want_dist):
    S, R = words.shape
    F = len(ptr) - 1
    t_w = torch.as_tensor(words.view(np.int64), device=DEV)
    face = torch.full((S * F + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    dist = torch.full((S * R + GUARD,), -7.0, dtype=torch.float64, device=DEV) if want_dist else None
    t_ptr, t_rows = torch.as_tensor(ptr, device=DEV), torch.as_tensor(rows, device=DEV)
    _native.check(_native.load().flooder_face_max_f64(_native.ptr(t_w), S, R, _native.ptr(t_ptr), _native.ptr(t_rows), F,
                                                      _native.ptr(face), _native.ptr(dist), _stream()),
                  "flooder_face_max_f64")
    face = face.cpu().numpy()
    assert (face[S * F:] == -7.0).all()
    if want_dist:
        dist = dist.cpu().numpy()
        assert (dist[S * R:] == -7.0).all()
        dist = dist[:S * R].reshape(S, R)
    assert torch.equal(t_w.cpu(), torch.as_tensor(words.view(np.int64))), "the d2 words were changed"
    return face[:S * F].reshape(S, F), dist


@gpu
@pytest.mark.parametrize("R", FACE_R)
def test_face_max_bitwise(R):
    """``out_face`` is, bit for bit, ``np.sqrt`` of the numpy maximum over the face's rows and ``out_dist`` ``np.sqrt``
    of every word: the device square root of a double is correctly rounded, denormals included."""
    rng = np.random.default_rng(R)
    for S in (1, 3, 1000):
        words = _face_words(rng, S, R)
        for n_faces in (1, 5, 32):
            ptr, rows = _face_table(rng, R, n_faces)
            want = np.stack([words[:, rows[ptr[f]:ptr[f + 1]]].max(axis=1) for f in range(n_faces)], axis=1)
            with np.errstate(all="ignore"):
                want, want_dist = np.sqrt(want), np.sqrt(words)
            for with_dist in (False, True):
                face, dist = _face_max(words, ptr, rows, with_dist)
                bad = np.argwhere(face.view(np.int64) != want.view(np.int64))
                assert len(bad) == 0, (S, n_faces, with_dist, bad[:5].tolist())
                if with_dist:
                    assert np.array_equal(dist.view(np.int64), want_dist.view(np.int64)), (S, n_faces)


@gpu
def test_face_max_empty_face_is_zero():
    """A face without rows (``face_ptr[f] == face_ptr[f + 1]``) gets +0.0: the maximum starts from the zero word."""
    words = _face_words(np.random.default_rng(3), 5, 70) + 1.0
    ptr = np.asarray([0, 0, 3, 3, 70], dtype=np.int32)
    rows = np.concatenate([[4, 69, 0], np.arange(3, 70)]).astype(np.int32)
    face, _ = _face_max(words, ptr, rows, True)
    assert (face[:, [0, 2]].view(np.int64) == 0).all()
    assert np.array_equal(face[:, 1], np.sqrt(words[:, [4, 69, 0]].max(axis=1)))
    assert np.array_equal(face[:, 3], np.sqrt(words[:, 3:].max(axis=1)))


# ------------------------------------------------------------------------------------------------ end to end
def _fc(*args, **kw):
    with pytest.warns(RuntimeWarning):
        return fa.flood_complex(*args, **kw)


@functools.lru_cache(maxsize=None)
def _offset_cloud(name):
    """(points, landmarks) float64 numpy and the keyword arguments of the call."""
    from oracle import flood_oracle as fo

    if name == "torus":
        P = fr.noisy_torus_f64(30_000, seed=5) + np.array([1e6, -1e6, 1e6])
        return P, P[fo.exact_fps(P, 150, 0)], (("points_per_edge", 12),)
    P = fr.figure_eight_f64(20_000, seed=6) + np.array([2.0 ** 20, -2.0 ** 20])
    return P, P[fo.exact_fps(P, 100, 0)], (("points_per_edge", None), ("num_rand", 200))


@functools.lru_cache(maxsize=None)
def _unsharded(name):
    P, L, kw = _offset_cloud(name)
    torch.manual_seed(7)
    return _fc(torch.as_tensor(P, device=DEV), torch.as_tensor(L, device=DEV), **dict(kw))


@gpu
@pytest.mark.parametrize("name", ["torus", "eight"])
def test_offset_cloud_matches_the_kdtree_path(name):
    """ROCm float64 ``flood_complex`` against the CPU float64 one (kd-tree over the same doubles), within the gate of
    ``test_float64_input_gpu``; rounding the cloud to float32 moves these points by up to 0.06."""
    P, L, kw = _offset_cloud(name)
    fr.assert_float32_cannot_hold(P)
    got = _unsharded(name)
    torch.manual_seed(7)
    ref = _fc(torch.as_tensor(P), torch.as_tensor(L), **dict(kw))
    assert set(got) == set(ref)
    keys = sorted(ref)
    a, b = np.array([got[k] for k in keys]), np.array([ref[k] for k in keys])
    scale = float(np.abs(P).max())
    gate = 1e-12 * scale + 1e-11 * np.abs(b).max()
    worst = float(np.abs(a - b).max())
    print(f"{name}: {len(keys)} simplices, largest value {b.max():.4f}, worst |device - kd-tree| {worst:.3e}, gate {gate:.3e}")
    assert worst <= gate, worst


@gpu
def test_point_shards_min_reduce_int64_words():
    """Three point shards, MIN of the (S, R) int64 words through ``reduce_hook``: the unsharded dict, bit for bit."""
    P, L, kw = _offset_cloud("torus")
    full = _unsharded("torus")
    tp, tl = torch.as_tensor(P, device=DEV), torch.as_tensor(L, device=DEV)
    axis = int(np.argmax(P.max(0) - P.min(0)))
    captured = []
    for r in range(3):
        _fc(tp[r::3].contiguous(), tl, sort_axis=axis, reduce_hook=lambda buf, c=captured: c.append(buf.clone()), **dict(kw))
    assert len(captured) == 3 and all(b.dtype is torch.int64 and b.dim() == 2 for b in captured)
    assert not torch.equal(captured[0], captured[1])
    merged = torch.minimum(torch.minimum(captured[0], captured[1]), captured[2])
    out = _fc(tp[0::3].contiguous(), tl, sort_axis=axis, reduce_hook=lambda buf: buf.copy_(merged), **dict(kw))
    assert out == full


@gpu
def test_simplex_shards_min_reduce_float64_faces():
    """Three simplex shards, MIN of the (S, F) float64 face values through ``face_reduce_hook``: the unsharded dict."""
    P, L, kw = _offset_cloud("torus")
    full = _unsharded("torus")
    tp, tl = torch.as_tensor(P, device=DEV), torch.as_tensor(L, device=DEV)
    bufs = []
    for r in range(3):
        _fc(tp, tl, simplex_shard=(r, 3), face_reduce_hook=lambda buf, c=bufs: c.append(buf.clone()), **dict(kw))
    assert len(bufs) == 3 and all(b.dtype is torch.float64 for b in bufs)
    merged = torch.minimum(torch.minimum(bufs[0], bufs[1]), bufs[2])
    assert bool(torch.isfinite(merged).all()) and not bool(torch.isfinite(bufs[0]).all())
    out = _fc(tp, tl, simplex_shard=(0, 3), face_reduce_hook=lambda buf: buf.copy_(merged), **dict(kw))
    assert out == full
