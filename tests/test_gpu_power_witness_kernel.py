"""``flooder_witness_power`` on its own, through ``_native``: bit for bit against an integer brute force of
``min_x 4 d^2 + 4 w_x^2`` (quarter units) and the smallest id attaining it - one to four tree levels, padded last
leaves, a single point, duplicated points with equal weights, more queries than waves, queries without a witness, zero
weights against ``flooder_witness_search``, the refusals.  The shapes are those of
``test_gpu_flood_grad_kernels.test_witness_search_smallest_id``."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64             # words behind out_point that no call may touch
SENTINEL = -7


def _stream():
    return _native.current_stream_ptr(DEV)


def _brute_power_int(P2, W4, Q2, chunk_elems=1 << 26):
    """Integer brute force on the device.  P2, Q2: coordinates in half units (int32), W4 = 4 w^2 (int32).  Per row of
    Q2: (the minimum word 4 d^2 + 4 w^2, the smallest row of P2 attaining it, the number of rows attaining it, the
    minimum 4 d^2, the smallest row attaining that, is the word's row one of the Euclidean nearest)."""
    n, dim = P2.shape
    per = max(1, chunk_elems // n)
    ids = torch.arange(n, device=P2.device, dtype=torch.int32)
    out = [[] for _ in range(6)]
    for a in range(0, Q2.shape[0], per):
        q = Q2[a:a + per]
        d = (q[:, 0:1] - P2[:, 0].unsqueeze(0)) ** 2
        for k in range(1, dim):
            d += (q[:, k:k + 1] - P2[:, k].unsqueeze(0)) ** 2
        dm = d.min(dim=1).values
        e_first = torch.where(d == dm.unsqueeze(1), ids.unsqueeze(0), n).min(dim=1).values
        word = d + W4.unsqueeze(0)
        m = word.min(dim=1).values
        at = word == m.unsqueeze(1)
        first = torch.where(at, ids.unsqueeze(0), n).min(dim=1).values
        for lst, t in zip(out, (m, first, at.sum(dim=1), dm, e_first,
                                d.gather(1, first.long().unsqueeze(1)).squeeze(1) == dm)):
            lst.append(t)
    return tuple(torch.cat(lst) for lst in out)


# integer coordinates in [0, hi): dense enough that points tied at the minimum are common at half-integer queries
HI = {2: 256, 3: 64, 5: 16, 8: 8}
W_MAX = 3              # integer weights 0 .. W_MAX

SEARCH_CASES = (
    # one tree level; 15 / 17: a padded last leaf; 1: a single point.  (n, dim, duplicated, queries, vertices per query)
    [(n, dim, n > 1 and dim in (3, 8), 500, 2 if dim in (2, 5) else 1) for n in (1, 15, 16, 17) for dim in (2, 3, 5, 8)]
    # one level full / two levels, two levels full / three; more queries than the 16 384 waves of the grid
    + [(1024, 2, False, 70_000, 2), (1024, 8, True, 70_000, 1), (1025, 3, True, 70_000, 1), (1025, 5, False, 70_000, 2),
       (65_536, 3, False, 70_000, 2), (65_536, 5, True, 70_000, 1), (65_537, 2, True, 70_000, 2),
       (65_537, 8, False, 70_000, 1)]
    # four levels: node_w is indexed by the level's offset
    + [(4_300_000, 3, False, 2000, 2)])


def _case(n, dim, dup, n_q, k1):
    """The cloud, its integer weights (the two copies of a doubled point share one), the query table."""
    rng = np.random.default_rng(n * 10 + dim)
    hi = 256 if n > 1_000_000 else HI[dim]
    if dup:            # every point twice (but one, n odd), the copies anywhere in the cloud, with the SAME weight
        half = (n + 1) // 2
        base, wb = rng.integers(0, hi, size=(half, dim)), rng.integers(0, W_MAX + 1, size=half)
        perm = rng.permutation(n)
        P, w = np.concatenate([base, base])[:n][perm], np.concatenate([wb, wb])[:n][perm]
    else:
        P, w = rng.integers(0, hi, size=(n, dim)), rng.integers(0, W_MAX + 1, size=n)
    # query vertices: inside the box, on its boundary, outside it (|coordinate| < 512)
    n_s = n_q // 2 + 1
    kind = rng.random((n_s, k1, 1))
    verts = np.where(kind < 0.6, rng.integers(0, hi, size=(n_s, k1, dim)),
                     np.where(kind < 0.8, rng.choice([0, hi - 1], size=(n_s, k1, dim)),
                              rng.integers(-511, 512, size=(n_s, k1, dim)))).astype(np.float64)
    if k1 == 1:
        verts = verts + rng.choice([0.0, 0.5], size=verts.shape) * (np.abs(verts) < 511)   # half-integer positions
        W = np.array([[1.0]])
    else:
        W = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])       # the midpoint of two integer vertices: half-integers
    q_s = rng.integers(0, n_s, size=n_q).astype(np.int32)
    q_r = rng.integers(0, W.shape[0], size=n_q).astype(np.int32)
    pos = np.einsum("qk,qkd->qd", W[q_r], verts[q_s])
    assert np.array_equal(pos * 2, np.round(pos * 2)) and np.abs(pos).max() < 512
    return P, w, verts, W, q_s, q_r, pos, n_s


def _launch(index, w_sorted, node_w, dim, k1, verts, W, n_s, q_s, q_r, bits, entry="flooder_witness_power"):
    """-> (out_point (n_q,) with its guard checked, not_found)."""
    n_q = q_s.shape[0]
    buf = torch.full((n_q + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    not_found = torch.zeros(1, dtype=torch.int32, device=DEV)
    blk = _native.WitnessSearch(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=k1, nodes=index.nodes,
                                order=index.order32, verts=verts, weights=W, R=W.shape[0], n_simplices=n_s,
                                n_queries=n_q, q_simplex=q_s, q_row=q_r, q_d2=bits, out_point=buf[:n_q],
                                not_found=not_found)
    lib = _native.load()
    if entry == "flooder_witness_power":
        rc = lib.flooder_witness_power(ctypes.byref(blk), _native.ptr(w_sorted), _native.ptr(node_w), _stream())
    else:
        rc = lib.flooder_witness_search(ctypes.byref(blk), _stream())
    _native.check(rc, entry)
    assert bool((buf[n_q:] == SENTINEL).all()), "guard words behind out_point were written"
    return buf[:n_q], int(not_found.item())


@pytest.mark.parametrize("n,dim,dup,n_q,k1", SEARCH_CASES)
def test_witness_power_smallest_id(n, dim, dup, n_q, k1):
    P, w, verts, W, q_s, q_r, pos, n_s = _case(n, dim, dup, n_q, k1)
    R = W.shape[0]
    # exactness: in half units every difference is an integer; per axis the largest |q - p|, squared and summed, plus
    # the largest 4 w^2 bounds EVERY word of every (query, point) pair in quarter units: below 2**24 the kernel's fma
    # chain, whatever its order, and the integer brute force give the same number
    far = np.maximum(pos.max(0) - P.min(0), P.max(0) - pos.min(0))
    assert int(((2 * far) ** 2).sum()) + 4 * int(w.max()) ** 2 < 2 ** 24

    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    tw = torch.as_tensor(w, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    order = index.order32.long()
    assert torch.equal(torch.sort(order).values, torch.arange(n, device=DEV))
    w_sorted, node_w = core._power_weights(index, tw)
    assert w_sorted.shape[0] == index.pts.shape[0] and bool(torch.isinf(w_sorted[n:]).all())   # the padded last leaf
    assert torch.equal(w_sorted[:n], tw[order])

    P2 = torch.as_tensor(2 * P, dtype=torch.int32, device=DEV)
    Q2 = torch.as_tensor(np.round(2 * pos), dtype=torch.int32, device=DEV)
    word, first, count, dmin, e_first, euclid = _brute_power_int(P2, torch.as_tensor(4 * w * w, dtype=torch.int32, device=DEV), Q2)
    assert int(word.max()) < 2 ** 24
    bits = (word.to(torch.float32) / 4).contiguous().view(torch.int32).clone()   # exact: an integer below 2**24 over four
    want = first.long().cpu().numpy()
    # the reference alone: the case has something to decide
    tied, decided = float((count[:500] > 1).float().mean()), float((~euclid).float().mean())
    print(f"n {n} dim {dim} dup {dup}: more than one point at the minimum on {tied:.1%} of the first 500 queries, "
          f"the power-nearest point is no Euclidean nearest point on {decided:.1%}")
    if dup and n >= 1024:
        assert tied > 0.5
    if not dup and n >= 1024:
        assert decided > 0.02

    # queries without a witness, as data: a target one ulp above the true word (word < 2**20: the next float is no
    # multiple of a quarter, no point can be there), a row index of R, a simplex index of -1 and of n_simplices
    small = np.nonzero((word.cpu().numpy() < 4 * 2 ** 20))[0]
    bad_ulp, bad_row, bad_s, bad_s2 = small[:3], np.array([5, 6]) % n_q, np.array([7]) % n_q, np.array([8]) % n_q
    bad_ulp = bad_ulp[~np.isin(bad_ulp, np.concatenate([bad_row, bad_s, bad_s2]))]
    assert bad_ulp.size > 0
    bits[torch.as_tensor(bad_ulp, device=DEV)] += 1
    q_r, q_s = q_r.copy(), q_s.copy()
    q_r[bad_row] = R
    q_s[bad_s] = -1
    q_s[bad_s2] = n_s
    bad = np.unique(np.concatenate([bad_ulp, bad_row, bad_s, bad_s2]))
    want[bad] = -1

    t_verts = torch.as_tensor(verts, dtype=torch.float32, device=DEV).contiguous()
    t_w = torch.as_tensor(W, dtype=torch.float32, device=DEV).contiguous()
    t_qs, t_qr = torch.as_tensor(q_s, device=DEV), torch.as_tensor(q_r, device=DEV)
    out, missing = _launch(index, w_sorted, node_w, dim, k1, t_verts, t_w, n_s, t_qs, t_qr, bits)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5].ravel(), got[got != want][:5], want[got != want][:5])
    assert missing == bad.size

    # zero weights: the Euclidean words, and the outputs of flooder_witness_search on the same block, word for word
    zero_sorted, zero_node = core._power_weights(index, torch.zeros_like(tw))
    e_bits = (dmin.to(torch.float32) / 4).contiguous().view(torch.int32).clone()
    e_bits[torch.as_tensor(bad_ulp, device=DEV)] += 1
    out0, missing0 = _launch(index, zero_sorted, zero_node, dim, k1, t_verts, t_w, n_s, t_qs, t_qr, e_bits)
    out1, missing1 = _launch(index, None, None, dim, k1, t_verts, t_w, n_s, t_qs, t_qr, e_bits, "flooder_witness_search")
    assert torch.equal(out0, out1) and missing0 == missing1
    e_want = e_first.long().cpu().numpy()
    e_want[bad] = -1
    assert np.array_equal(out0.cpu().numpy(), e_want)


def test_refused_calls_leave_the_outputs_alone():
    rng = np.random.default_rng(3)
    n, dim, n_q = 300, 3, 40
    tp = torch.as_tensor(rng.integers(0, 32, size=(n, dim)), dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    w_sorted, node_w = core._power_weights(index, torch.ones(n, device=DEV))
    verts = tp[:n_q].clone().unsqueeze(1).contiguous()
    one = torch.ones((1, 1), dtype=torch.float32, device=DEV)
    q_s = torch.arange(n_q, dtype=torch.int32, device=DEV)
    q_r = torch.zeros(n_q, dtype=torch.int32, device=DEV)
    bits = torch.ones(n_q, dtype=torch.float32, device=DEV).view(torch.int32)     # the word of a landmark: 0 + 1^2
    out = torch.full((n_q,), SENTINEL, dtype=torch.int64, device=DEV)
    not_found = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = _native.load()

    def call(ws=w_sorted, nw=node_w, tweak=None, **kw):
        fields = dict(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=1, nodes=index.nodes, order=index.order32,
                      verts=verts, weights=one, R=1, n_simplices=n_q, n_queries=n_q, q_simplex=q_s, q_row=q_r,
                      q_d2=bits, out_point=out, not_found=not_found)
        fields.update(kw)
        blk = _native.WitnessSearch(**fields)
        if tweak:
            tweak(blk)
        return lib.flooder_witness_power(ctypes.byref(blk), _native.ptr(ws), _native.ptr(nw), _stream())

    def bad_abi(blk):
        blk.abi = 2

    def bad_size(blk):
        blk.size += 8

    def short_size(blk):
        blk.size = 4

    for what, rc in (("null w_sorted", call(ws=None)), ("null node_w", call(nw=None)), ("dim 1", call(dim=1)),
                     ("dim 9", call(dim=9)), ("abi", call(tweak=bad_abi)), ("size", call(tweak=bad_size)),
                     ("short size", call(tweak=short_size)),
                     ("null block", lib.flooder_witness_power(None, _native.ptr(w_sorted), _native.ptr(node_w), _stream()))):
        assert rc == -1, what
        assert lib.flooder_last_error().decode().startswith("flooder_witness_power"), what
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and int(not_found.item()) == 0, what
    assert call(n_queries=0) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and int(not_found.item()) == 0
    # ... and the call they refuse parts of works: every landmark is a cloud point of weight 1
    assert call() == 0
    assert int(not_found.item()) == 0 and bool((tp[out] == tp[:n_q]).all())
