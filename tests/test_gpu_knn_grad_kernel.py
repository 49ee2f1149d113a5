"""``flooder_witness_knn`` on its own, bit for bit against an integer brute force over all points: the k smallest
(d2, original id) keys in order, their d2 words, the refusal of queries whose statistic does not match - on clouds
where equidistant points at the k-th place are the rule (integer coordinates, half-integer queries, doubled points),
from one point to four tree levels, with padded last leaves, k = n, and a grid-stride loop that wraps."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import grad_reference as gr
import knn_grad_reference as kr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KS = kr.KS
HI = {2: 256, 3: 64, 5: 16, 8: 8}      # the coordinate ranges of test_witness_search_smallest_id

# (n points, dim, every point doubled, queries per k, the k to run)
CASES = (
    # one tree level; 1: a single point; 15 / 17 / 33: a padded last leaf; k = n: its rows must not leak in; 33 points
    # with k = 32: a list longer than half a wave
    [(n, dim, n > 1 and dim in (3, 8), 500, KS) for n in (1, 15, 16, 17, 32, 33) for dim in (2, 3, 5, 8)]
    # two levels; (1025, 3): more queries than the 16 384 waves of the grid at one k
    + [(1024, 2, False, 2000, KS), (1024, 8, True, 2000, KS), (1025, 3, True, 2000, KS), (1025, 5, False, 2000, KS),
       (1025, 3, True, 70_000, (5,))]
    # three levels
    + [(65_536, 3, False, 2000, KS), (65_536, 5, True, 2000, KS), (65_537, 2, True, 2000, KS),
       (65_537, 8, False, 2000, KS)]
    # four levels
    + [(4_300_001, 3, False, 500, (1, 5, 32))])


def make_case(n, dim, dup, n_q):
    """(P (n, dim) int, verts (n_s, k1, dim) f64, W (R, k1) f64, q_s, q_r, pos (n_q, dim) f64), as
    test_witness_search_smallest_id builds them."""
    rng = np.random.default_rng(n * 10 + dim + (7 if n_q > 10_000 else 0))
    hi = 256 if n > 1_000_000 else HI[dim]
    if dup:            # every point twice (but one, n odd), the copies anywhere in the cloud
        base = rng.integers(0, hi, size=((n + 1) // 2, dim))
        P = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        P = rng.integers(0, hi, size=(n, dim))
    k1 = 2 if dim in (2, 5) else 1
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
    return P, hi, verts, W, q_s, q_r, pos


def reference(P, pos, dev):
    """(d2 in quarters (n_q, m) int64, id (n_q, m) int64), m = min(33, n): the smallest keys, one more than the largest
    k so that "more than k points within the k-th distance" can be read off."""
    return kr.smallest_keys_int(torch.as_tensor(2 * P, dtype=torch.int64, device=dev),
                                torch.as_tensor(np.round(2 * pos), dtype=torch.int64, device=dev), min(33, P.shape[0]))


def tie_share(d2q, k, inside):
    """Among the queries inside the cloud's box: the share with more than k points within the k-th distance."""
    more = d2q[:, k] == d2q[:, k - 1]
    return float(more[inside].float().mean())


def check_tie_condition(n, dup, ks, d2q, inside):
    """The tie rule is really exercised - from the reference alone."""
    for k in ks:
        if k >= d2q.shape[1]:
            continue
        if dup and n >= 1024 and k % 2 == 1:
            assert tie_share(d2q, k, inside) >= 0.9, (n, k, tie_share(d2q, k, inside))
        if not dup and n in (65_536, 65_537):
            assert tie_share(d2q, k, inside) >= 0.3, (n, k, tie_share(d2q, k, inside))


@pytest.mark.parametrize("n,dim,dup,n_q,ks", CASES)
def test_witness_knn_bitwise(n, dim, dup, n_q, ks):
    P, hi, verts, W, q_s, q_r, pos = make_case(n, dim, dup, n_q)
    R, k1, n_s = W.shape[0], W.shape[1], verts.shape[0]
    # exactness: in half units every difference is an integer and the largest d2 (quarters) stays below 2**24
    gr.assert_exact_inputs(P, P, 3, queries=pos)
    assert np.array_equal(pos * 2, np.round(pos * 2)) and np.abs(pos).max() < 512

    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    order = index.order32.long().cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(n))
    assert index.pts.shape[0] % 16 == 0 and bool(torch.isinf(index.pts[n:, :dim]).all())   # the padded last leaf

    d2q, ids = reference(P, pos, DEV)
    inside = torch.as_tensor(((pos >= 0) & (pos <= hi - 1)).all(axis=1), device=DEV)
    check_tie_condition(n, dup, ks, d2q, inside)
    d2f = (d2q.to(torch.float32) / 4).cpu().numpy()          # exact: an integer below 2**24 over four
    ids = ids.cpu().numpy()

    # queries without a witness, as data: a target one ulp off, a row index of R, a simplex index of -1 and n_simplices
    bad_ulp, bad_row, bad_s, bad_s2 = np.array([0, 1, 2]) % n_q, np.array([5, 6]) % n_q, np.array([7]) % n_q, np.array([8]) % n_q
    bad_ulp = bad_ulp[~np.isin(bad_ulp, np.concatenate([bad_row, bad_s, bad_s2]))]
    q_r, q_s = q_r.copy(), q_s.copy()
    q_r[bad_row] = R
    q_s[bad_s] = -1
    q_s[bad_s2] = n_s
    bad = np.unique(np.concatenate([bad_ulp, bad_row, bad_s, bad_s2]))

    lib = _native.load()
    t_verts = torch.as_tensor(verts, dtype=torch.float32, device=DEV).contiguous()
    t_w = torch.as_tensor(W, dtype=torch.float32, device=DEV).contiguous()
    t_qs, t_qr = torch.as_tensor(q_s, device=DEV), torch.as_tensor(q_r, device=DEV)
    for k in ks:
        if k > n:
            continue
        for stat in (0, 1):
            target = d2f[:, k - 1].copy() if stat == 0 else kr.dtm_words(d2f, k)
            bits = target.view(np.int32).copy()
            bits[bad_ulp] += 1
            want_ids = ids[:, :k].copy()
            want_d2 = d2f[:, :k].view(np.uint32).copy()
            want_ids[bad] = -1
            want_d2[bad] = 0xffffffff
            out_ids = torch.full((n_q, k), -7, dtype=torch.int64, device=DEV)
            out_d2 = torch.full((n_q, k), 7, dtype=torch.int32, device=DEV)
            not_found = torch.zeros(1, dtype=torch.int32, device=DEV)
            blk = _native.WitnessKnn(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=k1, nodes=index.nodes,
                                     order=index.order32, verts=t_verts, weights=t_w, R=R, k=k, n_simplices=n_s,
                                     n_queries=n_q, q_simplex=t_qs, q_row=t_qr, q_stat=torch.as_tensor(bits, device=DEV),
                                     out_ids=out_ids, out_d2=out_d2 if stat == 0 or k % 2 else None,
                                     not_found=not_found, stat=stat)
            _native.check(lib.flooder_witness_knn(ctypes.byref(blk), _native.current_stream_ptr(DEV)),
                          "flooder_witness_knn")
            got = out_ids.cpu().numpy()
            assert np.array_equal(got, want_ids), (k, stat, np.argwhere(got != want_ids)[:5].tolist())
            if stat == 0 or k % 2:
                got = out_d2.cpu().numpy().view(np.uint32)
                assert np.array_equal(got, want_d2), (k, stat, np.argwhere(got != want_d2)[:5].tolist())
            else:          # (no d2 asked for: nothing written)
                assert bool((out_d2 == 7).all())
            assert int(not_found.item()) == bad.size, (k, stat)


def test_witness_knn_refuses_more_neighbours_than_points():
    tp = torch.rand(20, 3, device=DEV)
    index = core.PointIndex(tp)
    z = torch.zeros(1, dtype=torch.int32, device=DEV)
    blk = _native.WitnessKnn(pts_sorted=index.pts, n_pts=index.n, dim=3, k1=1, nodes=index.nodes, order=index.order32,
                             verts=tp[:1].contiguous(), weights=torch.ones((1, 1), device=DEV), R=1, k=21, n_simplices=1,
                             n_queries=1, q_simplex=z, q_row=z, q_stat=z,
                             out_ids=torch.zeros((1, 21), dtype=torch.int64, device=DEV), not_found=z.clone())
    assert _native.load().flooder_witness_knn(ctypes.byref(blk), _native.current_stream_ptr(DEV)) != 0
