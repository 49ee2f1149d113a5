"""The three entry points of csrc/flood_grad.hip on their own, bit for bit against numpy / integer brute force:
``flooder_face_argmax_f32``, ``flooder_witness_search``, ``flooder_segment_sum_f32`` - at the edges the end-to-end
tests never reach (grid-stride loops that wrap, segments around the wave size, one to four tree levels, padded last
leaves, duplicated points, queries without a witness)."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import grad_reference as gr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _stream():
    return _native.current_stream_ptr(DEV)


# ------------------------------------------------------------------------------------------------ face argmax
D2_BITS = np.array([0x00000000, 0x00000001, 0x3f800000, 0x3f800001, 0x42c80000, 0x7f7fffff], dtype=np.uint32)


def _argmax_expected(d2, ptr, cols, row_id):
    """(max bits << 32) | (0xffffffff - smallest row id among the columns holding the max), per (simplex, face)."""
    out = np.empty((d2.shape[0], len(ptr) - 1), dtype=np.uint64)
    for f in range(len(ptr) - 1):
        c = cols[ptr[f]:ptr[f + 1]]
        ids = (c if row_id is None else row_id[c]).astype(np.int64)
        if d2.shape[0] <= 8:
            for s in range(d2.shape[0]):
                mx = d2[s, c].max()
                out[s, f] = (np.uint64(mx) << np.uint64(32)) | np.uint64(0xffffffff - ids[d2[s, c] == mx].min())
        else:   # (the same rule, all simplices of a face at once)
            sub = d2[:, c]
            mx = sub.max(axis=1)
            best = np.where(sub == mx[:, None], ids[None, :], 1 << 32).min(axis=1)
            out[:, f] = (mx.astype(np.uint64) << np.uint64(32)) | (0xffffffff - best).astype(np.uint64)
    return out


def _faces(rng, R, n_faces):
    """CSR of face segments (ascending columns, as the caller sorts them): one face = the whole row; fifteen = lengths
    1, 2, 64, 65 and R in turn (cut to R)."""
    lens = [R] if n_faces == 1 else [min(R, (1, 2, 64, 65, R)[f % 5]) for f in range(n_faces)]
    cols = [np.sort(rng.choice(R, size=n, replace=False)) for n in lens]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate(cols).astype(np.int32)


ARGMAX_CASES = ([(3, R, nf, rid) for R in (1, 63, 64, 65, 4960) for nf in (1, 15) for rid in (True, False)]
                + [(1, 65, 15, True), (1, 4960, 1, False), (40_000, 65, 15, True), (40_000, 63, 1, False)])


@pytest.mark.parametrize("S,R,n_faces,with_row_id", ARGMAX_CASES)
def test_face_argmax_bitwise(S, R, n_faces, with_row_id):
    rng = np.random.default_rng(1000 * R + 10 * n_faces + S % 7 + int(with_row_id))
    # few distinct values: equal maxima in one lane's columns (64 apart), in neighbouring lanes, everywhere
    d2 = D2_BITS[rng.choice(len(D2_BITS), size=(S, R), p=[0.3, 0.2, 0.2, 0.15, 0.1, 0.05])]
    d2[0] = 0                                          # all zero bits: the key is (0, ~smallest id of the face)
    if S > 1:
        d2[1] = np.where(rng.random(R) < 0.3, 0x7f7fffff, d2[1])
    if S > 2:                                          # the maximum twice, 64 columns apart and side by side
        d2[2] = 1
        d2[2, [c for c in (0, 64, R - 1, R - 2) if 0 <= c < R]] = 0x42c80000
    ptr, cols = _faces(rng, R, n_faces)
    row_id = rng.permutation(R).astype(np.int32) if with_row_id else None
    want = _argmax_expected(d2, ptr, cols, row_id)
    lib = _native.load()
    t_d2 = torch.as_tensor(d2.view(np.int32), device=DEV)
    t_ptr, t_cols = torch.as_tensor(ptr, device=DEV), torch.as_tensor(cols, device=DEV)
    t_id = torch.as_tensor(row_id, device=DEV) if with_row_id else None
    keys = torch.full((S, n_faces), -1, dtype=torch.int64, device=DEV)
    _native.check(lib.flooder_face_argmax_f32(_native.ptr(t_d2), S, R, _native.ptr(t_ptr), _native.ptr(t_cols),
                                              _native.ptr(t_id), n_faces, _native.ptr(keys), _stream()),
                  "flooder_face_argmax_f32")
    got = keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# ------------------------------------------------------------------------------------------------ witness search
def _brute_int(P2, Q2, chunk_elems=1 << 26):
    """Integer brute force on the device: per row of Q2 the minimum squared distance to the rows of P2 (int32, all
    values below 2**24 by construction) and the smallest row index attaining it."""
    n, dim = P2.shape
    per = max(1, chunk_elems // n)
    ids = torch.arange(n, device=P2.device, dtype=torch.int32)
    dmin, first = [], []
    for a in range(0, Q2.shape[0], per):
        q = Q2[a:a + per]
        d = (q[:, 0:1] - P2[:, 0].unsqueeze(0)) ** 2
        for k in range(1, dim):
            d += (q[:, k:k + 1] - P2[:, k].unsqueeze(0)) ** 2
        m = d.min(dim=1).values
        dmin.append(m)
        first.append(torch.where(d == m.unsqueeze(1), ids.unsqueeze(0), n).min(dim=1).values)
    return torch.cat(dmin), torch.cat(first)


# integer coordinates in [0, hi): dense enough that equidistant points are common at half-integer queries
HI = {2: 256, 3: 64, 5: 16, 8: 8}

SEARCH_CASES = (
    # one tree level; 15 / 17: a padded last leaf; 1: a single point.  (n, dim, duplicated, queries, vertices per query)
    [(n, dim, n > 1 and dim in (3, 8), 500, 2 if dim in (2, 5) else 1) for n in (1, 15, 16, 17) for dim in (2, 3, 5, 8)]
    # one level full / two levels, two levels full / three; more queries than the 16 384 waves of the grid
    + [(1024, 2, False, 70_000, 2), (1024, 8, True, 70_000, 1), (1025, 3, True, 70_000, 1), (1025, 5, False, 70_000, 2),
       (65_536, 3, False, 70_000, 2), (65_536, 5, True, 70_000, 1), (65_537, 2, True, 70_000, 2),
       (65_537, 8, False, 70_000, 1)]
    # four levels
    + [(4_300_000, 3, False, 2000, 2)])


@pytest.mark.parametrize("n,dim,dup,n_q,k1", SEARCH_CASES)
def test_witness_search_smallest_id(n, dim, dup, n_q, k1):
    rng = np.random.default_rng(n * 10 + dim)
    hi = 256 if n > 1_000_000 else HI[dim]
    if dup:            # every point twice (but one, n odd), the copies anywhere in the cloud
        base = rng.integers(0, hi, size=((n + 1) // 2, dim))
        P = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        P = rng.integers(0, hi, size=(n, dim))
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
    R = W.shape[0]
    q_s = rng.integers(0, n_s, size=n_q).astype(np.int32)
    q_r = rng.integers(0, R, size=n_q).astype(np.int32)
    pos = np.einsum("qk,qkd->qd", W[q_r], verts[q_s])
    # exactness: in half units every difference is an integer, and the largest d2 (quarters) stays below 2**24, so the
    # kernel's fma chain, whatever its order, and the integer brute force give the same number
    gr.assert_exact_inputs(P, P, 3, queries=pos)
    assert np.array_equal(pos * 2, np.round(pos * 2)) and np.abs(pos).max() < 512

    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    index = core.PointIndex(tp)
    order = index.order32.long().cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(index.pts[:n, :dim].cpu().numpy(), P[order].astype(np.float32))
    assert index.pts.shape[0] % 16 == 0 and bool(torch.isinf(index.pts[n:, :dim]).all())   # the padded last leaf

    d2q, first = _brute_int(torch.as_tensor(2 * P, dtype=torch.int32, device=DEV),
                            torch.as_tensor(np.round(2 * pos), dtype=torch.int32, device=DEV))
    assert int(d2q.max()) < 2 ** 24
    target = (d2q.to(torch.float32) / 4).contiguous()           # exact: an integer below 2**24 over four
    bits = target.view(torch.int32).clone()
    want = first.long().cpu().numpy()
    if dup and n >= 1024:    # (the reference alone: most queries see more than one point at the minimum)
        P2 = torch.as_tensor(2 * P, dtype=torch.int32, device=DEV)
        Q2 = torch.as_tensor(np.round(2 * pos[:500]), dtype=torch.int32, device=DEV)
        at_min = (((Q2.unsqueeze(1) - P2.unsqueeze(0)) ** 2).sum(dim=2) == d2q[:500].unsqueeze(1)).sum(dim=1)
        assert float((at_min > 1).float().mean()) > 0.5

    # queries without a witness, as data: a target one ulp above the true d2 (d2 < 2**20: the next float is no multiple
    # of a quarter, no point can be there), a row index of R, a simplex index of -1 and of n_simplices
    small = np.nonzero((d2q.cpu().numpy() < 4 * 2 ** 20))[0]
    bad_ulp, bad_row, bad_s, bad_s2 = small[:3], np.array([5, 6]) % n_q, np.array([7]) % n_q, np.array([8]) % n_q
    bad_ulp = bad_ulp[~np.isin(bad_ulp, np.concatenate([bad_row, bad_s, bad_s2]))]
    assert bad_ulp.size > 0
    bits[torch.as_tensor(bad_ulp, device=DEV)] += 1
    q_r[bad_row] = R
    q_s[bad_s] = -1
    q_s[bad_s2] = n_s
    bad = np.unique(np.concatenate([bad_ulp, bad_row, bad_s, bad_s2]))
    want[bad] = -1

    t_verts = torch.as_tensor(verts, dtype=torch.float32, device=DEV).contiguous()
    t_w = torch.as_tensor(W, dtype=torch.float32, device=DEV).contiguous()
    t_qs, t_qr = torch.as_tensor(q_s, device=DEV), torch.as_tensor(q_r, device=DEV)
    out = torch.full((n_q,), -7, dtype=torch.int64, device=DEV)
    not_found = torch.zeros(1, dtype=torch.int32, device=DEV)
    blk = _native.WitnessSearch(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=k1, nodes=index.nodes,
                                order=index.order32, verts=t_verts, weights=t_w, R=R, n_simplices=n_s, n_queries=n_q,
                                q_simplex=t_qs, q_row=t_qr, q_d2=bits, out_point=out, not_found=not_found)
    _native.check(_native.load().flooder_witness_search(ctypes.byref(blk), _stream()), "flooder_witness_search")
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5].ravel(), got[got != want][:5], want[got != want][:5])
    assert int(not_found.item()) == bad.size


# ------------------------------------------------------------------------------------------------ segment sum
@pytest.mark.parametrize("dim,n_seg", [(1, 1_100_000), (2, 20_000), (3, 20_000), (6, 20_000), (8, 140_000)])
def test_segment_sum_bitwise(dim, n_seg):
    """out[target[g]] = the float32 sum of the segment's rows taken in order, exactly (a sequential float32 sum is what
    np.cumsum computes); n_seg * dim above 1 048 576 (dim 1 and 8) makes the grid-stride loop wrap."""
    rng = np.random.default_rng(dim)
    lens = rng.choice([1, 2], size=n_seg)
    lens[rng.choice(n_seg, size=20, replace=False)] = 0                 # empty segments: the row is set to 0
    lens[rng.choice(n_seg, size=5, replace=False)] = 1000
    big = int(rng.integers(1, n_seg - 1))
    lens[big], lens[big + 1] = 100_000, 1                               # one entry next to a hundred thousand
    seg_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(seg_ptr[-1])
    # twelve orders of magnitude, both signs: any other summation order changes bits
    vals = (10.0 ** rng.uniform(-6, 6, size=(N, dim)) * rng.choice([-1.0, 1.0], size=(N, dim))).astype(np.float32)
    order = rng.permutation(N).astype(np.int64)
    n_out = 3 * n_seg
    target = rng.choice(n_out, size=n_seg, replace=False).astype(np.int64)   # distinct, neither sorted nor contiguous
    sentinel = np.float32(-12345.0)
    want = np.full((n_out, dim), sentinel, dtype=np.float32)
    for L in np.unique(lens):
        gs = np.nonzero(lens == L)[0]
        if L == 0:
            want[target[gs]] = 0.0
            continue
        rows = order[seg_ptr[gs][:, None] + np.arange(L)[None, :]]           # (segments, L) in summation order
        want[target[gs]] = np.cumsum(vals[rows], axis=1, dtype=np.float32)[:, -1]
    t = [torch.as_tensor(a, device=DEV) for a in (vals, order, seg_ptr, target)]
    out = torch.full((n_out, dim), float(sentinel), dtype=torch.float32, device=DEV)
    _native.check(_native.load().flooder_segment_sum_f32(_native.ptr(t[0]), dim, _native.ptr(t[1]), _native.ptr(t[2]),
                                                         _native.ptr(t[3]), n_seg, _native.ptr(out), _stream()),
                  "flooder_segment_sum_f32")
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:5]
    assert (got[np.setdiff1d(np.arange(n_out), target)] == sentinel).all()
