"""``flooder_dtm_grad_queries_f32`` and ``flooder_dtm_grad_points_f32`` on their own (ctypes), bit for bit against the
int64 brute force of ``dtm_grad_reference``: integer clouds and integer coefficients 1..4, so that every difference,
product and partial sum is an exact float32 integer (the reference asserts the bound for its own neighbour sets) and
the int64 gradient is THE answer, whatever the order of a sum.  The ids come from the reference's (d2, id) rule, not
from the device.  Covered: k from 33 to 1024 in 2 to 8 dimensions, doubled points, k = n, separate queries (most
targets without an entry), a hub (every target's segment has 20 000 entries), the "kth" form (m = 1, the column
k - 1), Q = 1, Q no multiple of a workgroup's four waves, groups of query rows that continue out_p, both forms of the
segment list, the refusals and the empty calls."""

import functools

import numpy as np
import pytest
import torch

from flooder_amd import _native

import dtm_grad_reference as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG = -1
GUARD = 64      # words behind every output buffer that must stay untouched
BASE = 5.0      # what out_p holds before a launch: the sums continue it, rows without an entry keep it

# (n, dim, hi, k, every point twice, separate queries or None: every point a query)
CASES = [(3000, 2, 128, 65, False, None), (4000, 3, 64, 100, True, None), (3000, 5, 16, 257, True, None),
         (2048, 8, 8, 1024, False, None), (1024, 3, 64, 1024, False, None), (1500, 3, 64, 33, False, 7)]


@functools.lru_cache(maxsize=None)
def _case(n, dim, hi, k, twice, n_q):
    P = ref.integer_cloud(n, dim, hi, seed=n + dim, twice=twice)
    rng = np.random.default_rng(k)
    Qs = P if n_q is None else rng.integers(0, hi, size=(n_q, dim), dtype=np.int64)
    ids = ref.knn_ids(P, Qs, k)
    coef = rng.integers(1, 5, size=Qs.shape[0], dtype=np.int64)
    return P, Qs, ids, coef


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _entries(ids, n, packed=True):
    """The sorted entry list of ``ids`` (Q, m) -> (entries int64, seg_ptr int64, seg_target int32 or None): stably sorted by
    target, so ascending by query row inside a target.  ``packed``: keys (target << 32) | row and one segment per row of
    the cloud; else plain rows and one segment per target that occurs."""
    Q, m = ids.shape
    tg = ids.reshape(-1)
    rows = np.repeat(np.arange(Q, dtype=np.int64), m)
    order = np.argsort(tg, kind="stable")
    tg, rows = tg[order], rows[order]
    if packed:
        return (tg << 32) | rows, np.searchsorted(tg, np.arange(n + 1)).astype(np.int64), None
    uniq, first = np.unique(tg, return_index=True)
    return rows, np.concatenate([first, [tg.shape[0]]]).astype(np.int64), uniq.astype(np.int32)


def grad_queries(P, Qs, ids, coef, first=0, m=None):
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    (n, dim), Q, k = P.shape, Qs.shape[0], ids.shape[1]
    m = k if m is None else m
    p, q, i, c = _dev(P, torch.float32), _dev(Qs, torch.float32), _dev(ids, torch.int32), _dev(coef, torch.float32)
    out = torch.full((Q * dim + GUARD,), -7.0, dtype=torch.float32, device=DEV)
    _native.check(lib.flooder_dtm_grad_queries_f32(_native.ptr(p), n, _native.ptr(q), Q, dim, _native.ptr(i) + 4 * first, k,
                                                   m, _native.ptr(c), _native.ptr(out), st), "flooder_dtm_grad_queries_f32")
    assert bool((out[Q * dim:] == -7.0).all()), "the guard band was written"
    return out[:Q * dim].reshape(Q, dim).cpu()


def grad_points(P, Qs, ids, coef, groups=1, packed=True):
    """out_p from BASE, the query rows in ``groups`` consecutive launches."""
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    (n, dim), Q = P.shape, Qs.shape[0]
    p, q, c = _dev(P, torch.float32), _dev(Qs, torch.float32), _dev(coef, torch.float32)
    out = torch.full((n * dim + GUARD,), BASE, dtype=torch.float32, device=DEV)
    cuts = np.linspace(0, Q, groups + 1).astype(np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        a, b = int(a), int(b)
        ent, seg_ptr, seg_target = _entries(ids[a:b], n, packed)
        ent, seg_ptr = _dev(ent, torch.int64), _dev(seg_ptr, torch.int64)
        seg_target = None if seg_target is None else _dev(seg_target, torch.int32)
        _native.check(lib.flooder_dtm_grad_points_f32(_native.ptr(p), n, _native.ptr(q[a:b]), b - a, dim,
                                                      _native.ptr(c[a:b]), _native.ptr(ent), _native.ptr(seg_ptr),
                                                      _native.ptr(seg_target), seg_ptr.shape[0] - 1, _native.ptr(out), st),
                      "flooder_dtm_grad_points_f32")
    assert bool((out[n * dim:] == BASE).all()), "the guard band was written"
    return out[:n * dim].reshape(n, dim).cpu()


def _f32(a):
    return torch.as_tensor(a).to(torch.float32)


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}-d{c[1]}-k{c[3]}" for c in CASES])
def test_both_kernels_are_the_integer_brute_force(case):
    P, Qs, ids, coef = _case(*case)
    n, k = P.shape[0], ids.shape[1]
    gq, gp, largest = ref.integer_grads(P, Qs, ids, coef)
    print(f"largest sum of |terms| of a word: {largest}")
    assert torch.equal(grad_queries(P, Qs, ids, coef), _f32(gq))
    assert torch.equal(grad_points(P, Qs, ids, coef), _f32(gp) + BASE)
    # groups of ascending query rows continue the sums: the same words; so does the compact segment list
    assert torch.equal(grad_points(P, Qs, ids, coef, groups=3), _f32(gp) + BASE)
    assert torch.equal(grad_points(P, Qs, ids, coef, groups=2, packed=False), _f32(gp) + BASE)
    if case[5] is not None:
        assert int((gp == 0).all(axis=1).sum()) > n // 2          # most targets have an empty reverse list
    # the "kth" form: x_(k) alone
    last = ids[:, -1:]
    gq1, gp1, _ = ref.integer_grads(P, Qs, last, coef)
    assert torch.equal(grad_queries(P, Qs, ids, coef, first=k - 1, m=1), _f32(gq1))
    assert torch.equal(grad_points(P, Qs, last, coef), _f32(gp1) + BASE)
    # Q = 1 and a Q that is no multiple of the four waves of a workgroup
    for Q in (1, 7):
        gq2, gp2, _ = ref.integer_grads(P, Qs[:Q], ids[:Q], coef[:Q])
        assert torch.equal(grad_queries(P, Qs[:Q], ids[:Q], coef[:Q]), _f32(gq2))
        assert torch.equal(grad_points(P, Qs[:Q], ids[:Q], coef[:Q]), _f32(gp2) + BASE)


def test_hub_every_segment_has_20000_entries():
    rng = np.random.default_rng(600)
    P = rng.integers(0, 64, size=(600, 2), dtype=np.int64)
    Qs = rng.integers(0, 64, size=(20_000, 2), dtype=np.int64)
    ids = ref.knn_ids(P, Qs, 600)
    coef = np.ones(20_000, dtype=np.int64)
    gq, gp, largest = ref.integer_grads(P, Qs, ids, coef)
    print(f"largest sum of |terms| of a word: {largest}")
    assert largest < 1 << 23
    assert torch.equal(grad_queries(P, Qs, ids, coef), _f32(gq))
    assert torch.equal(grad_points(P, Qs, ids, coef), _f32(gp) + BASE)
    assert torch.equal(grad_points(P, Qs, ids, coef, groups=4), _f32(gp) + BASE)


def test_refusals_and_empty_calls():
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    p = torch.zeros((8, 3), dtype=torch.float32, device=DEV)
    ids = torch.zeros((8, 4), dtype=torch.int32, device=DEV)
    coef = torch.ones(8, dtype=torch.float32, device=DEV)
    ent = torch.zeros(32, dtype=torch.int64, device=DEV)
    seg = torch.zeros(9, dtype=torch.int64, device=DEV)
    out = torch.full((8, 3), -7.0, dtype=torch.float32, device=DEV)
    P, I, C, E, S, O = (_native.ptr(t) for t in (p, ids, coef, ent, seg, out))

    def queries(points=P, n=8, qs=P, Q=8, dim=3, i=I, ld=4, m=4, c=C, o=O):
        return lib.flooder_dtm_grad_queries_f32(points, n, qs, Q, dim, i, ld, m, c, o, st)

    def points(pp=P, n=8, qs=P, Q=8, dim=3, c=C, e=E, s=S, t=None, n_seg=8, o=O):
        return lib.flooder_dtm_grad_points_f32(pp, n, qs, Q, dim, c, e, s, t, n_seg, o, st)

    bad_q = [dict(dim=1), dict(dim=9), dict(m=0), dict(m=1025, ld=1025), dict(ld=3), dict(n=-1), dict(Q=-1),
             dict(points=None), dict(qs=None), dict(i=None), dict(c=None), dict(o=None)]
    bad_p = [dict(dim=1), dict(dim=9), dict(n=-1), dict(Q=-1), dict(n_seg=-1), dict(pp=None), dict(qs=None), dict(c=None),
             dict(e=None), dict(s=None), dict(o=None)]
    for fn, name, bad in ((queries, "flooder_dtm_grad_queries_f32", bad_q), (points, "flooder_dtm_grad_points_f32", bad_p)):
        for kw in bad:
            assert fn(**kw) == E_ARG, (name, kw)
            assert lib.flooder_last_error().decode().startswith(name), (name, kw)
    # nothing to do: FLOODER_OK and nothing is touched (the pointers may be anything valid)
    assert queries(Q=0) == 0 and points(Q=0) == 0 and points(n_seg=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
