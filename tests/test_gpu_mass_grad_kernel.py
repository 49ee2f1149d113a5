"""``flooder_mass_grad_queries_f32``, ``flooder_mass_grad_points_f32`` and ``flooder_mass_grad_masses_f32`` on their own
(ctypes), bit for bit against the int64 brute force of ``mass_grad_reference``: integer clouds, integer masses 0..3, tau a power of two and integer
coefficients, so that every mass sum, rho, product, difference and partial sum is an exact float32 (float64) integer -
the reference asserts the bound for its own rows - and the int64 answer is THE answer, whatever the order of a sum.  The
id rows are hand-built: the nearest sites by (d2, id), cut at a count the case chooses (1, 63, 64, 65, 129, the row
length L; a count of 0, a negative one and one beyond the row), padded with -1, with a -1 and an id beyond the cloud
inside a list.  Covered: L = 64 and 1024, dim 2, 3, 8, a cloud of fewer than 64 sites, listed sites of mass 0, a zero
coefficient, groups of query rows that continue out_p and out_m, both forms of the segment list, the words of the plain
pair at unit masses, the refusals and the empty calls."""

import functools

import numpy as np
import pytest
import torch

from flooder_amd import _native

import dtm_grad_reference as dref
import mass_grad_reference as mref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E_ARG = -1
GUARD = 64      # words behind every output buffer that must stay untouched
BASE = 5.0      # what out_p and out_m hold before a launch: the sums continue it, words without an entry keep it
TAU = 4096      # a power of two above every cumulative mass of a list (1023 sites of mass <= 3 hold 3069 at most)

# (n, dim, hi, L, the counts the rows cycle through)
CASES = [(1500, 3, 16, 1024, (1, 63, 64, 65, 129, 1024)), (1500, 8, 4, 1024, (1, 63, 64, 65, 129, 1024)),
         (300, 2, 16, 64, (1, 63, 64, 17, 70)), (40, 3, 8, 64, (1, 17, 40))]
N_ROWS = 26


@functools.lru_cache(maxsize=None)
def _case(n, dim, hi, L, counts):
    rng = np.random.default_rng(n + dim + L)
    P = dref.integer_cloud(n, dim, hi, seed=n + dim)
    masses = rng.integers(0, 4, size=n, dtype=np.int64)
    Qs = rng.integers(0, hi, size=(N_ROWS, dim), dtype=np.int64)
    kq = min(L, n)
    near = dref.knn_ids(P, Qs, kq)
    count = np.array([counts[r % len(counts)] for r in range(N_ROWS)], dtype=np.int64)
    count[3], count[5] = 0, -2                            # rows without a list
    ids = np.full((N_ROWS, L), -1, dtype=np.int64)
    ids[:, :kq] = near
    ids[np.arange(L)[None, :] >= np.minimum(count, kq)[:, None]] = -1
    for r in range(N_ROWS):                               # inside a long enough list: a -1 and an id beyond the cloud
        if count[r] >= 17 and r % 2 == 0:
            ids[r, 2], ids[r, 9] = -1, n + 5
    coef = rng.integers(1, 5, size=N_ROWS, dtype=np.int64)
    coef[7] = 0                                           # a zero coefficient
    want = mref.integer_grads(P, masses, Qs, ids, count, TAU, coef, coef)      # (h = coef: twice the kernel's h)
    listed = np.arange(L)[None, :] < np.minimum(count, L)[:, None]
    assert (want["rho"][count > 0] > 0).all()
    assert (masses[np.where(listed & (ids >= 0) & (ids < n), ids, 0)][listed] == 0).any(), "no listed site of mass 0"
    return P, masses, Qs, ids, count, coef, want


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _f32(a):
    return torch.as_tensor(np.asarray(a)).to(torch.float32)


def _sites(P, masses):
    """The (n, dim + 1) rows of the device entries: the coordinates, then the mass."""
    return _dev(np.concatenate([np.asarray(P, dtype=np.float64), np.asarray(masses, dtype=np.float64)[:, None]], axis=1),
                torch.float32)


def _qrow(coef, rho, cross, dstar):
    """The (Q, 4) crossing rows: coefficient, rho, crossing id (its int32 bits), dstar2."""
    row = torch.zeros((len(coef), 4), dtype=torch.float32)
    row[:, 0], row[:, 1], row[:, 3] = _f32(coef), _f32(rho), _f32(dstar)
    row.view(torch.int32)[:, 2] = torch.as_tensor(np.asarray(cross)).to(torch.int32)
    return row.to(DEV)


def grad_queries(P, masses, Qs, ids, count, coef, tau=TAU):
    """-> (out_q, rho, cross, dstar2, the coefficient word as the kernel left it)."""
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    (n, dim), (Q, L) = P.shape, ids.shape
    sites, q = _sites(P, masses), _dev(Qs, torch.float32)
    i, cnt = _dev(ids, torch.int32), _dev(count, torch.int32)
    t = torch.tensor([float(tau)], dtype=torch.float64, device=DEV)
    out = torch.full((Q * dim + GUARD,), -7.0, dtype=torch.float32, device=DEV)
    qrow = torch.full((Q + GUARD // 4, 4), -7.0, dtype=torch.float32, device=DEV)
    qrow[:Q, 0] = _dev(coef, torch.float32)
    _native.check(lib.flooder_mass_grad_queries_f32(_native.ptr(sites), n, _native.ptr(q), Q, dim, _native.ptr(i), L,
                                                    _native.ptr(cnt), _native.ptr(t), _native.ptr(qrow), _native.ptr(out),
                                                    st), "flooder_mass_grad_queries_f32")
    assert bool((out[Q * dim:] == -7.0).all()) and bool((qrow[Q:] == -7.0).all()), "the guard band was written"
    qrow = qrow[:Q].cpu()
    return out[:Q * dim].reshape(Q, dim).cpu(), qrow[:, 1], qrow.view(torch.int32)[:, 2], qrow[:, 3], qrow[:, 0]


def _entries(ids, count, n, packed=True):
    """The sorted entry list of the listed positions of ``ids`` (the -1 dropped, as the negative keys of the caller drop
    out; an id beyond the cloud stays: it falls behind the last segment) -> (entries, seg_ptr, seg_target or None),
    stably sorted by target, so ascending by query row inside a target."""
    Q, L = ids.shape
    listed = (np.arange(L)[None, :] < np.minimum(count, L)[:, None]) & (ids >= 0)
    tg = ids[listed]
    rows = np.repeat(np.arange(Q, dtype=np.int64), L).reshape(Q, L)[listed]
    order = np.argsort(tg, kind="stable")
    tg, rows = tg[order], rows[order]
    if packed:
        return (tg << 32) | rows, np.searchsorted(tg, np.arange(n + 1)).astype(np.int64), None
    uniq, first = np.unique(tg, return_index=True)
    return rows, np.concatenate([first, [tg.shape[0]]]).astype(np.int64), uniq.astype(np.int32)


def grad_points(P, masses, Qs, ids, count, coef, want, groups=1, packed=True, with_p=True, with_m=True):
    """(out_p, out_m) from BASE, the query rows in ``groups`` consecutive launches of each transpose; rho, the crossing
    ids and dstar2 of the crossing rows are the reference's."""
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    (n, dim), Q = P.shape, Qs.shape[0]
    sites, q = _sites(P, masses), _dev(Qs, torch.float32)
    qrow = _qrow(coef, want["rho"], want["cross"], want["dstar"])
    out_p = torch.full((n * dim + GUARD,), BASE, dtype=torch.float32, device=DEV)
    out_m = torch.full((n + GUARD,), BASE, dtype=torch.float32, device=DEV)
    cuts = np.linspace(0, Q, groups + 1).astype(np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        a, b = int(a), int(b)
        ent, seg_ptr, seg_target = _entries(ids[a:b], count[a:b], n, packed)
        ent, seg_ptr = _dev(ent, torch.int64), _dev(seg_ptr, torch.int64)
        seg_target = None if seg_target is None else _dev(seg_target, torch.int32)
        for name, out, wanted in (("flooder_mass_grad_points_f32", out_p, with_p), ("flooder_mass_grad_masses_f32", out_m, with_m)):
            if wanted:
                _native.check(getattr(lib, name)(_native.ptr(sites), n, _native.ptr(q[a:b]), b - a, dim,
                                                 _native.ptr(qrow[a:b]), _native.ptr(ent), _native.ptr(seg_ptr),
                                                 _native.ptr(seg_target), seg_ptr.shape[0] - 1, _native.ptr(out), st), name)
    assert bool((out_p[n * dim:] == BASE).all()) and bool((out_m[n:] == BASE).all()), "the guard band was written"
    return out_p[:n * dim].reshape(n, dim).cpu(), out_m[:n].cpu()


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}-d{c[1]}-L{c[3]}" for c in CASES])
def test_the_kernels_are_the_integer_brute_force(case):
    P, masses, Qs, ids, count, coef, want = _case(*case)
    print(f"largest sum of |terms| of a word: {want['largest']}")
    out_q, rho, cross, dstar, left = grad_queries(P, masses, Qs, ids, count, coef)
    assert torch.equal(out_q, _f32(want["out_q"]))
    assert torch.equal(rho, _f32(want["rho"])) and torch.equal(dstar, _f32(want["dstar"]))
    assert torch.equal(cross, torch.as_tensor(want["cross"]).to(torch.int32))
    assert torch.equal(left, _f32(coef)), "the coefficient word is the caller's"
    # rows without a list and the row with a zero coefficient wrote their words: zeros, and no crossing
    for r in (3, 5):
        assert not bool(out_q[r].any()) and float(rho[r]) == 0.0 and int(cross[r]) == -1 and float(dstar[r]) == 0.0
    assert not bool(out_q[7].any()) and float(rho[7]) == float(want["rho"][7]) and int(cross[7]) == int(want["cross"][7])
    # (the mass kernel weighs a term by h = coef / 2: the reference ran with h = coef, its words are twice the kernel's)
    wp, wm = _f32(want["out_p"]) + BASE, _f32(want["out_m"]) * 0.5 + BASE
    out_p, out_m = grad_points(P, masses, Qs, ids, count, coef, want)
    assert torch.equal(out_p, wp) and torch.equal(out_m, wm)
    assert bool((out_m != BASE).any()) and bool((out_p != BASE).any())
    # groups of ascending query rows continue the sums: the same words; so does the compact segment list
    for kw in (dict(groups=3), dict(groups=2, packed=False)):
        got_p, got_m = grad_points(P, masses, Qs, ids, count, coef, want, **kw)
        assert torch.equal(got_p, wp) and torch.equal(got_m, wm), kw
    # Q = 1 and a Q that is no multiple of the four waves of a workgroup
    for Q in (1, 7):
        sub = mref.integer_grads(P, masses, Qs[:Q], ids[:Q], count[:Q], TAU, coef[:Q], coef[:Q])
        got = grad_queries(P, masses, Qs[:Q], ids[:Q], count[:Q], coef[:Q])
        assert torch.equal(got[0], _f32(sub["out_q"])) and torch.equal(got[1], _f32(sub["rho"]))
        got_p, got_m = grad_points(P, masses, Qs[:Q], ids[:Q], count[:Q], coef[:Q], sub)
        assert torch.equal(got_p, _f32(sub["out_p"]) + BASE) and torch.equal(got_m, _f32(sub["out_m"]) * 0.5 + BASE)


def test_unit_masses_are_the_words_of_the_plain_pair():
    """Masses all 1, tau = k, every count k: out_q and out_p are those of ``flooder_dtm_grad_*_f32`` at m = k, on a FLOAT
    cloud (the orders of the sums, not only their values, are the same), rho is 1 and the crossing id the k-th."""
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    rng = np.random.default_rng(11)
    n, dim, k, Q = 700, 3, 129, 50
    P, Qs = rng.random((n, dim)).astype(np.float32), rng.random((Q, dim)).astype(np.float32)
    ids = np.argsort(((Qs[:, None, :].astype(np.float64) - P[None]) ** 2).sum(axis=2), axis=1, kind="stable")[:, :k]
    coef = rng.random(Q).astype(np.float32)
    ones, count = np.ones(n), np.full(Q, k)
    out_q, rho, cross, dstar, _ = grad_queries(P, ones, Qs, ids, count, coef, tau=k)
    p, q, i, c = _dev(P, torch.float32), _dev(Qs, torch.float32), _dev(ids, torch.int32), _dev(coef, torch.float32)
    plain_q = torch.empty((Q, dim), dtype=torch.float32, device=DEV)
    _native.check(lib.flooder_dtm_grad_queries_f32(_native.ptr(p), n, _native.ptr(q), Q, dim, _native.ptr(i), k, k,
                                                   _native.ptr(c), _native.ptr(plain_q), st), "flooder_dtm_grad_queries_f32")
    assert torch.equal(out_q, plain_q.cpu()) and bool((rho == 1.0).all())
    assert torch.equal(cross, torch.as_tensor(ids[:, -1]).to(torch.int32))
    ent, seg_ptr, _ = _entries(ids, count, n)
    ent, seg_ptr = _dev(ent, torch.int64), _dev(seg_ptr, torch.int64)
    plain_p = torch.full((n, dim), BASE, dtype=torch.float32, device=DEV)      # (both continue the same start)
    _native.check(lib.flooder_dtm_grad_points_f32(_native.ptr(p), n, _native.ptr(q), Q, dim, _native.ptr(c), _native.ptr(ent),
                                                  _native.ptr(seg_ptr), None, n, _native.ptr(plain_p), st),
                  "flooder_dtm_grad_points_f32")
    want = dict(rho=rho.numpy(), cross=cross.numpy(), dstar=dstar.numpy())
    out_p, _ = grad_points(P, ones, Qs, ids, count, coef, want, with_m=False)
    assert torch.equal(out_p, plain_p.cpu())


def test_refusals_and_empty_calls():
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    sites = torch.zeros((8, 4), dtype=torch.float32, device=DEV)
    qs = torch.zeros((8, 3), dtype=torch.float32, device=DEV)
    ids = torch.zeros((8, 4), dtype=torch.int32, device=DEV)
    cnt = torch.ones(8, dtype=torch.int32, device=DEV)
    tau = torch.ones(1, dtype=torch.float64, device=DEV)
    ent = torch.zeros(32, dtype=torch.int64, device=DEV)
    seg = torch.zeros(9, dtype=torch.int64, device=DEV)
    qrow = torch.full((8, 4), -7.0, dtype=torch.float32, device=DEV)
    out = torch.full((8, 3), -7.0, dtype=torch.float32, device=DEV)
    S, QS, I, N, T, E, SP, R, O = (_native.ptr(t) for t in (sites, qs, ids, cnt, tau, ent, seg, qrow, out))

    def queries(s=S, n=8, q=QS, Q=8, dim=3, i=I, ld=4, cn=N, t=T, r=R, o=O):
        return lib.flooder_mass_grad_queries_f32(s, n, q, Q, dim, i, ld, cn, t, r, o, st)

    def transpose(name):
        def call(s=S, n=8, q=QS, Q=8, dim=3, r=R, e=E, sp=SP, t=None, n_seg=8, o=O):
            return getattr(lib, name)(s, n, q, Q, dim, r, e, sp, t, n_seg, o, st)
        return call

    bad_q = [dict(dim=1), dict(dim=9), dict(ld=0), dict(ld=1025), dict(n=-1), dict(Q=-1), dict(s=None), dict(q=None),
             dict(i=None), dict(cn=None), dict(t=None), dict(r=None), dict(o=None)]
    bad_t = [dict(dim=1), dict(dim=9), dict(n=-1), dict(Q=-1), dict(n_seg=-1), dict(s=None), dict(q=None), dict(r=None),
             dict(e=None), dict(sp=None), dict(o=None)]
    points, masses = transpose("flooder_mass_grad_points_f32"), transpose("flooder_mass_grad_masses_f32")
    for fn, name, bad in ((queries, "flooder_mass_grad_queries_f32", bad_q), (points, "flooder_mass_grad_points_f32", bad_t),
                          (masses, "flooder_mass_grad_masses_f32", bad_t)):
        for kw in bad:
            assert fn(**kw) == E_ARG, (name, kw)
            assert lib.flooder_last_error().decode().startswith(name), (name, kw)
    # nothing to do: FLOODER_OK and nothing is touched
    assert queries(Q=0) == 0
    for fn in (points, masses):
        assert fn(Q=0) == 0 and fn(n_seg=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((qrow == -7.0).all())
