"""``flooder_knn_mass_f32`` on its own, against the rule of ``include/flooder_hip.h`` evaluated in float64 numpy over the
keys of an integer brute force (``knn_mass_reference``): unit masses word for word against ``flooder_knn_wide_f32``,
integer masses (count, ids and ``"kth"`` exact, ``"dtm"`` exact against the float32 replay AND within the derived
bound), zero masses in front of the crossing, a heavy site, the not-reached rule, general float masses, ``sample_order``
and the refusals.  The shapes are the smallest that can go wrong: a padded single leaf (15 points), one, two and three
tree levels, none a multiple of 16; every point doubled in half of the cases (ties decided by id); 1, 63, 65 and 300
cells; capacities 64, 256 and 1024; rows of the capacity and shorter.  Two more cases (``WRAP``: 16 684 cells, capacities 64
and 256) make every wave of the grid-stride loop handle a second cell - a list that shrank to its crossing in one cell
must start the next at its full length - in the unit, integer and zero mass tests.  Guard words behind every output;
every launch is made twice and must write the same words."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import grad_reference as gr
import knn_mass_reference as km
import knn_wide_reference as kw

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HI = {2: 256, 3: 64, 5: 16, 8: 8}      # coordinate ranges (test_gpu_knn_wide_kernel's)
GUARD = 64                              # words behind every output buffer that must stay untouched
FILL = -7
NS, DIMS, QS, CAPS = (15, 1000, 1025, 30_001, 70_001), (2, 3, 5, 8), (1, 63, 65, 300), (64, 256, 1024)
# (n points, dim, every point doubled, cells, capacity)
CASES = [(n, dim, (i + j) % 2 == 1, QS[(i + j) % 4], CAPS[(i + 2 * j) % 3])
         for i, n in enumerate(NS) for j, dim in enumerate(DIMS)]
WHOLE_CLOUD = (1000, 3, False, 65, 1024)      # n_pts <= C: the list holds the whole cloud
# more cells than the grid has waves (4 waves in each of 256 * 16 blocks), no multiple of 3: the query form; SLOTS 1 and 4
WRAP = [(1025, 3, True, 4 * 256 * 16 + 300, 64), (1025, 3, True, 4 * 256 * 16 + 300, 256)]


def case_ids(cases):
    return [f"n{n}-d{d}-{'dup' if dup else 'single'}-q{q}-c{c}" for n, d, dup, q, c in cases]


IDS = case_ids(CASES)


def test_cases_cover_what_they_must():
    assert {c[0] for c in CASES} == set(NS) and {c[1] for c in CASES} == set(DIMS)
    assert {c[3] for c in CASES} == set(QS) and {c[4] for c in CASES} == set(CAPS)
    assert sum(c[2] for c in CASES) * 2 == len(CASES) and all(n % 16 for n in NS)
    for n in NS:                                   # every size meets a capacity below it (but 15) and doubled points
        assert any(c[0] == n and c[2] for c in CASES) and (n == 15 or any(c[0] == n and c[4] < n for c in CASES))
    assert any(c[0] < c[4] for c in CASES)         # a cloud smaller than the capacity
    assert any(c[3] > 4 * 256 * 16 for c in WRAP)  # the grid-stride loop wraps ...
    assert {c[4] for c in WRAP} == {64, 256} and all(c[2] and c[3] % 3 for c in WRAP)   # ... with SLOTS = 1 and above


@functools.lru_cache(maxsize=None)
def inputs(n, dim, dup, n_cells, cap, dev=None):
    """The inputs of a case and the reference keys (brute force on ``dev``): integer points (doubled: ids 2i and 2i + 1
    are one place; where n is odd the last point has no copy), positions inside the cloud, on its corners and outside
    it, integers or half-integers, the first cell(s) AT point 0.  Lattice form (k1 = 2, R = 3) where the cells divide by
    three in 2-D and 5-D, else the query form."""
    rng = np.random.default_rng(1000 * dim + n + n_cells)
    hi = HI[dim]
    if dup:
        P = np.repeat(rng.integers(0, hi, size=((n + 1) // 2, dim)), 2, axis=0)[:n]
    else:
        P = rng.integers(0, hi, size=(n, dim))
    lattice = dim in (2, 5) and n_cells % 3 == 0
    k1 = 2 if lattice else 1
    W = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]]) if lattice else np.array([[1.0]])
    n_s = n_cells // W.shape[0]
    kind = rng.random((n_s, k1, 1))
    verts = np.where(kind < 0.5, rng.integers(0, hi, size=(n_s, k1, dim)),
                     np.where(kind < 0.7, rng.choice([0, hi - 1], size=(n_s, k1, dim)),
                              rng.integers(-300, 301, size=(n_s, k1, dim)))).astype(np.float64)
    if k1 == 1:
        verts = verts + rng.choice([0.0, 0.5], size=verts.shape)      # half-integer positions
    verts[0] = P[0]                                                   # the first simplex: every sample AT point 0
    pos = np.einsum("rk,skd->srd", W, verts).reshape(-1, dim)
    gr.assert_exact_inputs(P, P, 3, queries=pos)
    d2f, ids, _ = kw.smallest_keys(P, pos, cap, DEV if dev is None else dev)      # min(cap + 1, n) keys per cell
    return dict(n=n, dim=dim, dup=dup, cap=cap, L=min(cap, n), P=P, pos=pos, k1=k1, R=W.shape[0], n_s=n_s, N=pos.shape[0],
                d2f=d2f, ids=ids, rng_seed=n + dim, verts_np=verts, weights_np=W)


@functools.lru_cache(maxsize=None)
def case(n, dim, dup, n_cells, cap):
    """``inputs`` with the point index and the device tensors of a launch."""
    c = dict(inputs(n, dim, dup, n_cells, cap))
    c.update(index=core.PointIndex(torch.as_tensor(c["P"], dtype=torch.float32, device=DEV)),
             verts=torch.as_tensor(c["verts_np"], dtype=torch.float32, device=DEV).contiguous(),
             weights=torch.as_tensor(c["weights_np"], dtype=torch.float32, device=DEV).contiguous())
    return c


def integer_masses(c):
    return np.random.default_rng(c["rng_seed"]).integers(1, 10, size=c["n"]).astype(np.float32)


def zero_masses(c):
    masses = np.random.default_rng(c["rng_seed"] + 1).integers(1, 10, size=c["n"]).astype(np.float32)
    masses[0:c["n"] - 1:2] = 0.0
    return masses


def float_masses(c):
    masses = np.random.default_rng(c["rng_seed"] + 2).random(c["n"], dtype=np.float32)
    masses[masses == 0] = 0.5
    return masses


def integer_taus(c):
    return sorted({1.0, 2.5, float(max(1, c["L"] // 2)), float(c["L"])})


def zero_taus(c):
    return [t for t in sorted({1.0, float(max(1, c["L"] // 4)) + 0.5, float(c["L"] // 2)}) if t <= c["L"] // 2]


def float_taus(c):
    return (0.3, c["L"] / 4.0)


def mass_entry(capacity, masses, target, ld_out, out_count, **block):
    """``flooder_knn_mass_f32`` by name: the wide block (its k is the capacity) and what the entry adds -> return code."""
    blk = block.pop("block", None) or _native.KnnWide(k=capacity, **block)
    return _native.load().flooder_knn_mass_f32(ctypes.byref(blk), _native.ptr(masses), _native.ptr(target), int(ld_out),
                                               _native.ptr(out_count), _native.current_stream_ptr(DEV))


def launch(c, masses, tau, stat, want, ld_out=None, sample_order=None, cap=None):
    """One ``flooder_knn_mass_f32`` writing the outputs named in ``want`` -> {name: array}; made TWICE into fresh
    buffers, which must agree; the guard band behind every buffer is checked."""
    N, cap = c["N"], c["cap"] if cap is None else cap
    ld = km.capacity_of(cap) if ld_out is None else ld_out
    shapes = {"ids": N * ld, "d2": N * ld, "bits": N, "count": N}
    m = torch.as_tensor(np.asarray(masses, dtype=np.float32), device=DEV)
    t = torch.tensor([tau], dtype=torch.float64, device=DEV)
    runs = []
    for _ in range(2):
        bufs = {name: torch.full((shapes[name] + GUARD,), FILL, dtype=torch.int32, device=DEV) for name in want}
        rc = mass_entry(cap, m, t, ld, bufs.get("count"), pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"],
                        nodes=c["index"].nodes, verts=c["verts"], weights=c["weights"], R=c["R"], n_simplices=c["n_s"],
                        stat=stat, order=c["index"].order32, sample_order=sample_order, out_bits=bufs.get("bits"),
                        out_ids=bufs.get("ids"), out_d2=bufs.get("d2"))
        _native.check(rc, "flooder_knn_mass_f32")
        out = {}
        for name, b in bufs.items():
            assert bool((b[shapes[name]:] == FILL).all()), f"{name}: the guard band was written"
            a = b[:shapes[name]].cpu().numpy()
            out[name] = (a.reshape(N, ld) if name == "ids" else a.view(np.uint32).reshape(N, ld) if name == "d2"
                         else a.view(np.uint32) if name == "bits" else a)
        runs.append(out)
    for name in want:
        assert np.array_equal(runs[0][name], runs[1][name]), f"{name}: two launches differ"
    return runs[0]


def wide(c, k, stat):
    """``flooder_knn_wide_f32`` at k on the same inputs -> (bits (N,), ids (N, k), d2 (N, k))."""
    N = c["N"]
    bits = torch.empty(N, dtype=torch.int32, device=DEV)
    ids, d2 = (torch.empty((N, k), dtype=torch.int32, device=DEV) for _ in range(2))
    blk = _native.KnnWide(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                          verts=c["verts"], weights=c["weights"], R=c["R"], k=k, n_simplices=c["n_s"], stat=stat,
                          order=c["index"].order32, out_bits=bits, out_ids=ids, out_d2=d2)
    _native.check(_native.load().flooder_knn_wide_f32(ctypes.byref(blk), _native.current_stream_ptr(DEV)),
                  "flooder_knn_wide_f32")
    return bits.cpu().numpy().view(np.uint32), ids.cpu().numpy(), d2.cpu().numpy().view(np.uint32)


def check_rows(got, c, count, ld):
    """out_ids / out_d2 rows of ``ld`` entries against the reference keys: the first min(count, ld) keys, then -1 / +inf."""
    cols = np.arange(ld)[None, :]
    listed = cols < np.minimum(count, ld)[:, None]
    m = min(ld, c["ids"].shape[1])
    want_ids = np.full((c["N"], ld), -1, dtype=np.int64)
    want_d2 = np.full((c["N"], ld), km.INF_WORD, dtype=np.uint32)
    want_ids[:, :m] = c["ids"][:, :m]
    want_d2[:, :m] = np.ascontiguousarray(c["d2f"][:, :m]).view(np.uint32)
    want_ids[~listed] = -1
    want_d2[~listed] = km.INF_WORD
    if "ids" in got:
        assert np.array_equal(got["ids"], want_ids), np.argwhere(got["ids"] != want_ids)[:5].tolist()
    if "d2" in got:
        assert np.array_equal(got["d2"], want_d2), np.argwhere(got["d2"] != want_d2)[:5].tolist()


def check_against_reference(c, masses, tau, got_kth, got_dtm, ld, exact_replay):
    """Count, ids, d2 rows and ``"kth"`` words exact; ``"dtm"`` within the derived bound (and, for masses whose prefix
    sums are exact, equal to the float32 replay)."""
    ref = km.crossing(c["d2f"], c["ids"], masses, tau, c["L"])
    for got in (got_kth, got_dtm):
        assert np.array_equal(got["count"], ref["count"]), np.argwhere(got["count"] != ref["count"])[:5].tolist()
        check_rows(got, c, ref["count"], ld)
    want_kth = np.where(ref["reached"], ref["kth"], np.inf).astype(np.float32).view(np.uint32)
    assert np.array_equal(got_kth["bits"], want_kth)
    dtm = got_dtm["bits"].view(np.float32).astype(np.float64)
    r = ref["reached"]
    assert np.array_equal(got_dtm["bits"][~r], np.full((~r).sum(), km.INF_WORD, dtype=np.uint32))
    err = np.abs(dtm[r] - ref["dtm"][r])
    tol = km.dtm_bound(ref["count"][r]) * ref["dtm"][r]
    print(f"dtm: largest error / bound {float((err / np.maximum(tol, 1e-300)).max()) if r.any() else 0:.3f}")
    assert np.all(err <= tol)
    if exact_replay and r.any():
        want = km.dtm_words(c["d2f"][r], c["ids"][r], masses, tau, ref["count"][r])
        assert np.array_equal(got_dtm["bits"][r], want)
    return ref


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", CASES + WRAP, ids=IDS + case_ids(WRAP))
def test_unit_masses_are_the_wide_kernel(n, dim, dup, n_cells, cap):
    c = case(n, dim, dup, n_cells, cap)
    ones = np.ones(n, dtype=np.float32)
    C = km.capacity_of(cap)
    ks = [k for k in (1, 40, 64, 65, 1000) if k <= c["L"]]
    assert ks
    for i, k in enumerate(ks):
        ld = C if i % 2 == 0 else max(k, 1)                 # rows of the capacity, and rows just long enough
        for stat in (0, 1):
            got = launch(c, ones, float(k), stat, ("bits", "count", "ids", "d2"), ld_out=ld)
            w_bits, w_ids, w_d2 = wide(c, k, stat)
            assert np.array_equal(got["bits"], w_bits), (k, stat)
            assert np.array_equal(got["ids"][:, :k], w_ids) and np.array_equal(got["d2"][:, :k], w_d2), (k, stat)
            assert bool((got["count"] == k).all())
            assert bool((got["ids"][:, k:] == -1).all()) and bool((got["d2"][:, k:] == km.INF_WORD).all())


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", CASES + WRAP, ids=IDS + case_ids(WRAP))
def test_integer_masses(n, dim, dup, n_cells, cap):
    """Masses in 1..9 and tau <= L = min(C, n): any L sites hold at least L, so every cell is reached."""
    c = case(n, dim, dup, n_cells, cap)
    masses = integer_masses(c)
    C = km.capacity_of(cap)
    for i, tau in enumerate(integer_taus(c)):
        ld = C if i % 2 == 0 else max(1, C // 2 - 1)
        names = ("bits", "count", "ids", "d2")
        ref = check_against_reference(c, masses, tau, launch(c, masses, tau, 0, names, ld_out=ld),
                                      launch(c, masses, tau, 1, names, ld_out=ld), ld, True)
        assert ref["reached"].all()


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", [c for c in CASES if c[2]] + WRAP,
                         ids=[i for i, c in zip(IDS, CASES) if c[2]] + case_ids(WRAP))
def test_zero_masses_in_front_of_the_crossing(n, dim, dup, n_cells, cap):
    """Doubled points: the even id of a place has mass 0, the odd one a mass in 1..9 (the last point, which has no copy,
    too).  Equal d2 words order by id, so the copies of a place are neighbours in every list and its first L keys hold
    floor(L / 2) whole places: tau <= L // 2 is reached by construction, with a zero-mass key in front of every other."""
    c = case(n, dim, dup, n_cells, cap)
    masses = zero_masses(c)
    for tau in zero_taus(c):
        names = ("bits", "count", "ids")
        ref = check_against_reference(c, masses, tau, launch(c, masses, tau, 0, names), launch(c, masses, tau, 1, names),
                                      km.capacity_of(cap), True)
        assert ref["reached"].all()
        # a zero-mass key comes first, unless the point without a copy is the nearest
        assert ((ref["count"] >= 2) | (c["ids"][:, 0] == n - 1)).all()


def test_whole_cloud_in_the_list():
    """n_pts = 1000 <= C = 1024: the list holds the whole cloud; masses in 0..9, tau up to the total."""
    c = case(*WHOLE_CLOUD)
    rng = np.random.default_rng(77)
    masses = rng.integers(0, 10, size=c["n"]).astype(np.float32)
    total = float(masses.astype(np.float64).sum())
    names = ("bits", "count", "ids", "d2")
    for tau in (total, total / 2, 3.0):
        ref = check_against_reference(c, masses, tau, launch(c, masses, tau, 0, names), launch(c, masses, tau, 1, names),
                                      1024, True)
        assert ref["reached"].all()
    last_heavy = np.max(np.nonzero(masses)[0])
    ref = km.crossing(c["d2f"], c["ids"], masses, total, 1000)
    assert ref["count"].min() > 900 and last_heavy > 900       # tau = the total: the crossing is the last site with mass
    # one more than the total: not reached, the count is the whole cloud
    got = launch(c, masses, total + 1, 1, ("bits", "count", "ids"))
    assert bool((got["bits"] == km.INF_WORD).all()) and bool((got["count"] == 1000).all())
    check_rows(got, c, np.full(c["N"], 1000), 1024)


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", CASES[::3], ids=IDS[::3])
def test_heavy_site(n, dim, dup, n_cells, cap):
    """Point 0 holds more than tau and is the first key of the cells AT it (d2 = 0 and the smallest id of its place)."""
    c = case(n, dim, dup, n_cells, cap)
    masses = np.ones(n, dtype=np.float32)
    tau = float(min(c["L"], 37))
    masses[0] = tau + 5
    names = ("bits", "count", "ids", "d2")
    got0, got1 = launch(c, masses, tau, 0, names), launch(c, masses, tau, 1, names)
    check_against_reference(c, masses, tau, got0, got1, km.capacity_of(cap), True)
    at = c["R"]                                  # the samples of the first simplex
    for got in (got0, got1):
        assert bool((got["count"][:at] == 1).all()) and bool((got["ids"][:at, 0] == 0).all())
        assert bool((got["ids"][:at, 1] == -1).all()) and bool((got["bits"][:at] == 0).all())


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", CASES[1::2], ids=IDS[1::2])
def test_crossing_moves_back_and_falls_off_the_end(n, dim, dup, n_cells, cap):
    """Point 0 alone has mass; every other site has none.  A walk that meets point 0 early has a crossing at once, and
    every site nearer to the cell that it meets later moves the crossing back by a place - until, where more than L - 1
    sites are nearer, it falls off the end: that cell is not reached.  Some sites with a small mass beside it make
    crossings that need several of them."""
    c = case(n, dim, dup, n_cells, cap)
    for light, tau in ((0.0, 5.0), (0.25, 5.0)):
        masses = np.zeros(n, dtype=np.float32)
        masses[1::3] = light
        masses[0] = 10.0
        names = ("bits", "count", "ids", "d2")
        ref = check_against_reference(c, masses, tau, launch(c, masses, tau, 0, names), launch(c, masses, tau, 1, names),
                                      km.capacity_of(cap), True)
        print(f"light {light}: {int((~ref['reached']).sum())} of {c['N']} cells not reached, "
              f"counts {int(ref['count'].min())} .. {int(ref['count'].max())}")
        if n <= cap:
            assert ref["reached"].all()          # the list holds the whole cloud, point 0 included
        assert ref["reached"][:c["R"]].all()     # the cells AT point 0


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", CASES, ids=IDS)
def test_not_reached(n, dim, dup, n_cells, cap):
    """All masses 1 and tau = L + 1: no L sites hold it.  The word is +inf, the count L, the ids the L nearest."""
    c = case(n, dim, dup, n_cells, cap)
    ones = np.ones(n, dtype=np.float32)
    L, C = c["L"], km.capacity_of(cap)
    for stat in (0, 1):
        got = launch(c, ones, float(L + 1), stat, ("bits", "count", "ids", "d2"))
        assert bool((got["bits"] == km.INF_WORD).all()) and bool((got["count"] == L).all())
        check_rows(got, c, np.full(c["N"], L), C)
    got = launch(c, ones, float("nan"), 1, ("bits", "count"))          # a tau that is no number is never reached
    assert bool((got["bits"] == km.INF_WORD).all()) and bool((got["count"] == L).all())


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", CASES, ids=IDS)
def test_float_masses(n, dim, dup, n_cells, cap):
    """Masses uniform in (0, 1), float32.  The reference adds the same float32 masses in float64 in position order, the
    kernel in scan order: the prefix sums differ by at most L * 2^-53 * tau, so where the reference's crossing has a margin
    of 1e-9 * tau the position is the same; elsewhere (at most 1 % of the cells) only the value is compared - the two
    readings of an ambiguous crossing differ by at most margin / tau * w_next, which the tolerance carries."""
    c = case(n, dim, dup, n_cells, cap)
    masses, L = float_masses(c), c["L"]
    for tau in float_taus(c):
        ref = km.crossing(c["d2f"], c["ids"], masses, tau, L)
        sure = ref["margin"] >= 1e-9 * tau
        excluded = 1.0 - sure.mean()
        print(f"tau {tau}: {excluded:.2%} of {c['N']} cells excluded from the exact comparison, "
              f"{(~ref['reached']).sum()} not reached")
        assert (~sure).sum() <= 0.01 * c["N"]
        got0 = launch(c, masses, tau, 0, ("bits", "count", "ids"))
        got1 = launch(c, masses, tau, 1, ("bits", "count", "d2"))
        assert np.array_equal(got0["count"][sure], ref["count"][sure]) and np.array_equal(got1["count"][sure], ref["count"][sure])
        cols = np.arange(got0["ids"].shape[1])[None, :]
        want_ids = np.full(got0["ids"].shape, -1, dtype=np.int64)
        m = min(want_ids.shape[1], c["ids"].shape[1])
        want_ids[:, :m] = c["ids"][:, :m]
        want_ids[cols >= ref["count"][:, None]] = -1
        assert np.array_equal(got0["ids"][sure], want_ids[sure])
        r = ref["reached"] & sure
        assert np.array_equal(got0["bits"][r], ref["kth"][r].astype(np.float32).view(np.uint32))
        assert bool((got1["bits"][~ref["reached"] & sure] == km.INF_WORD).all())
        rr = ref["reached"]
        dtm = got1["bits"].view(np.float32).astype(np.float64)
        w_next = c["d2f"][np.arange(c["N"]), np.minimum(ref["count"], c["d2f"].shape[1] - 1)].astype(np.float64)
        tol = (km.dtm_bound(ref["count"] + 1) + 1e-12) * ref["dtm"] + 1e-9 * w_next
        ok = np.isfinite(dtm[rr]) & (np.abs(dtm[rr] - ref["dtm"][rr]) <= tol[rr])
        assert ok.all()


def test_sample_order():
    """NULL, a permutation, and a permutation with an entry out of range: the same words wherever a cell is computed,
    and the skipped cell - alone - keeps what the buffers held."""
    assert (1025, 3, True, 300, 256) in CASES
    c = case(1025, 3, True, 300, 256)
    rng = np.random.default_rng(11)
    masses = rng.integers(0, 10, size=c["n"]).astype(np.float32)
    tau, names = 40.0, ("bits", "count", "ids", "d2")
    base = launch(c, masses, tau, 1, names)
    perm = rng.permutation(c["N"]).astype(np.int32)
    got = launch(c, masses, tau, 1, names, sample_order=torch.as_tensor(perm, device=DEV))
    assert all(np.array_equal(got[k], base[k]) for k in names)
    bad = perm.copy()
    skipped = int(bad[5])
    bad[5] = c["N"] + 3
    got = launch(c, masses, tau, 1, names, sample_order=torch.as_tensor(bad, device=DEV))
    keep = np.arange(c["N"]) != skipped
    assert all(np.array_equal(got[k][keep], base[k][keep]) for k in names)
    assert int(got["count"][skipped]) == FILL and bool((got["ids"][skipped] == FILL).all())
    assert int(got["bits"][skipped]) == np.uint32(FILL & 0xFFFFFFFF) and bool((got["d2"][skipped] == np.uint32(FILL & 0xFFFFFFFF)).all())


def test_refusals_and_empty_calls():
    c = case(*WHOLE_CLOUD)
    lib, st = _native.load(), _native.current_stream_ptr(DEV)
    masses = torch.ones(c["n"], dtype=torch.float32, device=DEV)
    tau = torch.tensor([5.0], dtype=torch.float64, device=DEV)
    outs = {k: torch.full((c["N"] * (64 if k in ("out_ids", "out_d2") else 1),), FILL, dtype=torch.int32, device=DEV)
            for k in ("out_bits", "out_count", "out_ids", "out_d2")}
    good = dict(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes,
                verts=c["verts"], weights=c["weights"], R=c["R"], capacity=64, n_simplices=c["n_s"], stat=1, ld_out=64,
                order=c["index"].order32, masses=masses, target=tau, **outs)

    def call(**change):
        return None, mass_entry(**{**good, **change})

    def refused(message, **change):
        _, rc = call(**change)
        assert rc != 0, message
        got = lib.flooder_last_error().decode()
        assert got.startswith("flooder_knn_mass_f32: ") and message in got, (message, got)

    assert call()[1] == 0
    extra = ("capacity", "masses", "target", "ld_out", "out_count")
    for spoil in ("abi", "size"):
        blk = _native.KnnWide(k=64, **{k: v for k, v in good.items() if k not in extra})
        if spoil == "abi":
            blk.abi = 2
        else:
            blk.size = ctypes.sizeof(blk) + 8
        assert mass_entry(block=blk, **{k: good[k] for k in extra}) != 0
        assert b"flooder_knn_mass_f32: bad parameter block" in lib.flooder_last_error()
    assert lib.flooder_knn_mass_f32(None, _native.ptr(masses), _native.ptr(tau), 64, None, st) != 0
    for cap in (0, -1, 1025):
        refused("capacity (the block's k) must be in 1..1024", capacity=cap)
    for dim in (1, 9):
        refused("dim must be in 2..8", dim=dim)
    for stat in (-1, 2):
        refused("stat must be 0 (kth) or 1 (dtm)", stat=stat)
    refused("no points", n_pts=0)
    refused("more than 2^31 - 1 points", n_pts=1 << 31)
    refused("n_simplices * R must be below 2^32 - 2", n_simplices=(1 << 32) - 2, R=1)
    refused("no output", out_bits=None, out_count=None, out_ids=None, out_d2=None)
    refused("out_ids needs order", order=None)
    for ld in (0, 65, -3):
        refused("ld_out must be in 1..64", ld_out=ld)
    refused("ld_out must be in 1..128", ld_out=129, capacity=65)
    refused("masses and target must not be NULL", masses=None)
    refused("masses and target must not be NULL", target=None)
    refused("bad argument", verts=None)
    # ld_out is not looked at without rows; an empty call writes nothing
    assert call(ld_out=0, out_ids=None, out_d2=None)[1] == 0
    for t in outs.values():
        t.fill_(FILL)
    assert call(n_simplices=0)[1] == 0 and call(R=0)[1] == 0
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in outs.values())
