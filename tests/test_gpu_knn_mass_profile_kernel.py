"""``flooder_knn_mass_profile_f32`` on its own, through ``_native``: ONE walk of the mass kernel to the largest target
writes a plane of statistic words and a plane of counts per listed (target, stat) column, and every plane equals, word
for word, what a single ``flooder_knn_mass_f32`` launch at that target, stat and capacity writes - whatever the order of
the columns (ascending, descending, shuffled: in the last two the largest target is not the last one).  Also against the float64 rule over the keys of the integer brute
force (``knn_mass_reference``), with unit masses against ``flooder_knn_wide_f32``, with zero masses in front of the
crossing, with columns that are reached and columns that are not in one launch, with general float masses, and the
refusals.  The shapes are a subset of ``test_gpu_knn_mass_kernel``'s cases (its inputs, references and single launches
are imported, not copied); planes lie ``N + GAP`` words apart with sentinel words between and behind them, every launch
is made twice and must write the same words."""

import ctypes

import numpy as np
import pytest
import torch

from flooder_amd import _native

import knn_mass_reference as km
import knn_wide_reference as kw  # noqa: F401  (the brute force behind ``case``: named here as the reference it is)
from test_gpu_knn_mass_kernel import (CASES, WRAP, case, case_ids, float_masses, float_taus, integer_masses, launch, wide,
                                      zero_masses, zero_taus)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GAP = 37            # words between the planes (and behind the last) that must stay untouched
FILL = -7
WHO = "flooder_knn_mass_profile_f32"
# (n points, dim, every point doubled, cells, capacity): a subset of the single entry's cases
SUBSET = [(15, 2, False, 1, 64), (1000, 3, False, 65, 64), (1000, 5, True, 300, 1024), (1025, 3, True, 300, 256),
          (1025, 8, True, 63, 1024), (30_001, 2, True, 300, 64), (30_001, 5, True, 63, 256)]
ALL = SUBSET + WRAP[:1]
IDS = case_ids(ALL)
# the cases in which, with masses 1..9, the target 5 * L is reached by some cells and not by others (n > C, so that
# the L nearest sites differ from cell to cell; asserted from the reference in the test)
MIXED = [(1000, 3, False, 65, 64), (1025, 3, True, 300, 256), (30_001, 2, True, 300, 64), (30_001, 5, True, 63, 256),
         WRAP[0]]


def test_cases_cover_what_they_must():
    assert all(c in CASES for c in SUBSET) and all(c in ALL for c in MIXED)
    assert {c[0] for c in SUBSET} == {15, 1000, 1025, 30_001} and {c[1] for c in SUBSET} == {2, 3, 5, 8}
    assert {c[4] for c in SUBSET} == {64, 256, 1024} and {c[3] for c in SUBSET} == {1, 63, 65, 300}
    assert any(c[2] for c in SUBSET) and any(not c[2] for c in SUBSET)         # doubled points, and single ones
    assert any(c[0] < c[4] for c in SUBSET)                                    # the whole cloud is in the list
    assert any(c[0] > c[4] and c[4] == cap for c in SUBSET for cap in (64, 256, 1024))
    assert len(ALL) == len(SUBSET) + 1 and ALL[-1][3] > 4 * 256 * 16           # more cells than the grid has waves
    assert all(c[0] > c[4] for c in MIXED)


def profile_entry(block, masses, n_cols, targets, col_stat, plane_stride, out_count):
    """``flooder_knn_mass_profile_f32`` by name -> return code (``col_stat``: a ctypes int32 array or None)."""
    return _native.load().flooder_knn_mass_profile_f32(ctypes.byref(block), _native.ptr(masses), int(n_cols),
                                                       _native.ptr(targets), col_stat, int(plane_stride),
                                                       _native.ptr(out_count), _native.current_stream_ptr(DEV))


def block_of(c, **fields):
    kw_ = dict(pts_sorted=c["index"].pts, n_pts=c["n"], dim=c["dim"], k1=c["k1"], nodes=c["index"].nodes, verts=c["verts"],
               weights=c["weights"], R=c["R"], k=c["cap"], n_simplices=c["n_s"], stat=0, order=c["index"].order32)
    kw_.update(fields)
    return _native.KnnWide(**kw_)


def stat_array(stats):
    return (ctypes.c_int32 * max(len(stats), 1))(*[int(s) for s in stats])


def profile(c, masses, cols, stride=None, sample_order=None, with_count=True):
    """One ``flooder_knn_mass_profile_f32`` over ``cols`` = [(tau, stat), ...] -> (words (n_cols, N) uint32, counts
    (n_cols, N) int32 or None); made TWICE into fresh buffers, which must agree; the words between and behind the planes
    must keep their fill."""
    N = c["N"]
    stride = N + GAP if stride is None else stride
    m = torch.as_tensor(np.asarray(masses, dtype=np.float32), device=DEV)
    t = torch.tensor([tau for tau, _ in cols], dtype=torch.float64, device=DEV)
    runs = []
    for _ in range(2):
        bits = torch.full((len(cols) * stride + GAP,), FILL, dtype=torch.int32, device=DEV)
        count = torch.full((len(cols) * stride + GAP,), FILL, dtype=torch.int32, device=DEV) if with_count else None
        blk = block_of(c, sample_order=sample_order, out_bits=bits)
        _native.check(profile_entry(blk, m, len(cols), t, stat_array([s for _, s in cols]), stride, count), WHO)
        out = []
        for buf in (bits, count):
            if buf is None:
                out.append(None)
                continue
            assert bool((buf[len(cols) * stride:] == FILL).all()), "the words behind the planes were written"
            planes = buf[:len(cols) * stride].view(len(cols), stride)
            assert bool((planes[:, N:] == FILL).all()), "the words between the planes were written"
            out.append(planes[:, :N].contiguous().cpu().numpy())
        runs.append((out[0].view(np.uint32), out[1]))
    assert np.array_equal(runs[0][0], runs[1][0]), "two launches differ (words)"
    assert not with_count or np.array_equal(runs[0][1], runs[1][1]), "two launches differ (counts)"
    return runs[0]


def orders(cols):
    """The columns ascending, descending and shuffled; in the last two the largest target is not the last column."""
    cols = sorted(cols)
    rng = np.random.default_rng(len(cols))
    shuffled = [cols[i] for i in rng.permutation(len(cols))]
    if shuffled[-1][0] == cols[-1][0]:
        shuffled = shuffled[::-1]
    out = [cols, cols[::-1], shuffled]
    for o in out[1:]:
        assert sorted(o) == cols and (o[-1][0] < cols[-1][0] or len({t for t, _ in cols}) == 1)
    return out


def singles(c, masses, cols):
    """{(tau, stat): (words, counts)} of single ``flooder_knn_mass_f32`` launches."""
    out = {}
    for tau, stat in cols:
        got = launch(c, masses, tau, stat, ("bits", "count"))
        out[(tau, stat)] = (got["bits"], got["count"])
    return out


def assert_planes(words, counts, cols, want, rows=None):
    for i, col in enumerate(cols):
        w, n = want[col]
        sel = slice(None) if rows is None else rows[col]
        assert np.array_equal(words[i][sel], w[sel]), (col, np.argwhere(words[i] != w)[:5].tolist())
        if counts is not None:
            assert np.array_equal(counts[i][sel], n[sel]), (col, np.argwhere(counts[i] != n)[:5].tolist())


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", ALL, ids=IDS)
def test_integer_masses_planes_are_the_single_calls(n, dim, dup, n_cells, cap):
    """Masses 1..9, targets {1, 2.5, L // 2, L} (all reached: any L sites hold at least L), both stats, three orders."""
    c = case(n, dim, dup, n_cells, cap)
    masses, L = integer_masses(c), c["L"]
    taus = sorted({1.0, 2.5, float(max(1, L // 2)), float(L)})
    cols = [(tau, stat) for tau in taus for stat in (0, 1)]
    want = singles(c, masses, cols)
    # ... which are themselves the rule: the crossing of the reference and the float32 replay of the "dtm" word (a
    # Python loop per row: every 16th row where there are thousands - the single entry's own test replays them all)
    some = slice(None) if c["N"] <= 1000 else slice(None, None, 16)
    for tau in taus:
        ref = km.crossing(c["d2f"], c["ids"], masses, tau, L)
        assert ref["reached"].all()
        assert np.array_equal(want[(tau, 0)][1], ref["count"]) and np.array_equal(want[(tau, 1)][1], ref["count"])
        assert np.array_equal(want[(tau, 0)][0], ref["kth"].astype(np.float32).view(np.uint32))
        assert np.array_equal(want[(tau, 1)][0][some],
                              km.dtm_words(c["d2f"][some], c["ids"][some], masses, tau, ref["count"][some]))
    for o in orders(cols):
        words, counts = profile(c, masses, o)
        assert_planes(words, counts, o, want)
    # planes exactly N words apart, a permuted sample_order, no counts: the same words
    o = orders(cols)[1]
    perm = torch.as_tensor(np.random.default_rng(5).permutation(c["N"]).astype(np.int32), device=DEV)
    words, counts = profile(c, masses, o, stride=c["N"], sample_order=perm, with_count=False)
    assert counts is None
    assert_planes(words, None, o, want)
    # one column alone is the single entry
    for col in (cols[-1], cols[2]):
        words, counts = profile(c, masses, [col])
        assert_planes(words, counts, [col], want)


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", [c for c in ALL if c[2]], ids=[i for i, c in zip(IDS, ALL) if c[2]])
def test_zero_masses_in_front_of_the_crossing(n, dim, dup, n_cells, cap):
    """Doubled points, the even id of a place without mass: a zero-mass key in front of every other (the single
    entry's test says why every tau of ``zero_taus`` is reached)."""
    c = case(n, dim, dup, n_cells, cap)
    masses = zero_masses(c)
    taus = zero_taus(c)
    assert taus
    cols = [(tau, stat) for tau in taus for stat in (0, 1)]
    want = singles(c, masses, cols)
    for tau in taus:
        ref = km.crossing(c["d2f"], c["ids"], masses, tau, c["L"])
        assert ref["reached"].all() and np.array_equal(want[(tau, 1)][1], ref["count"])
        assert ((ref["count"] >= 2) | (c["ids"][:, 0] == n - 1)).all()
    o = cols[::-1]
    words, counts = profile(c, masses, o)
    assert_planes(words, counts, o, want)


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", ALL, ids=IDS)
def test_unit_masses_are_the_wide_kernel(n, dim, dup, n_cells, cap):
    c = case(n, dim, dup, n_cells, cap)
    ks = [k for k in (1, 40, 64, 65, 1000) if k <= c["L"]]
    assert ks
    cols = [(float(k), stat) for k in ks[::-1] for stat in (1, 0)]
    cols = cols[1:] + cols[:1]                                    # (the largest target is not last)
    words, counts = profile(c, np.ones(n, dtype=np.float32), cols)
    for i, (tau, stat) in enumerate(cols):
        w_bits, _, _ = wide(c, int(tau), stat)
        assert np.array_equal(words[i], w_bits), (tau, stat)
        assert bool((counts[i] == int(tau)).all())


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", MIXED, ids=case_ids(MIXED))
def test_reached_and_not_reached_in_one_launch(n, dim, dup, n_cells, cap):
    """Masses 1..9, targets L / 2 (reached everywhere), 5 * L (the mean mass: some cells are reached, some are not) and
    10 * L (L sites hold at most 9 * L: nowhere).  A column that is not reached has the word of +inf and the count L;
    the smaller columns of a cell whose WALK is not reached still equal their single calls."""
    c = case(n, dim, dup, n_cells, cap)
    masses, L = integer_masses(c), c["L"]
    taus = (L / 2.0, 5.0 * L, 10.0 * L)
    refs = [km.crossing(c["d2f"], c["ids"], masses, tau, L) for tau in taus]
    assert refs[0]["reached"].all() and not refs[2]["reached"].any()
    mid = refs[1]["reached"]
    assert mid.any() and not mid.all(), "the case is wrong: the middle target needs cells of both kinds"
    cols = [(taus[2], 1), (taus[0], 1), (taus[1], 0), (taus[2], 0), (taus[0], 0), (taus[1], 1)]
    words, counts = profile(c, masses, cols)
    for i, (tau, stat) in enumerate(cols):
        ref = refs[taus.index(tau)]
        r = ref["reached"]
        assert np.array_equal(counts[i], ref["count"]) and bool((counts[i][~r] == L).all())
        assert bool((words[i][~r] == km.INF_WORD).all())
        if stat == 0:
            assert np.array_equal(words[i][r], ref["kth"][r].astype(np.float32).view(np.uint32))
        elif r.any():
            some = np.flatnonzero(r)[::1 if c["N"] <= 1000 else 16]    # (a Python loop per row)
            assert np.array_equal(words[i][some], km.dtm_words(c["d2f"][some], c["ids"][some], masses, tau, ref["count"][some]))
    assert_planes(words, counts, cols, singles(c, masses, cols))
    # ... and with the middle target as the walk's own: its cells of both kinds, the smaller column beside them
    cols = [(taus[1], 1), (taus[0], 1)]
    words, counts = profile(c, masses, cols)
    assert_planes(words, counts, cols, singles(c, masses, cols))
    assert bool((words[0][~mid] == km.INF_WORD).all()) and bool((words[1] != km.INF_WORD).all())


@pytest.mark.parametrize("n,dim,dup,n_cells,cap", SUBSET, ids=case_ids(SUBSET))
def test_float_masses(n, dim, dup, n_cells, cap):
    """Masses uniform in (0, 1), float32.  The reference adds them in float64 in position order, the kernel in scan
    order: the prefix sums differ by at most L * 2^-53 * tau, so where the reference's crossing has a margin above
    1e-9 * tau the position is the same in the reference, the single call and the profile.  On those rows (at least
    99 % of them, counted from the reference alone): counts and "kth" words exact, "dtm" within the header's bound plus
    what the differing prefix sum can move rho by (L * 2^-52 * tau of weight on the crossing's d2, over tau), and the
    planes equal to the single calls word for word."""
    c = case(n, dim, dup, n_cells, cap)
    masses, L = float_masses(c), c["L"]
    taus = sorted(set(float_taus(c)))
    cols = [(taus[-1], 0)] + [(tau, 1) for tau in taus] + [(tau, 0) for tau in taus[:-1]]
    assert cols[-1][0] < taus[-1] or len(taus) == 1
    want = singles(c, masses, cols)
    words, counts = profile(c, masses, cols)
    sure = {}
    for tau in taus:
        ref = km.crossing(c["d2f"], c["ids"], masses, tau, L)
        ok = ref["margin"] > 1e-9 * tau
        print(f"tau {tau}: {1.0 - ok.mean():.2%} of {c['N']} cells excluded, {(~ref['reached']).sum()} not reached")
        assert ok.sum() >= 0.99 * c["N"]
        for stat in (0, 1):
            sure[(tau, stat)] = ok
            i = cols.index((tau, stat))
            assert np.array_equal(counts[i][ok], ref["count"][ok])
            r = ok & ref["reached"]
            assert bool((words[i][ok & ~ref["reached"]] == km.INF_WORD).all())
            if stat == 0:
                assert np.array_equal(words[i][r], ref["kth"][r].astype(np.float32).view(np.uint32))
            else:
                got = words[i].view(np.float32).astype(np.float64)
                tol = km.dtm_bound(ref["count"]) * ref["dtm"] + L * 2.0 ** -52 * ref["kth"]
                err = np.abs(got[r] - ref["dtm"][r])
                print(f"  dtm: largest error / bound {float((err / np.maximum(tol[r], 1e-300)).max()) if r.any() else 0:.3f}")
                assert np.all(err <= tol[r])
    assert_planes(words, counts, cols, want, rows=sure)


def test_refusals_and_empty_calls():
    c = case(1000, 3, False, 65, 64)
    lib, N = _native.load(), c["N"]
    masses = torch.ones(c["n"], dtype=torch.float32, device=DEV)
    targets = torch.tensor([5.0, 2.0, 5.0], dtype=torch.float64, device=DEV)
    bits = torch.full((3 * N,), FILL, dtype=torch.int32, device=DEV)
    count = torch.full((3 * N,), FILL, dtype=torch.int32, device=DEV)
    rows = torch.full((N * 64,), FILL, dtype=torch.int32, device=DEV)
    good = dict(masses=masses, n_cols=3, targets=targets, col_stat=stat_array([1, 0, 1]), plane_stride=N, out_count=count)

    def call(block=None, **change):
        fields = {k: change.pop(k) for k in list(change) if k not in good}
        blk = block_of(c, **{"out_bits": bits, **fields}) if block is None else block
        return profile_entry(blk, **{**good, **change})

    def refused(message, **change):
        assert call(**change) != 0, message
        got = lib.flooder_last_error().decode()
        assert got.startswith(WHO + ": ") and message in got, (message, got)

    assert call() == 0                     # (two columns with the same target and stat are legal)
    assert call(out_count=None) == 0
    for spoil in ("abi", "size"):
        blk = block_of(c, out_bits=bits)
        if spoil == "abi":
            blk.abi = 2
        else:
            blk.size = ctypes.sizeof(blk) + 8
        assert call(block=blk) != 0
        assert (WHO + ": bad parameter block").encode() in lib.flooder_last_error()
    assert lib.flooder_knn_mass_profile_f32(None, _native.ptr(masses), 3, _native.ptr(targets), good["col_stat"], N, None,
                                            _native.current_stream_ptr(DEV)) == -1
    for n_cols in (0, -1, _native.KNN_COLS_MAX + 1):
        refused("n_cols must be in 1..64", n_cols=n_cols)
    refused("targets and col_stat must not be NULL", targets=None)
    refused("targets and col_stat must not be NULL", col_stat=None)
    for s in (-1, 2):
        refused("col_stat must be 0 (kth) or 1 (dtm)", col_stat=stat_array([1, s, 0]))
    for cap in (0, -1, 1025):
        refused("capacity (the block's k) must be in 1..1024", k=cap)
    for dim in (1, 9):
        refused("dim must be in 2..8", dim=dim)
    for stat in (-1, 2):
        refused("stat must be 0 (kth) or 1 (dtm)", stat=stat)
    refused("no points", n_pts=0)
    refused("more than 2^31 - 1 points", n_pts=1 << 31)
    refused("n_simplices * R must be below 2^32 - 2", n_simplices=(1 << 32) - 2, R=1, plane_stride=1 << 33)
    refused("out_ids and out_d2 must be NULL", out_ids=rows)
    refused("out_ids and out_d2 must be NULL", out_d2=rows)
    refused("out_bits (the planes) must not be NULL", out_bits=None)
    refused("masses must not be NULL", masses=None)
    refused("plane_stride must be at least n_simplices * R", plane_stride=N - 1)
    refused("bad argument", verts=None)
    # an empty call writes nothing (a plane_stride of 0 is then at least n_simplices * R)
    torch.cuda.synchronize()
    assert bool((rows == FILL).all())
    bits.fill_(FILL)
    count.fill_(FILL)
    assert call(n_simplices=0, plane_stride=0) == 0 and call(R=0) == 0
    torch.cuda.synchronize()
    assert bool((bits == FILL).all()) and bool((count == FILL).all())
