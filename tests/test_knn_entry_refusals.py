"""What the entry points of the k-nearest family refuse, with which code and which message: ``flooder_sweep_knn_f32``,
``flooder_sweep_knn_sorted_f32``, ``flooder_knn_ids_sorted_f32``, ``flooder_sweep_knn_profile_f32``,
``flooder_witness_knn``, ``flooder_knn_merge_f32``, ``flooder_knn_wide_f32`` and ``flooder_witness_search``.  Every call here returns before a pointer is looked at or a kernel
is launched (no device needed; the non-null "pointers" are the number 4096).  A block that is wrong in two ways gets the
message of the check that comes first: the order of the checks is part of the table.

The expected codes and messages were recorded from the library as it was while every entry still made its own checks,
before the three sweep entries and the witness entry came to share them (the wide entry and the witness search: before
the wide entry took the family's range check and the three stack walks one refusal of a cloud too large for the stack
word): the table asserts those values, not what the code gives now."""
import ctypes

from flooder_amd import _native

OK, E_ARG = 0, -1
P = 4096              # a pointer that is not NULL (never dereferenced: every call below is refused, or has nothing to do)
TWO31 = 1 << 31       # one point more than 32-bit ids hold

SWEEP = ("flooder_sweep_knn_f32", _native.KnnSweep)
SORTED = ("flooder_sweep_knn_sorted_f32", _native.KnnSorted)
IDS = ("flooder_knn_ids_sorted_f32", _native.KnnIds)
PROFILE = ("flooder_sweep_knn_profile_f32", _native.KnnProfile)
WITNESS = ("flooder_witness_knn", _native.WitnessKnn)
MERGE = ("flooder_knn_merge_f32", _native.KnnMerge)
WIDE = ("flooder_knn_wide_f32", _native.KnnWide)
SEARCH = ("flooder_witness_search", _native.WitnessSearch)
FAMILY = (SWEEP, SORTED, IDS)

# the messages, without the "<entry>: " in front of them
SIZE = "bad parameter block (abi / size)"
K = "k must be in 1..32"
DIM = "dim must be in 2..8"
STAT = "stat must be 0 (kth) or 1 (dtm)"
ARG = "bad argument (null pointer, fewer points than k, k1, R)"
NO_SAMPLE_ORDER = "sample_order is NULL"
NO_ORDER = "order is NULL"
NO_OUT_IDS = "out_ids is NULL"
TOO_MANY_SAMPLES = "n_simplices * R must be below 2^32 - 2"
TOO_MANY_POINTS = "more than 2^31 - 1 points"
N_COLS = "n_cols must be in 1..64"
COL_K = "col_k must be in 1..32"
COL_STAT = "col_stat must be 0 (kth) or 1 (dtm)"
COL_TWICE = "a (k, stat) column is listed twice"
FEWER_THAN_LARGEST = "fewer points than the largest k"
PROFILE_ARG = "bad argument (null pointer, k1, R)"
FEWER = "fewer points than k"
WITNESS_ARG = "bad argument (null pointer, k1, R, n_queries)"
N_LISTS = "n_lists must be at least 1"
N_CELLS = "n_cells must not be negative"
MERGE_ARG = "bad argument (null pointer, more than 2^32 - 256 cells)"
WIDE_K = "k must be in 1..1024"
WIDE_NO_OUTPUT = "no output (out_bits, out_ids and out_d2 are all NULL)"
WIDE_NO_ORDER = "out_ids needs order (tree row -> original id)"
WIDE_ARG = "bad argument (null pointer, k1, R, n_simplices)"
SEARCH_ARG = "bad argument"

_LATTICE = dict(n_pts=1000, dim=3, k1=4, R=70, n_simplices=10)
_POINTERS = {k: P for k in "pts_sorted nodes verts weights queue out_bits".split()}
GOOD = {   # what each entry would accept (and launch: never passed on as it is)
    SWEEP: dict(_LATTICE, k=8, stat=1, **_POINTERS),
    SORTED: dict(_LATTICE, k=8, stat=1, sample_order=P, **_POINTERS),
    IDS: dict(_LATTICE, k=8, stat=1, sample_order=P, order=P, out_ids=P, **_POINTERS),
    PROFILE: dict(_LATTICE, columns=[(2, 0), (3, 1)], **_POINTERS),
    WITNESS: dict(_LATTICE, k=8, stat=0, n_queries=5, **{k: P for k in (
        "pts_sorted nodes order verts weights q_simplex q_row q_stat out_ids not_found").split()}),
    MERGE: dict(n_cells=100, n_lists=2, k=8, stat=0, lists=P, out_bits=P),
    WIDE: dict(n_pts=5000, dim=3, k1=4, R=10, n_simplices=7, k=200, stat=1,
               **{k: P for k in "pts_sorted nodes verts weights out_bits".split()}),
    SEARCH: dict(_LATTICE, n_queries=5, **{k: P for k in (
        "pts_sorted nodes order verts weights q_simplex q_row q_d2 out_point not_found").split()}),
}


def _pointers(entry, but=()):
    return [f for f, v in GOOD[entry].items() if v == P and f not in but]


def _cases():
    """(entry, what differs from GOOD[entry], recorded code, recorded message behind "<entry>: " or None)."""
    out = []

    def bad(entry, text, **change):
        out.append((entry, change, E_ARG, text))

    def nothing_to_do(entry, **change):
        out.append((entry, {**{f: None for f in _pointers(entry)}, **change}, OK, None))

    # ---- the three sweeps of one block family
    for entry in FAMILY:
        for field in _pointers(entry, but=("sample_order", "order", "out_ids", "out_bits")):
            bad(entry, ARG, **{field: None})
        for k in (0, 33):
            bad(entry, K, k=k)
        for dim in (1, 9):
            bad(entry, DIM, dim=dim)
        for stat in (2, -1):
            bad(entry, STAT, stat=stat)
        for k1 in (0, 10):
            bad(entry, ARG, k1=k1)
        bad(entry, ARG, R=-1)
        bad(entry, ARG, n_simplices=-1)
        bad(entry, ARG, n_pts=7)                               # fewer points than k
        nothing_to_do(entry, n_simplices=0)
        nothing_to_do(entry, R=0)
        # inside the bound: refused by a later check
        for change in (dict(k=1), dict(k=32), dict(dim=2), dict(dim=8), dict(stat=0), dict(k1=1), dict(k1=9), dict(n_pts=8)):
            bad(entry, ARG, pts_sorted=None, **change)
        # wrong in two ways: the first check in the entry's order speaks
        bad(entry, K, k=0, dim=9)
        bad(entry, K, k=33, stat=2, n_simplices=0)
        bad(entry, DIM, dim=9, stat=2)
        bad(entry, DIM, dim=1, R=0)
        bad(entry, STAT, stat=2, pts_sorted=None)
        bad(entry, STAT, stat=2, n_pts=7)
        bad(entry, ARG, n_pts=7, n_simplices=(1 << 31) - 1, R=2)
        # the size rule
        bad(entry, SIZE, abi=2)
        bad(entry, SIZE, size=4)
        bad(entry, SIZE, size=ctypes.sizeof(entry[1]) + 8)
        # out_bits NULL: the others stop at the pointer check (the ids entry goes on to its next checks: below)
        if entry is not IDS:
            bad(entry, ARG, out_bits=None)
    for entry in (SORTED, IDS):
        bad(entry, NO_SAMPLE_ORDER, sample_order=None)
        bad(entry, TOO_MANY_SAMPLES, n_simplices=(1 << 31) - 1, R=2)        # 2^32 - 2 samples
        bad(entry, TOO_MANY_SAMPLES, n_simplices=(1 << 32) - 1, R=1)
        bad(entry, NO_SAMPLE_ORDER, sample_order=None, n_simplices=(1 << 31) - 1, R=2)
        bad(entry, ARG, sample_order=None, weights=None)
        bad(entry, NO_SAMPLE_ORDER, size=ctypes.sizeof(_native.KnnSweep))   # a sweep-sized block: the tail reads as NULL
    bad(SWEEP, SIZE, size=ctypes.sizeof(_native.KnnIds))                    # an ids-sized block
    bad(SWEEP, SIZE, size=ctypes.sizeof(_native.KnnSorted))
    bad(SORTED, SIZE, size=ctypes.sizeof(_native.KnnIds))
    bad(SORTED, ARG, out_bits=None, sample_order=None)
    # the ids entry's own
    bad(IDS, NO_ORDER, order=None)
    bad(IDS, NO_OUT_IDS, out_ids=None)
    bad(IDS, NO_ORDER, size=ctypes.sizeof(_native.KnnSorted))               # a sorted-sized block
    bad(IDS, NO_ORDER, out_bits=None, order=None)
    bad(IDS, NO_SAMPLE_ORDER, out_bits=None, sample_order=None, order=None)
    bad(IDS, NO_ORDER, order=None, out_ids=None)
    bad(IDS, NO_OUT_IDS, out_ids=None, n_simplices=(1 << 31) - 1, R=2)
    bad(IDS, TOO_MANY_POINTS, n_pts=TWO31)
    bad(IDS, TOO_MANY_POINTS, n_pts=TWO31, n_simplices=0)                   # before "nothing to do"
    bad(IDS, TOO_MANY_POINTS, n_pts=TWO31, R=0, **{f: None for f in _pointers(IDS)})
    bad(IDS, TOO_MANY_POINTS, n_pts=TWO31, pts_sorted=None, order=None)
    bad(IDS, STAT, n_pts=TWO31, stat=2)
    bad(IDS, ARG, n_pts=TWO31 - 1, pts_sorted=None)

    # ---- the profile sweep
    for field in _pointers(PROFILE):
        bad(PROFILE, PROFILE_ARG, **{field: None})
    for n_cols in (0, 65):
        bad(PROFILE, N_COLS, n_cols=n_cols)
    for k in (0, 33):
        bad(PROFILE, COL_K, columns=[(2, 0), (k, 0)])
    for stat in (2, -1):
        bad(PROFILE, COL_STAT, columns=[(2, 0), (3, stat)])
    bad(PROFILE, COL_TWICE, columns=[(2, 0), (3, 1), (2, 0)])
    for dim in (1, 9):
        bad(PROFILE, DIM, dim=dim)
    bad(PROFILE, FEWER_THAN_LARGEST, n_pts=2)
    for k1 in (0, 10):
        bad(PROFILE, PROFILE_ARG, k1=k1)
    bad(PROFILE, PROFILE_ARG, R=-1)
    bad(PROFILE, PROFILE_ARG, n_simplices=-1)
    nothing_to_do(PROFILE, n_simplices=0)
    nothing_to_do(PROFILE, R=0)
    for change in (dict(n_cols=1), dict(columns=[(1, 0), (32, 1)]), dict(dim=2), dict(dim=8), dict(n_pts=3), dict(k1=1),
                   dict(k1=9)):
        bad(PROFILE, PROFILE_ARG, pts_sorted=None, **change)
    bad(PROFILE, N_COLS, n_cols=0, dim=9)
    bad(PROFILE, COL_K, columns=[(0, 0)], dim=9)
    bad(PROFILE, COL_K, columns=[(33, 2)])
    bad(PROFILE, COL_STAT, columns=[(2, 0), (2, 2), (2, 0)])
    bad(PROFILE, DIM, dim=9, n_pts=2)
    bad(PROFILE, DIM, dim=1, n_simplices=0)
    bad(PROFILE, FEWER_THAN_LARGEST, n_pts=2, n_simplices=0)
    bad(PROFILE, FEWER_THAN_LARGEST, n_pts=2, pts_sorted=None)
    bad(PROFILE, SIZE, abi=0)
    bad(PROFILE, SIZE, size=ctypes.sizeof(_native.KnnProfile) + 8)

    # ---- the witnesses of the robust values
    for field in _pointers(WITNESS):
        bad(WITNESS, WITNESS_ARG, **{field: None})
    for k in (0, 33):
        bad(WITNESS, K, k=k)
    for dim in (1, 9):
        bad(WITNESS, DIM, dim=dim)
    for stat in (2, -1):
        bad(WITNESS, STAT, stat=stat)
    bad(WITNESS, FEWER, n_pts=7)
    bad(WITNESS, TOO_MANY_POINTS, n_pts=TWO31)
    bad(WITNESS, WITNESS_ARG, k1=0)
    for R in (0, -1):
        bad(WITNESS, WITNESS_ARG, R=R)
    bad(WITNESS, WITNESS_ARG, n_queries=-1)
    nothing_to_do(WITNESS, n_queries=0)
    for change in (dict(k=1), dict(k=32), dict(dim=2), dict(dim=8), dict(stat=1), dict(n_pts=8), dict(n_pts=TWO31 - 1),
                   dict(k1=1), dict(R=1)):
        bad(WITNESS, WITNESS_ARG, pts_sorted=None, **change)
    bad(WITNESS, K, k=0, dim=9)
    bad(WITNESS, DIM, dim=9, stat=2)
    bad(WITNESS, STAT, stat=2, n_pts=7)
    bad(WITNESS, FEWER, n_pts=7, n_queries=0)
    bad(WITNESS, FEWER, n_pts=7, pts_sorted=None)
    bad(WITNESS, TOO_MANY_POINTS, n_pts=TWO31, n_queries=0)
    bad(WITNESS, TOO_MANY_POINTS, n_pts=TWO31, order=None)
    bad(WITNESS, SIZE, abi=2)
    bad(WITNESS, SIZE, size=ctypes.sizeof(_native.WitnessKnn) + 8)

    # ---- the merge of the point shards' lists
    for field in _pointers(MERGE):
        bad(MERGE, MERGE_ARG, **{field: None})
    for k in (0, 33):
        bad(MERGE, K, k=k)
    for stat in (2, -1):
        bad(MERGE, STAT, stat=stat)
    bad(MERGE, N_LISTS, n_lists=0)
    bad(MERGE, N_CELLS, n_cells=-1)
    bad(MERGE, MERGE_ARG, n_cells=0xffffff01)
    nothing_to_do(MERGE, n_cells=0)
    for change in (dict(k=1), dict(k=32), dict(stat=1), dict(n_lists=1), dict(n_cells=0xffffff00)):
        bad(MERGE, MERGE_ARG, lists=None, **change)
    bad(MERGE, K, k=0, stat=2)
    bad(MERGE, STAT, stat=2, n_lists=0)
    bad(MERGE, N_LISTS, n_lists=0, n_cells=-1)
    bad(MERGE, N_CELLS, n_cells=-1, lists=None)
    bad(MERGE, K, k=33, n_cells=0)
    bad(MERGE, SIZE, abi=2)
    bad(MERGE, SIZE, size=ctypes.sizeof(_native.KnnMerge) + 8)

    # ---- the wide sweep (k up to 1024)
    for k in (0, -3, 1025):
        bad(WIDE, WIDE_K, k=k)
    for dim in (1, 9):
        bad(WIDE, DIM, dim=dim)
    for stat in (2, -1):
        bad(WIDE, STAT, stat=stat)
    bad(WIDE, FEWER, n_pts=199)
    bad(WIDE, TOO_MANY_POINTS, n_pts=TWO31)
    bad(WIDE, TOO_MANY_SAMPLES, n_simplices=TWO31, R=2)
    bad(WIDE, TOO_MANY_SAMPLES, n_simplices=(1 << 32) - 2, R=1)
    bad(WIDE, WIDE_NO_OUTPUT, out_bits=None)
    bad(WIDE, WIDE_NO_ORDER, out_ids=P)
    bad(WIDE, WIDE_NO_ORDER, out_ids=P, out_bits=None)
    for field in _pointers(WIDE, but=("out_bits",)):
        bad(WIDE, WIDE_ARG, **{field: None})
    for k1 in (0, -1):
        bad(WIDE, WIDE_ARG, k1=k1)
    bad(WIDE, WIDE_ARG, R=-1)
    bad(WIDE, WIDE_ARG, n_simplices=-1)
    nothing_to_do(WIDE, n_simplices=0, out_bits=P)
    nothing_to_do(WIDE, R=0, out_bits=P)
    nothing_to_do(WIDE, n_simplices=0, out_bits=None, out_d2=P)
    # inside the bound: refused by a later check
    for change in (dict(k=1), dict(k=33), dict(k=1024), dict(dim=2), dict(dim=8), dict(stat=0), dict(n_pts=200),
                   dict(n_pts=TWO31 - 1), dict(n_simplices=(1 << 32) - 3, R=1), dict(out_ids=P, order=P),
                   dict(out_bits=None, out_d2=P)):
        bad(WIDE, WIDE_ARG, pts_sorted=None, **change)
    # wrong in two ways: the first check in the entry's order speaks (fewer points than k and more than 2^31 - 1 of
    # them cannot both hold with k in range: each is paired with the check behind it instead)
    bad(WIDE, WIDE_K, k=0, dim=9)
    bad(WIDE, WIDE_K, k=1025, stat=2, n_simplices=0)
    bad(WIDE, DIM, dim=9, stat=2)
    bad(WIDE, DIM, dim=1, R=0)
    bad(WIDE, STAT, stat=2, n_pts=199)
    bad(WIDE, STAT, stat=2, n_pts=TWO31)
    bad(WIDE, FEWER, n_pts=199, n_simplices=TWO31, R=2)
    bad(WIDE, FEWER, n_pts=-1, out_bits=None)
    bad(WIDE, FEWER, n_pts=199, n_simplices=0)                              # before "nothing to do"
    bad(WIDE, TOO_MANY_POINTS, n_pts=TWO31, n_simplices=TWO31, R=2)
    bad(WIDE, TOO_MANY_POINTS, n_pts=TWO31, R=0)
    bad(WIDE, TOO_MANY_SAMPLES, n_simplices=TWO31, R=2, out_bits=None)
    bad(WIDE, WIDE_NO_OUTPUT, out_bits=None, out_ids=None, order=None, n_simplices=0)
    bad(WIDE, WIDE_NO_OUTPUT, out_bits=None, pts_sorted=None)
    bad(WIDE, WIDE_NO_ORDER, out_ids=P, n_simplices=0)
    bad(WIDE, WIDE_NO_ORDER, out_ids=P, pts_sorted=None)
    bad(WIDE, WIDE_NO_ORDER, out_ids=P, R=-1)
    bad(WIDE, SIZE, abi=2)
    bad(WIDE, SIZE, size=4)
    bad(WIDE, SIZE, size=ctypes.sizeof(_native.KnnWide) + 8)
    bad(WIDE, WIDE_NO_OUTPUT, size=ctypes.sizeof(_native.KnnSweep) - 24)      # a block that ends before out_bits

    # ---- the witness search of the plain values: one refusal for everything behind the size rule
    for field in _pointers(SEARCH):
        bad(SEARCH, SEARCH_ARG, **{field: None})
    for change in (dict(n_pts=0), dict(n_pts=TWO31), dict(k1=0), dict(R=0), dict(R=-1), dict(n_queries=-1), dict(dim=1),
                   dict(dim=9), dict(dim=9, n_pts=0), dict(n_pts=TWO31, order=None)):
        bad(SEARCH, SEARCH_ARG, **change)
    for change in (dict(n_pts=1), dict(n_pts=TWO31 - 1), dict(k1=1), dict(R=1), dict(dim=2), dict(dim=8), dict(n_simplices=0)):
        bad(SEARCH, SEARCH_ARG, pts_sorted=None, **change)
    nothing_to_do(SEARCH, n_queries=0)
    nothing_to_do(SEARCH, n_queries=0, dim=9, n_pts=TWO31)                  # "nothing to do" comes first
    bad(SEARCH, SIZE, abi=2)
    bad(SEARCH, SIZE, size=4, n_queries=0)
    bad(SEARCH, SIZE, size=ctypes.sizeof(_native.WitnessSearch) + 8)
    return out


def _block(entry, change):
    fields = {**GOOD[entry], **{f: v for f, v in change.items() if f != "n_cols"}}
    columns = fields.pop("columns", None)
    blk = entry[1](columns, **fields) if columns is not None else entry[1](**fields)
    if "n_cols" in change:   # (the columns fill it: set it behind them)
        blk.n_cols = change["n_cols"]
    return blk


def test_table_covers_what_it_must():
    cases = _cases()
    assert {c[0] for c in cases} == set(GOOD) and len(cases) > 300
    assert sum(1 for c in cases if c[2] == OK) == 15
    assert sum(1 for c in cases if c[2] != OK and len(c[1]) >= 2 and "size" not in c[1]) >= 100   # wrong in two ways
    assert sum(1 for c in cases if c[0] is WIDE) >= 55 and sum(1 for c in cases if c[0] is SEARCH) >= 30
    # the three blocks are what the size cases take them for
    assert ctypes.sizeof(_native.KnnSweep) < ctypes.sizeof(_native.KnnSorted) < ctypes.sizeof(_native.KnnIds)


def test_refusals_codes_and_messages_are_the_recorded_ones():
    lib = _native.load()
    wrong = []
    for entry, change, code, text in _cases():
        name = entry[0]
        blk = _block(entry, change)
        rc = getattr(lib, name)(ctypes.byref(blk), None)
        msg = lib.flooder_last_error().decode()
        if rc != code or (text is not None and msg != f"{name}: {text}"):
            wrong.append((name, change, rc, msg, code, text))
    assert not wrong, wrong


def test_a_null_block_is_a_bad_parameter_block():
    lib = _native.load()
    for name, _ in GOOD:
        assert getattr(lib, name)(None, None) == E_ARG
        assert lib.flooder_last_error().decode() == f"{name}: {SIZE}"
