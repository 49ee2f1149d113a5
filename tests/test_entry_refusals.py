"""The entry points that have a parameter block refuse the same inputs with the same code through the block and through
their positional twin.  Every call here returns before a pointer is looked at or a kernel is launched (no device
needed; the non-null "pointers" are the number 4096).  The expected codes were recorded from the library as it was before
the positional functions became adapters of the block functions: the table asserts them, not what the code gives now."""
from flooder_amd import _native

OK, E_ARG = 0, -1
P = 4096         # a pointer that is not NULL (never dereferenced: every call below is refused, or has nothing to do)
BIG = 1 << 30    # points whose rows (16 bytes in 3-D) pass the 32-bit byte offsets of the witness and the cell sweep

# positional argument order of every twin, as field names of its block
WITNESS = ("flooder_fused_witness", "flooder_sweep_witness_f32", _native.FusedSweep,
           """pts_sorted n_pts dim nodes verts weights k1 R n_simplices coarse_rows n_coarse parents wit_queue d2_scratch memb
           n_faces face_bits face_slot flag_list flag_count flag_key flag_hist top top_list top_count simplex_weight
           wit_item_list plane_scratch wit_stats""")
CELL = ("flooder_fused_cell", "flooder_sweep_cell_faces_f32", _native.FusedSweep,
        """pts_sorted n_pts dim nodes verts weights k1 R n_simplices alpha cell_queue d2_scratch memb n_faces face_bits
        face_slot flag_list flag_count flag_key flag_hist top top_list top_count defer_list defer_c defer_ctl simplex_weight
        light_list heavy_list plane_scratch density_grid cloud_box cell_stats""")
FINISH = ("flooder_fused_finish", "flooder_finish_faces_f32", _native.FusedSweep,
          """pts_sorted n_pts dim nodes verts weights k1 R n_simplices flag_list flag_count flag_key flag_hist flag_sorted
          finish_ctl top top_list probed d2_scratch memb n_faces face_bits face_slot hard_scratch hard_cap finish_stats""")
FACES = ("flooder_sorted_faces", "flooder_sweep_bvh_sorted_faces_f32", _native.SortedSweep,
         "pts_sorted n_pts dim nodes verts weights k1 R n_simplices sample_order queue memb n_faces face_bits face_slot stats")
MINIMA = ("flooder_sorted_minima", "flooder_sweep_bvh_sorted_f32", _native.SortedSweep,
          "pts_sorted n_pts dim nodes verts weights k1 R n_simplices sample_order queue out_d2 stats")
SHARD = ("flooder_sorted_minima", "flooder_sweep_bvh_sorted_shard_f32", _native.SortedSweep,
         "pts_sorted n_pts dim nodes verts weights k1 R n_simplices sample_order shard_rank shard_world queue out_d2 stats")
FPS = ("flooder_fps_batched", "flooder_fps_batched_f32", _native.FpsBatched,
       """pts n_pts dim ld pts_sorted order n_lms start out_idx minsq bucket_box bucket_keys bucket_coord work_best work_rec
       work_ctr launches_out""")

SWEEP = dict(n_pts=1000, dim=3, k1=4, R=1024, n_simplices=10, n_faces=15)
GOOD = {   # what each entry would accept (and launch: never passed on as it is)
    WITNESS: dict(SWEEP, n_coarse=100, **{k: P for k in (
        "pts_sorted nodes verts weights coarse_rows parents wit_queue d2_scratch memb face_bits flag_list flag_count "
        "simplex_weight wit_item_list plane_scratch").split()}),
    CELL: dict(SWEEP, alpha=1.35, **{k: P for k in (
        "pts_sorted nodes verts weights cell_queue d2_scratch memb face_bits flag_list flag_count plane_scratch").split()}),
    FINISH: dict(SWEEP, **{k: P for k in (
        "pts_sorted nodes verts weights flag_list flag_count finish_ctl top top_list d2_scratch memb face_bits").split()}),
    FACES: dict(SWEEP, dim=4, k1=5, **{k: P for k in "pts_sorted nodes verts weights sample_order queue memb face_bits".split()}),
    MINIMA: dict(SWEEP, dim=4, k1=5, n_faces=0, **{k: P for k in "pts_sorted nodes verts weights sample_order queue out_d2".split()}),
    FPS: dict(n_pts=1000, dim=3, ld=3, n_lms=64, start=0, **{k: P for k in (
        "pts pts_sorted order out_idx minsq bucket_box bucket_keys bucket_coord work_best work_rec work_ctr").split()}),
}
GOOD[SHARD] = dict(GOOD[MINIMA], shard_rank=1, shard_world=3)


def _cases():
    """(entry, what differs from GOOD[entry], recorded code, which forms: "both" / "block" / "positional")."""
    out = []

    def bad(entry, forms="both", **change):
        out.append((entry, change, E_ARG, forms))

    for entry, good in GOOD.items():
        for field, value in good.items():   # every required pointer, NULL
            if value == P:
                bad(entry, **{field: None})
        bad(entry, n_pts=0)
        if entry is FPS:
            continue
        # nothing to do: accepted before any pointer is looked at
        out.append((entry, {k: (None if v == P else 0) for k, v in good.items()} | {"n_simplices": 0},
                    OK, "both"))
        out.append((entry, {k: None for k, v in good.items() if v == P} | {"R": 0}, OK, "both"))
        for k1 in (0, 10):
            bad(entry, k1=k1)
    for entry in (WITNESS, CELL, FINISH, FACES):
        for n_faces in (0, 33):
            bad(entry, n_faces=n_faces)
    for entry in (WITNESS, CELL):
        for dim in (1, 4):
            bad(entry, dim=dim)
        bad(entry, top=P)                          # top without its list and count
        bad(entry, top=P, top_list=P)
        bad(entry, n_simplices=1 << 31)
        bad(entry, n_simplices=(1 << 31) - 1, R=8192)   # more than 2^31 - 1 (simplex, tile) pairs
        bad(entry, n_pts=BIG)                      # rows beyond a 32-bit byte offset
    # the witness sweep's own
    bad(WITNESS, R=8193)                           # FLOODER_WIT_MAX_ROWS
    for n_coarse in (0, 257):
        bad(WITNESS, n_coarse=n_coarse)
    bad(WITNESS, flag_key=P)                       # bounds without their histogram
    for run_len, n_runs, k1 in ((6, 4, 4), (4, 4, 4), (2048, 1, 4), (64, 17, 4), (64, 4, 5)):   # a bad run table
        bad(WITNESS, "block", wit_runs=P, wit_run_len=run_len, wit_n_runs=n_runs, k1=k1)
    # the cell sweep's own
    for alpha in (0.0, -1.0, float("nan")):
        bad(CELL, alpha=alpha)
    bad(CELL, defer_list=P)                        # deferred chunks without their cell sizes / control words
    bad(CELL, defer_list=P, defer_c=P)
    bad(CELL, simplex_weight=P)                    # weights without the lists they split into
    bad(CELL, simplex_weight=P, defer_list=P, defer_c=P, defer_ctl=P, light_list=P)
    bad(CELL, flag_key=P, flag_hist=P)             # bounds without the probe that computes them
    bad(CELL, flag_key=P, top=P, top_list=P, top_count=P)
    # the finish's own
    bad(FINISH, R=-1)
    bad(FINISH, hard_cap=-1)
    for dim in (0, 1, 4, 8, 9):
        bad(FINISH, dim=dim)
    # the sorted sweeps' own
    for entry in (FACES, MINIMA, SHARD):
        bad(entry, R=-1)
        bad(entry, n_simplices=1 << 22, R=1024)    # 2^32 samples
        for dim in (0, 9):
            bad(entry, dim=dim)
    bad(SHARD, shard_rank=3)                       # shard_rank >= shard_world
    bad(SHARD, shard_rank=-1)
    bad(SHARD, "positional", shard_world=0, shard_rank=0)   # (the block reads shard_world 0 as "all tiles")
    # the landmark selection's own
    bad(FPS, n_lms=0)
    bad(FPS, n_lms=1001)
    bad(FPS, start=-1)
    bad(FPS, start=1000)
    bad(FPS, ld=2)
    for dim in (0, 9):
        bad(FPS, dim=dim, ld=9)
    bad(FPS, n_pts=0xffffffff, ld=3)
    return out


def test_block_and_positional_form_refuse_alike():
    import ctypes

    lib = _native.load()
    cases = _cases()
    assert {c[0] for c in cases} == set(GOOD) and len(cases) > 150 and sum(1 for c in cases if c[2] == OK) == 12
    wrong = []
    for entry, change, code, forms in cases:
        block_fn, positional_fn, block_cls, order = entry
        blk = block_cls(**{**GOOD[entry], **change})
        if forms != "positional":
            rc = getattr(lib, block_fn)(ctypes.byref(blk), None)
            if rc != code:
                wrong.append((block_fn, change, rc, code, lib.flooder_last_error()))
        if forms != "block":
            rc = getattr(lib, positional_fn)(*[getattr(blk, name) for name in order.split()], None)
            if rc != code:
                wrong.append((positional_fn, change, rc, code, lib.flooder_last_error()))
    assert not wrong, wrong
