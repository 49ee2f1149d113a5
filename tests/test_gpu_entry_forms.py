"""The launches that have a parameter block give the same words through the block entry and through the positional
function of the same launch (include/flooder_hip.h, "parameter blocks": inside the library both are one function on the
block).  Fused 2-D / 3-D sweep (witness, cell, finish), sorted sweep above 3-D (minima whole and in shards, face maxima),
batched landmark selection: fresh buffers of the same layout for each form, equal words required.
Runs on a real MI355X only (-m gpu)."""
import ctypes

import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from helpers import get_options, set_options

pytestmark = pytest.mark.gpu

N_POINTS = 20_000             # three levels of the box tree (16 * 64 < 20 000 <= 16 * 64 * 64)
INF_BITS = 0x7F800000
ptr = _native.ptr


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    _native.load()
    return torch.device("cuda:0")


def top_simplices(pts, n_landmarks, dim):
    lms = fa.generate_landmarks(pts, n_landmarks, start_idx=0)
    return lms[torch.as_tensor(core._build_complex(lms, dim)[1][dim], device=pts.device)].contiguous().float()


def lattice(ppe, dim, dev):
    weights, _, face_idxs = core.generate_grid(ppe, dim, dev, torch.float32)
    faces = core._FaceTable(face_idxs, weights.shape[0], dev)
    return weights, faces, core.SamplePlan(weights, faces)


def fused_chain(index, verts, plan, F, positional):
    """prepare -> witness -> cell -> finish -> face values, on the buffers of a core.FusedWorkspace.
    Returns (face value bits (S, F), simplices the witness sweep handled, flagged tiles the finish was given)."""
    lib, dev = _native.load(), verts.device
    st = _native.current_stream_ptr(dev)
    S, k1, _ = verts.shape
    R = plan.w_perm.shape[0]
    ws = core.FusedWorkspace(S, R, F, None, dev, wit=True, owner=False)
    ws.arena.fill_(7)   # (the prepare launch clears it)
    flags, split, d2 = ws.flags, ws.split, ws.d2
    stats = torch.zeros(40, dtype=torch.int64, device=dev)
    coarse_rows, parents, n_coarse = plan.wit
    _native.check(lib.flooder_simplex_prepare_f32(ptr(index.nodes), index.n, index.dim, ptr(verts), k1, S, ptr(ws.wgt),
                                                  ptr(ws.planes), ptr(ws.arena), ws.n_words, st), "flooder_simplex_prepare_f32")
    if positional:
        p, n, dim = ptr(index.pts), index.n, index.dim
        _native.check(lib.flooder_sweep_witness_f32(
            p, n, dim, ptr(index.nodes), ptr(verts), ptr(plan.w_perm), k1, R, S, ptr(coarse_rows), n_coarse, ptr(parents),
            ptr(ws.wit_queue), ptr(d2), ptr(plan.memb_all), F, ptr(ws.face_bits), None, ptr(flags[0]),
            ptr(ws.flag_count), ptr(flags[1]), ptr(ws.flag_hist), ptr(ws.top), ptr(ws.top_list),
            ptr(ws.top_count), ptr(ws.wgt), ptr(split[0]), ptr(ws.planes), stats[16:].data_ptr(), st),
            "flooder_sweep_witness_f32")
        _native.check(lib.flooder_sweep_cell_faces_f32(
            p, n, dim, ptr(index.nodes), ptr(verts), ptr(plan.w_perm), k1, R, S, float(core.CELL_ALPHA), ptr(ws.cell_queue),
            ptr(d2), ptr(plan.memb_all), F, ptr(ws.face_bits), None, ptr(flags[0]), ptr(ws.flag_count),
            ptr(flags[1]), ptr(ws.flag_hist), ptr(ws.top), ptr(ws.top_list), ptr(ws.top_count), ptr(ws.defer_list),
            ptr(ws.defer_c), ptr(ws.defer_ctl), ptr(ws.wgt), ptr(split[0]), ptr(split[1]), ptr(ws.planes),
            ptr(index.dens), ptr(index.box), stats[0:].data_ptr(), st), "flooder_sweep_cell_faces_f32")
        _native.check(lib.flooder_finish_faces_f32(
            p, n, dim, ptr(index.nodes), ptr(verts), ptr(plan.w_perm), k1, R, S, ptr(flags[0]), ptr(ws.flag_count),
            ptr(flags[1]), ptr(ws.flag_hist), ptr(flags[2]), ptr(ws.finish_ctl), ptr(ws.top), ptr(ws.top_list), 1,
            ptr(d2), ptr(plan.memb_all), F, ptr(ws.face_bits), None, ptr(ws.hard), core.FINISH_HARD_CAP,
            stats[9:].data_ptr(), st), "flooder_finish_faces_f32")
    else:
        blk = _native.FusedSweep(
            pts_sorted=index.pts, n_pts=index.n, dim=index.dim, k1=k1, nodes=index.nodes, density_grid=index.dens,
            cloud_box=index.box, verts=verts, weights=plan.w_perm, R=R, n_faces=F, n_simplices=S, memb=plan.memb_all,
            alpha=float(core.CELL_ALPHA), cell_stats=stats[0:].data_ptr(), probed=1, finish_stats=stats[9:].data_ptr(),
            n_coarse=n_coarse, coarse_rows=coarse_rows, parents=parents, wit_stats=stats[16:].data_ptr(), planes_ready=1,
            **ws.block_fields())
        if plan.wit_runs is not None:
            blk.wit_runs, blk.wit_run_len, blk.wit_n_runs = plan.wit_runs[0].data_ptr(), plan.wit_runs[1], plan.wit_runs[2]
        _native.check(lib.flooder_fused_witness(ctypes.byref(blk), st), "flooder_fused_witness")
        _native.check(lib.flooder_fused_cell(ctypes.byref(blk), st), "flooder_fused_cell")
        _native.check(lib.flooder_fused_finish(ctypes.byref(blk), st), "flooder_fused_finish")
    out = torch.empty((S, F), dtype=torch.float32, device=dev)
    _native.check(lib.flooder_face_values_f32(ptr(ws.face_bits), S * F, ptr(out), st), "flooder_face_values_f32")
    torch.cuda.synchronize()
    return out.view(torch.int32).cpu(), int(stats[16].item()), int(ws.flag_count[0].item())


@pytest.mark.parametrize("dim,ppe", [(2, 32), (3, 14)])   # 528 / 560 rows: the first lattices of core.WIT_MIN_ROWS rows
def test_fused_sweep_gives_the_same_words_through_both_forms(dim, ppe, dev):
    pts = torch.randn(N_POINTS, dim, generator=torch.Generator().manual_seed(3 + dim)).to(dev)
    index = core.PointIndex(pts)
    verts = top_simplices(pts, 300, dim)
    weights, faces, plan = lattice(ppe, dim, dev)
    assert core.WIT_MIN_ROWS <= weights.shape[0] <= core.WIT_MAX_ROWS and plan.wit is not None and plan.memb_all is not None
    by_block, handled_b, flagged_b = fused_chain(index, verts, plan, faces.n_faces, positional=False)
    by_position, handled_p, flagged_p = fused_chain(index, verts, plan, faces.n_faces, positional=True)
    for what, handled, flagged in (("block", handled_b, flagged_b), ("positional", handled_p, flagged_p)):
        assert handled > 0, f"{what}: the witness sweep handled no simplex"
        assert flagged > 0, f"{what}: the finish was given no tile"
    assert torch.equal(by_block, by_position), f"dim {dim}: block and positional entries differ"
    tree, _ = core._sweep_dimension_bvh(index, verts, weights, faces, None, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(by_block, tree.view(torch.int32).cpu()), f"dim {dim}: the fused path differs from the tree sweep"


def test_sorted_sweep_gives_the_same_words_through_both_forms(dev):
    lib, dim = _native.load(), 4
    st = _native.current_stream_ptr(dev)
    pts = torch.randn(N_POINTS, dim, generator=torch.Generator().manual_seed(41)).to(dev)
    index = core.PointIndex(pts)
    verts = top_simplices(pts, 60, dim)
    weights, faces, plan = lattice(5, dim, dev)
    S, k1, _ = verts.shape
    R, F, n_s = weights.shape[0], faces.n_faces, verts.shape[0] * weights.shape[0]
    assert n_s > 4 * 256 and plan.late_rows is not None, "more than one workgroup of tiles"
    common = (ptr(index.pts), index.n, dim, ptr(index.nodes), ptr(verts), ptr(plan.w_perm), k1, R, S)
    block = dict(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=k1, nodes=index.nodes, verts=verts, weights=plan.w_perm,
                 R=R, n_simplices=S)
    tmp_bytes = int(lib.flooder_index_sort_bytes(n_s))
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
    keys, keys_sorted = (torch.empty(n_s, dtype=torch.int32, device=dev) for _ in range(2))

    def sample_order(late):
        order = torch.empty(n_s, dtype=torch.int32, device=dev)
        if late:
            _native.check(lib.flooder_sample_keys_late_f32(ptr(verts), ptr(plan.w_perm), k1, R, S, dim, ptr(index.box),
                                                           ptr(plan.late_rows), ptr(keys), st), "flooder_sample_keys_late_f32")
        else:
            _native.check(lib.flooder_sample_keys_f32(ptr(verts), ptr(plan.w_perm), k1, R, S, dim, ptr(index.box), ptr(keys),
                                                      st), "flooder_sample_keys_f32")
        bits = 32 if late else int(lib.flooder_sample_key_bits(dim))
        _native.check(lib.flooder_index_sort(ptr(keys), n_s, bits, ptr(keys_sorted), ptr(order), ptr(tmp), tmp_bytes, st),
                      "flooder_index_sort")
        return order

    queue = lambda: torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=dev)   # noqa: E731
    fresh = lambda: torch.full((S, R), INF_BITS, dtype=torch.int32, device=dev)    # noqa: E731
    order = sample_order(late=False)

    def minima(positional, shard=None):
        d2, q = fresh(), queue()
        if positional and shard is None:
            rc = lib.flooder_sweep_bvh_sorted_f32(*common, ptr(order), ptr(q), ptr(d2), None, st)
        elif positional:
            rc = lib.flooder_sweep_bvh_sorted_shard_f32(*common, ptr(order), shard, 3, ptr(q), ptr(d2), None, st)
        else:
            blk = _native.SortedSweep(**block, sample_order=order, queue=q, out_d2=d2,
                                      shard_rank=shard or 0, shard_world=0 if shard is None else 3)
            rc = lib.flooder_sorted_minima(ctypes.byref(blk), st)
        _native.check(rc, "sorted minima")
        torch.cuda.synchronize()
        return d2

    whole = minima(positional=False)
    assert int(whole.max()) < INF_BITS, "a sample without a minimum"
    assert torch.equal(whole, minima(positional=True)), "minima: block and positional entries differ"
    combined = fresh()
    for rank in range(3):
        part = minima(positional=False, shard=rank)
        assert torch.equal(part, minima(positional=True, shard=rank)), f"shard {rank} of 3: the entries differ"
        assert 0 < int((part != INF_BITS).sum()) < n_s, f"shard {rank} of 3 is not a proper part"
        combined = torch.minimum(combined, part)
    assert torch.equal(combined, whole), "the three shards do not add up to the whole sweep"

    order = sample_order(late=True)
    bits = []
    for positional in (False, True):
        face_bits, q = torch.zeros(S * F, dtype=torch.int32, device=dev), queue()
        if positional:
            rc = lib.flooder_sweep_bvh_sorted_faces_f32(*common, ptr(order), ptr(q), ptr(plan.memb_all), F, ptr(face_bits),
                                                        None, None, st)
        else:
            blk = _native.SortedSweep(**block, n_faces=F, sample_order=order, queue=q, memb=plan.memb_all, face_bits=face_bits)
            rc = lib.flooder_sorted_faces(ctypes.byref(blk), st)
        _native.check(rc, "sorted faces")
        torch.cuda.synchronize()
        bits.append(face_bits)
    assert int(bits[0].max()) > 0 and torch.equal(bits[0], bits[1]), "face maxima: block and positional entries differ"


def test_batched_landmark_selection_gives_the_same_indices_through_both_forms(dev):
    lib, dim, n_lms = _native.load(), 3, 64
    pts = torch.randn(N_POINTS, dim, generator=torch.Generator().manual_seed(5)).to(dev).contiguous()
    index = core.PointIndex(pts)
    n, dp, nb = N_POINTS, index.dp, int(lib.flooder_fps_bucket_count(N_POINTS))
    st = _native.current_stream_ptr(dev)

    def select(positional):
        out_idx = torch.empty(n_lms, dtype=torch.int64, device=dev)
        minsq = torch.empty(n, dtype=torch.float32, device=dev)
        box = torch.empty(2 * dp * nb, dtype=torch.float32, device=dev)
        keys = torch.empty(3 * nb, dtype=torch.int64, device=dev)
        bcoord = torch.empty(dp * nb, dtype=torch.float32, device=dev)
        rec = torch.empty(int(lib.flooder_fps_batched_rec_words(n, dim, n_lms)), dtype=torch.int32, device=dev)
        best = torch.zeros(64 * n_lms, dtype=torch.int64, device=dev)
        ctr = torch.zeros(n_lms + 4, dtype=torch.int32, device=dev)
        launches = ctypes.c_int32(0)
        if positional:
            rc = lib.flooder_fps_batched_f32(ptr(pts), n, dim, dim, ptr(index.pts), ptr(index.order32), n_lms, 0, ptr(out_idx),
                                             ptr(minsq), ptr(box), ptr(keys), ptr(bcoord), ptr(best), ptr(rec), ptr(ctr),
                                             ctypes.addressof(launches), st)
        else:
            blk = _native.FpsBatched(pts=pts, n_pts=n, dim=dim, ld=dim, pts_sorted=index.pts, order=index.order32, start=0,
                                     n_lms=n_lms, out_idx=out_idx, minsq=minsq, bucket_box=box, bucket_keys=keys,
                                     bucket_coord=bcoord, work_best=best, work_rec=rec, work_ctr=ctr,
                                     launches_out=ctypes.addressof(launches))
            rc = lib.flooder_fps_batched(ctypes.byref(blk), st)
        _native.check(rc, "batched selection")
        torch.cuda.synchronize()
        return out_idx.cpu(), int(launches.value)

    keep = get_options(lib, b"fps_switch")
    try:
        set_options(lib, {b"fps_switch": 8})   # (the batched launches from the 8th landmark on: 64 would all be single steps)
        by_block, launches_b = select(positional=False)
        by_position, launches_p = select(positional=True)
    finally:
        set_options(lib, keep)
    assert 7 < launches_b < n_lms - 1 and 7 < launches_p < n_lms - 1, "no launch selected more than one landmark"
    assert by_block[0] == 0 and len(set(by_block.tolist())) == n_lms
    assert torch.equal(by_block, by_position), "block and positional entries select different landmarks"
