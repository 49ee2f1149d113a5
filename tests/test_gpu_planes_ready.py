"""`planes_ready` of flooder_fused_sweep_t (include/flooder_hip.h): the caller, not a note inside the library, says whether
plane_scratch holds the face-plane rows of these simplices.  The chain the product runs - flooder_simplex_prepare_f32,
flooder_fused_witness, flooder_fused_cell, flooder_fused_finish, flooder_face_values_f32 - is called here entry by
entry, on the buffers of a core.FusedWorkspace.  Runs on a real MI355X only (-m gpu)."""
import ctypes

import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from helpers import get_options, set_options

pytestmark = pytest.mark.gpu

N_POINTS, N_LANDMARKS, POINTS_PER_EDGE = 20_000, 40, 10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    _native.load()
    return torch.device("cuda:0")


def fused_chain(index, verts, plan, n_faces, planes_ready, between=None, planes=None):
    """prepare on `verts` -> between(verts, planes) -> witness, cell, finish (all three with `planes_ready`; all valid
    inputs) -> face values.  `planes`: the caller's buffer for the 24 S plane words (tests/test_gpu_plane_rows.py puts
    guard words behind it).  Returns (face value bits (S, F) int32, the witness sweep's 24 counters, planes)."""
    lib, dev = _native.load(), verts.device
    st = _native.current_stream_ptr(dev)
    S, k1, _ = verts.shape
    R, F = plan.w_perm.shape[0], n_faces
    assert planes is None or (planes.numel() == 24 * S and planes.is_contiguous())
    ws = core.FusedWorkspace(S, R, F, None, dev, wit=True, owner=False, planes=planes)
    ws.arena.fill_(7)   # (the prepare launch clears it)
    planes = ws.planes
    stats = torch.zeros(40, dtype=torch.int64, device=dev)
    _native.check(lib.flooder_simplex_prepare_f32(_native.ptr(index.nodes), index.n, index.dim, _native.ptr(verts), k1, S,
                                                  _native.ptr(ws.wgt), _native.ptr(planes), _native.ptr(ws.arena), ws.n_words,
                                                  st), "flooder_simplex_prepare_f32")
    if between is not None:
        between(verts, planes)
    blk = _native.FusedSweep(
        pts_sorted=index.pts, n_pts=index.n, dim=index.dim, k1=k1, nodes=index.nodes, density_grid=index.dens,
        cloud_box=index.box, verts=verts, weights=plan.w_perm, R=R, n_faces=F, n_simplices=S, memb=plan.memb_all,
        alpha=float(core.CELL_ALPHA), cell_stats=stats[0:9], probed=1, finish_stats=stats[9:16], n_coarse=plan.wit[2],
        coarse_rows=plan.wit[0], parents=plan.wit[1], wit_stats=stats[16:40], planes_ready=planes_ready,
        **ws.block_fields())
    if plan.wit_runs is not None:
        blk.wit_runs, blk.wit_run_len, blk.wit_n_runs = plan.wit_runs[0].data_ptr(), plan.wit_runs[1], plan.wit_runs[2]
    _native.check(lib.flooder_fused_witness(ctypes.byref(blk), st), "flooder_fused_witness")
    _native.check(lib.flooder_fused_cell(ctypes.byref(blk), st), "flooder_fused_cell")
    _native.check(lib.flooder_fused_finish(ctypes.byref(blk), st), "flooder_fused_finish")
    out = torch.empty((S, F), dtype=torch.float32, device=dev)
    _native.check(lib.flooder_face_values_f32(_native.ptr(ws.face_bits), S * F, _native.ptr(out), st),
                  "flooder_face_values_f32")
    torch.cuda.synchronize()
    return out.view(torch.int32).cpu(), stats[16:40].cpu(), planes


@pytest.mark.parametrize("dim", [2, 3])
def test_plane_rows_are_handed_over_by_the_caller(dim, dev, monkeypatch):
    """Step 1: with planes_ready = 1 behind the prepare launch the two sweeps read its rows; with 0, and the rows
    overwritten with NaN, they write them themselves - same face values bit for bit.  Step 2: prepare on vertices A,
    the SAME verts tensor overwritten in place with vertices B (a second landmark set, same shape), then the sweeps
    with planes_ready = 0 - the values of a fresh run on B, not those of A's stale rows.

    (A lattice of 10 points per edge has fewer rows than core.WIT_MIN_ROWS, below which the product builds no witness
    plan: the switch is lowered here, like WIT_MIN_SIMPLICES, so that the witness sweep's entry runs in both steps.)"""
    lib = _native.load()
    monkeypatch.setattr(core, "WIT_MIN_SIMPLICES", 0)
    monkeypatch.setattr(core, "WIT_MIN_ROWS", 0)
    pts = torch.randn(N_POINTS, dim, generator=torch.Generator().manual_seed(11 + dim)).to(dev)
    index = core.PointIndex(pts)
    tops = []
    for start in (0, 777):   # landmark sets A and B: the same count from another start index
        lms = fa.generate_landmarks(pts, N_LANDMARKS, start_idx=start)
        tops.append(lms[torch.as_tensor(core._build_complex(lms, dim)[1][dim], device=dev)].contiguous().float())
    n = min(t.shape[0] for t in tops)   # (the two triangulations need not have the same number of top simplices)
    verts_a, verts_b = tops[0][:n].contiguous(), tops[1][:n].contiguous()
    assert n > 0 and not torch.equal(verts_a, verts_b)
    weights, _, face_idxs = core.generate_grid(POINTS_PER_EDGE, dim, dev, torch.float32)
    faces = core._FaceTable(face_idxs, weights.shape[0], dev)
    plan = core.SamplePlan(weights, faces)
    assert plan.memb_all is not None and plan.wit is not None, "no witness plan for this lattice"
    keep = get_options(lib, b"wit_surface_pct")
    try:
        assert lib.flooder_set_option(b"wit_surface_pct", 0) == 0
        nan_rows = lambda verts, planes: planes.fill_(float("nan"))   # noqa: E731
        ready, wit_1, _ = fused_chain(index, verts_a.clone(), plan, faces.n_faces, 1)
        launched, wit_0, _ = fused_chain(index, verts_a.clone(), plan, faces.n_faces, 0, between=nan_rows)
        rewritten, wit_2, _ = fused_chain(index, verts_a.clone(), plan, faces.n_faces, 0,
                                       between=lambda verts, planes: verts.copy_(verts_b))
        fresh, _, _ = fused_chain(index, verts_b.clone(), plan, faces.n_faces, 1)
    finally:
        set_options(lib, keep)
    for what, counters in (("planes_ready 1", wit_1), ("planes_ready 0", wit_0), ("rewritten verts", wit_2)):
        assert int(counters[:4].sum()) > 0, f"{what}: the witness sweep looked at no simplex"
    assert torch.equal(ready, launched), f"dim {dim}: planes_ready 1 / 0 differ"
    assert torch.equal(rewritten, fresh), f"dim {dim}: verts rewritten in place after the prepare launch: stale plane rows"
    assert not torch.equal(ready, fresh)   # (A and B are different complexes: the comparison above can fail)
