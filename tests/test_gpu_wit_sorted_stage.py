"""Ordered stage of the witness sweep (csrc/flood_wit.hip: the stage filled by excess bin, the pair loops of phases 3 and
5 left at the first bin no sample of the wave needs) on the GPU: option "wit_sorted_stage" 1 / 0 and the witness sweep
off give the same face values bit for bit, and with the option on fewer pairs are evaluated for the same simplices.

Every case is ONE child process under a time limit of its own (this file run as a script); after a case that ended
abnormally (signal, time limit) no further case is started.  Runs on a real MI355X only (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_TIMEOUT_S = 300
ST_HANDLED, ST_PAIRS = 16 + 0, 16 + 10   # words of the sweep statistics (include/flooder_hip.h, flooder_sweep_witness_f32)
CASES = ["gauss3d", "gauss2d", "doubled", "lattice", "tiny", "random_weights"]
_ended_abnormally = []

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- child process
def _child(case):
    import torch

    import flooder_amd as fa
    from flooder_amd import _native, core

    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    lib = _native.load()
    dev = torch.device("cuda:0")
    core.WIT_MIN_SIMPLICES = 0                   # (as tests/test_gpu_witness.py: the sweep is wanted on short queues,
    core.WIT_MAX_POINTS_PER_SIMPLEX = 1 << 40    # on clouds with many points per simplex
    assert lib.flooder_set_option(b"wit_surface_pct", 0) == 0   # and on clouds that lie on a surface)

    def values(pts, lms, witness, ordered, seed=None, **kw):
        core.CELL_WITNESS = witness
        assert lib.flooder_set_option(b"wit_sorted_stage", 1 if ordered else 0) == 0
        if seed is not None:
            torch.manual_seed(seed)
        out = fa.flood_complex(pts, lms, method="cell", **kw)
        keys = sorted(out)
        return keys, np.array([out[k] for k in keys], dtype=np.float32)

    def same(a, b):
        return a[0] == b[0] and bool((a[1].view(np.uint32) == b[1].view(np.uint32)).all())

    def counters(pts, lms, ppe, ordered):
        """the sweep's counters for the top simplices: (simplices handled, pairs evaluated)"""
        core.CELL_WITNESS = True
        assert lib.flooder_set_option(b"wit_sorted_stage", 1 if ordered else 0) == 0
        d = pts.shape[1]
        _, simplices = core._build_complex(lms, d)
        verts = lms[torch.as_tensor(simplices[d], device=dev)].contiguous()
        weights, _, face_idxs = core.generate_grid(ppe, d, dev, torch.float32)
        faces = core._FaceTable(face_idxs, weights.shape[0], dev)
        st = torch.zeros(40, dtype=torch.int64, device=dev)
        core._sweep_dimension_cell(core.PointIndex(pts), verts, weights, faces, None, stats=st)
        torch.cuda.synchronize()
        st = st.cpu().numpy()
        return int(st[ST_HANDLED]), int(st[ST_PAIRS])

    g = torch.Generator().manual_seed(7)
    seed, kw, ppe = None, {}, 30
    if case in ("gauss3d", "doubled", "random_weights"):
        pts = torch.randn(100_000, 3, generator=g).to(dev)
        lms = fa.generate_landmarks(pts, 200, start_idx=0)
        if case == "doubled":          # every point stored twice: exact distance ties, two candidates for every witness
            pts = torch.cat([pts, pts]).contiguous()
        if case == "random_weights":
            seed, kw = 0, dict(num_rand=3000, max_dimension=3)
    elif case == "gauss2d":
        pts = torch.randn(150_000, 2, generator=torch.Generator().manual_seed(21)).to(dev)
        lms, ppe = fa.generate_landmarks(pts, 2500, start_idx=0), 40
        kw = dict(points_per_edge=ppe)
    elif case == "lattice":
        # integer cloud, landmarks among its points, dyadic weights (i / 16): samples and differences are exact, many
        # points at exactly the same distance from a sample and at exactly the same excess
        ax = torch.arange(48, dtype=torch.float32)
        pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
        pts = pts[torch.randperm(pts.shape[0], generator=g)].contiguous().to(dev)
        lms, ppe = fa.generate_landmarks(pts, 150, start_idx=0), 17
        kw = dict(points_per_edge=ppe)
    elif case == "tiny":
        # a handful of points around every simplex: stages of fewer than four points and of no multiple of four, empty
        # bins in the middle of the stage
        pts = torch.randn(2_000, 3, generator=g).to(dev)
        lms = fa.generate_landmarks(pts, 40, start_idx=0)
    else:
        raise ValueError(case)
    on = values(pts, lms, True, True, seed, **kw)
    off = values(pts, lms, True, False, seed, **kw)
    none = values(pts, lms, False, True, seed, **kw)
    res = {"case": case, "values": int(on[1].size), "on_equals_off": same(on, off), "on_equals_no_witness_sweep": same(on, none)}
    if case != "random_weights":
        res["counters_on"] = counters(pts, lms, ppe, True)
        res["counters_off"] = counters(pts, lms, ppe, False)
    return res


# ---------------------------------------------------------------------------------------------- the tests
def _run_case(case, tmp_path):
    if _ended_abnormally:
        pytest.fail(f"case {_ended_abnormally[0]} ended abnormally: nothing more is started on the GPU")
    out = tmp_path / f"{case}.json"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    try:
        flags = ["-s"] if sys.flags.no_user_site else []
        p = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), case, str(out)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _ended_abnormally.append(case)
        pytest.fail(f"case {case}: no result within {CASE_TIMEOUT_S} s")
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _ended_abnormally.append(case)
    assert p.returncode == 0, f"case {case}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    res = json.loads(out.read_text())
    print(json.dumps(res))
    return res


@pytest.mark.parametrize("case", CASES)
def test_ordered_stage_changes_no_face_value(case, tmp_path):
    res = _run_case(case, tmp_path)
    assert res["values"] > 0, res
    assert res["on_equals_off"], f"{case}: face values differ between wit_sorted_stage 1 and 0"
    assert res["on_equals_no_witness_sweep"], f"{case}: face values differ from those without the witness sweep"
    if case == "gauss3d":
        (handled_on, pairs_on), (handled_off, pairs_off) = res["counters_on"], res["counters_off"]
        assert handled_on > 0 and handled_on == handled_off, res
        assert pairs_on < pairs_off, res


if __name__ == "__main__":
    result = _child(sys.argv[1])
    with open(sys.argv[2], "w") as fh:
        json.dump(result, fh)
