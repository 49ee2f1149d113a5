"""Run test of the witness sweep (csrc/flood_wit.hip, phase 4a) on the GPU: dropping whole runs of samples with one
bound changes no face value - option "wit_runs" 1 / 0 and the witness sweep off give the same bits on the clouds of
tests/test_gpu_witness.py -, it does drop runs on a Gaussian, and without the run table nothing is counted.

Every case is ONE child process under a time limit of its own (this file run as a script); after a case that ended
abnormally (signal, time limit) no further case is started.  Runs on a real MI355X only (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_TIMEOUT_S = 420
ST_RUNS = 16 + 21     # word of the sweep statistics: runs dropped (include/flooder_hip.h, flooder_sweep_witness_f32)
_ended_abnormally = []

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- child process
def _clouds(name, n):
    import torch
    from oracle import flood_oracle as fo

    g = torch.Generator().manual_seed(7)
    if name == "gauss":
        return torch.randn(n, 3, generator=g)
    if name == "torus":
        return torch.as_tensor(fo.noisy_torus(n, seed=3))
    if name == "plane":
        return torch.randn(n, 2, generator=torch.Generator().manual_seed(21))
    raise ValueError(name)


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

    def values(pts, lms, witness, runs, seed=None, **kw):
        core.CELL_WITNESS = witness
        assert lib.flooder_set_option(b"wit_runs", 1 if runs else 0) == 0
        if seed is not None:
            torch.manual_seed(seed)
        out = fa.flood_complex(pts, lms, method="cell", **kw)
        keys = sorted(out)
        return keys, np.array([out[k] for k in keys], dtype=np.float32)

    def same(a, b):
        return a[0] == b[0] and bool((a[1].view(np.uint32) == b[1].view(np.uint32)).all())

    def dropped(pts, lms, ppe, table, option):
        """the sweep's counters for the top simplices, with / without the run table in the parameter block"""
        core.CELL_WITNESS, core.WIT_RUNS = True, table
        assert lib.flooder_set_option(b"wit_runs", option) == 0
        d = pts.shape[1]
        _, simplices = core._build_complex(lms, d)
        verts = lms[torch.as_tensor(simplices[d], device=dev)].contiguous()
        weights, _, face_idxs = core.generate_grid(ppe, d, dev, torch.float32)
        faces = core._FaceTable(face_idxs, weights.shape[0], dev)
        st = torch.zeros(40, dtype=torch.int64, device=dev)
        core._sweep_dimension_cell(core.PointIndex(pts), verts, weights, faces, None, stats=st)
        torch.cuda.synchronize()
        core.WIT_RUNS = True
        st = st.cpu().numpy()
        return int(st[16]), int(st[ST_RUNS])

    res = {"case": case, "checks": {}}
    runs_of = []   # (label, points, landmarks, seed, keywords)
    if case in ("gauss", "torus"):
        n, n_l = (200_000, 400) if case == "gauss" else (150_000, 300)
        pts = _clouds(case, n).to(dev)
        runs_of.append((case, pts, fa.generate_landmarks(pts, n_l, start_idx=0), None, {}))
    elif case == "random_weights":
        pts = _clouds("gauss", 100_000).to(dev)
        lms = fa.generate_landmarks(pts, 200, start_idx=0)
        for seed in (0, 1):
            runs_of.append((f"random weights, seed {seed}", pts, lms, seed, dict(num_rand=3000, max_dimension=3)))
        g = torch.Generator().manual_seed(5)
        runs_of.append(("landmarks off the cloud", pts, (torch.randn(150, 3, generator=g) * 1.5).to(dev), None, {}))
    elif case == "plane":
        pts = _clouds("plane", 150_000).to(dev)
        runs_of.append((case, pts, fa.generate_landmarks(pts, 2500, start_idx=0), None, dict(points_per_edge=40)))
    else:
        raise ValueError(case)
    for label, pts, lms, seed, kw in runs_of:
        on = values(pts, lms, True, True, seed, **kw)
        off = values(pts, lms, True, False, seed, **kw)
        none = values(pts, lms, False, True, seed, **kw)
        res["checks"][label] = {"values": int(on[1].size), "runs_on_equals_runs_off": same(on, off),
                                "runs_on_equals_no_witness_sweep": same(on, none)}
    if case in ("gauss", "plane"):
        label, pts, lms, _, kw = runs_of[0]
        ppe = kw.get("points_per_edge", 30)
        res["counter"] = {"table_option_1": dropped(pts, lms, ppe, True, 1), "table_option_0": dropped(pts, lms, ppe, True, 0),
                          "no_table": dropped(pts, lms, ppe, False, 1)}
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


@pytest.mark.parametrize("case", ["gauss", "torus", "random_weights", "plane"])
def test_run_test_changes_no_face_value(case, tmp_path):
    res = _run_case(case, tmp_path)
    assert res["checks"], res
    for label, c in res["checks"].items():
        assert c["values"] > 0, (label, c)
        assert c["runs_on_equals_runs_off"], f"{label}: face values differ between wit_runs 1 and 0"
        assert c["runs_on_equals_no_witness_sweep"], f"{label}: face values differ from those without the witness sweep"
    if case in ("gauss", "plane"):
        handled, n_dropped = res["counter"]["table_option_1"]
        assert handled > 0, res["counter"]
        if case == "gauss":
            assert n_dropped > 0, "no run dropped on a Gaussian cloud"
        assert res["counter"]["table_option_0"][1] == 0, "runs counted with the option off"
        assert res["counter"]["no_table"][0] > 0 and res["counter"]["no_table"][1] == 0, \
            "runs counted without a run table in the parameter block"


if __name__ == "__main__":
    result = _child(sys.argv[1])
    with open(sys.argv[2], "w") as fh:
        json.dump(result, fh)
