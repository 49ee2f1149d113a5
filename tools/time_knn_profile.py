"""Cost of the neighbour profile (``flood_profile``, ``flooder_sweep_knn_profile_f32``) on one MI355X next to one
``flood_complex`` call per column.

Workload: cfg 2 of ``bench.py``, columns (1, 2, 4, 8, 16, 32) x ("kth", "dtm").  Three measurements, each the median of
``--reps`` runs after a warm-up:

* the ``sweep`` and ``face_max`` spans (device events on the launch stream) of ``core._sweep_dimension_knn_profile``
  over the top-dimensional simplices - one sweep at k = 32 and twelve face-max launches;
* the same spans of what the twelve single calls run for those simplices: ``core._sweep_dimension_knn`` for the ten
  columns with k > 1, and for the two k = 1 columns the pass ``flood_complex`` makes at k = 1 (the fused cell sweep:
  all its spans, summed under ``k1_pass``);
* the whole calls (host clock around the call and a device synchronisation): ``flood_profile`` against the sum of the
  twelve ``flood_complex`` calls, both returning simplex trees.

usage: python tools/time_knn_profile.py [cfg2] [--reps N] [--out profiles/knn_profile_times.jsonl]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from flooder_amd import core  # noqa: E402

KS = (1, 2, 4, 8, 16, 32)
STATS = ("kth", "dtm")


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def spans_ms(fn, reps):
    """{span: median ms} over ``reps`` calls of ``fn(timer)`` after one warm-up call."""
    def once():
        timer = core._KernelTimer()
        fn(timer)
        torch.cuda.synchronize()
        return timer.totals_ms()

    once()
    runs = [once() for _ in range(reps)]
    return {name: round(median([r[name] for r in runs]), 3) for name in runs[0]}


def wall_ms(fn, reps):
    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    once()
    return round(median([once() for _ in range(reps)]), 3)


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_profile_times.jsonl")
    dev = torch.device("cuda:0")
    columns = [(k, s) for k in KS for s in STATS]
    lines = []
    for name in names:
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev)
        lms, index = fa.generate_landmarks(tp, w["n_lms"], start_idx=0, return_index=True)
        top = w.get("max_dim") or w["dim"]
        _, simplices = core._build_complex(lms, top)
        lm_np = lms.cpu().numpy()
        box = index.box.cpu()
        axis = int(torch.argmax(box[8:8 + w["dim"]] - box[:w["dim"]]).item())
        v_np = lm_np[simplices[top]]
        verts = torch.as_tensor(np.ascontiguousarray(v_np[np.argsort(v_np[:, :, axis].sum(axis=1), kind="stable")]), device=dev)
        weights, _, _, faces, plan, _ = core._grid_tables(w["ppe"], top, dev, torch.float32)
        S, R = int(verts.shape[0]), int(weights.shape[0])
        head = {"workload": name, "points": int(tp.shape[0]), "dim": w["dim"], "landmarks": int(lms.shape[0]),
                "simplices": S, "samples_per_simplex": R, "columns": [list(c) for c in columns],
                "plane_buffer_bytes": 4 * len(columns) * S * R, "reps": reps}

        prof = spans_ms(lambda timer: core._sweep_dimension_knn_profile(index, verts, weights, faces, columns, plan=plan,
                                                                        timer=timer), reps)
        singles = {"sweep": 0.0, "face_max": 0.0, "k1_pass": 0.0}
        per_column = {}
        for k, stat in columns:
            if k == 1:    # what flood_complex runs at k = 1 in 2-D / 3-D: the fused cell sweep (all its spans)
                sweep_1 = core._sweep_dimension_cell if w["dim"] in (2, 3) else core._sweep_dimension_bvh
                got = spans_ms(lambda timer: sweep_1(index, verts, weights, faces, None, plan=plan, timer=timer), reps)
                singles["k1_pass"] += sum(got.values())
            else:
                got = spans_ms(lambda timer: core._sweep_dimension_knn(index, verts, weights, faces, k, stat, plan=plan,
                                                                       timer=timer), reps)
                singles["sweep"] += got["sweep"]
                singles["face_max"] += got["face_max"]
            per_column[f"{k} {stat}"] = got
        kw = dict(points_per_edge=w["ppe"], return_simplex_tree=True, index=index)
        call_profile = wall_ms(lambda: fa.flood_profile(tp, lms, top, neighbors=KS, neighbor_stat=STATS, **kw), reps)
        call_singles = sum(wall_ms(lambda: fa.flood_complex(tp, lms, top, neighbors=k, neighbor_stat=s, **kw), reps)
                           for k, s in columns)
        lines.append({**head, "profile_spans_ms": prof, "single_spans_sum_ms": {n: round(v, 3) for n, v in singles.items()},
                      "single_spans_ms": per_column, "profile_call_ms": call_profile,
                      "single_calls_sum_ms": round(call_singles, 3)})
        print(json.dumps(lines[-1]), flush=True)
        del tp, lms, index, verts
        torch.cuda.empty_cache()
    if lines:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
