"""Cost of the weighted (power-distance) tree sweep (``csrc/flood_power.hip``) on one MI355X next to its comparators of
the same run.

Per workload the top-dimensional simplices of the complex are swept against the cloud's index by
``core._sweep_dimension_power`` with DTM weights (``distance_to_measure(points, neighbors=64)``) and with zero weights,
and by ``core._sweep_dimension_bvh`` (the unchanged k = 1 tree sweep, ``method="bvh"``); what is timed is the ``sweep``
span of each (device events on the launch stream, after a warm-up call, median of ``--reps`` calls, the calls of the
three alternating so that all see the same clocks).  The counters come from one extra call with a ``stats`` buffer.

Then the end-to-end recipe at k = 64 and k = 1024 - ``w = distance_to_measure(points, neighbors=k)`` and
``flood_complex(points, n_lms, point_weights=w)``, each between device events - next to
``flood_complex(points, n_lms, neighbor_mass=k / N)``, median of ``--reps`` calls after a warm-up call; a call whose
warm-up takes longer than five seconds is timed once (``reps`` in the line says so).

usage: python tools/time_power.py [cfg2,cfg4] [--reps N] [--ks 64,1024] [--out profiles/power_sweep_times.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from flooder_amd import core  # noqa: E402

from time_knn import alternating_ms, counters  # noqa: E402


def event_ms(fn, reps):
    """Median, min, max of the device time of ``fn()`` between two events over ``reps`` calls after one warm-up call;
    a warm-up above five seconds is followed by one timed call only."""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    first = once()
    times = sorted(once() for _ in range(1 if first > 5000.0 else reps))
    return times[len(times) // 2], times[0], times[-1], len(times)


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2,cfg4").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    ks = [int(k) for k in (argv[argv.index("--ks") + 1] if "--ks" in argv else "64,1024").split(",") if k]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "power_sweep_times.jsonl")
    dev = torch.device("cuda:0")
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:      # (rewritten line by line: a run that is cut short keeps what it measured)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")

    for name in names:
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev)
        n = int(tp.shape[0])
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
        head = {"workload": name, "points": n, "dim": w["dim"], "landmarks": int(lms.shape[0]), "simplices": S,
                "samples_per_simplex": R}

        # ---- the sweep span: DTM weights, zero weights, the k = 1 tree sweep
        dtm = fa.distance_to_measure(tp, neighbors=64, index=index)
        tables = {"dtm weights (k=64)": core._power_weights(index, dtm),
                  "zero weights": core._power_weights(index, torch.zeros_like(dtm))}

        def power(which):
            w_sorted, node_w = tables[which]
            return lambda timer, stats: core._sweep_dimension_power(index, verts, weights, faces, w_sorted, node_w, None,
                                                                    plan=plan, timer=timer, stats=stats)

        bvh = lambda timer, stats: core._sweep_dimension_bvh(index, verts, weights, faces, None, plan=plan,  # noqa: E731
                                                             stats=stats, timer=timer)
        sorted_tiles = core.knn_sorts_samples(w["dim"], S, R)
        fns = [("bvh k=1", bvh)] + [(f"power, {which}", power(which)) for which in tables]
        timed = alternating_ms([fn for _, fn in fns], reps)
        base = timed[0][0]
        for (label, fn), (ms, lo, hi, n_rep) in zip(fns, timed):
            line = {**head, "sweep": label, "sweep_ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                    "reps": n_rep, "ratio_to_bvh_k1": round(ms / base, 2)}
            if label.startswith("power"):   # tiles: 64 entries of the sorted order, or 64 rows of one simplex
                line.update(form="sorted tiles (span includes sample keys + radix sort)" if sorted_tiles
                            else "identity order, a simplex's rows per tile",
                            **counters(fn, -(-S * R // 64) if sorted_tiles else S * -(-R // 64)))
            emit(line)

        # ---- end to end: the recipe next to neighbor_mass
        for k in ks:
            if k > n:
                continue
            box_w = {}

            def weights_call():
                box_w["w"] = fa.distance_to_measure(tp, neighbors=k)

            for label, fn in ((f"distance_to_measure k={k}", weights_call),
                              (f"flood_complex point_weights (weights of k={k})",
                               lambda: fa.flood_complex(tp, w["n_lms"], points_per_edge=w["ppe"], max_dimension=w.get("max_dim"),
                                                        point_weights=box_w["w"])),
                              (f"flood_complex neighbor_mass k={k} dtm",
                               lambda: fa.flood_complex(tp, w["n_lms"], points_per_edge=w["ppe"], max_dimension=w.get("max_dim"),
                                                        neighbor_mass=k / n, neighbor_stat="dtm"))):
                ms, lo, hi, n_rep = event_ms(fn, reps)
                emit({**head, "call": label, "ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "reps": n_rep})
        ms, lo, hi, n_rep = event_ms(lambda: fa.flood_complex(tp, w["n_lms"], points_per_edge=w["ppe"],
                                                              max_dimension=w.get("max_dim")), reps)
        emit({**head, "call": "flood_complex plain", "ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
              "reps": n_rep})
        del tp, lms, index, verts, tables, dtm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
