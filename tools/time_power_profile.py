"""Cost of the mass profile (``distance_to_measure_profile``, ``flooder_sweep_power_profile_f32``, ``dtm_profile``) on
one MI355X next to the single calls it replaces, all in the same run.

Per workload, with the columns k = 64, 128, 256, 512, 1024 and ``"dtm"``:

1. ``distance_to_measure_profile(points, neighbors=ks)`` against the five ``distance_to_measure`` calls and against the
   one at the largest k (device events around whole calls, a warm-up call, median of ``--reps``, the three alternating);
2. the ``sweep`` span of ONE ``core._sweep_dimension_power_profile`` over the top-dimensional simplices against the sum
   of the five ``core._sweep_dimension_power`` spans (``time_knn.alternating_ms``), with the leaf-test and
   leaf-evaluation counters of both from one extra call each;
3. ``dtm_profile`` end to end against five times (``distance_to_measure`` + ``flood_complex(point_weights=...)``); a
   call whose warm-up takes longer than five seconds is timed once (``reps`` in the line says so).

usage: python tools/time_power_profile.py [cfg2,cfg4] [--reps N] [--ks 64,128,256,512,1024]
                                          [--out profiles/power_profile_times.jsonl] [--no-end-to-end]
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


def alternating_event_ms(fns, reps):
    """Median, min, max, reps of the device time of whole calls between two events, the calls of ``fns`` alternating
    after one warm-up call each; a warm-up above five seconds is followed by one timed round only."""
    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    first = [once(fn) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(1 if max(first) > 5000.0 else reps):
        for i, fn in enumerate(fns):
            times[i].append(once(fn))
    return [(sorted(t)[len(t) // 2], min(t), max(t), len(t)) for t in times]


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2,cfg4").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    ks = [int(k) for k in (argv[argv.index("--ks") + 1] if "--ks" in argv else "64,128,256,512,1024").split(",") if k]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "power_profile_times.jsonl")
    end_to_end = "--no-end-to-end" not in argv
    dev = torch.device("cuda:0")
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:      # (rewritten line by line: a run that is cut short keeps what it measured)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")

    def timed(head, what, labels, fns):
        out = alternating_event_ms(fns, reps)
        base = out[0][0]
        for label, (ms, lo, hi, n_rep) in zip(labels, out):
            emit({**head, "compare": what, "call": label, "ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                  "reps": n_rep, "ratio_to_profile": round(ms / base, 3)})

    for name in names:
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev)
        n = int(tp.shape[0])
        lms, index = fa.generate_landmarks(tp, w["n_lms"], start_idx=0, return_index=True)
        top = w.get("max_dim") or w["dim"]
        head = {"workload": name, "points": n, "dim": w["dim"], "landmarks": int(lms.shape[0]), "ks": ks}

        # ---- 1. the weights: one wide walk at the largest k against the five walks, and against the one at the largest k
        timed(head, "weights", ["distance_to_measure_profile", f"{len(ks)} x distance_to_measure",
                                f"distance_to_measure k={max(ks)}"],
              [lambda: fa.distance_to_measure_profile(tp, neighbors=ks, index=index),
               lambda: [fa.distance_to_measure(tp, neighbors=k, index=index) for k in ks],
               lambda: fa.distance_to_measure(tp, neighbors=max(ks), index=index)])

        # ---- 2. the sweep span over the top-dimensional simplices: one profile sweep against the single sweeps
        _, simplices = core._build_complex(lms, top)
        lm_np = lms.cpu().numpy()
        box = index.box.cpu()
        axis = int(torch.argmax(box[8:8 + w["dim"]] - box[:w["dim"]]).item())
        v_np = lm_np[simplices[top]]
        verts = torch.as_tensor(np.ascontiguousarray(v_np[np.argsort(v_np[:, :, axis].sum(axis=1), kind="stable")]), device=dev)
        weights, _, _, faces, plan, _ = core._grid_tables(w["ppe"], top, dev, torch.float32)
        S, R = int(verts.shape[0]), int(weights.shape[0])
        dtm = fa.distance_to_measure_profile(tp, neighbors=ks, index=index)            # (N, len(ks))
        groups = [(min(core.POWER_COLS_MAX, len(ks) - a), *core._power_weight_columns(index, dtm[:, a:a + core.POWER_COLS_MAX]))
                  for a in range(0, len(ks), core.POWER_COLS_MAX)]
        singles = [core._power_weights(index, dtm[:, c].contiguous()) for c in range(len(ks))]
        profile_fn = lambda timer, stats: core._sweep_dimension_power_profile(index, verts, weights, faces, groups,  # noqa: E731
                                                                              plan=plan, stats=stats, timer=timer)

        def single_fn(c):
            return lambda timer, stats: core._sweep_dimension_power(index, verts, weights, faces, *singles[c], None,
                                                                    plan=plan, timer=timer, stats=stats)

        fns = [profile_fn] + [single_fn(c) for c in range(len(ks))]
        out = alternating_ms(fns, reps)
        sorted_tiles = core.knn_sorts_samples(w["dim"], S, R)
        n_tiles = -(-S * R // 64) if sorted_tiles else S * -(-R // 64)
        sweep_head = {**head, "compare": "sweep span", "simplices": S, "samples_per_simplex": R,
                      "form": "sorted tiles (span includes sample keys + radix sort)" if sorted_tiles
                      else "identity order, a simplex's rows per tile"}
        single_sum = sum(o[0] for o in out[1:])
        emit({**sweep_head, "sweep": f"profile, {len(ks)} columns", "sweep_ms": round(out[0][0], 3),
              "min_ms": round(out[0][1], 3), "max_ms": round(out[0][2], 3), "reps": out[0][3],
              "ratio_to_sum_of_singles": round(out[0][0] / single_sum, 3), **counters(profile_fn, n_tiles)})
        total = {"leaf_evals": 0, "leaf_tests": 0, "node_tests": 0}
        for c, k in enumerate(ks):
            cnt = counters(single_fn(c), n_tiles)
            for key in total:
                total[key] += cnt[key]
            emit({**sweep_head, "sweep": f"single, weights of k={k}", "sweep_ms": round(out[1 + c][0], 3),
                  "min_ms": round(out[1 + c][1], 3), "max_ms": round(out[1 + c][2], 3), "reps": out[1 + c][3], **cnt})
        emit({**sweep_head, "sweep": f"sum of the {len(ks)} single sweeps", "sweep_ms": round(single_sum, 3), **total})
        del groups, singles, verts, dtm

        # ---- 3. end to end
        if end_to_end:
            kw = dict(points_per_edge=w["ppe"], max_dimension=w.get("max_dim"))
            timed(head, "end to end", ["dtm_profile", f"{len(ks)} x (distance_to_measure + flood_complex point_weights)"],
                  [lambda: fa.dtm_profile(tp, w["n_lms"], neighbors=ks, **kw),
                   lambda: [fa.flood_complex(tp, w["n_lms"], point_weights=fa.distance_to_measure(tp, neighbors=k), **kw)
                            for k in ks]])
        del tp, lms, index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
