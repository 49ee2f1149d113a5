"""Cost of the differentiable weighted filtration on one MI355X next to its comparators of the same run.

Per workload (the cloud, the landmarks and the index of ``bench.py``; weights ``neighbor_distance(points,
neighbors=32, neighbor_stat="dtm")``, the README's recipe) the calls

    flood_complex, flood_complex(point_weights=w), flood_filtration, power_filtration      forward, no grad needed
    the backward of power_filtration w.r.t. points and weights (a fixed linear functional of all values)
    power_distance and power_nearest with every point of the cloud as a query

are timed between device events on the current stream.  One warm-up call each, then ``--reps`` rounds in which the
calls of a group follow one another, so that every comparator sees the same clocks; the median per call is reported
with its minimum and maximum.  The calls include their host work (Delaunay triangulation, the hand-off of the values).

usage: python tools/time_power_grad.py [cfg2,cfg4] [--reps N] [--out profiles/power_grad_times.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def rounds_ms(fns, reps):
    """{label: (median, min, max)} of ``reps`` rounds over the calls of ``fns`` after one warm-up call each."""
    for _, fn in fns:
        fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in fns}
    for _ in range(reps):
        for label, fn in fns:
            times[label].append(once_ms(fn))
    return {label: (sorted(t)[len(t) // 2], min(t), max(t)) for label, t in times.items()}


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2,cfg4").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "power_grad_times.jsonl")
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
        lms, index = fa.generate_landmarks(tp, w["n_lms"], start_idx=0, return_index=True)
        wt = fa.neighbor_distance(tp, neighbors=32, neighbor_stat="dtm", index=index)
        kw = dict(points_per_edge=w["ppe"], max_dimension=w.get("max_dim"), index=index)
        head = {"workload": name, "points": int(tp.shape[0]), "dim": w["dim"], "landmarks": int(lms.shape[0]),
                "points_per_edge": w["ppe"], "weights": "neighbor_distance k=32 dtm", "reps": reps}

        # ---- forward: the four producers of the same complex on the same inputs
        forward = [("flood_complex", lambda: fa.flood_complex(tp, lms, **kw)),
                   ("flood_complex point_weights", lambda: fa.flood_complex(tp, lms, point_weights=wt, **kw)),
                   ("flood_filtration", lambda: fa.flood_filtration(tp, lms, **kw)),
                   ("flood_filtration bvh", lambda: fa.flood_filtration(tp, lms, method="bvh", **kw)),
                   ("power_filtration", lambda: fa.power_filtration(tp, lms, wt, **kw))]
        got = rounds_ms(forward, reps)
        for label, (ms, lo, hi) in got.items():
            emit({**head, "call": label, "ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                  "ratio_to_flood_complex": round(ms / got["flood_complex"][0], 2),
                  "ratio_to_flood_complex_point_weights": round(ms / got["flood_complex point_weights"][0], 2)})

        # ---- backward: points and weights from one graph, kept for every round
        a, b = tp.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        F = fa.power_filtration(a, lms, b, **kw)
        loss = sum((torch.linspace(0.5, 1.5, v.shape[0], device=dev) * v).sum() for v in F.values)
        n_values = sum(int(v.shape[0]) for v in F.values)
        ms, lo, hi = rounds_ms([("backward", lambda: torch.autograd.grad(loss, (a, b), retain_graph=True))], reps)["backward"]
        emit({**head, "call": "power_filtration backward (points, weights)", "values": n_values, "ms": round(ms, 3),
              "min_ms": round(lo, 3), "max_ms": round(hi, 3)})
        del F, loss, a, b

        # ---- queries: every point of the cloud
        got = rounds_ms([("power_distance", lambda: fa.power_distance(tp, wt, index=index)),
                         ("power_nearest", lambda: fa.power_nearest(tp, wt, index=index))], reps)
        for label, (ms, lo, hi) in got.items():
            emit({**head, "call": f"{label}, every cloud point a query", "ms": round(ms, 3), "min_ms": round(lo, 3),
                  "max_ms": round(hi, 3), "ratio_to_power_distance": round(ms / got["power_distance"][0], 2)})
        del tp, lms, index, wt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
