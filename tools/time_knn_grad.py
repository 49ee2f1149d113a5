"""Cost of the differentiable robust filtration on one MI355X: ``flood_filtration(neighbors=k)`` next to
``flood_complex(neighbors=k)`` (returning its tree), the ``flooder_witness_knn`` launches of a forward on their own,
and the backward of a linear functional of all values.

Device events on the launch stream, one warm-up call, median of ``--reps`` calls (min and max are kept).  The witness
launches are timed by wrapping the entry point of the loaded library for the duration of one forward.

usage: python tools/time_knn_grad.py [cfg2] [--reps N] [--out profiles/knn_grad_times.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from flooder_amd import _native  # noqa: E402


def timed(fn, reps):
    """(median, min, max) ms of ``fn()`` by device events after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def witness_launches_ms(forward, reps):
    """(median ms of the sum over the launches of one forward, launches, queries) of ``flooder_witness_knn``."""
    lib = _native.load()
    real = lib.flooder_witness_knn
    spans, queries = [], []

    def wrapped(blk, stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = real(blk, stream)
        b.record()
        spans.append((a, b))
        queries.append(int(blk._obj.n_queries))
        return rc

    totals = []
    lib.flooder_witness_knn = wrapped
    try:
        for i in range(reps + 1):
            del spans[:], queries[:]
            forward()
            torch.cuda.synchronize()
            if i:
                totals.append(sum(a.elapsed_time(b) for a, b in spans))
    finally:
        lib.flooder_witness_knn = real
    totals.sort()
    return totals[len(totals) // 2], len(spans), sum(queries)


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_grad_times.jsonl")
    dev = torch.device("cuda:0")
    lines = []
    for name in names:
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev).requires_grad_(True)
        lms, index = fa.generate_landmarks(tp.detach(), w["n_lms"], start_idx=0, return_index=True)
        kw = dict(points_per_edge=w["ppe"], index=index)
        if w.get("max_dim"):
            kw["max_dimension"] = w["max_dim"]
        head = {"workload": name, "points": int(tp.shape[0]), "dim": w["dim"], "landmarks": int(lms.shape[0])}
        for k in (2, 8, 32):
            for stat in ("kth", "dtm"):
                kn = dict(neighbors=k, neighbor_stat=stat)
                comp = timed(lambda: fa.flood_complex(tp.detach(), lms, return_simplex_tree=True, **kw, **kn), reps)
                forward = lambda: fa.flood_filtration(tp, lms, **kw, **kn)  # noqa: E731
                fwd = timed(forward, reps)
                wit, launches, queries = witness_launches_ms(forward, reps)
                F = forward()
                coef = [torch.linspace(0.5, 1.5, v.shape[0], device=dev) for v in F.values]
                loss = sum((c * v).sum() for c, v in zip(coef, F.values))
                bwd = timed(lambda: torch.autograd.grad(loss, tp, retain_graph=True), reps)
                lines.append({**head, "neighbors": k, "neighbor_stat": stat, "reps": reps,
                              "flood_complex_ms": round(comp[0], 3), "flood_complex_min_max": [round(comp[1], 3), round(comp[2], 3)],
                              "forward_ms": round(fwd[0], 3), "forward_min_max": [round(fwd[1], 3), round(fwd[2], 3)],
                              "forward_ratio": round(fwd[0] / comp[0], 2),
                              "witness_knn_ms": round(wit, 3), "witness_knn_launches": launches, "witness_knn_queries": queries,
                              "backward_ms": round(bwd[0], 3), "backward_min_max": [round(bwd[1], 3), round(bwd[2], 3)],
                              "simplices": int(sum(v.shape[0] for v in F.values))})
                print(json.dumps(lines[-1]), flush=True)
        del tp, lms, index
        torch.cuda.empty_cache()
    if lines:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
