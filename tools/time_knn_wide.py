"""Cost of the wide k-nearest kernel (``flooder_knn_wide_f32``: one wave per query, the k best in LDS) on one MI355X.

Per cloud - the 1 M-point 3-D Gaussian of cfg 2 and the 6-D Gaussian of cfg 4 - every point is a query, and for
k = 32, 64, 256, 1024 two things are timed by device events on the launch stream (one warm-up call, then ``--reps``
calls; median, min, max):

  values   ``distance_to_measure(points, None, neighbors=k, squared=True)``: sample keys, radix sort, the wide kernel
           writing the statistic word;
  ids      the same with ``return_neighbors=True``: ids and d2 words of all k neighbours as well.

Next to the k = 32 row, from the same run, the register family's sweeps over sorted tiles at k = 32 - the yardstick:
``neighbor_distance`` (``flooder_sweep_knn_sorted_f32``) and ``neighbors._knn_ids_hip``
(``flooder_knn_ids_sorted_f32``).  Then ``flood_complex(points, 1000, neighbor_mass=k / N)`` on the cfg 2 cloud for
k = 64 and 1024.  A call whose warm-up took more than ``SLOW_S`` seconds is timed once (``reps`` says so).

Every line is appended to the output as soon as it is measured.

usage: python tools/time_knn_wide.py [cfg2,cfg4] [--reps N] [--out profiles/knn_wide_times.jsonl] [--no-flood]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from flooder_amd import core, neighbors  # noqa: E402

KS = (32, 64, 256, 1024)
SLOW_S = 20.0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def timed(fn, reps):
    """(median, min, max, reps used) in ms after one warm-up call."""
    t0 = time.perf_counter()
    event_ms(fn)
    if time.perf_counter() - t0 > SLOW_S:
        reps = 1
    t = sorted(event_ms(fn)[0] for _ in range(reps))
    return t[len(t) // 2], t[0], t[-1], reps


def emit(out_path, line):
    print(json.dumps(line), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(line) + "\n")


def put(line, name, stats):
    med, lo, hi, reps = stats
    line.update({f"{name}_ms": round(med, 3), f"{name}_min_ms": round(lo, 3), f"{name}_max_ms": round(hi, 3),
                 f"{name}_reps": reps})


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2,cfg4").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_wide_times.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("time_knn_wide.py needs a GPU: a timing taken anywhere else says nothing")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    dev = torch.device("cuda:0")
    for name in names:
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev).to(torch.float32).contiguous()
        index = core.PointIndex(tp)
        n = int(tp.shape[0])
        head = {"workload": name, "points": n, "dim": int(tp.shape[1]), "queries": n}
        for k in KS:
            line = {**head, "what": "queries", "k": k}
            put(line, "wide_values", timed(lambda: fa.distance_to_measure(tp, None, neighbors=k, squared=True, index=index),
                                           reps))
            put(line, "wide_ids", timed(lambda: fa.distance_to_measure(tp, None, neighbors=k, squared=True, index=index,
                                                                       return_neighbors=True), reps))
            if k <= core.KNN_MAX:   # the yardstick: the register family on the same cloud in the same run
                put(line, "sorted_values", timed(lambda: fa.neighbor_distance(tp, None, k, "dtm", squared=True, index=index),
                                                 reps))
                put(line, "sorted_ids", timed(lambda: neighbors._knn_ids_hip(tp, tp, k, "dtm", index, want_d2=True,
                                                                             want_bits=True), reps))
                a = fa.distance_to_measure(tp, None, neighbors=k, squared=True, index=index)
                b = fa.neighbor_distance(tp, None, k, "dtm", squared=True, index=index)
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the wide kernel's words differ at k = 32"
            line["wide_values_us_per_query"] = round(1e3 * line["wide_values_ms"] / n, 4)
            emit(out_path, line)
        if name == "cfg2" and "--no-flood" not in argv:
            for k in (64, 1024):
                line = {**head, "what": "flood_complex(points, 1000, neighbor_mass=k / N)", "k": k}
                put(line, "flood", timed(lambda: fa.flood_complex(tp, 1000, neighbor_mass=k / n, neighbor_stat="dtm",
                                                                  index=index), reps))
                emit(out_path, line)
        del tp, index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
