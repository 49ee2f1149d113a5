"""Cost of the weighted-measure kernel (``flooder_knn_mass_f32``: one wave per query, the nearest sites up to a cumulative
mass) on one MI355X, against the plain wide k-nearest kernel in the same run.

The cloud is cfg 2's (1 M-point 3-D Gaussian); every cloud point is a query.  Per cell size of ``CELLS`` the coreset
``voxel_measure(points, cell)`` is built (timed), and per mass of ``MASSES`` - both are more than 1024 points, where
``distance_to_measure`` refuses - and list capacity of ``CAPACITIES``

  weighted   ``distance_to_weighted_measure(sites, mu, queries=points, mass=m, max_neighbors=C, squared=True)``: sample
             keys, radix sort, the kernel writing the statistic word (the index of the sites is built beforehand);

is timed by device events around the whole call (one warm-up call, then ``--reps`` calls; median, min, max), with the
median and the largest number of neighbours used and the share of queries not reached.  Comparators from the same run:
``distance_to_measure(points, None, neighbors=k, squared=True)`` at the k nearest the median count (1..1024) and at
k = 1024.  Every line is appended to the output as soon as it is measured.

usage: python tools/time_knn_mass.py [--reps N] [--out profiles/knn_mass_times.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from flooder_amd import core, neighbors  # noqa: E402

CELLS = (0.1, 0.2)
MASSES = (0.002, 0.005)
CAPACITIES = (256, 1024)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def timed(fn, reps):
    """(median, min, max, reps) in ms after one warm-up call."""
    event_ms(fn)
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
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_mass_times.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("time_knn_mass.py needs a GPU: a timing taken anywhere else says nothing")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    dev = torch.device("cuda:0")
    tp = bench.make_points(bench.WORKLOADS["cfg2"]).to(dev).to(torch.float32).contiguous()
    n = int(tp.shape[0])
    cloud_index = core.PointIndex(tp)
    head = {"workload": "cfg2", "points": n, "dim": int(tp.shape[1]), "queries": n}
    plain = {}                     # k -> timing of the plain wide kernel, measured once per k

    def plain_ms(k):
        if k not in plain:
            plain[k] = timed(lambda: fa.distance_to_measure(tp, None, neighbors=k, squared=True, index=cloud_index), reps)
        return plain[k]

    for cell in CELLS:
        line = {**head, "what": "voxel_measure", "cell": cell}
        put(line, "voxel_measure", timed(lambda: fa.voxel_measure(tp, cell), reps))
        sites, mu = fa.voxel_measure(tp, cell)
        line["sites"] = int(sites.shape[0])
        emit(out_path, line)
        index = core.PointIndex(sites)
        for mass in MASSES:
            k_points = core.mass_neighbors(mass, n)
            for cap in CAPACITIES:
                line = {**head, "what": "distance_to_weighted_measure", "cell": cell, "sites": int(sites.shape[0]),
                        "mass": mass, "k_points": k_points, "capacity": cap}
                put(line, "weighted", timed(lambda: fa.distance_to_weighted_measure(
                    sites, mu, queries=tp, mass=mass, max_neighbors=cap, squared=True, index=index), reps))
                # (the counts without the (Q, C) rows of return_neighbors=True: the driver's own outputs)
                _, _, count, bits = neighbors._weighted_sweep_hip(sites, mu, tp, neighbors._mass_target(mu, mass), cap,
                                                                  "dtm", index, False)
                reached = torch.isfinite(bits.view(torch.float32))
                used = count[reached] if bool(reached.any()) else count
                line.update(count_median=int(used.median()), count_max=int(used.max()),
                            not_reached_share=round(1.0 - float(reached.float().mean()), 6),
                            weighted_us_per_query=round(1e3 * line["weighted_ms"] / n, 4))
                del bits, count, reached, used
                k_near = max(1, min(core.KNN_WIDE_MAX, line["count_median"]))
                line["plain_k"] = k_near
                put(line, "plain_at_count", plain_ms(k_near))
                put(line, "plain_1024", plain_ms(core.KNN_WIDE_MAX))
                emit(out_path, line)
        del sites, mu, index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
