"""Cost of the weighted-measure MASS PROFILE (``flooder_knn_mass_profile_f32``: one walk of the sites per query to the
largest target, one crossing scan per column) on one MI355X, against the single calls in the same run.

The cloud is cfg 2's (1 M-point 3-D Gaussian); every cloud point is a query; the coreset is ``voxel_measure(points,
0.2)``, the list capacity 1024, the masses ``MASSES`` (500 to 5000 points: all but the first above the 1024 neighbours
at which the plain measure stops), ``"dtm"``, squared values.  Timed by device events around whole calls (one warm-up
call, then ``--reps`` calls; median, min, max), every comparator in the same run:

  profile        ``distance_to_weighted_measure_profile(sites, mu, points, MASSES, ...)``;
  single         ``distance_to_weighted_measure(sites, mu, points, mass=m, ...)`` per mass, their sum, and the one at the
                 largest mass - the expectation to confirm or refute is "the profile costs about the single call at
                 the largest mass, below the sum of the singles";
  end to end     ``dtm_profile(points, landmarks, masses, cell_size=0.2)`` next to, per mass, ``voxel_measure`` + the
                 weighted call + ``flood_complex(point_weights=w)`` (cfg 2's landmarks, given; its points_per_edge).
                 ``dtm_profile`` refuses a mass at which some point is not reached, so the end-to-end figures are taken
                 over the masses at which every point is (the line says which, and how many points the others miss).

Every line is appended to the output as soon as it is measured.

usage: python tools/time_knn_mass_profile.py [--reps N] [--out profiles/knn_mass_profile_times.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from flooder_amd import core  # noqa: E402

CELL = 0.2
CAPACITY = 1024
MASSES = (0.0005, 0.001, 0.002, 0.005)
STAT = "dtm"


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
    out_path = (argv[argv.index("--out") + 1] if "--out" in argv
                else os.path.join(ROOT, "profiles", "knn_mass_profile_times.jsonl"))
    if not torch.cuda.is_available():
        raise SystemExit("time_knn_mass_profile.py needs a GPU: a timing taken anywhere else says nothing")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["cfg2"]
    tp = bench.make_points(w).to(dev).to(torch.float32).contiguous()
    n = int(tp.shape[0])
    sites, mu = fa.voxel_measure(tp, CELL)
    index = core.PointIndex(sites)
    head = {"workload": "cfg2", "points": n, "dim": int(tp.shape[1]), "queries": n, "cell": CELL,
            "sites": int(sites.shape[0]), "capacity": CAPACITY, "stat": STAT, "masses": list(MASSES)}
    kw = dict(neighbor_stat=STAT, max_neighbors=CAPACITY, squared=True, index=index)

    # ---- the weights: the profile call, the single calls
    line = {**head, "what": "distance_to_weighted_measure_profile"}
    put(line, "profile", timed(lambda: fa.distance_to_weighted_measure_profile(sites, mu, tp, MASSES, **kw), reps))
    values, counts = fa.distance_to_weighted_measure_profile(sites, mu, tp, MASSES, return_counts=True, **kw)
    missed = (~torch.isfinite(values)).sum(dim=0).tolist()
    line.update(not_reached=missed, count_median=[int(counts[:, c].median()) for c in range(len(MASSES))],
                count_max=[int(counts[:, c].max()) for c in range(len(MASSES))])
    total = 0.0
    for c, m in enumerate(MASSES):
        stats = timed(lambda: fa.distance_to_weighted_measure(sites, mu, tp, mass=m, **kw), reps)
        put(line, f"single_{m}", stats)
        total += stats[0]
        same = torch.equal(values[:, c], fa.distance_to_weighted_measure(sites, mu, tp, mass=m, **kw))
        line[f"column_equals_single_{m}"] = bool(same)
    line["singles_sum_ms"] = round(total, 3)
    line["single_largest_ms"] = line[f"single_{max(MASSES)}_ms"]
    line["profile_over_single_largest"] = round(line["profile_ms"] / line["single_largest_ms"], 4)
    line["profile_over_singles_sum"] = round(line["profile_ms"] / total, 4)
    emit(out_path, line)
    del values, counts

    # ---- end to end, over the masses at which every point is reached
    reached = tuple(m for m, k in zip(MASSES, missed) if k == 0)
    lms = fa.generate_landmarks(tp, w["n_lms"], start_idx=0)
    ppe = w["ppe"]
    line = {**head, "what": "dtm_profile(cell_size)", "landmarks": int(lms.shape[0]), "points_per_edge": ppe,
            "masses_end_to_end": list(reached),
            "masses_refused": {str(m): k for m, k in zip(MASSES, missed) if k}}
    if reached:
        put(line, "dtm_profile", timed(lambda: fa.dtm_profile(tp, lms, reached, points_per_edge=ppe, cell_size=CELL,
                                                              max_neighbors=CAPACITY, neighbor_stat=STAT), reps))

        def one(m):
            s, u = fa.voxel_measure(tp, CELL)
            wts = fa.distance_to_weighted_measure(s, u, tp, mass=m, neighbor_stat=STAT, max_neighbors=CAPACITY)
            return fa.flood_complex(tp, lms, points_per_edge=ppe, point_weights=wts)

        total = 0.0
        for m in reached:
            stats = timed(lambda: one(m), reps)
            put(line, f"separate_{m}", stats)
            total += stats[0]
        line["separate_sum_ms"] = round(total, 3)
        line["dtm_profile_over_separate_sum"] = round(line["dtm_profile_ms"] / total, 4)
        put(line, "voxel_measure", timed(lambda: fa.voxel_measure(tp, CELL), reps))
    emit(out_path, line)


if __name__ == "__main__":
    main()
