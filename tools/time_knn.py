"""Cost of the k-nearest tree sweep (``csrc/flood_knn.hip``) on one MI355X next to the nearest-point tree sweep.

Per workload the top-dimensional simplices of the complex are swept against the cloud's index by
``core._sweep_dimension_bvh`` (``method="bvh"`` at k = 1: the per-simplex tree sweep in 3-D, the sorted-sample sweep
above) and by ``core._sweep_dimension_knn`` at k = 2, 8, 32 with both statistics.  What is timed is the ``sweep`` span
of each (device events on the launch stream, after a warm-up call, median of ``--reps`` calls); landmark selection,
index, triangulation and face maxima are outside.  Every (k, statistic) is timed in BOTH forms of the k-nearest sweep,
alternating call by call so that both see the same clocks: ``per-simplex`` (a tile is one simplex,
``flooder_sweep_knn_f32``) and ``sorted tiles`` (a tile is 64 consecutive samples of the curve order over all simplices,
``flooder_sweep_knn_sorted_f32``; its span includes the sample keys and the radix sort), forced through
``core.KNN_SORTED_SAMPLES``; ``default_form`` names the one the library picks on its own.  The sweep counters (leaves evaluated / tested, node tests) come
from one extra call with a ``stats`` buffer and are reported per tile and as points compared per sample.

usage: python tools/time_knn.py [cfg2,cfg4] [--reps N] [--out profiles/knn_sweep_times.jsonl] [--only-k K] [--stats kth,dtm]
(``--only-k 8``: one warm-up and one ``kth`` call at that k and nothing else - what a run under
``rocprofv3 --kernel-trace --stats`` wants)
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


def sweep_ms(fn, reps):
    """Median, min and max of the ``sweep`` span over ``reps`` calls of ``fn(timer, stats)`` after one warm-up call;
    a warm-up that takes longer than five seconds is followed by one timed call only."""
    def once():
        timer = core._KernelTimer()
        fn(timer, None)
        torch.cuda.synchronize()
        return timer.totals_ms()["sweep"]

    first = once()
    times = sorted(once() for _ in range(1 if first > 5000.0 else reps))
    return times[len(times) // 2], times[0], times[-1], len(times)


def alternating_ms(fns, reps):
    """``sweep_ms`` for several functions whose timed calls alternate (a, b, a, b, ...) after one warm-up call each."""
    def once(fn):
        timer = core._KernelTimer()
        fn(timer, None)
        torch.cuda.synchronize()
        return timer.totals_ms()["sweep"]

    first = [once(fn) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(1 if max(first) > 5000.0 else reps):
        for i, fn in enumerate(fns):
            times[i].append(once(fn))
    return [(sorted(t)[len(t) // 2], min(t), max(t), len(t)) for t in times]


def counters(fn, n_tiles):
    """The sweep's counters from one call with a ``stats`` buffer.  A leaf evaluation compares the 16 points of a leaf
    with every sample of the tile that asked for it, so ``16 * leaf evaluations / tiles`` is the number of points an
    average sample is compared with - the figure that is comparable between sweeps whose tiles differ in size."""
    stats = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    fn(None, stats)
    torch.cuda.synchronize()
    ev, lt, nt, worst = (int(v) for v in stats[:4].cpu())
    return {"tiles": n_tiles, "leaf_evals": ev, "leaf_tests": lt, "node_tests": nt, "most_tests_of_a_tile": worst,
            "leaf_evals_per_tile": round(ev / n_tiles, 2), "leaf_tests_per_tile": round(lt / n_tiles, 1),
            "points_per_sample": round(ev * 16 / n_tiles, 1)}


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2,cfg4").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_sweep_times.jsonl")
    only_k = int(argv[argv.index("--only-k") + 1]) if "--only-k" in argv else None
    stat_names = (argv[argv.index("--stats") + 1] if "--stats" in argv else "kth,dtm").split(",")
    shipped = core.KNN_SORTED_SAMPLES
    dev = torch.device("cuda:0")
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
                "simplices": S, "samples_per_simplex": R}

        def knn(k, stat, sorted_tiles=None):
            def run(timer, stats):
                core.KNN_SORTED_SAMPLES = shipped if sorted_tiles is None else sorted_tiles
                try:
                    return core._sweep_dimension_knn(index, verts, weights, faces, k, stat, plan=plan, stats=stats,
                                                     timer=timer)
                finally:
                    core.KNN_SORTED_SAMPLES = shipped
            return run

        if only_k is not None:
            knn(only_k, "kth")(None, None)
            torch.cuda.synchronize()
            knn(only_k, "kth")(None, None)
            torch.cuda.synchronize()
            continue
        bvh = lambda timer, stats: core._sweep_dimension_bvh(index, verts, weights, faces, None, plan=plan,  # noqa: E731
                                                             stats=stats, timer=timer)
        base, lo, hi, n = sweep_ms(bvh, reps)
        # tiles of the k = 1 sweep: the sorted-sample sweep (its span holds the key generation and the radix sort of
        # the samples as well) cuts ALL samples into tiles of 64; the per-simplex sweep takes two samples per lane
        # for more than 64 samples per simplex.  The k-nearest sweep: 64 sample slots per simplex and tile.
        is_sorted = core.bvh_sorts_samples(w["dim"], S, R)
        per_tile = int(core._native.load().flooder_sorted_tile_samples()) if is_sorted else (64 if R <= 64 else 128)
        base_tiles = -(-S * R // per_tile) if is_sorted else S * -(-R // per_tile)
        forms = (("per-simplex", False, S * -(-R // 64)), ("sorted tiles", True, -(-S * R // 64)))
        default_form = forms[int(core.knn_sorts_samples(w["dim"], S, R))][0]
        lines.append({**head, "sweep": "bvh k=1" + (" (sorted samples; span includes sample keys + radix sort)" if is_sorted else ""),
                      "sweep_ms": round(base, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "reps": n,
                      **counters(bvh, base_tiles)})
        print(json.dumps(lines[-1]), flush=True)
        for k in (2, 8, 32):
            for stat in stat_names:
                timed = alternating_ms([knn(k, stat, forced) for _, forced, _ in forms], reps)
                for (form, forced, tiles), (ms, lo, hi, n) in zip(forms, timed):
                    lines.append({**head, "sweep": f"knn k={k} {stat}", "form": form, "default_form": default_form,
                                  "sweep_ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "reps": n,
                                  "ratio_to_bvh_k1": round(ms / base, 2), **counters(knn(k, stat, forced), tiles)})
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
