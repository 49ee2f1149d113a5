"""Host share of a short k-nearest call on one MI355X: wall clock of ``neighbor_distance`` at Q = 1000 queries on the
100 k-point 3-D Gaussian (``bench.py``'s "small" cloud), k = 8, with a prebuilt index.  At that size the call is
launch-bound: what it costs is Python, ctypes, the checks of the entry points and the launches themselves - the part a
change to the host code can move and ``tools/time_knn*.py`` (device events over millisecond sweeps) cannot see.

One or more checkouts are timed in fresh processes that alternate, ``--rounds`` times each, so that all see the same
clocks; a process makes ``--calls`` calls after a warm-up, synchronises after each and reports median, min and max in
microseconds.  A checkout is ``label=DIR`` (its ``flooder_amd`` and its built libraries are used; ``FLOODER_HIP_LIB``
is passed through as it is).

usage: python tools/time_knn_host.py [label=DIR ...] [--rounds 3] [--calls 300] [--out profiles/knn_host_times.jsonl]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES, K = 1000, 8


def child(tree, calls):
    sys.path.insert(0, tree)
    import torch

    import bench
    import flooder_amd as fa
    from flooder_amd import core

    dev = torch.device("cuda:0")
    tp = bench.make_points(bench.WORKLOADS["small"]).to(dev).to(torch.float32).contiguous()
    index = core.PointIndex(tp)
    q = tp[:QUERIES].contiguous()
    out = {}
    for stat in ("kth", "dtm"):
        for _ in range(20):
            fa.neighbor_distance(tp, q, K, stat, index=index)
        torch.cuda.synchronize()
        us = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fa.neighbor_distance(tp, q, K, stat, index=index)
            torch.cuda.synchronize()
            us.append(1e6 * (time.perf_counter() - t0))
        us.sort()
        out[stat] = {"median_us": round(us[len(us) // 2], 1), "min_us": round(us[0], 1), "max_us": round(us[-1], 1)}
    print(json.dumps(out), flush=True)


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--child"]:
        return child(argv[1], int(argv[2]))
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 3
    calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 300
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_host_times.jsonl")
    trees = [a.split("=", 1) for a in argv if "=" in a and not a.startswith("-")] or [["this", ROOT]]
    lines = []
    for r in range(rounds):
        for label, tree in trees:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(tree), str(calls)],
                                 check=True, capture_output=True, text=True, timeout=300)
            for stat, t in json.loads(res.stdout.strip().splitlines()[-1]).items():
                line = {"tool": "time_knn_host", "tree": label, "round": r, "points": 100_000, "dim": 3,
                        "queries": QUERIES, "k": K, "stat": stat, "calls": calls, **t}
                lines.append(line)
                print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
