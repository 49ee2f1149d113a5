"""Cost of the neighbour ids (``flooder_knn_ids_sorted_f32``) on one MI355X next to the values alone and next to
``flooder_witness_knn``.

Per cloud - the 1 M-point 3-D Gaussian of cfg 2 and the 2 M-point 6-D Gaussian of cfg 4 - the queries are the cloud's
own points, and for k = 2, 8, 32 three things are timed by device events on the launch stream (one warm-up call each,
then ``--reps`` calls, alternating between the first two so that both see the same clocks; median, min, max):

  values   ``neighbor_distance(points, None, k, "kth", squared=True)``: sample keys, radix sort,
           ``flooder_sweep_knn_sorted_f32`` - the path without grad;
  ids      the same stages with ``flooder_knn_ids_sorted_f32`` writing ids, d2 words and the statistic word
           (``neighbors._knn_ids_hip``: what ``nearest_neighbors`` and a forward with grad run);
  witness  ``flooder_witness_knn`` alone (one wave per query) on the first 65 536 queries, fed the statistic words of
           the value sweep.

``ids_over_values`` is the ratio of the medians; ``witness_over_ids_per_query`` compares microseconds per query.

usage: python tools/time_knn_ids.py [cfg2,cfg4] [--reps N] [--out profiles/knn_ids_times.jsonl]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from flooder_amd import _native, core, neighbors  # noqa: E402

WITNESS_QUERIES = 65_536


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternating_ms(fns, reps):
    for fn in fns:
        event_ms(fn)                       # warm-up: code objects, allocator blocks
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            times[i].append(event_ms(fn)[0])
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def witness_fn(lib, index, queries, k, q_stat):
    dev = queries.device
    n_q, dim = queries.shape
    verts = queries.unsqueeze(1).contiguous()
    one = torch.ones((1, 1), dtype=torch.float32, device=dev)
    q_s = torch.arange(n_q, dtype=torch.int32, device=dev)
    q_r = torch.zeros(n_q, dtype=torch.int32, device=dev)
    out_ids = torch.empty((n_q, k), dtype=torch.int64, device=dev)
    out_d2 = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    not_found = torch.zeros(1, dtype=torch.int32, device=dev)
    blk = _native.WitnessKnn(pts_sorted=index.pts, n_pts=index.n, dim=dim, k1=1, nodes=index.nodes, order=index.order32,
                             verts=verts, weights=one, R=1, k=k, n_simplices=n_q, n_queries=n_q, q_simplex=q_s, q_row=q_r,
                             q_stat=q_stat, out_ids=out_ids, out_d2=out_d2, not_found=not_found, stat=0)

    def run():
        _native.check(lib.flooder_witness_knn(ctypes.byref(blk), _native.current_stream_ptr(dev)), "flooder_witness_knn")
        return out_ids, not_found
    return run


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2,cfg4").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_ids_times.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("time_knn_ids.py needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib = _native.load()
    lines = []
    for name in names:
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev).to(torch.float32).contiguous()
        index = core.PointIndex(tp)
        n = int(tp.shape[0])
        n_w = min(WITNESS_QUERIES, n)
        head = {"workload": name, "points": n, "dim": int(tp.shape[1]), "queries": n, "witness_queries": n_w}
        for k in (2, 8, 32):
            values = lambda: fa.neighbor_distance(tp, None, k, "kth", squared=True, index=index)                # noqa: E731
            ids = lambda: neighbors._knn_ids_hip(tp, tp, k, "kth", index, want_d2=True, want_bits=True)         # noqa: E731
            (v_ms, v_lo, v_hi), (i_ms, i_lo, i_hi) = alternating_ms([values, ids], reps)
            words = values().view(torch.int32)
            got_ids, _, got_bits = ids()
            assert torch.equal(got_bits, words), "the ids sweep's statistic words differ from the value sweep's"
            wit = witness_fn(lib, index, tp[:n_w], k, words[:n_w].contiguous())
            (w_ms, w_lo, w_hi), = alternating_ms([wit], reps)
            w_ids, not_found = wit()
            assert int(not_found.item()) == 0 and torch.equal(w_ids, got_ids[:n_w].long()), "witness ids differ"
            line = {**head, "k": k, "reps": reps,
                    "values_ms": round(v_ms, 3), "values_min_ms": round(v_lo, 3), "values_max_ms": round(v_hi, 3),
                    "ids_ms": round(i_ms, 3), "ids_min_ms": round(i_lo, 3), "ids_max_ms": round(i_hi, 3),
                    "ids_over_values": round(i_ms / v_ms, 2),
                    "witness_ms": round(w_ms, 3), "witness_min_ms": round(w_lo, 3), "witness_max_ms": round(w_hi, 3),
                    "ids_us_per_query": round(1e3 * i_ms / n, 4), "witness_us_per_query": round(1e3 * w_ms / n_w, 4),
                    "witness_over_ids_per_query": round((w_ms / n_w) / (i_ms / n), 2)}
            lines.append(line)
            print(json.dumps(line), flush=True)
        del tp, index
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
