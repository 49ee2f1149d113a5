"""Cost of the robust filtration over point shards (``csrc/flood_knn_merge.hip``) on one MI355X, EMULATED shards.

cfg 2, W = 2 interleaved shards of the cloud, k = 2, 8, 32.  The two shards run one after the other on the one GPU
(the emulation of ``tests/test_gpu_knn_sharded.py``): rank 1's call keeps its lists, rank 0's call is the one that is
timed and its hook answers with the stack of both - what an all-gather leaves on every rank.  The all-gather itself is
NOT measured: no multi-GPU node was used.  Spans of ``core._sweep_dimension_knn_sharded`` by device events on the launch
stream, median of ``--reps`` calls after a warm-up: ``sweep`` (the local list sweep of one shard), ``merge``
(``flooder_knn_merge_f32``) and ``face_max``; next to them the ``sweep`` span of the unsharded
``core._sweep_dimension_knn`` on the whole cloud at the same k.

The merge kernel stops reading a list where no lane of a wave can still improve, so it reads fewer bytes than the
gathered buffer holds.  The tool replays that rule on the gathered lists (list 0 whole; of every further list, per
wave of 64 cells, plane after plane up to and including the first no lane improves on) and adds the bytes of every
plane read by a live lane to a counter word on the device; a ``torch`` device-to-device copy of that many bytes, timed
in the same run, is what moving them costs.

usage: python tools/time_knn_merge.py [--reps N] [--out profiles/knn_merge_times.jsonl] [--ks 2,8,32]
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

WORLD = 2


def median_spans(fn, reps, names):
    """Median over ``reps`` calls of ``fn(timer)`` after one warm-up call, per span name."""
    def once():
        timer = core._KernelTimer()
        fn(timer)
        torch.cuda.synchronize()
        t = timer.totals_ms()
        return [t[n] for n in names]

    once()
    runs = np.array([once() for _ in range(reps)])
    return {n: round(float(np.median(runs[:, i])), 3) for i, n in enumerate(names)}


def merge_bytes_read(gathered: torch.Tensor, chunk_cells: int = 1 << 21) -> int:
    """Bytes ``flooder_knn_merge_f32`` reads of ``gathered`` (W, k, n) int32: the kernel's own rule, replayed."""
    W, k, n = gathered.shape
    dev = gathered.device
    counter = torch.zeros(1, dtype=torch.int64, device=dev)     # the counter word
    big = torch.iinfo(torch.int32).max
    for a in range(0, n, chunk_cells):
        b = min(n, a + chunk_cells)
        m = b - a
        waves = -(-m // 64)
        lanes = torch.full((waves,), 64, dtype=torch.int64, device=dev)
        lanes[-1] = m - 64 * (waves - 1)
        counter += 4 * k * m                                     # list 0, every plane
        cur = gathered[0, :, a:b].t().contiguous()               # (m, k) ascending
        for w in range(1, W):
            active = torch.ones(waves, dtype=torch.bool, device=dev)
            for j in range(k):
                counter += 4 * (lanes * active).sum()            # this plane is loaded by the waves still in the list
                cand = gathered[w, j, a:b]
                passes = torch.zeros(waves * 64, dtype=torch.bool, device=dev)
                passes[:m] = cand < cur[:, -1]
                active &= passes.view(waves, 64).any(dim=1)      # the wave vote; no lane passes: the list ends here
                live = active.repeat_interleave(64)[:m]
                ins = torch.where(live, cand, torch.full_like(cand, big))
                cur = torch.sort(torch.cat([cur, ins[:, None]], dim=1), dim=1).values[:, :k]
                if not bool(active.any()):
                    break
    return int(counter.item())


def copy_ms(n_bytes: int, reps: int) -> float:
    src = torch.empty(max(1, n_bytes // 4), dtype=torch.int32, device="cuda:0").zero_()
    dst = torch.empty_like(src)
    times = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        if i:
            times.append(a.elapsed_time(b))
    return round(float(np.median(times)), 3)


def main():
    argv = sys.argv[1:]
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "knn_merge_times.jsonl")
    ks = [int(x) for x in (argv[argv.index("--ks") + 1] if "--ks" in argv else "2,8,32").split(",")]
    dev = torch.device("cuda:0")
    name = "cfg2"
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
    shards = [core.PointIndex(tp[r::WORLD].contiguous()) for r in range(WORLD)]
    head = {"workload": name, "points": int(tp.shape[0]), "dim": w["dim"], "landmarks": int(lms.shape[0]),
            "simplices": S, "samples_per_simplex": R, "shards": WORLD,
            "note": "emulated shards, one after the other on one GPU; the all-gather is not measured"}
    lines = []
    for k in ks:
        for stat in ("kth", "dtm"):
            kept = []

            def keep(lists):
                kept.append(lists.clone())
                return lists[None]

            keep.world_size = WORLD
            core._sweep_dimension_knn_sharded(shards[1], verts, weights, faces, k, stat, keep, plan=plan)
            assert len(kept) == 1, "cfg 2 fits one group"
            last = []

            def both(lists):
                last[:] = [torch.stack([lists, kept[0]])]
                return last[0]

            both.world_size = WORLD
            spans = median_spans(lambda timer: core._sweep_dimension_knn_sharded(
                shards[0], verts, weights, faces, k, stat, both, plan=plan, timer=timer), reps,
                ("sweep", "gather", "merge", "face_max"))
            whole = median_spans(lambda timer: core._sweep_dimension_knn(index, verts, weights, faces, k, stat, plan=plan,
                                                                         timer=timer), reps, ("sweep",))
            # the sharded values are the unsharded ones
            a, _ = core._sweep_dimension_knn_sharded(shards[0], verts, weights, faces, k, stat, both, plan=plan)
            b, _ = core._sweep_dimension_knn(index, verts, weights, faces, k, stat, plan=plan)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            gathered = last[0].reshape(WORLD, k, S * R)
            held = gathered.numel() * 4
            read = merge_bytes_read(gathered) if stat == "kth" else lines[-1]["merge_bytes_read"]   # (the same lists)
            lines.append({**head, "k": k, "stat": stat, "local_sweep_ms": spans["sweep"], "merge_ms": spans["merge"],
                          "face_max_ms": spans["face_max"], "emulated_gather_stack_ms": spans["gather"],
                          "unsharded_sweep_ms": whole["sweep"], "gathered_bytes": held, "merge_bytes_read": read,
                          "read_fraction": round(read / held, 4), "d2d_copy_same_bytes_ms": copy_ms(read, reps),
                          "reps": reps})
            print(json.dumps(lines[-1]), flush=True)
            del kept, last, gathered
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
