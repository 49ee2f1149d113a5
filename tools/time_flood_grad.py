"""Cost of the differentiable filtration on one MI355X: ``flood_filtration`` forward and backward next to
``flood_complex(..., return_simplex_tree=True)`` with the same cloud, landmarks and index (device events after warm-up;
the landmark selection and the index are outside the timed region).  The times of the new kernels
(``csrc/flood_grad.hip``) come from a run of this tool under ``rocprofv3 --kernel-trace --stats``.

usage: python tools/time_flood_grad.py [cfg2,cfg3,cfg4,cfg5] [--reps N]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402


def timed(fn, reps):
    out = None
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append((a.elapsed_time(b), (time.perf_counter() - t0) * 1e3))
    times.sort()
    return out, times[len(times) // 2]


def main():
    names = (sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "cfg2,cfg3,cfg4,cfg5").split(",")
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    dev = torch.device("cuda:0")
    for name in names:
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev)
        lms, index = fa.generate_landmarks(tp, w["n_lms"], start_idx=0, return_index=True)
        kw = dict(max_dimension=w.get("max_dim"), points_per_edge=w["ppe"], method=w.get("method"), index=index)
        # (the tree, not the dict: a dict of the 6-D complex of cfg 4 enumerates all its 15 M simplices on the host;
        # flood_filtration hands over the tables up to max_dimension only)
        fc_fn = lambda: fa.flood_complex(tp, lms, return_simplex_tree=True, **kw)   # noqa: E731
        pg = tp.detach().requires_grad_(True)
        ff_fn = lambda: fa.flood_filtration(pg, lms, **kw)   # noqa: E731
        fc_fn()
        F = ff_fn()        # warm-up (grid tables, plans, allocator)
        fc, (fc_ev, fc_wall) = timed(fc_fn, reps)
        F, (ff_ev, ff_wall) = timed(ff_fn, reps)
        assert F.to_dict() == fc.to_dict()
        loss_fn = lambda: torch.autograd.grad(sum(v.sum() for v in F.values), pg, retain_graph=True)   # noqa: E731
        loss_fn()
        _, (bw_ev, bw_wall) = timed(loss_fn, reps)
        n_simp = sum(int(s.shape[0]) for s in F.simplices)
        print(json.dumps({"workload": name, "points": int(tp.shape[0]), "landmarks": int(lms.shape[0]),
                          "simplices": n_simp, "flood_complex_ms": round(fc_ev, 3), "flood_complex_wall_ms": round(fc_wall, 3),
                          "flood_filtration_fwd_ms": round(ff_ev, 3), "flood_filtration_fwd_wall_ms": round(ff_wall, 3),
                          "backward_ms": round(bw_ev, 3), "backward_wall_ms": round(bw_wall, 3),
                          "fwd_over_flood_complex": round(ff_ev / fc_ev, 2)}), flush=True)
        del F, fc, pg, tp, lms, index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
