"""Cost of the differentiable distance to a measure and of ``dtm_filtration`` on one MI355X next to their comparators
of the same run.

Per workload (the cloud and the index of ``bench.py``, every point of the cloud a query) and per k the calls

    distance_to_measure(points, neighbors=k)                                   the forward without grad
    distance_to_measure(points.requires_grad_(), neighbors=k, differentiable=True)   the forward with grad (keeps the ids)
    its backward (a fixed linear functional of all values)
    at k = 32: neighbor_distance's forward with grad and its backward

and, on the first workload, ``dtm_filtration`` forward and backward at k = 64 and 1024 next to ``power_filtration``
with the same weights detached, are timed between device events on the current stream.  One warm-up call each, then
``--reps`` rounds in which the calls of a group follow one another, so that every comparator sees the same clocks; the
median per call is reported with its minimum and maximum.

usage: python tools/time_dtm_grad.py [cfg2,cfg4] [--reps N] [--ks 32,64,256,1024] [--out profiles/dtm_grad_times.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the workloads and their clouds)
import flooder_amd as fa  # noqa: E402
from time_power_grad import rounds_ms  # noqa: E402


def main():
    argv = sys.argv[1:]
    names = (argv[0] if argv and not argv[0].startswith("-") else "cfg2,cfg4").split(",")
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    ks = [int(k) for k in (argv[argv.index("--ks") + 1] if "--ks" in argv else "32,64,256,1024").split(",")]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "dtm_grad_times.jsonl")
    dev = torch.device("cuda:0")
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:      # (rewritten line by line: a run that is cut short keeps what it measured)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")

    def row(head, label, t, **more):
        ms, lo, hi = t
        emit({**head, "call": label, "ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), **more})

    for at, name in enumerate(names):
        w = bench.WORKLOADS[name]
        tp = bench.make_points(w).to(dev)
        lms, index = fa.generate_landmarks(tp, w["n_lms"], start_idx=0, return_index=True)
        n = int(tp.shape[0])
        coef = torch.linspace(0.5, 1.5, n, device=dev)
        for k in ks:
            head = {"workload": name, "points": n, "dim": w["dim"], "queries": n, "k": k, "stat": "dtm", "reps": reps}
            x = tp.clone().requires_grad_(True)
            fns = [("forward", lambda: fa.distance_to_measure(tp, neighbors=k, index=index)),
                   ("forward with grad", lambda: fa.distance_to_measure(x, neighbors=k, differentiable=True, index=index))]
            if k <= 32:
                fns.append(("neighbor_distance forward with grad",
                            lambda: fa.neighbor_distance(x, neighbors=k, neighbor_stat="dtm", index=index)))
            got = rounds_ms(fns, reps)
            loss = (coef * fa.distance_to_measure(x, neighbors=k, differentiable=True, index=index)).sum()
            fns = [("backward", lambda: torch.autograd.grad(loss, x, retain_graph=True))]
            if k <= 32:
                loss_nd = (coef * fa.neighbor_distance(x, neighbors=k, neighbor_stat="dtm", index=index)).sum()
                fns.append(("neighbor_distance backward", lambda: torch.autograd.grad(loss_nd, x, retain_graph=True)))
            got.update(rounds_ms(fns, reps))
            fwd = got["forward"][0]
            for label, t in got.items():
                row(head, f"distance_to_measure {label}" if not label.startswith("neighbor") else label, t,
                    ratio_to_forward=round(t[0] / fwd, 2))
            del loss, x
            if k <= 32:
                del loss_nd
            torch.cuda.empty_cache()
        if at == 0:      # dtm_filtration next to power_filtration with the same weights, detached
            kw = dict(points_per_edge=w["ppe"], max_dimension=w.get("max_dim"), index=index)
            for k in (64, 1024):
                head = {"workload": name, "points": n, "dim": w["dim"], "landmarks": int(lms.shape[0]),
                        "points_per_edge": w["ppe"], "k": k, "reps": reps}
                x = tp.clone().requires_grad_(True)
                wt = fa.distance_to_measure(tp, neighbors=k, index=index)
                got = rounds_ms([("dtm_filtration", lambda: fa.dtm_filtration(x, lms, neighbors=k, **kw)),
                                 ("power_filtration, detached weights", lambda: fa.power_filtration(x, lms, wt, **kw))], reps)

                def loss_of(F):
                    return sum((torch.linspace(0.5, 1.5, v.shape[0], device=dev) * v).sum() for v in F.values)

                la = loss_of(fa.dtm_filtration(x, lms, neighbors=k, **kw))
                lb = loss_of(fa.power_filtration(x, lms, wt, **kw))
                got.update(rounds_ms([("dtm_filtration backward", lambda: torch.autograd.grad(la, x, retain_graph=True)),
                                      ("power_filtration backward, detached weights",
                                       lambda: torch.autograd.grad(lb, x, retain_graph=True))], reps))
                for label, t in got.items():
                    row(head, label, t)
                del la, lb, x, wt
                torch.cuda.empty_cache()
        del tp, lms, index, coef
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
