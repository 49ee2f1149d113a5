"""Cost of the differentiable distance to a WEIGHTED measure and of ``dtm_filtration(cell_size=...)`` on one MI355X next
to their comparators of the same run.

The cloud is cfg 2's (1 M-point 3-D Gaussian, the cloud and the index of ``bench.py``); every cloud point is a query.
Per row of the README's weighted-measure table - cell size of ``CELLS``, mass of ``MASSES`` (both more than 1024
points, where ``distance_to_measure`` refuses), list capacity of ``CAPACITIES`` - the calls

    distance_to_weighted_measure(sites, mu, queries=points, mass=m, max_neighbors=C)          the forward without grad
    the same with differentiable=True on sites, masses and queries that require grad         the forward with grad
    its backward into sites and queries                                                      (a fixed linear functional
    its backward into sites, queries and masses                                               of all reached values)

and per cell size ``dtm_filtration(points, landmarks, mass, cell_size=cell)`` forward and backward at the first mass,
and once ``distance_to_measure(points, neighbors=1024, differentiable=True)`` forward and backward - the most the plain
path does - are timed between device events on the current stream.  One warm-up call each, then ``--reps`` rounds in
which the calls of a group follow one another; the median per call is reported with its minimum and maximum.  The index
of the sites is built beforehand.  Every line is written as soon as it is measured.

usage: python tools/time_mass_grad.py [--reps N] [--out profiles/mass_grad_times.jsonl]
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
from time_power_grad import rounds_ms  # noqa: E402

CELLS = (0.2, 0.1)
MASSES = (0.002, 0.005)
CAPACITIES = (1024, 256)


def main():
    argv = sys.argv[1:]
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "mass_grad_times.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("time_mass_grad.py needs a GPU: a timing taken anywhere else says nothing")
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

    w = bench.WORKLOADS["cfg2"]
    tp = bench.make_points(w).to(dev).to(torch.float32).contiguous()
    lms, cloud_index = fa.generate_landmarks(tp, w["n_lms"], start_idx=0, return_index=True)
    n = int(tp.shape[0])
    go = torch.linspace(0.5, 1.5, n, device=dev)
    base = {"workload": "cfg2", "points": n, "dim": int(tp.shape[1]), "queries": n, "reps": reps}

    # the comparator: the most the plain path does
    head = {**base, "k": core.KNN_WIDE_MAX}
    x = tp.clone().requires_grad_(True)
    got = rounds_ms([("distance_to_measure forward", lambda: fa.distance_to_measure(tp, neighbors=core.KNN_WIDE_MAX,
                                                                                   index=cloud_index)),
                     ("distance_to_measure forward with grad",
                      lambda: fa.distance_to_measure(x, neighbors=core.KNN_WIDE_MAX, differentiable=True,
                                                     index=cloud_index))], reps)
    loss = (go * fa.distance_to_measure(x, neighbors=core.KNN_WIDE_MAX, differentiable=True, index=cloud_index)).sum()
    got.update(rounds_ms([("distance_to_measure backward", lambda: torch.autograd.grad(loss, x, retain_graph=True))], reps))
    for label, t in got.items():
        row(head, label, t)
    del loss, x
    torch.cuda.empty_cache()

    for cell in CELLS:
        sites, mu = fa.voxel_measure(tp, cell)
        index = core.PointIndex(sites)
        for mass in MASSES:
            for cap in CAPACITIES:
                head = {**base, "cell": cell, "sites": int(sites.shape[0]), "mass": mass,
                        "k_points": core.mass_neighbors(mass, n), "capacity": cap}
                kw = dict(mass=mass, max_neighbors=cap, index=index)
                y, m, q = (t.clone().requires_grad_(True) for t in (sites, mu, tp))
                got = rounds_ms([("forward", lambda: fa.distance_to_weighted_measure(sites, mu, tp, **kw)),
                                 ("forward with grad",
                                  lambda: fa.distance_to_weighted_measure(y, m, q, differentiable=True, **kw))], reps)
                # (which gradients a backward forms is fixed by the inputs that require grad at the forward: two graphs)
                value = fa.distance_to_weighted_measure(y, m, q, differentiable=True, **kw)
                plain = fa.distance_to_weighted_measure(y, mu, q, differentiable=True, **kw)
                reached = torch.isfinite(value.detach())
                loss = (go * torch.where(reached, value, torch.zeros_like(value))).sum()
                loss_yq = (go * torch.where(reached, plain, torch.zeros_like(plain))).sum()
                got.update(rounds_ms([("backward, sites and queries",
                                       lambda: torch.autograd.grad(loss_yq, (y, q), retain_graph=True)),
                                      ("backward, sites, queries and masses",
                                       lambda: torch.autograd.grad(loss, (y, q, m), retain_graph=True))], reps))
                del plain, loss_yq
                fwd = got["forward"][0]
                for label, t in got.items():
                    row(head, f"distance_to_weighted_measure {label}", t, ratio_to_forward=round(t[0] / fwd, 2),
                        not_reached_share=round(1.0 - float(reached.float().mean()), 6))
                del loss, value, y, m, q, reached
                torch.cuda.empty_cache()
        # the one-call recipe at the first mass, the default capacity (a point that is not reached is refused)
        mass = MASSES[0]
        head = {**base, "cell": cell, "sites": int(sites.shape[0]), "mass": mass, "landmarks": int(lms.shape[0]),
                "points_per_edge": w["ppe"]}
        kw = dict(points_per_edge=w["ppe"], max_dimension=w.get("max_dim"), index=cloud_index, cell_size=cell)
        x = tp.clone().requires_grad_(True)
        try:
            got = rounds_ms([("dtm_filtration(cell_size)", lambda: fa.dtm_filtration(x, lms, mass, **kw))], reps)
            F = fa.dtm_filtration(x, lms, mass, **kw)
            loss = sum((torch.linspace(0.5, 1.5, v.shape[0], device=dev) * v).sum() for v in F.values)
            got.update(rounds_ms([("dtm_filtration(cell_size) backward",
                                   lambda: torch.autograd.grad(loss, x, retain_graph=True))], reps))
            for label, t in got.items():
                row(head, label, t)
            del F, loss
        except ValueError as e:          # (points that are not reached: the refusal is the result of this row)
            emit({**head, "call": "dtm_filtration(cell_size)", "refused": str(e)})
        del x, sites, mu, index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
