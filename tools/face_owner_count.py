"""Face ownership, counted on the CPU: how many (simplex, row) units of a grid sweep are duplicates that ownership
removes, and how many whole chunks (256 rows) and tiles (64 rows) disappear - with the rows grouped by facet
(core.FACE_OWNER_GROUPED) and in the patch order of core.sample_order.
usage: face_owner_count.py [landmarks=1000] [points_per_edge=30] [dim=3] [cloud points=200000]

Owners are chosen two ways: the lowest row among the incident simplices, and the lightest one (fewest cloud points in
the simplex's bounding box, counted with a kd-tree; ties to the lowest row) - the rule the cell sweep's entry applies,
short of the simplices the witness sweep has handled.  Last line: total chunk bounding-box volume on the regular simplex,
grouped order against the patch order (`core.sample_order`)."""
import sys

import numpy as np
import torch
from scipy.spatial import cKDTree

sys.path.insert(0, ".")
from flooder_amd import core  # noqa: E402

n_lms = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
ppe = int(sys.argv[2]) if len(sys.argv) > 2 else 30
dim = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n_pts = int(sys.argv[4]) if len(sys.argv) > 4 else 200_000

rng = np.random.default_rng(0)
cloud = rng.standard_normal((n_pts, dim)).astype(np.float32)
lms = cloud[rng.choice(n_pts, n_lms, replace=False)]
stree, simplices = core._build_complex(torch.as_tensor(lms), dim)
cells = np.sort(np.asarray(simplices[dim]), axis=1)
S = cells.shape[0]
weights, vertex_idxs, face_idxs = core.generate_grid(ppe, dim, "cpu", torch.float32)
faces = core._FaceTable(face_idxs, weights.shape[0], "cpu")
rows = stree._locate(dim, cells)
slot, n_slots, _ = core.shared_face_slots(stree, dim, rows, [v.numpy() for v in vertex_idxs], "cpu")
slot = slot.numpy()
F = slot.shape[1]

keep = core.FACE_OWNER, core.FACE_OWNER_GROUPED
try:
    core.FACE_OWNER, core.FACE_OWNER_GROUPED = True, True
    plan = core.SamplePlan(weights, faces)                  # rows grouped by facet
    core.FACE_OWNER_GROUPED = False
    plan_old = core.SamplePlan(weights, faces)              # patch order (the default)
finally:
    core.FACE_OWNER, core.FACE_OWNER_GROUPED = keep
R = weights.shape[0]

# weight of a simplex: cloud points inside its bounding box
tree = cKDTree(cloud)
v = lms[cells]
lo, hi = v.min(axis=1), v.max(axis=1)
wgt = np.empty(S)
for s in range(S):
    cand = tree.query_ball_point(0.5 * (lo[s] + hi[s]), 0.5 * (hi[s] - lo[s]).max(), p=np.inf)
    x = cloud[cand]
    wgt[s] = ((x >= lo[s]) & (x <= hi[s])).all(axis=1).sum()


def owners(key):
    """owner[slot] = the incident simplex with the smallest (key, row)"""
    order = np.lexsort((np.arange(S), key))                  # ascending key, ties by row
    own = np.full(n_slots, -1, dtype=np.int64)
    for s in order[::-1]:                                     # the best one writes last
        own[slot[s]] = s
    return own


def report(name, own, min_face):
    mine = own[slot] == np.arange(S)[:, None]                # (S, F): s evaluates the own samples of its face f
    mine[:, 0] = True
    units = mine[:, min_face]                                # (S, R)
    removed = (~units).sum()
    out = [f"{name}: units {S * R}, removed {removed} = {100.0 * removed / (S * R):.1f} %"]
    for run, what in ((256, "chunk"), (64, "tile")):
        n = (R + run - 1) // run
        pad = np.zeros((S, n * run), dtype=bool)
        pad[:, :R] = units
        gone = ~pad.reshape(S, n, run).any(axis=2)
        rows_gone = sum(int(gone[:, j].sum()) * (min(R, (j + 1) * run) - j * run) for j in range(n))
        out.append(f"  whole {what}s gone {gone.sum()} of {S * n} = {100.0 * gone.sum() / (S * n):.1f} %, "
                   f"their rows = {100.0 * rows_gone / max(removed, 1):.1f} % of the removed units")
    print("\n".join(out))


print(f"{S} simplices, {R} rows each, {F} faces per simplex, {n_slots} distinct faces")
for label, p in (("rows grouped by facet", plan), ("patch order", plan_old)):
    mf = p.min_face.numpy().astype(np.int64)                # sweep order
    report(f"{label}, lowest row", owners(np.zeros(S)), mf)
    report(f"{label}, lightest wins", owners(wgt), mf)


def chunk_volume(p):
    w = p.w_perm.numpy().astype(np.float64)
    k1 = w.shape[1]
    corners = np.eye(k1) - 1.0 / k1
    X = w @ (corners @ np.linalg.qr(corners.T)[0][:, :k1 - 1])
    return sum(float(np.prod(np.ptp(X[i:i + 256], axis=0))) for i in range(0, R, 256))


print(f"chunk box volume on the regular simplex: grouped order {chunk_volume(plan):.4f}, patch order {chunk_volume(plan_old):.4f}")
