"""Run test of the witness sweep (csrc/flood_wit.hip, phase 4a): how many aligned runs of G sweep-order samples can be
dropped with ONE bound per run, on the headline workload (cfg 2: 1 M Gaussian points, 1000 landmarks, 30 points per
edge)?  CPU only, about a minute: the cloud, exact farthest-point landmarks, their Delaunay tetrahedra, the package's own
sample plan and witness plan; thresholds are the face maxima the coarse samples alone establish (the kernel's are at
least as high).  Prints, per run length, the share of runs dropped with
  - the exact radius of the run about its box centre in space (what no kernel can afford),
  - the table's radius in weight space (core.witness_runs) times the spectral norm of the centred vertex matrix,
  - ... times the Gershgorin bound of that norm (what the kernel computes),
and the work left: (runs tested + samples of the surviving runs) / samples.

usage: python tools/wit_run_bound.py [--simplices 300] [--gpu]
  --gpu: instead, run the sweep of cfg 2 on the GPU and print the kernel's own counter of dropped runs."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flooder_amd import core  # noqa: E402


def on_gpu():
    import flooder_amd as fa

    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    pts = torch.randn(1_000_000, 3).to(dev)
    lms = fa.generate_landmarks(pts, 1000, start_idx=0)
    _, simplices = core._build_complex(lms, 3)
    verts = lms[torch.as_tensor(simplices[3], device=dev)].contiguous()
    weights, _, face_idxs = core.generate_grid(30, 3, dev, torch.float32)
    faces = core._FaceTable(face_idxs, weights.shape[0], dev)
    st = torch.zeros(40, dtype=torch.int64, device=dev)
    core._sweep_dimension_cell(core.PointIndex(pts), verts, weights, faces, None, stats=st)
    torch.cuda.synchronize()
    w = st[16:40].cpu().numpy()
    n_runs = (weights.shape[0] // core.WIT_RUN_LEN) * int(w[0])
    print(f"simplices handled {int(w[0])} of {verts.shape[0]}, runs of {core.WIT_RUN_LEN} dropped {int(w[21])} of {n_runs} "
          f"({100.0 * w[21] / max(n_runs, 1):.1f} %), samples live after the bounds {int(w[6])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--simplices", type=int, default=300)
    ap.add_argument("--gpu", action="store_true")
    args = ap.parse_args()
    if args.gpu:
        return on_gpu()
    from scipy.spatial import Delaunay, cKDTree

    t0 = time.time()
    torch.manual_seed(42)
    pts = torch.randn(1_000_000, 3).numpy().astype(np.float32)
    d = ((pts - pts[0]) ** 2).sum(1)
    idx = [0]
    for _ in range(999):
        j = int(d.argmax())
        idx.append(j)
        d = np.minimum(d, ((pts - pts[j]) ** 2).sum(1))
    lms = pts[idx].astype(np.float64)
    tets = Delaunay(lms).simplices
    w, _, fidx = core.generate_grid(30, 3, torch.device("cpu"), torch.float32)
    faces = core._FaceTable(fidx, w.shape[0], torch.device("cpu"))
    plan = core.SamplePlan(w, faces)
    w_perm = plan.w_perm.numpy()
    wp = w_perm.astype(np.float64)
    memb = plan.memb_all.numpy().view(np.uint32)
    rows_c, par, nc = core.witness_plan(w, plan._perm)
    rows_c = rows_c[:nc]
    R, F = wp.shape[0], faces.n_faces
    print(f"{len(tets)} tetrahedra, R {R}, {F} faces, {nc} coarse samples ({time.time() - t0:.0f} s)", flush=True)
    par4 = np.stack([(par >> (8 * j)) & 255 for j in range(4)], 1).astype(np.int64)
    tree = cKDTree(pts.astype(np.float64))
    V = lms[tets]
    lo, hi = V.min(1), V.max(1)
    bits = [((memb >> f) & 1) == 1 for f in range(F)]
    lengths = (8, 16, 32, 64)
    tabs = {G: core.witness_runs(w_perm, memb, par, G) for G in lengths}
    res = {G: np.zeros(4, dtype=np.int64) for G in lengths}   # runs, dropped: exact / spectral / Gershgorin
    tot = drop_s = used = 0
    for s in np.random.default_rng(0).permutation(len(tets)):
        c, r = (lo[s] + hi[s]) / 2, np.linalg.norm(hi[s] - lo[s]) / 2
        box = pts[tree.query_ball_point(c, r)]
        if int(((box >= lo[s]) & (box <= hi[s])).all(1).sum()) > 800:   # the witness sweep's gate ("wit_weight")
            continue
        used += 1
        P = wp @ V[s]
        dc, ic = tree.query(P[rows_c])
        X = pts[ic].astype(np.float64)                                   # witnesses of the coarse samples
        thr_f = np.array([(dc[bits[f][rows_c]] ** 2).max() if bits[f][rows_c].any() else 0.0 for f in range(F)])
        thr = np.full(R, np.inf)
        for f in range(F):
            thr[bits[f]] = np.minimum(thr[bits[f]], thr_f[f])
        ub = ((P[:, None, :] - X[par4]) ** 2).sum(2).min(1)
        tot += R
        drop_s += int((ub <= thr).sum())
        Wc = V[s] - V[s].mean(0)
        gram = Wc.T @ Wc
        sig = np.sqrt(np.linalg.eigvalsh(gram).max())
        ger = np.sqrt(np.abs(gram).sum(1).max())
        for G in lengths:
            n = R // G
            Pg = P[:n * G].reshape(n, G, 3)
            thr_g = thr[:n * G].reshape(n, G).min(1)
            g = (Pg.min(1) + Pg.max(1)) / 2
            rho = np.sqrt(((Pg - g[:, None, :]) ** 2).sum(2).max(1))
            near = ((Pg - g[:, None, :]) ** 2).sum(2).argmin(1)
            pj = par4[:n * G].reshape(n, G, 4)[np.arange(n), near]
            dg = np.sqrt(((g[:, None, :] - X[pj]) ** 2).sum(2)).min(1)
            res[G][0] += n
            res[G][1] += int(((dg + rho) ** 2 * (1 + 1e-5) <= thr_g).sum())
            tab = tabs[G]                                                  # the table the kernel reads
            cw = tab[:, :4].view(np.float32).astype(np.float64)
            rho_w = tab[:, 6].view(np.float32).astype(np.float64)
            pt = np.stack([(tab[:, 5] >> (8 * j)) & 255 for j in range(4)], 1).astype(np.int64)
            dt = np.sqrt((((cw @ V[s])[:, None, :] - X[pt]) ** 2).sum(2)).min(1)
            res[G][2] += int(((dt + rho_w * sig) ** 2 * (1 + 1e-5) <= thr_g).sum())
            res[G][3] += int(((dt + rho_w * ger) ** 2 * (1 + 1e-5) <= thr_g).sum())
        if used >= args.simplices:
            break
    print(f"{used} simplices pass the gate; per-sample drop rate {drop_s / tot:.4f}")
    print("| run length | dropped, exact radius | table radius x spectral norm | x Gershgorin bound | work left |")
    print("|---|---|---|---|---|")
    for G in lengths:
        n, ex, sp, ge = res[G]
        left = [(n + (n - k) * G + used * (R % G)) / tot for k in (ex, sp, ge)]
        print(f"| {G} | {100 * ex / n:.0f} % | {100 * sp / n:.0f} % | {100 * ge / n:.0f} % | "
              f"{left[0]:.2f} / {left[1]:.2f} / {left[2]:.2f} |")
    print(f"({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
