"""CPU estimate of what the cell sweep's leaf cull can drop (csrc/flood_planes.hpp: node_meets_slabs): of the leaves
whose box overlaps a chunk's box grown by the cell size c, how many also meet all DIM + 1 slabs of the chunk grown by c?

Set-up: a Gaussian cloud in the index's Hilbert order with 16-point leaves (tests/index_reference.py), the Delaunay
tetrahedra of FPS landmarks, a spread of the heavy tetrahedra (more than 800 points in the bounding box), their chunks of 256 samples in
core.sample_order order, c = 1.35 h with h = (box volume / points in the box)^(1/3); float64, no margins.  No GPU.

usage: python tools/gather_cull_estimate.py [n_points 1000000] [n_landmarks 1000] [n_tetrahedra 60] [points_per_edge 30]"""
import os
import sys

import numpy as np
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import index_reference as ir  # noqa: E402
from oracle import flood_oracle as fo  # noqa: E402


def main():
    n, n_l, n_tet, ppe = (int(a) for a in (sys.argv[1:5] + ["1000000", "1000", "60", "30"][len(sys.argv) - 1:]))
    import torch

    from flooder_amd import core

    pts = ir.gaussian(n, 3, 42)
    lo, hi = ir.bbox(pts)
    rows = pts[ir.curve_order(pts, lo, hi, ir.curve_bits(3))]
    leaf_lo, leaf_hi = (a.astype(np.float64) for a in ir.leaf_boxes(rows))
    n_leaves = leaf_lo.shape[0]
    rows64 = np.full((n_leaves * ir.LEAF, 3), np.inf)
    rows64[:n] = rows
    lms = pts[fo.exact_fps(pts, n_l, 0)].astype(np.float64)
    tets = Delaunay(lms).simplices
    w = fo.generate_grid(ppe, 3, np.float32)[0]
    w = w[core.sample_order(torch.as_tensor(w))].astype(np.float64)
    # heavy tetrahedra - those the witness sweep leaves to the cell sweep: more than "wit_weight" (800) points of the
    # cloud in the bounding box (counted through the leaves) - and of them n_tet, evenly spaced from the heaviest down
    weight = np.empty(len(tets))
    for i, t in enumerate(tets):
        a, b = lms[t].min(0), lms[t].max(0)
        over = np.flatnonzero((leaf_lo <= b).all(1) & (leaf_hi >= a).all(1))
        cand = rows64[np.repeat(over * ir.LEAF, ir.LEAF) + np.tile(np.arange(ir.LEAF), len(over))]
        weight[i] = ((cand >= a) & (cand <= b)).all(1).sum()
    heavy = np.argsort(-weight, kind="stable")[:int((weight > 800).sum())]
    print(f"{len(heavy)} of {len(tets)} tetrahedra hold more than 800 points in their box")
    heavy = heavy[np.linspace(0, len(heavy) - 1, min(n_tet, len(heavy))).astype(int)]
    tot = dict(chunks=0, box=0, both=0, in_box=0, kept=0)
    for t in tets[heavy]:
        v = lms[t]
        org = v[0]
        pn = np.empty((4, 3))
        po = np.empty(4)
        for f in range(4):
            idx = [j for j in range(4) if j != f]
            nrm = np.cross(v[idx[1]] - v[idx[0]], v[idx[2]] - v[idx[0]])
            nrm /= np.linalg.norm(nrm)
            pn[f], po[f] = nrm, nrm @ (v[idx[0]] - org)
        p = w @ v
        for q in range(0, p.shape[0], 256):
            ch = p[q:q + 256]
            blo, bhi = ch.min(0), ch.max(0)
            over = (leaf_lo <= bhi).all(1) & (leaf_hi >= blo).all(1)
            cand = rows64[np.repeat(np.flatnonzero(over) * ir.LEAF, ir.LEAF) + np.tile(np.arange(ir.LEAF), int(over.sum()))]
            n0 = int(((cand >= blo) & (cand <= bhi)).all(1).sum())
            if n0 == 0:
                continue
            c = 1.35 * np.cbrt(np.prod(bhi - blo) / n0)
            dd = (ch - org) @ pn.T - po
            slo, shi = dd.min(0) - c, dd.max(0) + c
            over = (leaf_lo <= bhi + c).all(1) & (leaf_hi >= blo - c).all(1)
            a, b = leaf_lo[over] - org, leaf_hi[over] - org
            smin = np.minimum(a[:, None, :] * pn[None], b[:, None, :] * pn[None]).sum(2) - po
            smax = np.maximum(a[:, None, :] * pn[None], b[:, None, :] * pn[None]).sum(2) - po
            meets = ((smin <= shi) & (smax >= slo)).all(1)
            cand = rows64[np.repeat(np.flatnonzero(over) * ir.LEAF, ir.LEAF) + np.tile(np.arange(ir.LEAF), int(over.sum()))]
            in_box = ((cand >= blo - c) & (cand <= bhi + c)).all(1)
            ddc = (cand[in_box] - org) @ pn.T - po
            kept = ((ddc <= shi) & (ddc >= slo)).all(1)
            tot["chunks"] += 1
            tot["box"] += int(over.sum())
            tot["both"] += int(meets.sum())
            tot["in_box"] += int(in_box.sum())
            tot["kept"] += int(kept.sum())
    print(f"{n} points, {n_l} landmarks, {len(heavy)} tetrahedra, {tot['chunks']} chunks")
    print(f"leaves overlapping box + c: {tot['box']}")
    print(f"leaves that also meet all four slabs + c: {tot['both']} ({100.0 * (1 - tot['both'] / max(tot['box'], 1)):.1f} % would be dropped)")
    print(f"points in the box kept by the per-point test: {100.0 * tot['kept'] / max(tot['in_box'], 1):.1f} %")
    print(f"candidates per kept point: {tot['box'] * ir.LEAF / max(tot['kept'], 1):.1f} -> {tot['both'] * ir.LEAF / max(tot['kept'], 1):.1f}")


if __name__ == "__main__":
    main()
