"""Float32 numpy replica of the cell sweep's leaf cull (csrc/flood_planes.hpp: node_meets_slabs) and of the slab part of
its per-point test (csrc/flood_cell.hip: keep_point), in the style of wit_reference.py: `fma` where the source says
__builtin_fmaf, one float32 rounding per operation everywhere else (the device code runs with contraction off)."""
import itertools

import numpy as np

from wit_reference import f32, fma, plane_row

PAD_REL = f32(2.0 ** -20)   # GATHER_PAD_REL
PAD_ABS = f32(1.0e-36)      # GATHER_PAD_ABS


def plane_dd(x, pn, po, org):
    """(n, dim + 1): keep_point's dd of every plane for the points x (n, dim)"""
    xr = (x - org[None, :]).astype(f32)
    out = np.empty((x.shape[0], pn.shape[0]), f32)
    for f in range(pn.shape[0]):
        dd = np.full(x.shape[0], -po[f], f32)
        for k in range(x.shape[1]):
            dd = fma(pn[f, k], xr[:, k], dd)
        out[:, f] = dd
    return out


def keeps(dd, slab_lo, slab_hi):
    """keep_point's slab test (its box test left out: what it keeps here is a superset of what the kernel keeps)"""
    return ((dd <= slab_hi) & (dd >= slab_lo)).all(axis=1)


def node_meets_slabs(lo, hi, pn, po, org, slab_lo, slab_hi, pad_rel=PAD_REL, pad_abs=PAD_ABS):
    """node_meets_slabs for boxes lo, hi (n, dim); slab limits (dim + 1,) or one row per box (n, dim + 1)"""
    n, dim = lo.shape
    slab_lo = np.broadcast_to(np.asarray(slab_lo, f32), (n, dim + 1))
    slab_hi = np.broadcast_to(np.asarray(slab_hi, f32), (n, dim + 1))
    with np.errstate(invalid="ignore", over="ignore"):
        a = (lo - org[None, :]).astype(f32)
        b = (hi - org[None, :]).astype(f32)
        out = np.zeros(n, bool)
        for f in range(dim + 1):
            mag = np.full(n, np.abs(po[f]), f32)
            for k in range(dim):
                pa = (pn[f, k] * a[:, k]).astype(f32)
                pb = (pn[f, k] * b[:, k]).astype(f32)
                mn, mx = np.fmin(pa, pb), np.fmax(pa, pb)
                smin = mn if k == 0 else (smin + mn).astype(f32)
                smax = mx if k == 0 else (smax + mx).astype(f32)
                mag = (mag + np.fmax(np.abs(pa), np.abs(pb))).astype(f32)
            smin = (smin - po[f]).astype(f32)
            smax = (smax - po[f]).astype(f32)
            pad = fma(f32(pad_rel), mag, f32(pad_abs))
            out |= ((smin - pad).astype(f32) > slab_hi[:, f]) | ((smax + pad).astype(f32) < slab_lo[:, f])
    return ~out


def lattice(k1, per_edge):
    n = per_edge - 1
    rows = [c for c in itertools.product(range(n + 1), repeat=k1) if sum(c) == n]
    return (np.array(rows, f32) / f32(n)).astype(f32)


def samples(vs, w):
    """the kernel's samples: one fma per vertex"""
    p = np.zeros((w.shape[0], vs.shape[1]), f32)
    for j in range(vs.shape[0]):
        for k in range(vs.shape[1]):
            p[:, k] = fma(w[:, j], vs[j, k], p[:, k])
    return p


class Region:
    """what a work item of the cell sweep knows when it gathers with a cell size c: plane row, the box of its samples,
    their extent along every normal and the slab limits (flood_cell.hip; the products of `tol` may be contracted there -
    the property under test holds for ANY limits, these only have to be of the kernel's kind)"""

    def __init__(self, vs, p, c):
        self.vs, self.dim = vs, vs.shape[1]
        self.org, self.sext, self.pn, self.po, ps = plane_row(vs)
        self.blo, self.bhi = p.min(0), p.max(0)
        dd = plane_dd(p, self.pn, self.po, self.org)
        slo, shi = dd.min(0), dd.max(0)
        self.c = c = f32(c)
        with np.errstate(over="ignore"):
            tol = (f32(c * f32(1.001)) + ((ps + f32(1e-6)).astype(f32) * f32(self.sext + c)).astype(f32)).astype(f32)
            self.slab_lo, self.slab_hi = (slo - tol).astype(f32), (shi + tol).astype(f32)
        self.qlo, self.qhi = (self.blo - c).astype(f32), (self.bhi + c).astype(f32)

    def dd(self, x):
        return plane_dd(x, self.pn, self.po, self.org)
