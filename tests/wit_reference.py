"""Float32 numpy replica of the witness sweep's margin arithmetic, shared by the CPU tests that reason with it
(test_wit_sorted_stage_cpu.py) and the GPU tests that pin the kernel to it word for word (test_gpu_plane_rows.py):
the plane table row (csrc/flood_planes.hpp: simplex_planes_row), phase 1 of wit_sweep_kernel with `Region` and `Excess`
(csrc/flood_wit.hip), the pair loops' squared distance, and the inputs both kinds of test use.

The device code switches the compiler's contraction off where these numbers are made (#pragma clang fp contract(off))
and writes every fused step as an fma, so this file mirrors the source line by line: `fma` where the source says
__builtin_fmaf, one float32 rounding per operation everywhere else."""
import itertools

import numpy as np

f32 = np.float32
NBIN = 64
U = f32(1.1920929e-7)


def _fma_round_to_odd(a, b, c):
    """1-d float64 arrays holding float32 values -> fmaf, correctly rounded: the product of two float32 is exact in
    float64; the float64 sum is brought to ROUND-TO-ODD with the error term of TwoSum (a sum that was inexact and came
    out even moves one float64 ulp towards the exact value), and a round-to-odd value of 53 >= 2 * 24 + 2 bits rounds
    to float32 as the exact sum does."""
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)   # (sign-magnitude: + 1 on the bits is one ulp away from zero for either sign)
    fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
    bits += np.where(fix, np.where(np.signbit(err) == np.signbit(s), 1, -1), 0)
    return s.astype(f32)


def fma(a, b, c):
    """fmaf(a, b, c) for float32 inputs, correctly rounded.  A float64 product (exact) and sum, rounded to float32, is
    right except where the float64 sum was inexact AND landed on the midpoint of two float32 (or in float32's
    subnormal range, where that midpoint sits elsewhere): those elements are redone by `_fma_round_to_odd`."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.asarray(a * b + c)
        out = s.astype(f32)
        if s.ndim == 0:
            return f32(_fma_round_to_odd(*(np.atleast_1d(v).copy() for v in (a, b, c)))[0])
        redo = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
        redo |= (np.abs(s) < 2.0 ** -126) & (s != 0)
        if redo.any():
            ab, bb, cb = np.broadcast_arrays(a, b, c)
            out[redo] = _fma_round_to_odd(ab[redo], bb[redo], cb[redo])
    return out


# ------------------------------------------------------------------------------------ flood_planes.hpp, one simplex
def plane_row(vs, conditions=None):
    """vs (k1, dim) float32 -> org, sext, pn (dim + 1, dim), po, ps   (simplex_planes_row).  `conditions`: a list that
    receives, per face of a full simplex, the three terms of the kernel's `ok` as a tuple of bools."""
    k1, dim = vs.shape
    org = vs[0].copy()
    sext2 = f32(0)
    for j in range(1, k1):
        e2 = f32(0)
        for k in range(dim):
            t = f32(vs[j, k] - org[k])
            e2 = fma(t, t, e2)
        sext2 = max(sext2, e2)
    sext = np.sqrt(f32(sext2))
    pn = np.zeros((dim + 1, dim), f32)
    po = np.full(dim + 1, 3.0e38, f32)
    ps = np.zeros(dim + 1, f32)
    if k1 != dim + 1:   # (a face of lower dimension: every plane disabled)
        return org, sext, pn, po, ps
    for f in range(dim + 1):
        idx = [j for j in range(dim + 1) if j != f]
        if dim == 3:
            e1 = (vs[idx[1]] - vs[idx[0]]).astype(f32)
            e2_ = (vs[idx[2]] - vs[idx[0]]).astype(f32)
            l1 = l2 = f32(0)
            for k in range(3):
                l1 = fma(e1[k], e1[k], l1)
                l2 = fma(e2_[k], e2_[k], l2)
            nrm = np.array([fma(e1[1], e2_[2], -f32(e1[2] * e2_[1])), fma(e1[2], e2_[0], -f32(e1[0] * e2_[2])),
                            fma(e1[0], e2_[1], -f32(e1[1] * e2_[0]))], f32)
            l12 = f32(l1 * l2)
        else:
            ex = f32(vs[idx[1], 0] - vs[idx[0], 0])
            ey = f32(vs[idx[1], 1] - vs[idx[0], 1])
            nrm = np.array([ey, -ex], f32)
            l12 = fma(ex, ex, f32(ey * ey))
        len2 = side = f32(0)
        for k in range(dim):
            len2 = fma(nrm[k], nrm[k], len2)
            side = fma(nrm[k], f32(vs[f, k] - vs[idx[0], k]), side)
        terms = (bool(len2 > f32(1e-30)), bool(len2 >= f32(f32(1e-8) * l12)),
                 bool(f32(side * side) >= f32(f32(f32(1e-8) * len2) * sext2)))
        if conditions is not None:
            conditions.append(terms)
        ok = all(terms)
        # (a disabled plane keeps the normal's products with sc = 0: zeros that carry the sign of nrm[k])
        sc = f32((f32(-1) if side > 0 else f32(1)) / np.sqrt(f32(len2))) if ok else f32(0)
        off = f32(0)
        for k in range(dim):
            pn[f, k] = f32(nrm[k] * sc)
            off = fma(pn[f, k], f32(vs[idx[0], k] - org[k]), off)
        if ok:
            po[f] = off
            ps[f] = f32(f32(1e-6) * np.sqrt(f32(l12 / len2)))
    return org, sext, pn, po, ps


def plane_words(vs, conditions=None):
    """the 24 float32 words of the table row (layout of simplex_planes_row)"""
    dim = vs.shape[1]
    org, sext, pn, po, ps = plane_row(vs, conditions)
    row = np.zeros(24, f32)
    row[:dim] = org
    row[3] = sext
    for f in range(dim + 1):
        row[4 + 5 * f:4 + 5 * f + dim] = pn[f]
        row[4 + 5 * f + 3] = po[f]
        row[4 + 5 * f + 4] = ps[f]
    return row


# ------------------------------------------------------------------------------------ flood_wit.hip
class Region:
    """phase 1 of wit_sweep_kernel + struct Region + struct Excess, for one simplex and one c_max"""

    def __init__(self, vs, cmax_frac, excess_pad=2.0):   # (EXCESS_PAD of flood_wit.hip)
        self.vs = vs
        k1, dim = vs.shape
        self.dim = dim
        self.org, self.sext, self.pn, self.po, ps = plane_row(vs)
        self.ps = (ps + f32(1e-6)).astype(f32)
        self.blo, self.bhi = vs.min(0), vs.max(0)
        self.slo = np.full(dim + 1, np.inf, f32)
        self.shi = np.full(dim + 1, -np.inf, f32)
        for j in range(k1):
            dd = self.plane_dd(vs[j][None, :])[:, 0]
            self.slo = np.minimum(self.slo, dd)
            self.shi = np.maximum(self.shi, dd)
        self.epsb = f32(f32(f32(8) * U) * np.abs(vs).max())
        ext = (self.bhi - self.blo).max()
        self.c_max = f32(f32(cmax_frac) * ext)
        self.bin_scale = f32(f32(NBIN) / self.c_max)
        # Excess
        pad = f32(excess_pad)
        self.blo_e = fma(-f32(f32(1) + pad), self.epsb, self.blo)
        self.bhi_e = fma(f32(f32(1) + pad), self.epsb, self.bhi)
        tol = fma(self.ps, f32(self.sext + self.c_max), f32(pad * self.epsb))
        self.slo_t = (self.slo - tol).astype(f32)
        self.shi_t = (self.shi + tol).astype(f32)
        self.inv_den = (f32(1) / (f32(1.001) + self.ps)).astype(f32)

    def plane_dd(self, x):
        """(dim + 1, n): dd of every plane for points x (n, dim)"""
        xr = (x - self.org[None, :]).astype(f32)
        out = np.empty((self.dim + 1, x.shape[0]), f32)
        for f in range(self.dim + 1):
            dd = np.full(x.shape[0], -self.po[f], f32)
            for k in range(self.dim):
                dd = fma(self.pn[f, k], xr[:, k], dd)
            out[f] = dd
        return out

    def excess(self, x):
        e = np.zeros(x.shape[0], f32)
        for k in range(self.dim):
            e = np.maximum(e, np.maximum((x[:, k] - self.bhi_e[k]).astype(f32), (self.blo_e[k] - x[:, k]).astype(f32)))
        dd = self.plane_dd(x)
        for f in range(self.dim + 1):
            v = np.maximum((dd[f] - self.shi_t[f]).astype(f32), (self.slo_t[f] - dd[f]).astype(f32))
            e = np.maximum(e, (v * self.inv_den[f]).astype(f32))
        return e

    def slack(self, p):
        dl = np.full(p.shape[0], np.inf, f32)
        for k in range(self.dim):
            dl = np.minimum(dl, np.minimum((p[:, k] - self.blo[k]).astype(f32), (self.bhi[k] - p[:, k]).astype(f32)))
        dd = self.plane_dd(p)
        for f in range(self.dim + 1):
            if self.po[f] < f32(1.0e37):
                dl = np.minimum(dl, np.minimum((self.shi[f] - dd[f]).astype(f32), (dd[f] - self.slo[f]).astype(f32)))
        return dl

    @staticmethod
    def limit(dl, c, factor=0.999):
        rr = (f32(factor) * (c + np.maximum(dl, f32(0))).astype(f32)).astype(f32)
        return (rr * rr).astype(f32)

    def samples(self, per_edge=5):
        """lattice samples as make_sample builds them: p = fma chain over the vertices"""
        k1 = self.vs.shape[0]
        n = per_edge - 1
        rows = [c for c in itertools.product(range(n + 1), repeat=k1) if sum(c) == n]
        w = (np.array(rows, f32) / f32(n)).astype(f32)
        p = np.zeros((w.shape[0], self.dim), f32)
        for j in range(k1):
            for k in range(self.dim):
                p[:, k] = fma(w[:, j], self.vs[j, k], p[:, k])
        return p


def pair_d2(p, x):
    """(n_p, n_x) squared distances in the order of the kernel's pair loops"""
    t = (p[:, None, 0] - x[None, :, 0]).astype(f32)
    d2 = (t * t).astype(f32)
    for k in range(1, p.shape[1]):
        t = (p[:, None, k] - x[None, :, k]).astype(f32)
        d2 = fma(t, t, d2)
    return d2


# ------------------------------------------------------------------------------------ inputs
def simplices(dim):
    rng = np.random.default_rng(100 + dim)
    out = []
    for i in range(6):
        out.append((f"random {i}", rng.standard_normal((dim + 1, dim)).astype(f32)))
    for i in range(4):   # slivers: one edge 1e-3 of the others
        v = rng.standard_normal((dim + 1, dim)).astype(f32)
        v[1] = v[0] + f32(1e-3) * (v[1] - v[0])
        out.append((f"sliver {i}", v.astype(f32)))
    flat = rng.standard_normal((dim + 1, dim)).astype(f32)
    flat[dim] = flat[:dim].mean(0) + f32(1e-4) * rng.standard_normal(dim).astype(f32)   # a vertex almost on the opposite face
    out.append(("flat", flat.astype(f32)))
    unit = np.vstack([np.zeros(dim), np.eye(dim)]).astype(f32)   # axis-parallel: box sides ARE faces
    out.append(("unit", unit))
    out.append(("unit, dyadic", (unit * f32(0.25) + f32(0.5)).astype(f32)))
    for name, v in list(out):
        out.append((name + ", offset 1e3", (v + f32(1e3)).astype(f32)))
    return out


def points(rg, rng, n=3000):
    dim = rg.dim
    vs = rg.vs
    ext = (rg.bhi - rg.blo).max()
    grow = f32(1.3) * rg.c_max + f32(0.05) * ext
    pts = [rng.uniform(rg.blo - grow, rg.bhi + grow, (n, dim)).astype(f32)]
    # on the polytope: vertices, samples, points of the faces
    w = rng.dirichlet(np.ones(dim + 1), 400).astype(f32)
    w[:200, 0] = 0
    w[:200] /= w[:200].sum(1, keepdims=True)
    pts += [vs, rg.samples(), (w @ vs).astype(f32)]
    # exactly on bin boundaries (and one float to either side): straight out of every box side from vertices and
    # samples, and out of every face plane from points of that face
    base = np.vstack([vs, rg.samples()])
    ks = np.arange(0, NBIN + 1, dtype=f32)
    for k in range(dim):
        for sign, side in ((1, rg.bhi_e[k]), (-1, rg.blo_e[k])):
            tgt = (side + f32(sign) * (ks / rg.bin_scale).astype(f32)).astype(f32)
            for t in (tgt, np.nextafter(tgt, f32(np.inf)), np.nextafter(tgt, f32(-np.inf))):
                for b in base[:: max(1, len(base) // 12)]:
                    x = np.repeat(b[None, :], len(t), 0)
                    x[:, k] = t
                    pts.append(x)
    for f in range(dim + 1):
        if not rg.po[f] < f32(1.0e37):
            continue
        face = np.delete(vs, f, 0)
        on = np.vstack([face, face.mean(0, keepdims=True).astype(f32)])
        for c in (ks / rg.bin_scale).astype(f32):
            for scale in (f32(1), f32(1.0000005), f32(1.001)):
                pts.append((on + (c * scale) * rg.pn[f][None, :]).astype(f32))   # (pn points away from the simplex)
    x = np.vstack(pts).astype(f32)
    return x[np.isfinite(x).all(1)]


