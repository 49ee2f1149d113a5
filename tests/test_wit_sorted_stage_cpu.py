"""Early exit of the witness sweep's pair loops over the ordered stage (csrc/flood_wit.hip, phases 3 and 5), held to
account without tolerance: a float32 numpy replica of the plane table (flood_planes.hpp), of `Region`, `Excess`, the
binning `(int)(excess(x) * bin_scale)` and `Region::limit(slack(p), k / bin_scale)`.

The kernel leaves a pair loop at stage slot j once every sample p of the wave has a running minimum
<= limit(slack(p), k / bin_scale), k the smallest excess bin among the points from j on.  That is exact if and only if
EVERY point x of bin k or higher has an evaluated squared distance to p STRICTLY above that limit - which is what is
asserted here for every (sample, point) pair, on random and on degenerate simplices (slivers with one edge 1e-3 of the
others, coordinates offset by 1e3), with points placed exactly on bin boundaries and on the polytope's faces among the
inputs.  The same check with the kernel's factor 0.999 replaced by 1.001 must FAIL on these inputs: the test bites.
The statement is about the bins k >= 1; bin 0 - the points inside the polytope - carries no bound at all, and the
kernel never leaves a loop on it (last test).

fmaf is replayed as a float64 product (exact for float32 factors) and sum rounded to float32; every other operation
is a float32 numpy operation in the kernel's order."""
import itertools

import numpy as np
import pytest

f32 = np.float32
NBIN = 64
U = f32(1.1920929e-7)


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


# ------------------------------------------------------------------------------------ flood_planes.hpp, one simplex
def plane_row(vs):
    """vs (dim + 1, dim) float32 -> org, sext, pn (dim + 1, dim), po, ps   (simplex_planes_row)"""
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
    for f in range(dim + 1):
        idx = [j for j in range(dim + 1) if j != f]
        if dim == 3:
            e1 = (vs[idx[1]] - vs[idx[0]]).astype(f32)
            e2_ = (vs[idx[2]] - vs[idx[0]]).astype(f32)
            l1 = l2 = f32(0)
            for k in range(3):
                l1 = fma(e1[k], e1[k], l1)
                l2 = fma(e2_[k], e2_[k], l2)
            nrm = np.array([f32(e1[1] * e2_[2]) - f32(e1[2] * e2_[1]), f32(e1[2] * e2_[0]) - f32(e1[0] * e2_[2]),
                            f32(e1[0] * e2_[1]) - f32(e1[1] * e2_[0])], f32)
            l12 = f32(l1 * l2)
        else:
            ex = f32(vs[idx[1], 0] - vs[idx[0], 0])
            ey = f32(vs[idx[1], 1] - vs[idx[0], 1])
            nrm = np.array([ey, -ex], f32)
            l12 = f32(f32(ex * ex) + f32(ey * ey))
        len2 = side = f32(0)
        for k in range(dim):
            len2 = fma(nrm[k], nrm[k], len2)
            side = fma(nrm[k], f32(vs[f, k] - vs[idx[0], k]), side)
        ok = len2 > f32(1e-30) and len2 >= f32(f32(1e-8) * l12) and f32(side * side) >= f32(f32(f32(1e-8) * len2) * sext2)
        if not ok:
            continue
        sc = f32((f32(-1) if side > 0 else f32(1)) / np.sqrt(f32(len2)))
        off = f32(0)
        for k in range(dim):
            pn[f, k] = f32(nrm[k] * sc)
            off = fma(pn[f, k], f32(vs[idx[0], k] - org[k]), off)
        po[f] = off
        ps[f] = f32(f32(1e-6) * np.sqrt(f32(l12 / len2)))
    return org, sext, pn, po, ps


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
        self.blo_e = (self.blo - f32(f32(1) + pad) * self.epsb).astype(f32)
        self.bhi_e = (self.bhi + f32(f32(1) + pad) * self.epsb).astype(f32)
        tol = (self.ps * f32(self.sext + self.c_max) + f32(pad * self.epsb)).astype(f32)
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
def _simplices(dim):
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


def _points(rg, rng, n=3000):
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


def _violations(dim, factor, bins="outside"):
    """number of (sample, point) pairs whose evaluated d2 is NOT strictly above the limit of the point's bin; over the
    points of the bins k >= 1 (which violate a side of the polytope by at least k / bin_scale), or of bin 0 alone"""
    bad, pairs, boundary = 0, 0, 0
    worst = []
    for si, (name, vs) in enumerate(_simplices(dim)):
        for cmax_frac in (0.6, 0.15):
            rg = Region(vs, cmax_frac)
            x = _points(rg, np.random.default_rng(1000 * dim + si))
            eb = (rg.excess(x) * rg.bin_scale).astype(f32)
            keep = (eb < f32(NBIN)) & ((eb >= f32(1)) if bins == "outside" else (eb < f32(1)))
            x, eb = x[keep], eb[keep]
            k = eb.astype(np.int32)          # (int)eb
            boundary += int((eb == k).sum())
            c = (k.astype(f32) / rg.bin_scale).astype(f32)
            p = rg.samples()
            dl = rg.slack(p)
            lim = Region.limit(dl[:, None], c[None, :], factor)
            d2 = pair_d2(p, x)
            nb = ~(d2 > lim)
            pairs += d2.size
            if nb.any():
                bad += int(nb.sum())
                worst.append((name, cmax_frac, int(nb.sum())))
    return bad, pairs, boundary, worst


@pytest.mark.parametrize("dim", [2, 3])
def test_points_of_a_bin_are_strictly_beyond_its_limit(dim):
    bad, pairs, boundary, worst = _violations(dim, 0.999)
    print(f"dim {dim}: {pairs} pairs, {boundary} points exactly on a bin boundary, {bad} not beyond the limit {worst[:5]}")
    assert pairs > 1_000_000 and boundary > 100
    assert bad == 0, worst[:10]


@pytest.mark.parametrize("dim", [2, 3])
def test_the_check_bites_with_a_factor_above_one(dim):
    bad, pairs, _, worst = _violations(dim, 1.001)
    print(f"dim {dim}: factor 1.001: {bad} of {pairs} pairs not beyond the limit")
    assert bad > 0


@pytest.mark.parametrize("dim", [2, 3])
def test_bin_zero_carries_no_bound(dim):
    """Bin 0 holds the points INSIDE the polytope (and within c_max / 64 of it): they violate no side, and a sample's
    slack says nothing about them - a point may sit on the sample.  The kernel notes c = -inf for a group of stage slots
    that starts in bin 0, which makes the limit overflow, and an overflowed limit never lets a wave leave."""
    bad, pairs, _, _ = _violations(dim, 0.999, bins="zero")
    print(f"dim {dim}: bin 0: {bad} of {pairs} pairs within the limit a bound c = 0 would give")
    assert bad > 0
    with np.errstate(over="ignore", invalid="ignore"):
        lim = Region.limit(np.array([0.0, 0.25, 1e30], f32), f32(-np.inf))
    assert np.isinf(lim).all() and (lim > 0).all()
