"""Run test of the witness sweep (csrc/flood_wit.hip, phase 4a; table: ``core.witness_runs``), on the CPU: a float32
replica of the kernel's bound - same operations in the same order, fma emulated through float64 - must be at least the
float32 squared distance, evaluated as the kernel evaluates a pair, of EVERY member of the run to the same witness.
No tolerance: the margins the kernel states have to carry the rounding."""
import zlib

import numpy as np
import pytest
import torch

from flooder_amd import core

F32 = np.float32
RUN = core.WIT_RUN_LEN


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def combine(w, V):
    """rows of w (n, k1) times the vertices V (k1, dim): p = fma(w_j, v_j, p), j ascending, from 0 (make_sample)."""
    p = np.zeros((w.shape[0], V.shape[1]), F32)
    for j in range(V.shape[0]):
        for k in range(V.shape[1]):
            p[:, k] = fma(w[:, j], V[j, k], p[:, k])
    return p


def dist2(p, x):
    """squared distance as every kernel of the sweep evaluates a pair: (p0 - x0)^2, then one fma per further axis"""
    t = (p[..., 0] - x[..., 0]).astype(F32)
    d2 = (t * t).astype(F32)
    for k in range(1, p.shape[-1]):
        t = (p[..., k] - x[..., k]).astype(F32)
        d2 = fma(t, t, d2)
    return d2


def sigma_and_abs(V):
    """phase 1 of the kernel: bound of the centred vertex matrix's spectral norm, absolute rounding term"""
    k1, dim = V.shape
    c = np.zeros(dim, F32)
    for k in range(dim):
        for j in range(k1):
            c[k] = F32(c[k] + V[j, k])
        c[k] = F32(c[k] / F32(k1))
    wn = np.zeros((4, dim), F32)
    wn[:k1] = (V - c[None, :]).astype(F32)
    sc = F32(np.abs(wn).max())
    with np.errstate(all="ignore"):
        inv = F32(F32(1.0) / sc)
        ws = (wn * inv).astype(F32)
        sig2 = F32(0.0)
        for k in range(dim):
            row = F32(0.0)
            for m in range(dim):
                g = F32(0.0)
                for j in range(4):
                    g = fma(ws[j, k], ws[j, m], g)
                row = F32(row + np.abs(g))
            sig2 = np.fmax(sig2, row)    # (fmaxf: a NaN operand is dropped)
        if sc >= F32(1e-30):
            sigma = F32(F32(np.sqrt(sig2) * sc) * F32(1.00001))
        else:
            sigma = F32(0.0) if sc == 0 else F32(np.inf)
    amax = F32(np.abs(V).max())
    epsb = F32(F32(8.0) * F32(1.1920929e-7) * amax)
    return sigma, F32(F32(2.0) * epsb)


def run_bound(tab, V, x):
    """phase 4a: the bound of every run (rows of ``tab``) against the witnesses x (n_runs, n_x, dim)"""
    k1, dim = V.shape
    cw = tab[:, :4].view(F32)
    rho = tab[:, 6].view(F32)
    sigma, a_abs = sigma_and_abs(V)
    g = combine(cw[:, :k1], V)
    with np.errstate(all="ignore"):
        dg2 = dist2(g[:, None, :], x)
        t = (np.sqrt(dg2).astype(F32) + fma(rho, sigma, a_abs)[:, None]).astype(F32)
        b = ((t * t).astype(F32) * F32(1.000004)).astype(F32)
        b = np.where(b < F32(1e-30), F32(np.inf), b)
    return b


TABLE_NAMES = ["grid12_2d", "grid30_2d", "grid12_3d", "grid30_3d", "uniform_3d", "uniform_2d"]
_TABLES = {}


def table(name):
    """(weights, face rows) of a named table; the random ones are drawn with the global generator's state put back
    (nothing here may shift the random numbers other tests of the session see)"""
    if name not in _TABLES:
        if name.startswith("grid"):
            ppe, dim = int(name[4:6]), int(name[7])
            w, _, fi = core.generate_grid(ppe, dim, torch.device("cpu"), torch.float32)
        else:
            dim, n, seed = (3, 3000, 11) if name == "uniform_3d" else (2, 1000, 12)
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                w, fi = core.generate_uniform_weights(n, dim, torch.device("cpu"), torch.float32), None
        _TABLES[name] = (w, fi)
    return _TABLES[name]


def plan_of(w, fi):
    faces = core._FaceTable(fi, w.shape[0], torch.device("cpu"))
    plan = core.SamplePlan(w, faces)
    w_perm = plan.w_perm.numpy()
    memb = plan.memb_all.numpy().view(np.uint32)
    wp = core.witness_plan(w, plan._perm)
    parents = wp[1] if wp is not None else np.zeros(w.shape[0], np.uint32)   # (tables too small for the kernel)
    tab = core.witness_runs(w_perm, memb, parents)
    assert tab is not None
    return w_perm, memb, parents, tab


def simplices(dim, rng):
    """(label, vertices): regular-ish, random, slivers of 1e-6 of a regular simplex's volume, edge lengths from 1e-12
    to 1e12, clouds offset by 1e3 (and 1e6) from the origin, degenerate ones"""
    k1 = dim + 1
    reg = (np.eye(k1) - 1.0 / k1) @ np.linalg.qr((np.eye(k1) - 1.0 / k1).T)[0][:, :dim]   # edge sqrt(2), centred
    out = []
    for scale in (1.0, 1e-3, 1e-6, 1e-12, 1e-25, 1e3, 1e6, 1e12, 1e25):
        for off in (0.0, 1e3, -1e3, 1e6):
            for kind in ("regular", "random", "sliver", "needle"):
                q = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
                if kind == "regular":
                    v = reg
                elif kind == "random":
                    v = rng.standard_normal((k1, dim))
                elif kind == "sliver":   # one direction squashed: volume 1e-6 of the regular simplex's
                    v = reg * np.array([1.0] * (dim - 1) + [1e-6])[None, :]
                else:                    # all but one direction squashed
                    v = reg * np.array([1.0] + [1e-4] * (dim - 1))[None, :]
                v = (v @ q) * scale + off * np.sign(rng.standard_normal(dim))[None, :]
                out.append((f"{kind} scale {scale:g} offset {off:g}", v.astype(F32)))
    out.append(("one point", np.full((k1, dim), 3.25, F32)))
    out.append(("origin", np.zeros((k1, dim), F32)))
    return out


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_run_table_describes_its_members(name):
    w, fi = table(name)
    w_perm, memb, parents, tab = plan_of(w, fi)
    R, k1 = w_perm.shape
    n = R // RUN
    assert tab.shape == (n, 8) and tab.dtype == np.uint32 and n > 0
    wm = w_perm.astype(np.float64)[:n * RUN].reshape(n, RUN, k1)
    cw = tab[:, :4].view(F32).astype(np.float64)
    assert (cw >= 0).all() and (cw[:, k1:] == 0).all()
    assert np.abs(cw.sum(axis=1) - 1.0).max() <= 0.5 * core.WIT_RUN_SUM_TOL     # centre weights sum to 1 (float32 rows)
    assert np.abs(w_perm.astype(np.float64).sum(axis=1) - 1.0).max() <= 0.5 * core.WIT_RUN_SUM_TOL
    assert (tab[:, 4] == np.bitwise_or.reduce(memb[:n * RUN].reshape(n, RUN), axis=1)).all()   # OR of the members' masks
    rho = tab[:, 6].view(F32).astype(np.float64)
    d = np.sqrt(((wm - cw[:, None, :k1]) ** 2).sum(axis=2))
    assert (d <= rho[:, None]).all()                         # rho covers every member, in float64
    assert (rho <= d.max(axis=1) * (1 + 1e-6) + 1e-30).all()  # ... and is not padded
    # 2-norm of a weight difference = distance in the regular-simplex embedding witness_plan uses
    corners = np.eye(k1) - 1.0 / k1
    emb = corners @ np.linalg.qr(corners.T)[0][:, :k1 - 1]
    de = np.sqrt((((wm - cw[:, None, :k1]) @ emb) ** 2).sum(axis=2))
    assert np.abs(de - d).max() < 1e-6
    # the parent word is one of the members' own
    pm = parents[:n * RUN].reshape(n, RUN)
    assert (pm == tab[:, 5][:, None]).any(axis=1).all()
    assert (tab[:, 7] == 0).all()


def test_no_table_where_the_analysis_does_not_hold():
    w, _, fi = core.generate_grid(30, 3, torch.device("cpu"), torch.float32)
    w_perm, memb, parents, tab = plan_of(w, fi)
    bad = w_perm.copy()
    bad[5] *= F32(1.001)                                      # a row that does not sum to 1
    assert core.witness_runs(bad, memb, parents) is None
    neg = w_perm.copy()
    neg[7, 0], neg[7, 1] = F32(-0.25), F32(neg[7, 1] + neg[7, 0] + 0.25)
    assert core.witness_runs(neg, memb, parents) is None      # negative weights
    assert core.witness_runs(np.full((64, 5), 0.2, F32), np.zeros(64, np.uint32), np.zeros(64, np.uint32)) is None
    assert core.witness_runs(w_perm[:5], memb[:5], parents[:5]) is None   # not one whole run


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_run_bound_covers_every_member_in_float32(name):
    w, fi = table(name)
    w_perm, memb, parents, tab = plan_of(w, fi)
    R, k1 = w_perm.shape
    dim = k1 - 1
    n = R // RUN
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    worst = np.inf
    checked = 0
    for label, V in simplices(dim, rng):
        p = combine(w_perm[:n * RUN], V).reshape(n, RUN, dim)
        ext = float(np.abs(V.astype(np.float64) - V.astype(np.float64).mean(axis=0)).max())
        # witnesses: around the run at several distances, far away, and a member itself (distance 0 to it)
        base = p[:, rng.integers(0, RUN), :].astype(np.float64)
        xs = [base + rng.standard_normal((n, dim)) * ext * s for s in (0.0, 1e-3, 0.05, 0.5, 3.0, 100.0)]
        xs.append(rng.standard_normal((n, dim)) * max(ext, 1e-30) * 10.0)
        x = np.stack(xs, axis=1).astype(F32)                  # (n, n_x, dim)
        with np.errstate(all="ignore"):
            b = run_bound(tab, V, x)                          # (n, n_x)
            d2 = dist2(p[:, :, None, :], x[:, None, :, :])    # (n, RUN, n_x)
        ok = b[:, None, :] >= d2                              # (NaN bound: the kernel keeps the run - counted as covered)
        ok |= np.isnan(b)[:, None, :]
        assert ok.all(), (f"{name}, simplex '{label}': the bound of {int((~ok).any(axis=(1, 2)).sum())} runs is below a "
                          f"member's distance; worst ratio {float(np.nanmin(np.where(ok, np.inf, b[:, None, :] / d2))):.9f}")
        fin = np.isfinite(b)[:, None, :] & (d2 > 0)
        if fin.any():
            with np.errstate(all="ignore"):
                worst = min(worst, float((b[:, None, :].astype(np.float64) / d2)[fin].min()))
        checked += ok.size
    print(f"{name}: {checked} (member, witness) pairs, smallest bound / distance {worst:.9f}")
    assert checked > 0


def test_bound_is_useful_on_a_plain_simplex():
    """not only safe: on a well-shaped simplex the bound of a run stays within a lattice step or two of its members'
    distances (a bound of +inf everywhere would pass the test above)"""
    w, _, fi = core.generate_grid(30, 3, torch.device("cpu"), torch.float32)
    w_perm, memb, parents, tab = plan_of(w, fi)
    n = w_perm.shape[0] // RUN
    V = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.9, 0], [0.5, 0.3, 0.8]], F32)
    x = np.broadcast_to(np.array([0.4, 0.3, 2.5], F32), (n, 1, 3))
    b = np.sqrt(run_bound(tab, V, x)[:, 0].astype(np.float64))
    p = combine(w_perm[:n * RUN], V).reshape(n, RUN, 3)
    far = np.sqrt(dist2(p, x).astype(np.float64)).max(axis=1)
    assert np.isfinite(b).all() and (b >= far).all() and (b - far).max() < 0.25
