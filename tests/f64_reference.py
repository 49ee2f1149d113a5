"""Inputs for the float64 device route (``csrc/flood_f64.hip``) on coordinates float32 cannot hold, and the checks that
make such an input worth running - all from the inputs and the float64 brute force of ``grad_reference`` alone,
nothing of the kernels.

The exact family: every coordinate is ``off + i * 2**-10`` with ``off = +-2**20`` per axis and ``i`` a small integer, the
lattice step 1/(n-1) is a power of two.  Counted in units of ``2**-10 / (n-1)`` every coordinate, every product
weight x coordinate, every partial sum of a sample, every difference, every square and every partial sum of a squared
distance is an integer below 2**53: double arithmetic is exact whatever the order of the operations
(``assert_exact_inputs_f64``), so the brute force gives THE minimum and the kernel's words compare bit for bit.
float32 holds next to none of these coordinates (its ulp at 2**20 is 0.125 = 128 steps of 2**-10).
"""

import numpy as np
import torch

OFFSET = 2.0 ** 20            # magnitude of every axis offset: the coordinates straddle a power of two
GRID = 2.0 ** -10             # coordinate step of the exact family
ULP32_AT_OFFSET = 0.125       # float32 ulp in [2**20, 2**21)
U64 = 2.0 ** -53              # unit roundoff of float64


def tree_levels(n: int) -> int:
    """Levels of the box tree over n points: leaves of 16, fan-out 64."""
    leaves, lv = (n + 15) // 16, 1
    while leaves > 64:
        leaves, lv = (leaves + 63) // 64, lv + 1
    return lv


def axis_offsets(dim: int, rng) -> np.ndarray:
    """+-2**20 per axis: axis 0 positive, axis 1 negative, the others drawn."""
    sign = rng.choice([-1.0, 1.0], size=dim)
    sign[0], sign[1] = 1.0, -1.0
    return sign * OFFSET


def exact_case(dim: int, n: int, dup: bool, d: int, n_s: int, spread: int, seed: int):
    """(points (n, dim), vertices (n_s, d+1, dim), offsets (dim,)) float64: ``off + i * 2**-10``, i uniform in
    [-spread, spread]; ``dup``: every point of the cloud occurs twice; the first quarter of the simplices has its
    vertices on points of the cloud."""
    rng = np.random.default_rng(seed)
    off = axis_offsets(dim, rng)
    if dup:
        base = rng.integers(-spread, spread + 1, size=((n + 1) // 2, dim))
        I = np.concatenate([base, base])[:n][rng.permutation(n)]
    else:
        I = rng.integers(-spread, spread + 1, size=(n, dim))
    J = rng.integers(-spread, spread + 1, size=(n_s, d + 1, dim))
    J[: n_s // 4] = I[rng.integers(0, n, size=(n_s // 4, d + 1))]
    return off + I * GRID, off + J * GRID, off


def inexact_cloud(dim: int, n: int, off: np.ndarray, seed: int) -> np.ndarray:
    """``randn * 1e-3 + off``: doubles with full mantissas around the same offsets."""
    return np.random.default_rng(seed).standard_normal((n, dim)) * 1e-3 + off


def assert_exact_inputs_f64(points, verts, points_per_edge: int) -> int:
    """Points and vertices are multiples of 2**-10, the lattice step is a power of two, and in units of
    ``2**-10 / (points_per_edge - 1)`` every coordinate (hence every product weight x coordinate and every partial sum
    of a sample: the weights are non-negative and sum to 1) and the largest squared distance between a sample and a
    point, summed over the axes, stay below 2**53.  The samples lie in the bounding box of the vertices.  Returns the
    bound on the squared distances (units squared)."""
    P = np.asarray(points, dtype=np.float64)
    V = np.asarray(verts, dtype=np.float64).reshape(-1, P.shape[1])
    step = points_per_edge - 1
    assert step >= 1 and step & (step - 1) == 0, "points_per_edge - 1 must be a power of two"
    for A in (P, V):   # (scaling by a power of two is exact)
        assert np.array_equal(A / GRID, np.round(A / GRID)), "coordinates must be multiples of 2**-10"
    assert max(np.abs(P).max(), np.abs(V).max()) / GRID * step < 2 ** 53
    far = np.maximum(V.max(0) - P.min(0), P.max(0) - V.min(0)) / GRID * step        # per axis max |q - p|, in units
    assert (far >= 0).all() and far.max() < 2 ** 26
    bound = int((far ** 2).sum())
    assert bound < 2 ** 53, f"squared distances reach {bound} units: not exact in float64"
    return bound


def float32_survivors(points) -> float:
    """Share of the coordinates that a round trip through float32 leaves unchanged."""
    P = np.asarray(points, dtype=np.float64)
    return float((P.astype(np.float32).astype(np.float64) == P).mean())


def assert_float32_cannot_hold(points, limit: float = 0.05) -> float:
    share = float32_survivors(points)
    assert share <= limit, f"{share:.1%} of the coordinates are float32 numbers: the case does not leave float32"
    return share


def assert_neighbours_below_ulp(d2_ref) -> float:
    """The median true nearest-neighbour distance of the samples (float64 brute force) is below the float32 ulp at the
    offset: rounding the cloud to float32 moves the points by as much as the distances that are measured."""
    med = float(np.sqrt(np.median(np.asarray(d2_ref, dtype=np.float64))))
    assert med < ULP32_AT_OFFSET, f"median nearest-neighbour distance {med:.4f} is not below the float32 ulp 0.125"
    return med


def assert_leaves_need_widening(rows64: torch.Tensor, nodes: torch.Tensor, n: int, dim: int, need: float = 0.5) -> float:
    """``rows64`` (>= n, >= dim): the float64 rows in the order of the index; ``nodes``: the index's node array, leaves
    first, (lo[DP], hi[DP]) per node.  For every real leaf (16 consecutive rows) the box B the index stores must be the
    box of the float32-rounded rows, every float64 row must lie inside B widened by one float32 ulp per side
    (``np.nextafter``) - the premise of the float64 sweep - and at least ``need`` of the leaves must hold a float64 row
    strictly outside B: without the widening the box is no bound there.  Returns that share."""
    dp = nodes.shape[1] // 2
    leaves = (n + 15) // 16
    rows = rows64[:n, :dim].double()
    if leaves * 16 > n:      # fill the last leaf with copies of its last row: same box, same verdicts
        rows = torch.cat([rows, rows[-1:].expand(leaves * 16 - n, dim)])
    rows = rows.reshape(leaves, 16, dim)
    r32 = rows.to(torch.float32)
    lo, hi = nodes[:leaves, :dim], nodes[:leaves, dp:dp + dim]
    assert torch.equal(lo, r32.min(dim=1).values) and torch.equal(hi, r32.max(dim=1).values), \
        "leaf boxes of the index are not the boxes of the float32-rounded rows"
    lo_np, hi_np = lo.cpu().numpy(), hi.cpu().numpy()
    wide_lo = torch.as_tensor(np.nextafter(lo_np, np.float32(-np.inf)).astype(np.float64), device=rows.device)
    wide_hi = torch.as_tensor(np.nextafter(hi_np, np.float32(np.inf)).astype(np.float64), device=rows.device)
    inside = (rows >= wide_lo.unsqueeze(1)) & (rows <= wide_hi.unsqueeze(1))
    assert bool(inside.all()), "a float64 row lies outside its leaf box widened by one float32 ulp"
    outside = ((rows < lo.double().unsqueeze(1)) | (rows > hi.double().unsqueeze(1))).any(dim=2).any(dim=1)
    share = float(outside.double().mean())
    assert share >= need, f"only {share:.1%} of the leaves hold a row outside their float32 box"
    return share


def gamma(dim: int) -> float:
    """gamma_(dim+2) of float64: the relative error bound of a squared distance over ``dim`` axes - the rounded
    difference enters squared (2 u), the first square and the dim - 1 fused multiply-adds (or the dim - 1 additions of
    rounded squares) round once each on the path of any one term."""
    k = dim + 2
    return k * U64 / (1 - k * U64)


def noisy_torus_f64(n: int, seed: int, R: float = 3.0, r: float = 1.0, noise_std: float = 0.02) -> np.ndarray:
    """The noisy torus of the other tests, every step in float64."""
    rng = np.random.default_rng(seed)
    theta, phi = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    ring = R + r * np.cos(phi)
    p = np.stack((ring * np.cos(theta), ring * np.sin(theta), r * np.sin(phi)), axis=1)
    return p + rng.standard_normal(p.shape) * noise_std


def figure_eight_f64(n: int, seed: int) -> np.ndarray:
    """Two annuli (radii 0.2 to 0.3, area-uniform) around (0.3, 0.5) and (0.7, 0.5), in float64."""
    rng = np.random.default_rng(seed)
    c = np.array([[0.3, 0.5], [0.7, 0.5]])[rng.integers(0, 2, size=n)]
    rad = np.sqrt(rng.uniform(0.2 ** 2, 0.3 ** 2, size=n))
    ang = rng.uniform(0, 2 * np.pi, size=n)
    return c + np.stack((rad * np.cos(ang), rad * np.sin(ang)), axis=1)
