"""Plain references for the weighted filtration (``flood_complex(point_weights=w)``, ``power_distance``,
``flooder_sweep_power_f32``): the float64 brute force ``min_x |p - x|^2 + w_x^2`` over ALL points, the lifted cloud
``[x, |w|]``, the weight families and the case builders of the tests.  No kernels are called here."""

import itertools

import numpy as np
import torch

from flooder_amd import core

SENTINEL = -1          # no squared value has this word: every output word must have been overwritten
GUARD = 64             # words behind every output buffer that no call may touch


# ------------------------------------------------------------------------------------------------ brute force
def brute_power(points: torch.Tensor, w: torch.Tensor, samples: torch.Tensor, chunk_elems: int = 1 << 26):
    """Per row of ``samples`` (Q, dim): (min over ALL points x of |p - x|^2 + w_x^2, the first point that attains it,
    the nearest point), float64 on the device of ``points``; d2 added axis by axis (exact on integer inputs)."""
    P, W2, Q = points.double(), w.double() ** 2, samples.double()
    n, dim = P.shape
    per = max(1, chunk_elems // n)
    val, arg, near = [], [], []
    for a in range(0, Q.shape[0], per):
        q = Q[a:a + per]
        d2 = (q[:, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for c in range(1, dim):
            d2 += (q[:, c:c + 1] - P[:, c].unsqueeze(0)) ** 2
        near.append(d2.argmin(dim=1))
        d2 += W2.unsqueeze(0)
        m = d2.min(dim=1)
        val.append(m.values)
        arg.append(m.indices)
    return torch.cat(val), torch.cat(arg), torch.cat(near)


def lifted(points: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The cloud in one more dimension: row x becomes (x, |w_x|) - |p - x|^2 + w_x^2 is the squared distance from
    (p, 0) to it."""
    return torch.cat([points, w.abs().to(points.dtype).unsqueeze(1)], dim=1).contiguous()


def with_zero_column(x: torch.Tensor) -> torch.Tensor:
    return torch.cat([x, x.new_zeros(x.shape[:-1] + (1,))], dim=-1).contiguous()


def samples_of(verts: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """(S * R, dim) float64 samples p[s, r] = sum_j weights[r, j] verts[s, j]."""
    return torch.einsum("rk,skd->srd", weights.double(), verts.double()).reshape(-1, verts.shape[-1])


def brute_filtration(fc, points, w, landmarks, points_per_edge=None, weights_by_dim=None):
    """The value of every simplex of the dict ``fc`` from the brute force: the maximum of the power distance over the
    lattice of the simplex's own dimension (``core.generate_grid``) or over the drawn weights ``weights_by_dim[d]``,
    then the monotone pass over the faces (the form of ``test_knn_flood_cpu.brute_filtration``)."""
    by_dim = {}
    for key in fc:
        by_dim.setdefault(len(key) - 1, []).append(key)
    ref = {}
    for d in sorted(by_dim):
        keys = by_dim[d]
        if weights_by_dim is not None:
            bw = weights_by_dim[d]
        elif d == 0:
            bw = torch.ones((1, 1), dtype=points.dtype)     # a vertex is its own single sample
        else:
            bw = core.generate_grid(points_per_edge, d, "cpu", points.dtype)[0]
        verts = landmarks.double()[torch.tensor(keys, dtype=torch.long)]            # (S, d+1, dim)
        g = brute_power(points, w, samples_of(verts, bw))[0].sqrt().reshape(len(keys), -1)
        for key, v in zip(keys, g.max(dim=1).values.tolist()):
            for face in itertools.combinations(key, d) if d > 0 else ():
                v = max(v, ref[face])
            ref[key] = v
    return ref


# ------------------------------------------------------------------------------------------------ weight families
FAMILIES = ("zero", "constant", "mixed", "beacons", "heavy")
CONSTANT = 0.375       # 0.375^2 = 0.140625 = 9 / 64


def diameter_bound(P: np.ndarray) -> float:
    """The diagonal of the bounding box: at least the cloud's diameter."""
    return float(np.sqrt(((P.max(0) - P.min(0)).astype(np.float64) ** 2).sum()))


def median_nn_distance(P: np.ndarray) -> float:
    from scipy.spatial import KDTree

    if P.shape[0] < 2:
        return 1.0
    d, _ = KDTree(P).query(P, k=2)
    return float(np.median(d[:, 1]))


def weight_family(name: str, P: np.ndarray, rng, integer: bool = False) -> np.ndarray:
    """(n,) float64 weights of a family for the cloud ``P``; ``integer``: whole numbers (the exact lattice oracle).
    zero; constant 0.375 (3 on integers); mixed: uniform on [0, 2 x the median nearest-neighbour distance] (integers
    0..3); beacons: 10 x the diameter except (up to) three points with w = 0; heavy: all above the diameter."""
    n = P.shape[0]
    diam = max(diameter_bound(P), 1.0)
    if name == "zero":
        return np.zeros(n)
    if name == "constant":
        return np.full(n, 3.0 if integer else CONSTANT)
    if name == "mixed":
        return rng.integers(0, 4, size=n).astype(np.float64) if integer else rng.uniform(0.0, 2.0 * median_nn_distance(P), size=n)
    if name == "beacons":
        w = np.full(n, float(np.ceil(10.0 * diam)))
        w[rng.choice(n, size=min(3, n), replace=False)] = 0.0
        return w
    if name == "heavy":
        base = float(np.ceil(diam)) + 1.0
        return base + (rng.integers(0, 3, size=n).astype(np.float64) if integer else rng.uniform(0.0, 1.0, size=n))
    raise KeyError(name)


def tree_levels(n: int) -> int:
    leaves, lv = (n + 15) // 16, 1
    while leaves > 64:
        leaves, lv = (leaves + 63) // 64, lv + 1
    return lv


def node_min_reference(leaf_vals: np.ndarray, n: int) -> np.ndarray:
    """numpy form of ``flooder_node_min_f32``: levels of ``make_levels(n)``, each padded to x64 with +inf."""
    count = max(1, (n + 15) // 16)
    level = leaf_vals[:count * 16].reshape(count, 16).min(axis=1)
    out = []
    while True:
        padded = np.full((count + 63) // 64 * 64, np.inf, dtype=np.float32)
        padded[:count] = level
        out.append(padded)
        if count <= 64:
            break
        level = padded.reshape(-1, 64).min(axis=1)
        count = (count + 63) // 64
    return np.concatenate(out)
