"""Plain references for the weighted-measure kernel (``flooder_knn_mass_f32``) and ``distance_to_weighted_measure``:
the rule of ``include/flooder_hip.h`` in float64 numpy over ascending (d2 word, id) keys - those of
``knn_wide_reference.smallest_keys``, the integer brute force in the sweep's float32 arithmetic -, the numpy replay of
its float32 ``"dtm"`` word, the derived rounding bound, and a numpy ``voxel_measure``.

No tests here; builds on ``knn_wide_reference``, which stays as it is."""

import numpy as np

INF_WORD = np.uint32(0x7F800000)
CAPACITIES = (64, 128, 256, 512, 1024)


def capacity_of(n: int) -> int:
    return next(c for c in CAPACITIES if c >= n)


def dtm_bound(count) -> np.ndarray:
    """The header's bound on the relative error of the squared ``"dtm"`` word over kk = count positions: one rounding
    per product, ceil(kk / 64) - 1 + 63 on the longest chain of additions, one each for rho, (float)tau and the division,
    one more for the second-order terms and the float64 roundings of the prefix sums - (ceil(kk / 64) + 67) * 2^-24."""
    return (np.ceil(np.asarray(count, dtype=np.float64) / 64) + 67) * 2.0 ** -24


def crossing(d2: np.ndarray, ids: np.ndarray, masses: np.ndarray, tau: float, length: int):
    """The rule over the first ``length`` columns of the ascending keys (``d2`` (Q, m) float32 words as floats, ``ids``
    (Q, m)), ``masses`` (n,) float32, all sums in float64 -> dict of
      reached (Q,) bool, count (Q,) int64 (j* + 1; ``length`` where not reached),
      kth (Q,) float64 and dtm (Q,) float64: the SQUARED statistics (+inf where not reached),
      margin (Q,) float64: min(M_j* - tau, tau - M_(j*-1)) - how far the crossing is from moving by one position."""
    d2 = np.asarray(d2[:, :length], dtype=np.float64)
    mu = np.asarray(masses, dtype=np.float64)[ids[:, :length]]
    M = np.cumsum(mu, axis=1)
    crossed = M >= tau
    reached = crossed.any(axis=1)
    j = np.argmax(crossed, axis=1)
    rows = np.arange(d2.shape[0])
    m_prev = np.where(j > 0, M[rows, np.maximum(j - 1, 0)], 0.0)
    before = np.arange(length)[None, :] < j[:, None]
    dtm = ((mu * d2 * before).sum(axis=1) + (tau - m_prev) * d2[rows, j]) / tau
    inf = np.float64(np.inf)
    return dict(reached=reached, count=np.where(reached, j + 1, length).astype(np.int64),
                kth=np.where(reached, d2[rows, j], inf), dtm=np.where(reached, dtm, inf),
                margin=np.where(reached, np.minimum(M[rows, j] - tau, tau - m_prev), inf))


def dtm_words(d2_f32: np.ndarray, ids: np.ndarray, masses: np.ndarray, tau: float, count: np.ndarray) -> np.ndarray:
    """float32 replay of the kernel's ``"dtm"`` word for REACHED rows (count = j* + 1): t_i = float32(mu_i * w_i),
    t_j* = float32(rho * w_j*) with rho = float32(tau - M_(j*-1)) (float64 prefix sum in position order - exact for
    integer masses), the strided sum of the wide kernel over kk = count positions, / float32(tau) -> (Q,) uint32."""
    out = np.empty(d2_f32.shape[0], dtype=np.uint32)
    mu_all = np.asarray(masses, dtype=np.float32)
    for q in range(d2_f32.shape[0]):
        kk = int(count[q])
        w = d2_f32[q, :kk].astype(np.float32)
        mu = mu_all[ids[q, :kk]].copy()
        mu[kk - 1] = np.float32(tau - mu[:kk - 1].astype(np.float64).sum())
        t = (mu * w).astype(np.float32)
        L = min(kk, 64)
        S = t[:L].copy()
        for base in range(64, kk, 64):
            n = min(64, kk - base)
            S[:n] = (S[:n] + t[base:base + n]).astype(np.float32)
        acc = S[0]
        for l in range(1, L):
            acc = np.float32(acc + S[l])
        out[q] = np.float32(acc / np.float32(tau)).view(np.uint32)
    return out


def voxel_measure(points: np.ndarray, cell_size: float):
    """numpy ``voxel_measure``: cell = floor((x - min x) * (1 / cell_size)) in float64, per occupied cell the float64
    mean and the count, rows ascending by cell with axis 0 most significant -> (sites float64, counts int64, cells)."""
    x = np.asarray(points, dtype=np.float64)
    lo = x.min(axis=0)
    cell = np.floor((x - lo) * (1.0 / cell_size)).astype(np.int64)
    cells, inverse, counts = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    sites = np.stack([np.bincount(inverse, weights=x[:, a], minlength=len(cells)) for a in range(x.shape[1])], axis=1)
    return sites / counts[:, None], counts, cells


_TORUS = {}


def torus_coreset():
    """The inputs of the stability test, shared with the GPU tests (computed once, left unchanged): a 20 000-point noisy
    torus, its coreset at cell 0.1, every tenth point as a query, mass 0.02 (k = 400 points)."""
    if not _TORUS:
        import torch

        import flooder_amd as fa

        pts = fa.generate_noisy_torus_points_3d(20_000, seed=1).to(torch.float32)
        sites, mu = fa.voxel_measure(pts, 0.1)
        _TORUS.update(points=pts, sites=sites, masses=mu, queries=pts[::10].contiguous(), mass=0.02, cell=0.1)
    return _TORUS
