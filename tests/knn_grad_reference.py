"""Plain references for ``flood_filtration(neighbors=k)``: brute force over all points (int64 keys for the kernel-level
search, float64 for the end-to-end checks), no kd-tree, no box tree, nothing of ``flooder_amd.grad``; and the float64
closed-form gradient of the two statistics with the error bound of a float32 evaluation of the same formula.

Builds on ``grad_reference`` (lattice, exactness check of the inputs), which stays as it is.
"""

import math

import numpy as np
import torch

import grad_reference as gr

EPS32 = gr.EPS32
KS = (1, 2, 3, 5, 8, 16, 17, 32)
ID_BITS = 23          # ids below 2**23 (8.4 M points), d2 in integer units below 2**24: the key fits 47 bits


# ------------------------------------------------------------------------------------------------ kernel level
def smallest_keys_int(P2: torch.Tensor, Q2: torch.Tensor, m: int, chunk_elems: int = 1 << 27):
    """Integer brute force: per row of Q2 the ``m`` smallest keys ``d2 * 2**23 + id`` over ALL rows of P2 (int64
    coordinates, every d2 below 2**24), ascending -> (d2 (Q, m) int64, id (Q, m) int64)."""
    n, dim = P2.shape
    assert n < (1 << ID_BITS)
    per = max(1, chunk_elems // n)
    ids = torch.arange(n, device=P2.device, dtype=torch.int64).unsqueeze(0)
    out = []
    for a in range(0, Q2.shape[0], per):
        q = Q2[a:a + per]
        d = (q[:, 0:1] - P2[:, 0].unsqueeze(0)) ** 2
        for c in range(1, dim):
            d += (q[:, c:c + 1] - P2[:, c].unsqueeze(0)) ** 2
        assert int(d.max()) < 2 ** 24
        key = d * (1 << ID_BITS) + ids
        out.append(torch.topk(key, m, dim=1, largest=False, sorted=True).values)
    key = torch.cat(out)
    return key >> ID_BITS, key & ((1 << ID_BITS) - 1)


def dtm_words(d2_f32: np.ndarray, k: int) -> np.ndarray:
    """float32 replay of the sweep's mean: the first k columns of ``d2_f32`` (ascending) added smallest first by
    sequential float32 additions, divided by float32(k) -> (Q,) float32."""
    acc = d2_f32[:, 0].astype(np.float32).copy()
    for i in range(1, k):
        acc = (acc + d2_f32[:, i]).astype(np.float32)
    return (acc / np.float32(k)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ end to end, exact
def smallest_keys_f64(points: torch.Tensor, samples: torch.Tensor, m: int, unit: int, chunk_bytes: int = 512 << 20):
    """float64 brute force on an exact input: per row of ``samples`` the ``m`` smallest (d2, id) over ALL points,
    ascending by d2 then id -> (d2 (Q, m) float64, id (Q, m) int64).  d2 is accumulated axis by axis in float64; in
    units of 1 / ``unit`` (the squared lattice step) it is an integer below 2**24 - asserted -, so (d2, id) orders as the
    int64 key d2 * unit * 2**23 + id."""
    P, S = points.double(), samples.double()
    n, dim = P.shape
    assert n < (1 << ID_BITS)
    per = max(1, chunk_bytes // (8 * n * 3))
    ids = torch.arange(n, device=P.device, dtype=torch.int64).unsqueeze(0)
    keys = []
    for a in range(0, S.shape[0], per):
        s = S[a:a + per]
        d2 = (s[:, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for c in range(1, dim):
            d2 += (s[:, c:c + 1] - P[:, c].unsqueeze(0)) ** 2
        d2 *= unit
        du = d2.round().long()
        assert bool((du.double() == d2).all()) and int(du.max()) < 2 ** 24
        keys.append(torch.topk(du * (1 << ID_BITS) + ids, m, dim=1, largest=False, sorted=True).values)
    key = torch.cat(keys)
    return (key >> ID_BITS).double() / unit, key & ((1 << ID_BITS) - 1)


def statistic_f32(d2: torch.Tensor, k: int, stat: str) -> torch.Tensor:
    """The squared statistic in the sweep's arithmetic from the (Q, >= k) ascending d2 (exact in float32 on exact
    inputs): the k-th, or the sequential float32 sum of the first k over float32(k) - replayed in numpy on the host."""
    d = d2[:, :k].to(torch.float32)
    if stat == "kth":
        return d[:, -1].clone()
    return torch.as_tensor(dtm_words(d.cpu().numpy(), k), device=d2.device)


class ExactKnnFace:
    """Per simplex dimension: ``weights`` (R, d+1), ``samples`` (S, R, dim) f64, ``stat`` (S, R) the squared statistic
    in float32, ``ids`` (S, R, k) the k smallest by (d2, id), ``more`` (S, R) bool: more than k points within the k-th
    distance."""

    def __init__(self, weights, samples, stat, ids, more):
        self.weights, self.samples, self.stat, self.ids, self.more = weights, samples, stat, ids, more
        self.smax = stat.max(dim=1).values
        R = stat.shape[1]
        at = stat == self.smax.unsqueeze(1)
        self.row = torch.where(at, torch.arange(R, device=stat.device).unsqueeze(0), R).min(dim=1).values


def exact_knn_faces(simplices, points, landmarks, points_per_edge: int, k: int, stat: str):
    out = []
    dev = points.device
    for d, simp in enumerate(simplices):
        if simp.shape[0] == 0:
            out.append(None)
            continue
        W = gr.lattice(points_per_edge, d).to(dev)
        V = landmarks.double().to(dev)[simp.to(dev).long()]
        samples = torch.einsum("rk,skd->srd", W, V)
        S, R, dim = samples.shape
        d2, ids = smallest_keys_f64(points, samples.reshape(-1, dim), min(k + 1, points.shape[0]),
                                    (points_per_edge - 1) ** 2)
        more = (d2[:, k] == d2[:, k - 1]) if d2.shape[1] > k else torch.zeros(S * R, dtype=torch.bool, device=dev)
        out.append(ExactKnnFace(W, samples, statistic_f32(d2, k, stat).reshape(S, R), ids[:, :k].reshape(S, R, k),
                                more.reshape(S, R)))
    return out


def check_exact_knn_witnesses(F, faces, points):
    """Every simplex of every dimension of ``F`` against ``exact_knn_faces`` on an exact input: the value bits (the
    float32 square root of the largest squared statistic), the witness row (the smallest row at the maximum) and the
    neighbours (the k smallest by (d2, id), in order).  A facet's lattice is a subset of its coface's and the statistic
    of a sample does not depend on the simplex it is a sample of, so the monotone pass raises nothing here."""
    dev = points.device
    for d, simp in enumerate(F.simplices):
        if simp.shape[0] == 0:
            continue
        E = faces[d]
        want = E.smax.double().sqrt().to(torch.float32)   # (53 >= 2 * 24 + 2 bits: rounding twice is rounding once)
        assert torch.equal(F.values[d].detach().to(torch.float32).to(dev), want), f"dimension {d}: value bits differ"
        row = gr.lattice_row(E.weights, F.witness_weights[d].to(dev))
        assert torch.equal(row, E.row), f"dimension {d}: not the smallest sample row at the maximum"
        every = torch.arange(simp.shape[0], device=dev)
        assert torch.equal(F.witness_neighbors[d].to(dev), E.ids[every, E.row]), f"dimension {d}: neighbours differ"
        assert torch.equal(F.witness_point[d].to(dev), E.ids[every, E.row][:, -1])


def tie_share(faces) -> float:
    """Share of the simplices whose witness sample has more than k points within its k-th distance (reference alone)."""
    n = hit = 0
    for E in faces:
        if E is None:
            continue
        every = torch.arange(E.stat.shape[0], device=E.stat.device)
        n += E.stat.shape[0]
        hit += int(E.more[every, E.row].sum())
    return hit / max(n, 1)


# ------------------------------------------------------------------------------------------------ gradient
def values_from_witnesses(F, points: torch.Tensor, landmarks: torch.Tensor):
    """The values rebuilt in torch (differentiable, dtype of ``points``) from the witnesses ``F`` reports: per simplex
    |sum_j w_j L_j - x_(k)| ("kth") or sqrt(mean_i |sum_j w_j L_j - x_(i)|^2) ("dtm"); 0 where there is no witness."""
    out = []
    for d, simp in enumerate(F.simplices):
        nb = F.witness_neighbors[d].to(points.device)
        W = F.witness_weights[d].to(points.device).to(points.dtype)
        p = (W.unsqueeze(2) * landmarks[simp.to(points.device).long()]).sum(dim=1)
        ok = nb[:, -1] >= 0
        x = points[nb.clamp(min=0)]
        d2 = ((p.unsqueeze(1) - x) ** 2).sum(dim=2)
        sq = d2[:, -1] if F.neighbor_stat == "kth" or nb.shape[1] == 1 else d2.mean(dim=1)
        pos = ok & (sq > 0)
        out.append(torch.where(pos, torch.where(pos, sq, torch.ones_like(sq)).sqrt(), torch.zeros_like(sq)))
    return out


def reference_gradient_knn(F, points: torch.Tensor, landmarks: torch.Tensor, coef):
    """float64 gradient of ``sum_d (coef[d] * F.values[d]).sum()`` from the closed form of DESIGN.md section 8 and the
    witnesses ``F`` reports, with per output row the bound of a float32 evaluation of the same formula and the scale
    sum |g| |w| of the row's contributions - ``grad_reference.reference_gradient`` for the two statistics.

    "kth": f = |p* - x_(k)|: the formula and the bound of ``grad_reference.reference_gradient`` with j* = id_(k).

    "dtm": f = sqrt((1/k) sum_i |p* - x_(i)|^2), a contribution to point id_(i) is -g (p* - x_(i)) / (k f) (at most
    |g| / sqrt(k) per component: what the scale of a point row counts), to landmark j it is g w_j (p* - mean x) / f.
    With eps = 2**-24, c the largest |coordinate|, d+1 vertices, dim axes, first order, per component:

    * every diff_i = p* - x_(i) is off by at most (d+3) eps c, as for k = 1 (same p*, one subtraction).
    * k f^2 = sum_i |diff_i|^2: k dim products and k dim - 1 additions of non-negative terms, relative error at most
      (k dim + 1) eps from the arithmetic, plus 2 sqrt(k dim) (d+3) eps c sqrt(k) f from the diffs (Cauchy-Schwarz:
      sum_i,c 2 |diff_ic| |err| <= 2 (d+3) eps c sqrt(k dim) sqrt(k f^2)); the division by k, the square root: eps each.
      So |df| / f <= (k dim / 2 + 2) eps + sqrt(dim) (d+3) eps c / f.
    * one term t_i = g diff_i / (k f): |dt_i| <= |g| ((d+3) eps c / (k f) + |diff_ic| / (k f) (|df| / f + 3 eps))
      (the product k f, the division, the product with g).  |diff_ic| <= sqrt(k) f, so |t_ic| <= |g| / sqrt(k), and
      |dt_i| <= |g| / sqrt(k) ((1 + sqrt(dim)) (d+3) eps c / f + (k dim / 2 + 5) eps)
             <= |g| / sqrt(k) (2 sqrt(dim) (d+3) eps c / f + (k dim / 2 + 5) eps)   =: per_i.
      (1 / (k f) <= 1 / (sqrt(k) f) covers the first summand.)
    * the landmark's share sums the k terms first (k - 1 additions of terms bounded by |g| / sqrt(k): at most
      (k - 1) eps sqrt(k) |g|) and multiplies by w (eps): w (k per_i + ((k - 1) sqrt(k) + sqrt(k)) eps |g|)
      = w sqrt(k) |g| (2 sqrt(dim) (d+3) eps c / f + (k dim / 2 + 5 + k) eps); its magnitude is at most
      w |g| |p* - mean x| / f <= w |g| (Jensen: |p* - mean x|^2 <= mean |diff_i|^2 = f^2).
    * the in-order float32 sum of the m contributions of a row adds (m - 1) eps sum |terms|, with sum |terms| at most
      the row's scale: sum |g| / sqrt(k) for a point row, sum |g| w for a landmark row.
    * the row's bound is twice the sum (the first-order terms dropped above), as for k = 1.
    """
    if F.neighbors == 1 or F.neighbor_stat == "kth":
        return gr.reference_gradient(F, points, landmarks, coef)
    dev = points.device
    P, L = points.detach().double(), landmarks.detach().double()
    dim = P.shape[1]
    k = F.neighbors
    c = float(max(P.abs().max().item(), L.abs().max().item()))
    gp, gl = torch.zeros_like(P), torch.zeros_like(L)
    acc = {name: torch.zeros(t.shape[0], dtype=torch.float64, device=dev)
           for name, t in (("bp", P), ("sp", P), ("mp", P), ("bl", L), ("sl", L), ("ml", L))}
    rk = math.sqrt(k)
    for d, simp in enumerate(F.simplices):
        if simp.shape[0] == 0:
            continue
        g = torch.as_tensor(coef[d], device=dev).double()
        nb = F.witness_neighbors[d].to(dev)
        V = simp.to(dev).long()
        W = F.witness_weights[d].to(dev).double()
        keep = torch.nonzero((g != 0) & (nb[:, -1] >= 0)).reshape(-1)
        g, nb, V, W = g[keep], nb[keep], V[keep], W[keep]
        diffs = (W.unsqueeze(2) * L[V]).sum(dim=1).unsqueeze(1) - P[nb]          # (m, k, dim)
        f = ((diffs ** 2).sum(dim=2).mean(dim=1)).sqrt()
        pos = f > 0
        g, nb, V, W, diffs, f = g[pos], nb[pos], V[pos], W[pos], diffs[pos], f[pos]
        each = g.reshape(-1, 1, 1) * diffs / (k * f).reshape(-1, 1, 1)
        gu = each.sum(dim=1)
        rel = 2 * math.sqrt(dim) * (d + 3) * EPS32 * c / f
        per_pt = g.abs() / rk * (rel + (k * dim / 2 + 5) * EPS32)
        per_lm = g.abs() * rk * (rel + (k * dim / 2 + 5 + k) * EPS32)
        flat = nb.reshape(-1)
        gp.index_add_(0, flat, -each.reshape(-1, dim))
        acc["bp"].index_add_(0, flat, per_pt.repeat_interleave(k))
        acc["sp"].index_add_(0, flat, (g.abs() / rk).repeat_interleave(k))
        acc["mp"].index_add_(0, flat, torch.ones(flat.shape[0], dtype=torch.float64, device=dev))
        for i in range(d + 1):
            w = W[:, i]
            nz = w != 0
            gl.index_add_(0, V[nz, i], w[nz].unsqueeze(1) * gu[nz])
            acc["bl"].index_add_(0, V[nz, i], w[nz] * per_lm[nz])
            acc["sl"].index_add_(0, V[nz, i], w[nz] * g[nz].abs())
            acc["ml"].index_add_(0, V[nz, i], torch.ones_like(f[nz]))
    info = dict(bound_points=2 * (acc["bp"] + (acc["mp"] - 1).clamp(min=0) * EPS32 * acc["sp"]), scale_points=acc["sp"],
                bound_landmarks=2 * (acc["bl"] + (acc["ml"] - 1).clamp(min=0) * EPS32 * acc["sl"]),
                scale_landmarks=acc["sl"])
    return gp, gl, info
