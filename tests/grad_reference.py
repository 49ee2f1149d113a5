"""Plain references for ``flood_filtration``'s witnesses and gradients: brute force over all points in float64 (int64
for the kernel-level searches), no kd-tree, no box tree, nothing of ``flooder_amd.grad``.

On inputs where float32 arithmetic is exact (integer coordinates, dyadic lattice weights, every squared distance below
2**24 units of the squared weight step - ``assert_exact_inputs`` checks it) the float64 numbers here are the very
numbers a float32 fma chain produces, so the tests built on this module compare bit for bit.
"""

import itertools
import math

import numpy as np
import torch

EPS32 = 2.0 ** -24    # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ lattice
def lattice(points_per_edge: int, d: int) -> torch.Tensor:
    """(R, d+1) float64 barycentric lattice of a d-simplex: the compositions of n-1 into d+1 parts, in the order of the
    combinations that encode them, divided by n-1 (the contract of ``core.generate_grid``, rebuilt here)."""
    n = points_per_edge
    if d == 0:
        return torch.ones((1, 1), dtype=torch.float64)
    rows = []
    for comb in itertools.combinations(range(n + d - 1), d):
        ext = (-1,) + comb + (n + d - 1,)
        rows.append([ext[i + 1] - ext[i] - 1 for i in range(d + 1)])
    return torch.tensor(rows, dtype=torch.float64) / (n - 1)


def assert_exact_inputs(points, landmarks, points_per_edge: int, queries=None) -> int:
    """The inputs are integers, the lattice step 1/(n-1) is a power of two, and the largest squared distance between a
    sample and a point, counted in units of step**2, stays below 2**24: every sample coordinate, every difference, every
    square and every partial sum is then an integer multiple of the unit below 2**24 and float32 holds it exactly,
    whatever the order of the operations.  The samples lie in the bounding box of the landmarks; ``queries`` (multiples
    of the step) replaces them.  Returns the bound (units of step**2)."""
    P = torch.as_tensor(points).double()
    L = torch.as_tensor(landmarks).double()
    assert torch.equal(P, P.round()) and torch.equal(L, L.round()), "coordinates must be integers"
    step = points_per_edge - 1
    assert step >= 1 and step & (step - 1) == 0, "points_per_edge - 1 must be a power of two"
    Q = L if queries is None else torch.as_tensor(queries).double()
    assert torch.equal(Q * step, (Q * step).round()), "queries must be multiples of the lattice step"
    far = torch.maximum(Q.max(0).values - P.min(0).values, P.max(0).values - Q.min(0).values)   # per axis max |q - p|
    bound = int(((far * step) ** 2).sum().item())
    assert bound < 2 ** 24, f"squared distances reach {bound} units: not exact in float32"
    assert float(max(Q.abs().max(), P.abs().max())) * step < 2 ** 24
    return bound


# ------------------------------------------------------------------------------------------------ brute force
def nearest_points(points: torch.Tensor, samples: torch.Tensor, chunk_bytes: int = 256 << 20):
    """Per row of ``samples`` (Q, dim): (minimum d2 over ALL points, smallest id at that minimum, number of points at
    it), float64 / int64 / int64.  d2 is accumulated axis by axis in float64; the (chunk, N) block stays below
    ``chunk_bytes``."""
    P = points.double()
    S = samples.double()
    n, dim = P.shape
    per = max(1, chunk_bytes // (8 * n * 2))
    ids = torch.arange(n, device=P.device, dtype=torch.int64)
    dmin, first, count = [], [], []
    for a in range(0, S.shape[0], per):
        s = S[a:a + per]
        d2 = (s[:, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for k in range(1, dim):
            d2 += (s[:, k:k + 1] - P[:, k].unsqueeze(0)) ** 2
        m = d2.min(dim=1).values
        at = d2 == m.unsqueeze(1)
        dmin.append(m)
        count.append(at.sum(dim=1))
        first.append(torch.where(at, ids.unsqueeze(0), n).min(dim=1).values)
    return torch.cat(dmin), torch.cat(first), torch.cat(count)


def nearest_sets(points: torch.Tensor, samples: torch.Tensor):
    """The full sets: a list (one per sample) of the int64 ids of the points at the minimum d2 (small inputs)."""
    P, S = points.double(), samples.double()
    d2 = ((S.unsqueeze(1) - P.unsqueeze(0)) ** 2).sum(dim=2)
    m = d2.min(dim=1, keepdim=True).values
    return [torch.nonzero(row).reshape(-1) for row in (d2 == m)]


class ExactFace:
    """Result of ``exact_face``: ``weights`` (R, k+1) f64, ``samples`` (S, R, dim) f64, ``d2`` (S, R) the minimum d2 of
    every sample over all points, ``dmax`` (S,) its maximum per simplex, ``argmax`` (S, R) bool the samples attaining
    it, ``first`` / ``count`` (S, R) the smallest id and the number of points at each sample's minimum."""

    def __init__(self, weights, samples, d2, first, count):
        self.weights, self.samples, self.d2, self.first, self.count = weights, samples, d2, first, count
        self.dmax = d2.max(dim=1).values
        self.argmax = d2 == self.dmax.unsqueeze(1)


def exact_face(points: torch.Tensor, landmarks: torch.Tensor, simplex: torch.Tensor, weights: torch.Tensor) -> ExactFace:
    """Brute force for the simplices ``simplex`` (S, k+1) of landmark ids with the lattice ``weights`` (R, k+1): every
    sample sum_i w_i L_i against every point.  Runs on the device of ``points``."""
    dev = points.device
    W = weights.double().to(dev)
    V = landmarks.double().to(dev)[simplex.to(dev).long()]          # (S, k+1, dim)
    samples = torch.einsum("rk,skd->srd", W, V)                     # (S, R, dim)
    S, R, dim = samples.shape
    dmin, first, count = nearest_points(points, samples.reshape(-1, dim))
    return ExactFace(W, samples, dmin.reshape(S, R), first.reshape(S, R), count.reshape(S, R))


def lattice_row(weights: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """Index in the lattice ``weights`` (R, k+1) of every row of ``rows`` (S, k+1), -1 where it is no lattice row (exact
    comparison: lattice weights with a power-of-two step are the same numbers in float32 and float64)."""
    eq = (rows.double().unsqueeze(1) == weights.double().to(rows.device).unsqueeze(0)).all(dim=2)   # (S, R)
    idx = torch.arange(weights.shape[0], device=rows.device).unsqueeze(0).expand_as(eq)
    return torch.where(eq, idx, -1).max(dim=1).values


# ------------------------------------------------------------------------------------------------ gradient
def reference_gradient(F, points: torch.Tensor, landmarks: torch.Tensor, coef):
    """float64 gradient of ``sum_d (coef[d] * F.values[d]).sum()`` from the closed form and the
    witnesses ``F`` reports: with p* = sum_i w*_i L_i, x* = points[j*], f = |p* - x*| and u = (p* - x*) / f, a simplex
    with coefficient g adds ``-g u`` to row j* of the points' gradient and ``g w*_i u`` to landmark i; nothing for f = 0.

    Returns ``(grad_points, grad_landmarks, info)``; ``info`` holds per output row (points / landmarks) the error bound
    ``bound_*`` of a float32 evaluation of the same formula and the scale ``scale_* = sum |g| |w|`` over the row's
    contributions (w = 1 for a point row).

    The bound, eps = 2**-24, c = largest |coordinate|, k+1 vertices, dim axes, all to first order and per component:

    * p*: k+1 products w_i L_i, each off by at most eps w_i c (sum: eps c since the weights sum to 1), and k additions of
      partial sums of magnitude at most c: (k+1) eps c.  The difference p* - x* rounds by eps |p* - x*| <= 2 eps c.
      So each component of ``diff`` is off by at most (k+3) eps c and its norm f by at most sqrt(dim) (k+3) eps c.
    * f itself: dim squares, dim-1 additions and one square root add at most (dim/2 + 1) eps f.
    * u = diff / f: |du| <= |d diff| / f + |u| |df| / f + eps |u| <= (1 + sqrt(dim)) (k+3) eps c / f + (dim/2 + 2) eps,
      and 1 + sqrt(dim) <= 2 sqrt(dim).  The products g u and (landmarks) w (g u) add eps each.
      One contribution therefore carries at most |g| w (2 sqrt(dim) (k+3) eps c / f + (dim/2 + 4) eps).
    * the in-order float32 sum of the m contributions of a row adds at most (m-1) eps sum|terms|, with
      sum|terms| <= sum |g| w because |u_k| <= 1.  (Folding the landmarks' gradient into the points' is one more
      addition: ``fold_landmarks`` charges it, the landmark-tensor cases have none.)
    * the row's bound is twice the sum of the two (the first-order terms dropped above).
    """
    dev = points.device
    P, L = points.detach().double(), landmarks.detach().double()
    dim = P.shape[1]
    c = float(max(P.abs().max().item(), L.abs().max().item()))
    gp, gl = torch.zeros_like(P), torch.zeros_like(L)
    acc = {name: torch.zeros(t.shape[0], dtype=torch.float64, device=dev)
           for name, t in (("bp", P), ("sp", P), ("mp", P), ("bl", L), ("sl", L), ("ml", L))}
    for d, simp in enumerate(F.simplices):
        if simp.shape[0] == 0:
            continue
        g = torch.as_tensor(coef[d], device=dev).double()
        jp = F.witness_point[d].to(dev)
        V = simp.to(dev).long()
        W = F.witness_weights[d].to(dev).double()
        keep = torch.nonzero((g != 0) & (jp >= 0)).reshape(-1)
        g, jp, V, W = g[keep], jp[keep], V[keep], W[keep]
        diff = (W.unsqueeze(2) * L[V]).sum(dim=1) - P[jp]
        f = diff.norm(dim=1)
        pos = f > 0
        g, jp, V, W, diff, f = g[pos], jp[pos], V[pos], W[pos], diff[pos], f[pos]
        u = diff / f.unsqueeze(1)
        gu = g.unsqueeze(1) * u
        per = g.abs() * (2 * math.sqrt(dim) * (d + 3) * EPS32 * c / f + (dim / 2 + 4) * EPS32)
        gp.index_add_(0, jp, -gu)
        acc["bp"].index_add_(0, jp, per)
        acc["sp"].index_add_(0, jp, g.abs())
        acc["mp"].index_add_(0, jp, torch.ones_like(f))
        for i in range(d + 1):
            w = W[:, i]
            nz = w != 0
            gl.index_add_(0, V[nz, i], w[nz].unsqueeze(1) * gu[nz])
            acc["bl"].index_add_(0, V[nz, i], w[nz] * per[nz])
            acc["sl"].index_add_(0, V[nz, i], w[nz] * g[nz].abs())
            acc["ml"].index_add_(0, V[nz, i], torch.ones_like(f[nz]))
    info = dict(bound_points=2 * (acc["bp"] + (acc["mp"] - 1).clamp(min=0) * EPS32 * acc["sp"]), scale_points=acc["sp"],
                bound_landmarks=2 * (acc["bl"] + (acc["ml"] - 1).clamp(min=0) * EPS32 * acc["sl"]),
                scale_landmarks=acc["sl"])
    return gp, gl, info


def fold_landmarks(gp, gl, info, landmark_ids):
    """Integer landmarks: the landmarks' gradient flows into ``points`` at ``landmark_ids``; gradient, bound and scale
    are folded the same way, and the addition of the two partial sums charges one more eps sum|terms| (doubled like the
    rest of the bound) to the rows it touches.  Returns (grad_points, bound, scale)."""
    ids = landmark_ids.to(gp.device)
    scale = info["scale_points"].index_add(0, ids, info["scale_landmarks"])
    bound = info["bound_points"].index_add(0, ids, info["bound_landmarks"] + 2 * EPS32 * scale[ids])
    return gp.index_add(0, ids, gl), bound, scale


# ------------------------------------------------------------------------------------------------ the exact checks
def reference_faces(simplices, points, landmarks, points_per_edge: int):
    """``exact_face`` of every simplex of every dimension (each with the lattice of its own dimension); None for an
    empty dimension."""
    return [exact_face(points, landmarks, simp, lattice(points_per_edge, d)) if simp.shape[0] else None
            for d, simp in enumerate(simplices)]


def check_exact_witnesses(F, faces, points, smallest_id: bool):
    """Every simplex of every dimension of ``F`` against ``faces = reference_faces(F.simplices, ...)`` on an exact input
    (see the module docstring):

    * the value is, bit for bit in float32, the square root of the reference maximum d2;
    * the witness weights are a row of the simplex's own lattice, in the reference's argmax set - the smallest such row
      (the lattice of a face is its parent's restricted to the face, in the same order, so "the smallest sample row"
      of the parent's table is the smallest row here);
    * |p* - x*|**2 is the maximum, i.e. the witness point is A nearest point of the witness sample, and
      - ``smallest_id`` - it is the smallest id in the reference's set of nearest points.

    The lattice of a facet is a subset of its coface's, so on these inputs a simplex's own maximum is never below a
    facet's and the monotone pass raises nothing: the value compared is the simplex's OWN maximum, and a value raised
    above it fails the first check."""
    dev = points.device
    for d, simp in enumerate(F.simplices):
        if simp.shape[0] == 0:
            continue
        E = faces[d]
        W = E.weights
        own32 = E.dmax.sqrt().to(torch.float32)               # (d2 < 2**24 is exact in float32; sqrt rounds once in both)
        assert torch.equal(F.values[d].detach().to(torch.float32).to(dev), own32), \
            f"dimension {d}: values differ from the exact reference"
        wp = F.witness_point[d].to(dev)
        ww = F.witness_weights[d].to(dev)
        assert (wp >= 0).all() and (wp < points.shape[0]).all(), d
        row = lattice_row(W, ww)
        assert (row >= 0).all(), f"dimension {d}: witness weights that are no lattice row"
        every = torch.arange(simp.shape[0], device=dev)
        assert E.argmax[every, row].all(), f"dimension {d}: witness sample not at the maximum"
        smallest_row = torch.where(E.argmax, torch.arange(W.shape[0], device=dev).unsqueeze(0), W.shape[0]).min(dim=1).values
        assert torch.equal(row, smallest_row), f"dimension {d}: not the smallest sample row at the maximum"
        d2w = ((E.samples[every, row] - points.double()[wp]) ** 2).sum(dim=1)
        assert torch.equal(d2w, E.dmax), f"dimension {d}: witness point not at the exact distance"
        if smallest_id:
            assert torch.equal(wp, E.first[every, row]), f"dimension {d}: not the smallest id among the nearest points"


def tie_shares(faces):
    """(share of simplices whose witness sample has more than one nearest point, share with more than one sample at the
    maximum, number of simplices) - from the reference alone: the witness sample is the smallest argmax row."""
    n = pts_tie = arg_tie = 0
    for E in faces:
        if E is None:
            continue
        R = E.d2.shape[1]
        smallest_row = torch.where(E.argmax, torch.arange(R, device=E.d2.device).unsqueeze(0), R).min(dim=1).values
        cnt = E.count[torch.arange(E.d2.shape[0], device=E.d2.device), smallest_row]
        n += E.d2.shape[0]
        pts_tie += int((cnt > 1).sum())
        arg_tie += int((E.argmax.sum(dim=1) > 1).sum())
    return pts_tie / max(n, 1), arg_tie / max(n, 1), n
