"""Plain references for ``power_filtration``'s witnesses and gradients and for ``flooder_witness_power``: brute force
over all points in float64 (int32 for the kernel-level search), nothing of ``flooder_amd.grad``.  Built on
``grad_reference`` (lattice, ``ExactFace``, the exactness argument) and ``power_reference``.

On inputs where float32 is exact - integer coordinates, integer weights, a dyadic lattice, every word
``|p - x|^2 + w_x^2`` below 2**24 units of the squared lattice step (``assert_exact_power_inputs``) - the float64
numbers here are the very numbers the sweep's ``fmaf(w, w, d2)`` produces, so the tests compare bit for bit.
"""

import math

import torch

import grad_reference as gr

EPS32 = gr.EPS32


# ------------------------------------------------------------------------------------------------ exact inputs
def assert_exact_power_inputs(points, landmarks, w, points_per_edge: int, queries=None) -> int:
    """``grad_reference.assert_exact_inputs`` with the weights: they are integers and the largest word, the largest
    squared distance plus the largest squared weight in units of step**2, stays below 2**24.  Returns that bound."""
    bound = gr.assert_exact_inputs(points, landmarks, points_per_edge, queries=queries)
    W = torch.as_tensor(w).double()
    assert torch.equal(W, W.round()), "weights must be integers"
    step = points_per_edge - 1
    bound += int((W.abs().max().item() * step) ** 2)
    assert bound < 2 ** 24, f"power words reach {bound} units: not exact in float32"
    return bound


# ------------------------------------------------------------------------------------------------ brute force
def power_nearest_points(points: torch.Tensor, w: torch.Tensor, samples: torch.Tensor, chunk_bytes: int = 256 << 20):
    """Per row of ``samples`` (Q, dim): (minimum of |p - x|^2 + w_x^2 over ALL points, smallest id at that minimum,
    number of points at it, is that id one of the Euclidean nearest points of the sample), float64 / int64 / int64 /
    bool.  The form of ``grad_reference.nearest_points``."""
    P, W2, S = points.double(), w.double() ** 2, samples.double()
    n, dim = P.shape
    per = max(1, chunk_bytes // (8 * n * 2))
    ids = torch.arange(n, device=P.device, dtype=torch.int64)
    wmin, first, count, euclid = [], [], [], []
    for a in range(0, S.shape[0], per):
        s = S[a:a + per]
        d2 = (s[:, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for k in range(1, dim):
            d2 += (s[:, k:k + 1] - P[:, k].unsqueeze(0)) ** 2
        near = d2.min(dim=1).values
        word = d2 + W2.unsqueeze(0)
        m = word.min(dim=1).values
        at = word == m.unsqueeze(1)
        f = torch.where(at, ids.unsqueeze(0), n).min(dim=1).values
        wmin.append(m)
        count.append(at.sum(dim=1))
        first.append(f)
        euclid.append(d2.gather(1, f.unsqueeze(1)).squeeze(1) == near)
    return torch.cat(wmin), torch.cat(first), torch.cat(count), torch.cat(euclid)


def exact_power_face(points, w, landmarks, simplex, weights) -> "gr.ExactFace":
    """``grad_reference.exact_face`` of the weighted filtration: ``d2`` holds the power word of every sample, ``first`` /
    ``count`` the smallest id and the number of points at each sample's POWER minimum."""
    dev = points.device
    W = weights.double().to(dev)
    V = landmarks.double().to(dev)[simplex.to(dev).long()]
    samples = torch.einsum("rk,skd->srd", W, V)
    S, R, dim = samples.shape
    m, first, count, _ = power_nearest_points(points, w.to(dev), samples.reshape(-1, dim))
    return gr.ExactFace(W, samples, m.reshape(S, R), first.reshape(S, R), count.reshape(S, R))


def reference_power_faces(simplices, points, w, landmarks, points_per_edge: int):
    return [exact_power_face(points, w, landmarks, simp, gr.lattice(points_per_edge, d)) if simp.shape[0] else None
            for d, simp in enumerate(simplices)]


def check_exact_power_witnesses(F, faces, points, w):
    """``grad_reference.check_exact_witnesses`` for the weighted filtration, every simplex of every dimension: the value
    is, bit for bit, the root of the reference's largest power word; the witness sample is the smallest lattice row at
    that maximum; the witness point attains the word exactly and is the smallest id that does."""
    dev = points.device
    W2 = w.to(dev).double() ** 2
    for d, simp in enumerate(F.simplices):
        if simp.shape[0] == 0:
            continue
        E = faces[d]
        own32 = E.dmax.sqrt().to(torch.float32)
        assert torch.equal(F.values[d].detach().to(torch.float32).to(dev), own32), f"dimension {d}: values differ"
        wp = F.witness_point[d].to(dev)
        assert (wp >= 0).all() and (wp < points.shape[0]).all(), d
        row = gr.lattice_row(E.weights, F.witness_weights[d].to(dev))
        assert (row >= 0).all(), f"dimension {d}: witness weights that are no lattice row"
        every = torch.arange(simp.shape[0], device=dev)
        R = E.weights.shape[0]
        smallest_row = torch.where(E.argmax, torch.arange(R, device=dev).unsqueeze(0), R).min(dim=1).values
        assert torch.equal(row, smallest_row), f"dimension {d}: not the smallest sample row at the maximum"
        word = ((E.samples[every, row] - points.double()[wp]) ** 2).sum(dim=1) + W2[wp]
        assert torch.equal(word, E.dmax), f"dimension {d}: witness point not at the exact power distance"
        assert torch.equal(wp, E.first[every, row]), f"dimension {d}: not the smallest id at the power minimum"


# ------------------------------------------------------------------------------------------------ gradient
def reference_power_gradient(F, points, landmarks, w, coef):
    """float64 gradient of ``sum_d (coef[d] * F.values[d]).sum()`` of a ``power_filtration`` result from the closed form
    and the witnesses ``F`` reports: with p* = sum_i l_i L_i, x* = points[j*], w* = w[j*], f = sqrt(|p* - x*|^2 + w*^2) and
    u = (p* - x*) / f, a simplex with coefficient g adds ``-g u`` to row j* of the points' gradient, ``g l_i u`` to
    landmark i and ``g w* / f`` to entry j* of the weights' gradient; nothing for f = 0.

    Returns ``(grad_points, grad_landmarks, grad_weights, info)``; ``info`` holds per output row the error bound
    ``bound_*`` of a float32 evaluation of the same formula and the scale ``scale_*`` of the row: sum |g| l over its
    contributions (l = 1 for a point row) and, for a weight row, sum |g| |w*| / f - the size of the terms themselves, so
    that a dropped term is as visible there as in the other two.

    The bound extends ``grad_reference.reference_gradient``'s; eps = 2**-24, c = largest |coordinate|, k+1 vertices, dim
    axes, first order, per component:

    * each component of ``diff = p* - x*`` is off by at most (k+3) eps c (there), its norm n by sqrt(dim) (k+3) eps c.
    * f = sqrt(n^2 + w^2): n carries (dim/2 + 1) eps n of its own arithmetic, the two squares and the sum one eps each on
      f^2, the root halves relative errors and adds eps/2: at most (dim/2 + 3) eps f, and |df| <= |dn| n / f <= |dn|
      from the inputs.  So |df| <= sqrt(dim) (k+3) eps c + (dim/2 + 3) eps f.
    * u = diff / f: |du| <= |d diff| / f + |u| |df| / f + eps |u| <= (1 + sqrt(dim)) (k+3) eps c / f + (dim/2 + 4) eps
      with |u| <= 1; the products g u and l (g u) add eps each: one contribution carries at most
      |g| l (2 sqrt(dim) (k+3) eps c / f + (dim/2 + 6) eps).
    * t = g w* / f: the product and the quotient add eps each, f its relative error:
      |dt| <= |g| (|w*| / f) (sqrt(dim) (k+3) eps c / f + (dim/2 + 5) eps).
    * the in-order float32 sum of the m contributions of a row adds at most (m-1) eps sum|terms|; the row's bound is
      twice the sum of the two (the first-order terms dropped above), as there.
    """
    dev = points.device
    P, L, Wt = points.detach().double(), landmarks.detach().double(), w.detach().double()
    dim = P.shape[1]
    c = float(max(P.abs().max().item(), L.abs().max().item()))
    gp, gl, gw = torch.zeros_like(P), torch.zeros_like(L), torch.zeros_like(Wt)
    acc = {name: torch.zeros(t.shape[0], dtype=torch.float64, device=dev)
           for name, t in (("bp", P), ("sp", P), ("mp", P), ("bl", L), ("sl", L), ("ml", L), ("bw", P), ("sw", P))}
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
        ws = Wt[jp]
        f = ((diff * diff).sum(dim=1) + ws * ws).sqrt()
        pos = f > 0
        g, jp, V, W, diff, ws, f = g[pos], jp[pos], V[pos], W[pos], diff[pos], ws[pos], f[pos]
        gu = g.unsqueeze(1) * diff / f.unsqueeze(1)
        lead = math.sqrt(dim) * (d + 3) * EPS32 * c / f
        per = g.abs() * (2 * lead + (dim / 2 + 6) * EPS32)
        gp.index_add_(0, jp, -gu)
        acc["bp"].index_add_(0, jp, per)
        acc["sp"].index_add_(0, jp, g.abs())
        acc["mp"].index_add_(0, jp, torch.ones_like(f))
        size_w = g.abs() * ws.abs() / f
        gw.index_add_(0, jp, g * ws / f)
        acc["bw"].index_add_(0, jp, size_w * (lead + (dim / 2 + 5) * EPS32))
        acc["sw"].index_add_(0, jp, size_w)
        for i in range(d + 1):
            lam = W[:, i]
            nz = lam != 0
            gl.index_add_(0, V[nz, i], lam[nz].unsqueeze(1) * gu[nz])
            acc["bl"].index_add_(0, V[nz, i], lam[nz] * per[nz])
            acc["sl"].index_add_(0, V[nz, i], lam[nz] * g[nz].abs())
            acc["ml"].index_add_(0, V[nz, i], torch.ones_like(f[nz]))
    more_p = (acc["mp"] - 1).clamp(min=0) * EPS32
    info = dict(bound_points=2 * (acc["bp"] + more_p * acc["sp"]), scale_points=acc["sp"],
                bound_landmarks=2 * (acc["bl"] + (acc["ml"] - 1).clamp(min=0) * EPS32 * acc["sl"]),
                scale_landmarks=acc["sl"],
                bound_weights=2 * (acc["bw"] + more_p * acc["sw"]), scale_weights=acc["sw"])
    return gp, gl, gw, info
