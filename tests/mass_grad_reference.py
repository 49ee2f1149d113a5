"""References for the backward of ``distance_to_weighted_measure``: the rule as a torch float64 function of (sites,
masses, queries) on GIVEN ids and counts, differentiated by autograd (the oracle for float inputs, with the sums of
absolute contributions a rounding bound needs), an int64 brute force for integer inputs (THE answer, whatever the order
of a sum), and the bound helper.

No tests here; builds on ``knn_mass_reference`` and ``dtm_grad_reference``, which stay as they are."""

import numpy as np
import torch

import dtm_grad_reference as dref

EXACT = dref.EXACT


# ------------------------------------------------------------------------------------------------ float64 oracle
def rule(sites, masses, queries, ids, count, rows, mass, stat, squared):
    """The value of the rule for the query rows ``rows`` (an index tensor: the REACHED rows) as a differentiable float64
    torch function: ``ids`` (Q, L) int64 padded with -1 and ``count`` (Q,) are data, ``sites`` (n, d), ``masses`` (n,)
    and ``queries`` (Q, d) float64 tensors that may require grad.  tau = mass * sum(masses) depends on every mass.  The
    root has gradient 0 where the value is 0."""
    cnt = count[rows]
    width = int(cnt.max())
    nb = ids[rows][:, :width].clamp(min=0)
    cols = torch.arange(width).unsqueeze(0)
    last = (cnt - 1).unsqueeze(1)
    before, at = (cols < last).to(torch.float64), (cols == last).to(torch.float64)
    d2 = (queries[rows].unsqueeze(1) - sites[nb]).square().sum(dim=2)
    tau = mass * masses.sum()
    mu = masses[nb] * before
    dstar = (d2 * at).sum(dim=1)
    F = dstar if stat == "kth" else ((mu * d2).sum(dim=1) + (tau - mu.sum(dim=1)) * dstar) / tau
    if squared:
        return F
    pos = F > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, F, torch.ones_like(F))), torch.zeros_like(F))


def oracle(sites, masses, queries, ids, count, reached, grad_out, mass, stat, squared, own=False):
    """float64 autograd of sum(grad_out * rule) over the reached rows -> (g_sites, g_masses, g_queries) as numpy;
    ``own``: the queries ARE the sites (one leaf, both roles accumulate into g_sites; g_queries is None)."""
    f64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    y = f64(sites).requires_grad_(True)
    mu = f64(masses).requires_grad_(True)
    q = y if own else f64(queries).requires_grad_(True)
    rows = torch.nonzero(torch.as_tensor(np.asarray(reached, dtype=bool))).reshape(-1)
    ids, count = torch.as_tensor(np.asarray(ids, dtype=np.int64)), torch.as_tensor(np.asarray(count, dtype=np.int64))
    if rows.numel():
        value = rule(y, mu, q, ids, count, rows, mass, stat, squared)
        (value * f64(grad_out)[rows]).sum().backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return zero(y), zero(mu), (None if own else zero(q))


def closed_form(sites, masses, queries, ids, count, reached, grad_out, mass, squared, own=False):
    """The ``"dtm"`` closed form in float64 numpy with what a rounding bound needs -> dict of, per output word, the
    gradient, the sum of the absolute values of its contributions and their number: ``gq, abs_q, n_q`` (Q, d), ``gp,
    abs_p, n_p`` (n, d), ``gm, abs_m, n_m`` (n,) - the listed part of the mass gradient, a term h (d2 - dstar2) weighing
    |h| (d2 + dstar2) - and the scalar ``dense`` every mass gets besides, with ``abs_dense`` = mass * sum |h| (dstar2 + F).
    Rows that are not reached add nothing."""
    y, q = np.asarray(sites, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    mu_all = np.asarray(masses, dtype=np.float64)
    ids, count = np.asarray(ids, dtype=np.int64), np.asarray(count, dtype=np.int64)
    reached = np.asarray(reached, dtype=bool)
    g = np.where(reached, np.asarray(grad_out, dtype=np.float64), 0.0)
    n, dim = y.shape
    cnt = np.where(reached, count, 0)
    width = max(1, int(cnt.max()))
    nb = np.maximum(ids[:, :width], 0)
    cols = np.arange(width)[None, :]
    last = np.maximum(cnt - 1, 0)[:, None]
    before = (cols < last) & reached[:, None]
    at = (cols == last) & reached[:, None]
    tau = mass * mu_all.sum()
    mu = mu_all[nb] * before
    a = mu + at * (tau - mu.sum(axis=1))[:, None]
    diff = q[:, None, :] - y[nb]
    d2 = (diff * diff).sum(axis=2)
    dstar = (d2 * at).sum(axis=1)
    F = (a * d2).sum(axis=1) / tau
    if squared:
        c = g * 2.0 / tau
    else:
        f = np.sqrt(F)
        c = np.where(f > 0, g / (np.where(f > 0, f, 1.0) * tau), 0.0)
    terms = (c[:, None] * a)[:, :, None] * diff
    listed = (before | at).reshape(-1)
    flat = nb.reshape(-1)[listed]
    tp = terms.reshape(-1, dim)[listed]
    out = dict(gq=terms.sum(axis=1), abs_q=np.abs(terms).sum(axis=1),
               n_q=np.repeat(cnt[:, None], dim, axis=1), gp=-dref._scatter(flat, tp, n),
               abs_p=dref._scatter(flat, np.abs(tp), n),
               n_p=np.repeat(np.bincount(flat, minlength=n)[:, None], dim, axis=1))
    if own:
        out["gp"], out["abs_p"], out["n_p"] = out["gp"] + out["gq"], out["abs_p"] + out["abs_q"], out["n_p"] + out["n_q"]
    h = 0.5 * c
    tm = (h[:, None] * (d2 - dstar[:, None]))[before]
    fm = nb[before]
    am = (np.abs(h)[:, None] * (d2 + dstar[:, None]))[before]     # (both squared distances are rounded: their SUM scales)
    out.update(gm=np.bincount(fm, weights=tm, minlength=n), abs_m=np.bincount(fm, weights=am, minlength=n),
               n_m=np.bincount(fm, minlength=n), dense=float(mass * (h * (dstar - F)).sum()),
               abs_dense=float(mass * (np.abs(h) * (dstar + F)).sum()))
    return out


def within_bound(got, want, roundings, abs_sum, what, slack=0.0):
    """``|g - g64| <= roundings * 2^-24 * sum |c_i| + slack`` per word (``roundings``: a number or an array, the count of
    float32 roundings on the longest path to the word); prints and returns the largest ratio to the bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    bound = roundings * 2.0 ** -24 * abs_sum + slack
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: largest |g - g64| / bound = {ratio:.4f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, ratio)
    return ratio


def relative_close(got, want, rel, what):
    """``|got - want| <= rel * (|want| + max |want| / 1000)`` for every word (a word whose terms cancel to about nothing
    is judged against a thousandth of the output's largest word), no NaN or inf anywhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    scale = float(np.abs(want).max())
    err = np.abs(got - want)
    print(f"{what}: largest error {float(err.max()):.3e} on a scale of {scale:.3e}")
    assert (err <= rel * (np.abs(want) + 1e-3 * scale)).all(), (what, float(err.max()), scale)


# ------------------------------------------------------------------------------------------------ integer brute force
def integer_lists(sites, masses, queries, tau, capacity):
    """The lists of the rule on an integer cloud: the min(capacity, n) smallest keys (integer d2, id) per query, cut at the
    first position whose cumulative (integer) mass reaches ``tau`` -> (ids (Q, capacity) int64 padded with -1, count
    (Q,), reached (Q,) bool); rows that are not reached list all min(capacity, n)."""
    sites, queries = np.asarray(sites, dtype=np.int64), np.asarray(queries, dtype=np.int64)
    kq = min(capacity, sites.shape[0])
    near = dref.knn_ids(sites, queries, kq)
    M = np.cumsum(np.asarray(masses, dtype=np.int64)[near], axis=1)
    crossed = M >= tau
    reached = crossed.any(axis=1)
    count = np.where(reached, np.argmax(crossed, axis=1) + 1, kq).astype(np.int64)
    ids = np.full((queries.shape[0], capacity), -1, dtype=np.int64)
    ids[:, :kq] = near
    ids[np.arange(capacity)[None, :] >= count[:, None]] = -1
    return ids, count, reached


def integer_grads(sites, masses, queries, ids, count, tau, coef, h=None):
    """The three outputs of the device pair in int64 for integer ``sites``, ``masses``, ``queries``, ``tau``, ``coef`` (Q,)
    and ``h`` (Q,) over the rows ``ids`` (Q, L) with ``count`` (rows with count <= 0 list nothing) -> dict of
      out_q (Q, d) = coef_q * sum_t a_t (q - y_t), rho (Q,) = tau - M, cross (Q,) (-1 without a list), dstar (Q,) =
      d2(q, y_cross),
      out_p (n, d) = -sum over the entries with id j of coef_q * a_t * (q - y_j),
      out_m (n,) = sum over the entries BEFORE their query's crossing of h_q * (d2(q, y_j) - d2(q, y_cross)).
    Asserts that per output word the absolute values of all its terms add up to less than 2^24, and that so does every
    product coef * a and every d2: every partial sum, in whatever order, is then an exact float32 integer."""
    y, q = np.asarray(sites, dtype=np.int64), np.asarray(queries, dtype=np.int64)
    mu_all, ids = np.asarray(masses, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    cnt = np.maximum(np.minimum(np.asarray(count, dtype=np.int64), ids.shape[1]), 0)
    coef = np.asarray(coef, dtype=np.int64)
    h = np.zeros_like(coef) if h is None else np.asarray(h, dtype=np.int64)
    n, dim = y.shape
    L = ids.shape[1]
    cols = np.arange(L)[None, :]
    last = (cnt - 1)[:, None]
    has = (cnt > 0)[:, None]
    before, at = (cols < last) & has, (cols == last) & has
    valid = (ids >= 0) & (ids < n)
    nb = np.where(valid, ids, 0)
    mu = mu_all[nb] * (before & valid)
    rho = np.where(cnt > 0, tau - mu.sum(axis=1), 0)
    a = mu + (at & valid) * rho[:, None]
    diff = q[:, None, :] - y[nb]
    d2 = (diff * diff).sum(axis=2)
    cross = np.where(cnt > 0, np.take_along_axis(ids, np.maximum(last, 0), axis=1)[:, 0], -1)
    dstar = (d2 * at).sum(axis=1)
    e = coef[:, None] * a
    terms = e[:, :, None] * diff
    out_q = terms.sum(axis=1)
    listed = ((before | at) & valid).reshape(-1)
    flat, tp = nb.reshape(-1)[listed], terms.reshape(-1, dim)[listed].astype(np.float64)
    out_p = -np.rint(dref._scatter(flat, tp, n)).astype(np.int64)
    pick = before & valid
    tm = (h[:, None] * (d2 - dstar[:, None]))[pick].astype(np.float64)
    out_m = np.rint(np.bincount(nb[pick], weights=tm, minlength=n)).astype(np.int64)
    largest = int(max(np.abs(terms).sum(axis=1).max(), np.rint(dref._scatter(flat, np.abs(tp), n)).max(),
                      np.bincount(nb[pick], weights=np.abs(tm), minlength=n).max(), np.abs(e).max(),
                      (d2 * (before | at)).max()))
    assert largest < EXACT, f"a partial sum may reach {largest} >= 2^24: the case is not exact in float32"
    return dict(out_q=out_q, rho=rho, cross=cross, dstar=dstar, out_p=out_p, out_m=out_m, largest=largest)
