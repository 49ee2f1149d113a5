"""Brute-force reference of ``distance_to_measure``'s backward (numpy, on the host): the k smallest by (integer d2, id),
the gradients in int64 (integer clouds: THE answer) or float64 (the closed form on given ids, with the sums a rounding
bound needs), and the check that every partial sum of an integer case is an exact float32 integer."""

import numpy as np

EXACT = 1 << 24   # integers below this magnitude are float32 numbers, and so are their sums and differences


def integer_cloud(n, dim, hi, seed, twice=False):
    """``n`` integer points of [0, hi)^dim as int64; ``twice``: every point occurs twice (n // 2 distinct draws)."""
    rng = np.random.default_rng(seed)
    if not twice:
        return rng.integers(0, hi, size=(n, dim), dtype=np.int64)
    half = rng.integers(0, hi, size=(n // 2, dim), dtype=np.int64)
    return np.concatenate([half, half])[rng.permutation(2 * (n // 2))]


def knn_ids(points, queries, k, block=512):
    """(Q, k) int64: per query the k smallest keys (integer d2, id), ascending - the rule of the device's lists."""
    points, queries = np.asarray(points, dtype=np.int64), np.asarray(queries, dtype=np.int64)
    n = points.shape[0]
    out = np.empty((queries.shape[0], k), dtype=np.int64)
    for a in range(0, queries.shape[0], block):
        q = queries[a:a + block]
        d2 = np.zeros((q.shape[0], n), dtype=np.int64)
        for c in range(points.shape[1]):
            d2 += (q[:, c:c + 1] - points[None, :, c]) ** 2
        key = d2 * n + np.arange(n, dtype=np.int64)[None, :]          # distinct: one order
        part = np.argpartition(key, k - 1, axis=1)[:, :k] if k < n else np.broadcast_to(np.arange(n), key.shape)
        out[a:a + block] = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, axis=1), axis=1), axis=1)
    return out


def _scatter(ids, vals, n):
    """out[j, c] = sum of vals[e, c] over the entries e with ids[e] == j (float64 weights: exact for integers < 2^53)."""
    return np.stack([np.bincount(ids, weights=vals[:, c], minlength=n) for c in range(vals.shape[1])], axis=1)


def integer_grads(points, queries, ids, coef, own=False):
    """(grad_queries (Q, dim), grad_points (n, dim)) as int64 of integer ``points``, ``queries``, ``coef`` (Q,) over the
    listed ``ids`` (Q, m): out_q[q] = coef[q] * sum_i (q - x_i), out_p[j] = -sum over the entries with id j of
    coef[q] * (q - x_j); ``own``: grad_queries is added onto grad_points row by row.  Asserts that, per output word,
    the absolute values of all its terms add up to less than 2^24 - every partial sum, in whatever order, is then an exact
    float32 integer - and returns the largest such sum as third value."""
    points, queries = np.asarray(points, dtype=np.int64), np.asarray(queries, dtype=np.int64)
    ids, coef = np.asarray(ids, dtype=np.int64), np.asarray(coef, dtype=np.int64)
    n, dim = points.shape
    diffs = queries[:, None, :] - points[ids]                           # (Q, m, dim)
    gq = coef[:, None] * diffs.sum(axis=1)
    terms = (coef[:, None, None] * diffs).reshape(-1, dim)
    flat = ids.reshape(-1)
    gp = -np.rint(_scatter(flat, terms.astype(np.float64), n)).astype(np.int64)
    mass_q = np.abs(coef)[:, None] * np.abs(diffs).sum(axis=1)          # per word: sum of |terms|
    mass_p = np.rint(_scatter(flat, np.abs(terms).astype(np.float64), n)).astype(np.int64)
    if own:
        gp = gp + gq
        mass_p = mass_p + mass_q
    largest = int(max(mass_q.max(), mass_p.max()))
    assert largest < EXACT, f"a partial sum may reach {largest} >= 2^24: the case is not exact in float32"
    return gq, gp, largest


def closed_form(points, queries, ids, grad_out, stat, squared, own=False):
    """The closed form in float64 on the given ``ids`` (Q, k): ``(gq, gp, abs_q, abs_p, n_q, n_p)`` - the two gradients,
    per word the sum of |c_i| over its float64 contributions c_i and their number n.  ``points`` / ``queries``: the
    float32 (or float64) coordinates as they are; ``stat`` "dtm" (m = k terms) or "kth" (m = 1: the last column)."""
    points, queries = np.asarray(points, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    ids, g = np.asarray(ids, dtype=np.int64), np.asarray(grad_out, dtype=np.float64)
    n, dim = points.shape
    if stat == "kth":
        ids = ids[:, -1:]
    m = ids.shape[1]
    diffs = queries[:, None, :] - points[ids]
    f2 = (diffs * diffs).sum(axis=2).sum(axis=1) / m
    if squared:
        coef = g * (2.0 / m)
    else:
        f = np.sqrt(f2)
        coef = np.where(f > 0, g / (np.where(f > 0, f, 1.0) * m), 0.0)
    terms = coef[:, None, None] * diffs
    gq, abs_q = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    n_q = np.full(gq.shape, m, dtype=np.int64)
    flat = ids.reshape(-1)
    gp = -_scatter(flat, terms.reshape(-1, dim), n)
    abs_p = _scatter(flat, np.abs(terms).reshape(-1, dim), n)
    n_p = np.repeat(np.bincount(flat, minlength=n)[:, None], dim, axis=1)
    if own:
        gp, abs_p, n_p = gp + gq, abs_p + abs_q, n_p + n_q
    return gq, gp, abs_q, abs_p, n_q, n_p


def within_bound(got, want, n, abs_sum, what):
    """``|g - g64| <= (n + 64) * 2^-24 * sum |c_i|`` per component; returns the largest ratio to the bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    bound = (n + 64) * 2.0 ** -24 * abs_sum
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: largest |g - g64| / bound = {ratio:.4f}")
    assert (err <= bound).all(), (what, ratio)
    return ratio
