"""Plain references for the wide k-nearest kernel (``flooder_knn_wide_f32``, k up to 1024): the numpy replay of its
strided float32 sum, written from the rule in ``include/flooder_hip.h`` alone, and the exact inputs of its tests.  The
brute force is ``knn_grad_reference.smallest_keys_int`` (an integer key sort over all points: exact by construction).

No tests here; builds on ``knn_grad_reference`` and ``grad_reference``, which stay as they are."""

import numpy as np
import torch

import knn_grad_reference as kr

KNN_WIDE_MAX = 1024


def dtm_words_wide(d2_f32: np.ndarray, k: int) -> np.ndarray:
    """float32 replay of stat 1 of the wide kernel from the first k columns w_0 <= ... <= w_(k-1) of ``d2_f32``: with
    L = min(k, 64), S_l = w_l + w_(l+64) + w_(l+128) + ... over the positions < k, added left to right in float32; then
    S_0 + S_1 + ... + S_(L-1), added left to right in float32; divided by float32(k) -> (Q,) float32."""
    L = min(k, 64)
    S = d2_f32[:, :L].astype(np.float32).copy()
    for base in range(64, k, 64):                       # ascending stride: position l + base joins S_l
        w = min(64, k - base)
        S[:, :w] = (S[:, :w] + d2_f32[:, base:base + w].astype(np.float32)).astype(np.float32)
    acc = S[:, 0].copy()
    for l in range(1, L):
        acc = (acc + S[:, l]).astype(np.float32)
    return (acc / np.float32(k)).astype(np.float32)


def _agrees_with_the_sequential_sum_up_to_64():
    rng = np.random.default_rng(5)
    table = np.sort(rng.random((40, 64), dtype=np.float32) * np.float32(1000.0), axis=1)
    for k in range(1, 65):
        a, b = dtm_words_wide(table, k), kr.dtm_words(table, k)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


_agrees_with_the_sequential_sum_up_to_64()


def statistic_words(d2_f32: np.ndarray, k: int, stat: int) -> np.ndarray:
    """The (Q,) uint32 words ``out_bits`` must hold for ``stat`` (0: the k-th d2 word, 1: the strided sum)."""
    v = d2_f32[:, k - 1].astype(np.float32).copy() if stat == 0 else dtm_words_wide(d2_f32, k)
    return np.ascontiguousarray(v).view(np.uint32)


def smallest_keys(P: np.ndarray, pos: np.ndarray, k_max: int, dev):
    """Integer brute force for integer points ``P`` and half-integer positions ``pos``: the m = min(k_max + 1, n)
    smallest (d2, id) keys per position -> (d2 (Q, m) float32, exact; ids (Q, m) int64; d2 in quarters (Q, m) int64
    tensor on ``dev``)."""
    m = min(k_max + 1, P.shape[0])
    d2q, ids = kr.smallest_keys_int(torch.as_tensor(2 * P, dtype=torch.int64, device=dev),
                                    torch.as_tensor(np.round(2 * pos), dtype=torch.int64, device=dev), m)
    d2f = (d2q.to(torch.float32) / 4).cpu().numpy()      # exact: an integer below 2**24 over four
    return d2f, ids.cpu().numpy(), d2q


def brute_statistic(P, Q, k, stat):
    """float64 brute force over ALL points: the SQUARED statistic per row of Q (duplicates are separate columns)."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    out = np.empty(Q.shape[0])
    for a in range(0, Q.shape[0], 2048):
        d2 = np.sort(((Q[a:a + 2048, None, :] - P[None, :, :]) ** 2).sum(axis=2), axis=1)[:, :k]
        out[a:a + 2048] = d2[:, -1] if stat == "kth" else d2.sum(axis=1) / k
    return out


def brute_flood_reference(fc, P, L, k, stat, ppe):
    """{simplex: value} of every simplex of the dict ``fc`` from the float64 brute force over all points: the samples of
    the simplex's own lattice (float32 weights and vertices, as the sweep sees them), the maximum over them, then the
    monotone pass over the facets."""
    import itertools

    from flooder_amd import core

    by_dim = {}
    for key in fc:
        by_dim.setdefault(len(key) - 1, []).append(key)
    ref = {}
    for d in sorted(by_dim):
        keys = by_dim[d]
        w = np.ones((1, 1), dtype=np.float32) if d == 0 else core.generate_grid(ppe, d, "cpu", torch.float32)[0].numpy()
        verts = np.asarray(L, dtype=np.float32)[np.array(keys)]
        samples = np.matmul(w[None], verts).astype(np.float32).reshape(-1, P.shape[1])
        vals = np.sqrt(brute_statistic(P, samples, k, stat)).reshape(len(keys), w.shape[0]).max(axis=1)
        for key, v in zip(keys, vals.tolist()):
            for face in itertools.combinations(key, d) if d > 0 else ():
                v = max(v, ref[face])
            ref[key] = v
    return ref


def exact_flood_reference(fc, points: torch.Tensor, landmarks: torch.Tensor, ppe: int, k: int, stat: str):
    """{simplex: float32 value} of every simplex of ``fc`` on an EXACT input (integer points, dyadic lattice): per
    simplex the lattice samples in float64, the k smallest d2 of every sample by ``knn_grad_reference.smallest_keys_f64``
    (exact, equal to the float32 words), the statistic in the wide kernel's arithmetic (the strided sum), the maximum
    over the samples and its float32 root.  A facet's lattice is a subset of its coface's, so the monotone pass raises
    nothing."""
    import grad_reference as gr

    dev = points.device
    by_dim = {}
    for key in fc:
        by_dim.setdefault(len(key) - 1, []).append(key)
    ref = {}
    for d, keys in sorted(by_dim.items()):
        W = gr.lattice(ppe, d).to(dev)
        V = landmarks.double().to(dev)[torch.as_tensor(keys, device=dev).long()]
        samples = torch.einsum("rk,skd->srd", W, V)
        S, R, dim = samples.shape
        d2, _ = kr.smallest_keys_f64(points, samples.reshape(-1, dim), k, (ppe - 1) ** 2)
        d2f = d2.to(torch.float32).cpu().numpy()
        assert np.array_equal(d2f.astype(np.float64), d2.cpu().numpy())
        words = statistic_words(d2f, k, 0 if stat == "kth" else 1).view(np.float32).reshape(S, R)
        vals = np.sqrt(words.max(axis=1).astype(np.float64)).astype(np.float32)   # (53 >= 2 * 24 + 2 bits)
        ref.update(zip(keys, vals))
    return ref
