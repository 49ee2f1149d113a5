"""The clouds of the top-dimensional tests (``test_top_simplices_cpu.py``, ``test_gpu_top_simplices.py``): 5-D to 8-D,
``max_dimension`` left at its default, so the swept simplices have 6 to 9 vertices and 63 to 511 faces.  Everything
here is host-side and cached: a configuration, the oracle's dict and the CPU path's dict are computed once per run."""

import functools

import numpy as np
import torch

N_DUPLICATES = 300

# name -> (ambient dimension, points, landmarks, points_per_edge)
CONFIGS = {"A": (5, 20_000, 40, 4), "B": (6, 20_000, 24, 4), "C": (7, 10_000, 24, 3), "D": (8, 10_000, 20, 3),
           "E": (5, 20_000, 60, 5)}


@functools.lru_cache(maxsize=None)
def config(name):
    """(points (n, dim) float32 with 300 exact duplicate rows among them, landmarks by exact farthest-point sampling
    from row 0, points_per_edge); numpy, not to be written to."""
    from oracle import flood_oracle as fo

    dim, n, n_l, ppe = CONFIGS[name]
    rng = np.random.default_rng(100 * dim + n_l + ppe)
    P = rng.standard_normal((n - N_DUPLICATES, dim)).astype(np.float32)
    P = np.concatenate([P, P[rng.choice(n - N_DUPLICATES, size=N_DUPLICATES, replace=False)]])[rng.permutation(n)]
    P = np.ascontiguousarray(P)
    assert np.unique(P, axis=0).shape[0] == n - N_DUPLICATES
    L = np.ascontiguousarray(P[fo.exact_fps(P, n_l, 0)])
    return P, L, ppe


@functools.lru_cache(maxsize=None)
def oracle(name):
    from oracle import flood_oracle as fo

    P, L, ppe = config(name)
    return fo.flood_complex_oracle(P, L, points_per_edge=ppe)


@functools.lru_cache(maxsize=None)
def cpu_tree(name):
    """``flood_complex`` on CPU tensors, as a simplex tree."""
    import flooder_amd as fa

    P, L, ppe = config(name)
    return fa.flood_complex(torch.as_tensor(P), torch.as_tensor(L), points_per_edge=ppe, return_simplex_tree=True)


@functools.lru_cache(maxsize=None)
def cpu_dict(name):
    import flooder_amd as fa

    P, L, ppe = config(name)
    return fa.flood_complex(torch.as_tensor(P), torch.as_tensor(L), points_per_edge=ppe)


def n_faces(dim):
    return 2 ** (dim + 1) - 1


def rows_per_simplex(ppe, d):
    from math import comb

    return comb(ppe + d - 1, d)
