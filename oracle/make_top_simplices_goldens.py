"""Record ``flood_complex_oracle`` with random weights on the 5-D and 8-D clouds of ``tests/top_simplices_cases.py``.

    python oracle/make_top_simplices_goldens.py

writes ``tests/golden/top_rand_<config>_<num_rand>.npz`` (simplices padded with -1, float64 values, the seed).  The
oracle queries a kd-tree once per sample: 40 million queries in 8-D for 1100 weights per simplex of every dimension,
two minutes on eight cores - too long for a test that runs with every change, so its result is kept.  The weights come
from the global CPU generator of torch (``torch.manual_seed(SEED)``), as in the calls the tests compare with."""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SEED = 5
CASES = [("A", 40), ("A", 1100), ("D", 40), ("D", 1100)]


def main():
    import top_simplices_cases as cases
    from oracle import flood_oracle as fo

    for name, num_rand in CASES:
        P, L, _ = cases.config(name)
        torch.manual_seed(SEED)
        ref = fo.flood_complex_oracle(P, L, points_per_edge=None, num_rand=num_rand, workers=-1)
        keys = sorted(ref)
        simplices = np.full((len(keys), P.shape[1] + 1), -1, dtype=np.int16)
        for i, key in enumerate(keys):
            simplices[i, :len(key)] = key
        path = os.path.join(ROOT, "tests", "golden", f"top_rand_{name}_{num_rand}.npz")
        np.savez_compressed(path, simplices=simplices, filtration=np.array([ref[k] for k in keys], dtype=np.float64),
                            weight_seed=np.int64(SEED), num_rand=np.int64(num_rand))
        print(path, len(keys), os.path.getsize(path))


if __name__ == "__main__":
    main()
