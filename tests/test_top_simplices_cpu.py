"""The host half of the default call in 5-D to 8-D (Delaunay in n-D, face tables of up to 511 columns, the monotone
pass) without a GPU: ``flood_complex`` on CPU tensors with ``max_dimension`` left at its default against
``oracle.flood_oracle.flood_complex_oracle`` on the configurations A to D of ``top_simplices_cases``."""

import itertools

import numpy as np
import pytest

import top_simplices_cases as cases
from helpers import assert_close_filtration

NAMES = ("A", "B", "C", "D")


def test_configurations_sweep_six_to_nine_vertices():
    assert [cases.CONFIGS[n][0] for n in NAMES] == [5, 6, 7, 8]
    assert [cases.n_faces(cases.CONFIGS[n][0]) for n in NAMES] == [63, 127, 255, 511]
    for name in NAMES:
        dim, n, n_l, ppe = cases.CONFIGS[name]
        P, L, _ = cases.config(name)
        assert P.shape == (n, dim) and L.shape == (n_l, dim) and P.dtype == np.float32
        assert np.unique(P, axis=0).shape[0] == n - cases.N_DUPLICATES


@pytest.mark.parametrize("name", NAMES)
def test_cpu_path_equals_the_oracle(name):
    dim = cases.CONFIGS[name][0]
    P, L, ppe = cases.config(name)
    ref, got = cases.oracle(name), cases.cpu_dict(name)
    assert set(got) == set(ref)
    assert max(len(k) for k in ref) == dim + 1, "no top-dimensional simplex"
    keys = sorted(ref)
    worst = assert_close_filtration([got[k] for k in keys], [ref[k] for k in keys], P, name, strict=True)
    top = sum(len(k) == dim + 1 for k in keys)
    print(f"{name}: {len(keys)} simplices, {top} of {dim + 1} vertices, worst abs err {worst:.3e}")


@pytest.mark.parametrize("name", NAMES)
def test_tree_is_monotone_and_has_one_component(name):
    st = cases.cpu_tree(name)
    fc = st.to_dict() if hasattr(st, "to_dict") else {tuple(s): v for s, v in st.get_simplices()}
    assert fc == cases.cpu_dict(name)
    assert all(np.isfinite(v) and v >= 0 for v in fc.values())
    for key, v in fc.items():
        for face in itertools.combinations(key, len(key) - 1) if len(key) > 1 else ():
            assert fc[face] <= v, (face, key)
    st.compute_persistence()
    h0 = np.asarray(st.persistence_intervals_in_dimension(0))
    assert h0.ndim == 2 and int(np.isinf(h0[:, 1]).sum()) == 1, "exactly one infinite H0 bar: one component"
