"""The hand-off of a dimension pass (``core._handoff_items`` + ``core._apply_items``) against a plain dict.

Made-up, pairwise distinct face values go through the items onto the simplex tree; the reference is a Python dict
updated simplex by simplex and face by face in queue order, vertex tuples sorted - what the reference implementation's
``dict.update`` loop leaves behind.  Neighbouring Delaunay simplices share faces, so "later rows win" decides most
entries.  Everything is compared BEFORE ``make_filtration_non_decreasing``.
"""

import numpy as np
import pytest
import torch

from flooder_amd import core
from flooder_amd.simplex_tree import SimplexTree

N_LANDMARKS = 12


def _landmarks(dim):
    return torch.rand(N_LANDMARKS, dim, generator=torch.Generator().manual_seed(7 + dim), dtype=torch.float64)


def _passes(lms, simplices, num_rand, queue):
    return list(core._dimension_passes(simplices, lms, 0, 4, num_rand, queue))


def _made_up(p):
    """(S, F) distinct floats, distinct across the passes of a call as well."""
    S, F = p.order_np.shape[0], p.faces.n_faces
    return 1000.0 * p.d + np.arange(S * F, dtype=np.float64).reshape(S, F) / 8 + 0.125


def _naive(p, face_vals, into):
    for s, simplex in enumerate(p.simp_h.tolist()):
        if p.v_idx_np is None:                       # random samples: one face, the simplex itself
            into[tuple(sorted(simplex))] = face_vals[s, 0]
            continue
        col = 0
        for v_idx in p.v_idx_np:
            for positions in v_idx.tolist():
                into[tuple(sorted(simplex[i] for i in positions))] = face_vals[s, col]
                col += 1
    return into


def _assigned(tree):
    return {k: v for k, v in tree.to_dict().items() if not np.isnan(v)}


def _run(tree, passes):
    """-> (kinds of the items, values on the tree, the naive dict)."""
    items, want = [], {}
    for p in passes:
        vals = _made_up(p)
        items += core._handoff_items(tree, p, vals)
        _naive(p, vals, want)
    core._apply_items(tree, items)
    return {item[0] for item in items}, _assigned(tree), want


@pytest.mark.parametrize("queue", ["tree", "ball"])
@pytest.mark.parametrize("dim", [2, 3])
def test_grid_on_the_top_cells_goes_through_the_cell_face_index(dim, queue):
    lms = _landmarks(dim)
    tree, simplices = core._build_complex(lms, dim)
    passes = _passes(lms, simplices, None, queue)
    assert [p.d for p in passes] == [dim] and passes[0].order_np.shape[0] > 1
    kinds, got, want = _run(tree, passes)
    assert kinds == {"cells"}
    assert got == want and len(want) == tree.num_simplices()      # every simplex of the complex is a face of a cell


@pytest.mark.parametrize("queue", ["tree", "ball"])
@pytest.mark.parametrize("dim,max_dimension", [(2, 1), (3, 2)])
def test_grid_below_the_top_dimension_knows_its_own_rows_and_the_vertices(dim, max_dimension, queue):
    lms = _landmarks(dim)
    tree, simplices = core._build_complex(lms, max_dimension)
    kinds, got, want = _run(tree, _passes(lms, simplices, None, queue))
    assert kinds == ({"rows"} if max_dimension == 1 else {"rows", "bulk"})   # (the edges of triangles: located by key)
    assert got == want
    assert len(want) == sum(s.shape[0] for s in simplices)


@pytest.mark.parametrize("queue", ["tree", "ball"])
@pytest.mark.parametrize("dim", [2, 3])
def test_random_samples_assign_every_dimension_by_key(dim, queue):
    lms = _landmarks(dim)
    tree, simplices = core._build_complex(lms, dim)
    passes = _passes(lms, simplices, 5, queue)
    assert [p.d for p in passes] == list(range(dim + 1)) and all(p.weights.shape == (5, p.d + 1) for p in passes)
    kinds, got, want = _run(tree, passes)
    assert kinds == {"bulk"}
    assert got == want and len(want) == tree.num_simplices()


@pytest.mark.parametrize("dim", [2, 3])
def test_a_tree_without_cells_locates_faces_by_key(dim):
    lms = _landmarks(dim)
    _, simplices = core._build_complex(lms, dim)
    tree = SimplexTree.from_arrays(simplices)
    kinds, got, want = _run(tree, _passes(lms, simplices, None, "tree"))
    assert kinds == {"rows", "bulk"}
    assert got == want and len(want) == tree.num_simplices()


@pytest.mark.parametrize("dim", [2, 3])
def test_table_items_overwrite_whole_tables_in_their_place_in_the_order(dim):
    lms = _landmarks(dim)
    tree, simplices = core._build_complex(lms, dim)
    (p,) = _passes(lms, simplices, None, "tree")
    vals = _made_up(p)
    edges = tree.simplices_of_dimension(1)
    edge_vals = -1.0 - np.arange(edges.shape[0], dtype=np.float64)
    first = _made_up(p) + 5000.0
    items = (core._handoff_items(tree, p, first) + [("table", 1, None, edge_vals)]
             + [it for it in core._handoff_items(tree, p, vals) if it[1] != 1])
    core._apply_items(tree, items)
    want = _naive(p, first, {})
    want.update((tuple(e), v) for e, v in zip(edges.tolist(), edge_vals.tolist()))
    want.update((k, v) for k, v in _naive(p, vals, {}).items() if len(k) != 2)
    assert _assigned(tree) == want


@pytest.mark.parametrize("dim", [2, 3])
def test_slot_offsets_turn_one_value_per_distinct_face_into_table_items(dim):
    lms = _landmarks(dim)
    tree, simplices = core._build_complex(lms, dim)
    (p,) = _passes(lms, simplices, None, "tree")
    # the layout of shared_face_slots: codimension after codimension, the rows of each table in table order
    tables = [tree.simplices_of_dimension(v_idx.shape[1] - 1) for v_idx in p.v_idx_np]
    offsets = np.concatenate([[0], np.cumsum([t.shape[0] for t in tables])])
    slot_vals = 0.5 + np.arange(offsets[-1], dtype=np.float64)
    items = core._handoff_items(tree, p, slot_vals, offsets[:-1].tolist())
    assert {it[0] for it in items} == {"table"} and len(items) == dim + 1
    core._apply_items(tree, items)
    want = {tuple(r): slot_vals[off + i] for t, off in zip(tables, offsets) for i, r in enumerate(t.tolist())}
    assert _assigned(tree) == want
