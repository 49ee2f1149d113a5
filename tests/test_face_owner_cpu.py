"""Face ownership, the host side (no GPU): the row tables of ``SamplePlan`` (minimal face per row, groups, chunk and
tile masks, sub-face table), the precondition - a shared face's samples are bit-equal from every incident cell with
ascending vertex ids, and not in general otherwise -, and a numpy model of the whole scheme: every row evaluated once,
by the owner of its minimal face, delivered to the faces of that simplex, closure applied = the exhaustive maxima."""
import itertools

import numpy as np
import pytest
import torch

from flooder_amd import core

F32 = np.float32
CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def owner_on():
    keep = core.FACE_OWNER, core.FACE_OWNER_GROUPED
    core.FACE_OWNER = True
    yield
    core.FACE_OWNER, core.FACE_OWNER_GROUPED = keep


_PLANS = {}


def plan_of(dim, n, grouped=True):
    """the plan with the rows grouped by facet (core.FACE_OWNER_GROUPED) or in the patch order of sample_order"""
    if (dim, n, grouped) not in _PLANS:
        w, vi, fi = core.generate_grid(n, dim, CPU, torch.float32)
        core.FACE_OWNER_GROUPED = grouped
        plan = core.SamplePlan(w, core._FaceTable(fi, w.shape[0], CPU))
        vsets = [frozenset(int(x) for x in row) for v in vi for row in v.numpy()]
        _PLANS[(dim, n, grouped)] = (w.numpy(), vsets, plan)
    return _PLANS[(dim, n, grouped)]


GRIDS = [(dim, n) for dim in (2, 3) for n in (2, 3, 6, 12, 30)]


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("dim,n", GRIDS)
def test_minimal_face_against_brute_force(dim, n, grouped):
    w, vsets, plan = plan_of(dim, n, grouped)
    assert plan.owner_order and plan.min_face is not None
    got = plan.min_face.numpy()
    for pos, r in enumerate(plan._perm):
        supp = frozenset(np.nonzero(w[r])[0].tolist())
        holding = [f for f, vs in enumerate(vsets) if supp <= vs]
        fewest = min(len(vsets[f]) for f in holding)
        minimal = [f for f in holding if len(vsets[f]) == fewest]
        assert minimal == [int(got[pos])] and vsets[minimal[0]] == supp


@pytest.mark.parametrize("dim,n", GRIDS)
def test_groups_partition_the_rows_and_the_order_is_a_permutation(dim, n):
    w, vsets, plan = plan_of(dim, n)
    R = w.shape[0]
    assert sorted(plan._perm.tolist()) == list(range(R))
    assert np.array_equal(plan.inv.numpy()[plan._perm], np.arange(R))
    g = plan.row_group
    assert g.shape == (R,) and (np.diff(g) >= 0).all()                     # one contiguous block per group
    mf = plan.min_face.numpy()
    assert ((g == 0) == (mf == 0)).all()                                   # interior rows first, all of them
    for pos in range(R):                                                   # a boundary row sits with a facet it lies on
        if g[pos]:
            assert len(vsets[g[pos]]) == dim and vsets[mf[pos]] <= vsets[g[pos]]
    # the weights and the face table follow the order
    assert np.array_equal(plan.w_perm.numpy(), w[plan._perm].astype(F32))


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("dim,n", GRIDS)
def test_chunk_and_tile_masks_are_the_or_of_their_rows(dim, n, grouped):
    w, vsets, plan = plan_of(dim, n, grouped)
    bits = (1 << plan.min_face.numpy().astype(np.int64))
    for run, tab in ((256, plan.chunk_faces), (64, plan.tile_faces)):
        tab = tab.numpy().view(np.uint32)
        assert tab.shape[0] == -(-w.shape[0] // run)
        for j in range(tab.shape[0]):
            assert int(tab[j]) == int(np.bitwise_or.reduce(bits[j * run:(j + 1) * run]))
    if n == 30 and dim == 3:
        assert plan.chunk_faces.shape[0] == 20 and plan.tile_faces.shape[0] == 78


@pytest.mark.parametrize("dim,n", GRIDS)
def test_patch_order_is_the_order_of_sample_order(dim, n):
    """FACE_OWNER_GROUPED off (the default): the rows stay where sample_order puts them, the row tables follow"""
    w, vsets, plan = plan_of(dim, n, grouped=False)
    assert plan.owner_order and plan.row_group is None
    assert np.array_equal(plan._perm, core.sample_order(torch.as_tensor(w)))
    assert np.array_equal(plan.w_perm.numpy(), w[plan._perm].astype(F32))


@pytest.mark.parametrize("dim", [2, 3])
def test_sub_face_table_against_itertools(dim):
    w, vsets, plan = plan_of(dim, 6)
    combos = [frozenset(c) for k in range(dim + 1, 0, -1) for c in itertools.combinations(range(dim + 1), k)]
    assert sorted(map(sorted, combos)) == sorted(map(sorted, vsets))
    sub = plan.sub_faces.numpy().view(np.uint32)
    for f, vf in enumerate(vsets):
        assert int(sub[f]) == sum(1 << g for g, vg in enumerate(vsets) if vg <= vf)


def fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64 (a double rounding of the sum can
    differ from the hardware's in the last bit - both sides of a comparison below go through this same function)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def sample_chain(w, verts):
    """the kernels' sample: p = fma(w[j], v[j], p) over the vertices in ROW order, from p = 0; w (R, k1), verts (k1, dim)"""
    p = np.zeros((w.shape[0], verts.shape[1]), F32)
    for j in range(w.shape[1]):
        p = fma32(w[:, j:j + 1].astype(F32), verts[j][None, :].astype(F32), p)
    return p


def face_rows(w, cols_zero):
    return np.nonzero((w[:, cols_zero] == 0).all(axis=1))[0]


def test_shared_face_samples_are_bit_equal_with_ascending_ids_only():
    rng = np.random.default_rng(5)
    w = core.generate_grid(12, 3, CPU, torch.float32)[0].numpy().astype(F32)
    X = (rng.standard_normal((5, 3)) * 3 + 100).astype(F32)
    a, b = X[[0, 1, 2, 3]], X[[1, 2, 3, 4]]          # cells (0 1 2 3) and (1 2 3 4) share the triangle (1 2 3)
    ra, rb = face_rows(w, [0]), face_rows(w, [3])
    # the same lattice point of the face: weights (0, i, j, k) in the first cell, (i, j, k, 0) in the second
    key_a = {tuple(w[r, 1:]): r for r in ra}
    pa, pb = sample_chain(w, a), sample_chain(w, b)
    n = 0
    for r in rb:
        q = key_a[tuple(w[r, :3])]
        assert pa[q].tobytes() == pb[r].tobytes()
        n += 1
    assert n == len(ra) == 78
    # the precondition, written down: a cell that lists the shared vertices in another order - (1 3 2 4) - adds the same
    # three products in another order, and float32 addition is not associative
    c = X[[1, 3, 2, 4]]
    pc = sample_chain(w, c)
    differ = 0
    for r in rb:
        i, j, k = w[r, :3]
        r2 = np.nonzero((w[:, 0] == i) & (w[:, 1] == k) & (w[:, 2] == j) & (w[:, 3] == 0))[0][0]
        differ += pb[r].tobytes() != pc[r2].tobytes()
    assert differ > 0


# ---- the whole scheme in numpy

def exhaustive(w, memb_bits, cells, lms, cloud):
    """d2[s, r] over a cloud (float32 positions from the chain, float64 distances) and the per-(simplex, face) maxima"""
    S, F = cells.shape[0], memb_bits.shape[1]
    d2 = np.empty((S, w.shape[0]))
    for s in range(S):
        p = sample_chain(w, lms[cells[s]]).astype(np.float64)
        d2[s] = ((p[:, None, :] - cloud[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    face_max = np.stack([np.where(memb_bits[:, f][None, :], d2, -1.0).max(axis=1) for f in range(F)], axis=1)
    return d2, face_max


def owned_scheme(d2, memb_bits, min_face, sub, slot, n_slots, weight):
    S, F = slot.shape
    key = [(-1 if weight[s] < 0 else weight[s], s) for s in range(S)]       # handled, then lightest, then lowest row
    owner = np.full(n_slots, -1)
    for s in sorted(range(S), key=lambda s: key[s], reverse=True):
        owner[slot[s, 1:]] = s
    raw = np.zeros(n_slots)
    evaluated = np.zeros((n_slots,), np.int64)                              # simplices that evaluate a face's own rows
    for s in range(S):
        for f in range(1, F):
            evaluated[slot[s, f]] += owner[slot[s, f]] == s
        for r in range(d2.shape[1]):
            f0 = min_face[r]
            if f0 == 0 or owner[slot[s, f0]] == s:
                for f in np.nonzero(memb_bits[r])[0]:
                    raw[slot[s, f]] = max(raw[slot[s, f]], d2[s, r])
    out = np.full(n_slots, -1.0)
    for s in range(S):
        for f in range(F):
            v = max(raw[slot[s, g]] for g in range(F) if (int(sub[f]) >> g) & 1)
            assert out[slot[s, f]] in (-1.0, v)                             # duplicate writers write identical values
            out[slot[s, f]] = v
    return out, evaluated, raw


def complex_of(cells, n_points, dim):
    cells = np.sort(np.asarray(cells, np.int64), axis=1)
    stree, simplices = core._cell_complex(cells, n_points, dim)
    top = np.sort(np.asarray(simplices[dim]), axis=1)
    return stree, top


def check_scheme(dim, lms, cells, mine=None, seed=0):
    n = 4
    w, vsets, plan = plan_of(dim, n)
    w = w.astype(F32)
    vi = core.generate_grid(n, dim, CPU, torch.float32)[1]
    stree, top = complex_of(cells, lms.shape[0], dim)
    rows = stree._locate(dim, top)
    slot, n_slots, _ = core.shared_face_slots(stree, dim, rows, [v.numpy() for v in vi], CPU)
    slot = slot.numpy()
    if mine is not None:
        top, slot = top[mine], slot[mine]
    rng = np.random.default_rng(seed)
    cloud = rng.standard_normal((300, dim)) * 1.5
    F = slot.shape[1]
    memb = plan.memb_all.numpy().view(np.uint32)[plan.inv.numpy()]         # original row order, like w
    memb_bits = ((memb[:, None] >> np.arange(F)[None, :]) & 1).astype(bool)
    min_face = plan.min_face.numpy()[plan.inv.numpy()]
    d2, face_max = exhaustive(w, memb_bits, top, lms.astype(F32), cloud)
    # the values the project already relies on: every incident cell gives a face the same maximum
    want = np.full(n_slots, -1.0)
    for s in range(top.shape[0]):
        for f in range(F):
            assert want[slot[s, f]] in (-1.0, face_max[s, f])
            want[slot[s, f]] = face_max[s, f]
    weight = rng.integers(0, 5, top.shape[0]).astype(np.float64)            # ties on purpose
    weight[rng.random(top.shape[0]) < 0.3] = -1.0                          # ... and simplices the witness sweep handled
    out, evaluated, raw = owned_scheme(d2, memb_bits, min_face, plan.sub_faces.numpy().view(np.uint32), slot, n_slots, weight)
    touched = np.zeros(n_slots, bool)
    touched[slot.reshape(-1)] = True
    proper = np.zeros(n_slots, bool)
    proper[slot[:, 1:].reshape(-1)] = True
    assert (evaluated[proper] == 1).all() and (evaluated[~proper] == 0).all()   # every shared row once
    assert (raw <= np.where(touched, want, 0.0)).all()                          # a raw word never exceeds the value
    assert np.array_equal(out[touched], want[touched])                          # closure = exhaustive, exactly
    assert (out[~touched] == -1.0).all()
    return top, slot


@pytest.mark.parametrize("dim", [2, 3])
def test_model_on_a_random_delaunay_complex(dim):
    rng = np.random.default_rng(dim)
    lms = rng.standard_normal((14 if dim == 3 else 20, dim))
    cells = core.delaunay_cells(lms)
    top, slot = check_scheme(dim, lms, cells)
    # hull faces: facets with ONE incident cell are there and are owned by it like any other
    counts = np.bincount(slot[:, 1:dim + 2].reshape(-1))
    assert (counts == 1).any() and (counts == 2).any()


@pytest.mark.parametrize("dim", [2, 3])
def test_model_on_one_cell_and_on_two_cells_sharing_a_facet(dim):
    rng = np.random.default_rng(10 + dim)
    lms = rng.standard_normal((dim + 2, dim))
    check_scheme(dim, lms, [list(range(dim + 1))])
    check_scheme(dim, lms, [list(range(dim + 1)), list(range(1, dim + 2))])


@pytest.mark.parametrize("dim", [2, 3])
def test_model_on_a_share_of_the_cells(dim):
    """a rank's share (every third cell) chooses owners among its own cells: its faces' values stay complete"""
    rng = np.random.default_rng(20 + dim)
    lms = rng.standard_normal((16 if dim == 3 else 24, dim))
    cells = core.delaunay_cells(lms)
    n_cells = np.asarray(cells).shape[0]
    check_scheme(dim, lms, cells, mine=np.arange(0, n_cells, 3))
