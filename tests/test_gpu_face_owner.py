"""Face ownership on the GPU (core.FACE_OWNER; csrc/flood_cell.hip, flood_finish.hip: face_closure_kernel): with one
incident simplex evaluating a shared face's own samples and the closure in the last launch, every face value has the
same bits as with every simplex evaluating every row, and as the (S, F) path without shared slots.  Runs on a real
MI355X only (-m gpu)."""
import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from oracle import flood_oracle as fo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def cloud(name, n):
    g = torch.Generator().manual_seed(11)
    if name == "gauss":
        return torch.randn(n, 3, generator=g)
    if name == "cube":
        return torch.rand(n, 3, generator=g)
    if name == "torus":
        return torch.as_tensor(fo.noisy_torus(n, seed=3), dtype=torch.float32)
    if name == "plane":
        return torch.randn(n, 2, generator=g)
    raise ValueError(name)


class Case:
    """a cloud, a complex on landmarks of it (or on given cells) and the lattice: everything a sweep needs"""

    def __init__(self, pts, ppe, n_lms=None, lms=None, cells=None):
        self.pts = pts.to(DEV)
        d = self.d = pts.shape[1]
        self.lms = fa.generate_landmarks(self.pts, n_lms, start_idx=0) if lms is None else lms.to(DEV)
        if cells is None:
            self.stree, simplices = core._build_complex(self.lms, d)
        else:
            self.stree, simplices = core._cell_complex(np.asarray(cells, np.int64), self.lms.shape[0], d)
        self.simp = np.asarray(simplices[d])
        self.weights, self.vertex_idxs, face_idxs = core.generate_grid(ppe, d, DEV, torch.float32)
        self.faces = core._FaceTable(face_idxs, self.weights.shape[0], DEV)
        rows = self.stree._locate(d, np.sort(self.simp, axis=1))
        self.slot, self.n_slots, _ = core.shared_face_slots(self.stree, d, rows, [v.cpu().numpy() for v in self.vertex_idxs], DEV)
        self.index = core.PointIndex(self.pts)

    def sweep(self, owner, slots=True, mine=None, stats=None, grouped=False, spare=0):
        """`spare`: slots behind the complex's own that no simplex touches"""
        keep = core.FACE_OWNER, core.FACE_OWNER_GROUPED
        core.FACE_OWNER, core.FACE_OWNER_GROUPED = owner, grouped
        try:
            plan = core.SamplePlan(self.weights, self.faces)
            assert plan.owner_order == owner
            simp, slot = self.simp, self.slot
            if mine is not None:
                simp, slot = simp[mine], slot[torch.as_tensor(mine, device=DEV)].contiguous()
            verts = self.lms[torch.as_tensor(simp, device=DEV)].contiguous()
            out, _ = core._sweep_dimension_cell(self.index, verts, self.weights, self.faces, None, stats=stats, plan=plan,
                                                face_slots=(slot, self.n_slots + spare) if slots else None)
            if mine is not None and slots:   # (what a rank contributes to the MIN over the ranks: bench.py)
                out = torch.maximum(out, core.shard_slot_fill(slot, self.n_slots))
            torch.cuda.synchronize()
            return out.cpu().numpy().view(np.int32)
        finally:
            core.FACE_OWNER, core.FACE_OWNER_GROUPED = keep

    def check(self, **kw):
        """ownership on the patch order (the default) and on the rows grouped by facet, against ownership off"""
        on, grouped, off = self.sweep(True, **kw), self.sweep(True, grouped=True, **kw), self.sweep(False, **kw)
        assert on.shape == grouped.shape == off.shape == (self.n_slots,)
        assert np.array_equal(on, off) and np.array_equal(grouped, off)
        return on


def no_slot_gathered(case, values, mine=None):
    """the (S, F) path - no shared words, no ownership - gives every (simplex, face) the value of its slot"""
    sf = case.sweep(True, slots=False, mine=mine)
    slot = case.slot.cpu().numpy()
    if mine is not None:
        slot = slot[mine]
    assert sf.shape == slot.shape
    assert np.array_equal(sf, values[slot])


@pytest.fixture(scope="module")
def gauss():
    return Case(cloud("gauss", 30_000), 16, n_lms=40)


def test_lattice_of_the_3d_cases_straddles_chunks():
    w, _, fi = core.generate_grid(16, 3, DEV, torch.float32)
    keep = core.FACE_OWNER, core.FACE_OWNER_GROUPED
    core.FACE_OWNER = core.FACE_OWNER_GROUPED = True
    try:
        plan = core.SamplePlan(w, core._FaceTable(fi, w.shape[0], DEV))
    finally:
        core.FACE_OWNER, core.FACE_OWNER_GROUPED = keep
    masks = plan.chunk_faces.cpu().numpy()
    assert w.shape[0] == 816 and masks.shape[0] == 4
    assert any(bin(int(m) & 0x1e).count("1") > 1 for m in masks)     # a chunk holds rows of more than one facet group


def test_gaussian_on_equals_off_equals_no_slots(gauss):
    """dense core: stage overflow and exhaustive chunks; below WIT_MIN_SIMPLICES: no witness sweep"""
    assert gauss.simp.shape[0] < core.WIT_MIN_SIMPLICES
    no_slot_gathered(gauss, gauss.check())


@pytest.mark.parametrize("name", ["cube", "torus"])
def test_cube_and_torus_on_equals_off_equals_no_slots(name):
    """a uniform cube; a noisy torus (a surface: finish-heavy, nothing for the witness sweep)"""
    case = Case(cloud(name, 30_000), 16, n_lms=40)
    no_slot_gathered(case, case.check())


def test_plane_on_equals_off_equals_no_slots():
    case = Case(cloud("plane", 20_000), 24, n_lms=60)
    no_slot_gathered(case, case.check())


def test_one_tetrahedron_and_two_sharing_a_triangle():
    pts = cloud("gauss", 30_000)
    lms = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.3, 0.9, 0.1], [0.4, 0.3, 0.8], [0.9, 0.9, 0.9]])
    for cells in ([[0, 1, 2, 3]], [[0, 1, 2, 3], [1, 2, 3, 4]]):
        case = Case(pts, 16, lms=lms, cells=cells)
        assert case.simp.shape[0] == len(cells)
        no_slot_gathered(case, case.check())


def test_with_the_witness_sweep(gauss):
    """the witness sweep evaluates all rows of its simplices, whoever owns their faces; the simplices it has handled
    own their faces in the cell sweep that follows"""
    keep = core.WIT_MIN_SIMPLICES, core.WIT_MAX_POINTS_PER_SIMPLEX
    core.WIT_MIN_SIMPLICES, core.WIT_MAX_POINTS_PER_SIMPLEX = 0, 1 << 40
    try:
        st = torch.zeros(40, dtype=torch.int64, device=DEV)
        with_wit = gauss.sweep(True, stats=st)
        assert int(st[16]) > 0                                      # simplices the witness sweep handled
        assert np.array_equal(with_wit, gauss.sweep(False))
    finally:
        core.WIT_MIN_SIMPLICES, core.WIT_MAX_POINTS_PER_SIMPLEX = keep
    assert np.array_equal(with_wit, gauss.sweep(True))             # ... and the same without it


def test_a_share_of_the_simplices(gauss):
    """every third simplex, as a rank of bench.py: owners among its own simplices, complete values for their faces,
    +inf for the faces of the others"""
    mine = np.arange(0, gauss.simp.shape[0], 3)
    part = gauss.check(mine=mine)
    full = gauss.sweep(True)
    touched = np.zeros(gauss.n_slots, bool)
    touched[gauss.slot.cpu().numpy()[mine].reshape(-1)] = True
    assert np.array_equal(part[touched], full[touched])
    assert (part[~touched].view(np.float32) == np.inf).all()
    no_slot_gathered(gauss, part, mine=mine)


def test_ownership_removes_work_on_the_gaussian(gauss):
    """work counters of the cell sweep: evaluated pairs and staged points strictly below those without ownership"""
    counts = {}
    for owner, grouped in ((True, False), (True, True), (False, False)):
        st = torch.zeros(40, dtype=torch.int64, device=DEV)
        gauss.sweep(owner, stats=st, grouped=grouped)
        counts[owner, grouped] = st[:2].cpu().numpy()
    print("pairs, staged points with ownership", counts[True, False].tolist(), "on rows grouped by facet",
          counts[True, True].tolist(), "without", counts[False, False].tolist())
    for key in ((True, False), (True, True)):
        assert counts[key][0] < counts[False, False][0] and counts[key][1] < counts[False, False][1]


def test_both_parities_of_the_pad_word_before_the_owner_words():
    """the owner words are 64-bit and follow the face words in the sweep's arena (core.fused_layout): with one spare slot
    more the pad word in front of them comes or goes, and no value may move"""
    case = Case(cloud("gauss", 20_000), 10, n_lms=40)
    S, n = case.simp.shape[0], case.n_slots
    before = [sum(core.fused_layout(S, n + spare, False, True)[0]["face_bits"]) for spare in (0, 1)]
    assert before[0] & 1 != before[1] & 1   # (the witness queue in front, where it runs, is an even number of words)
    for spare in (0, 1):
        owner_at, owner_words = core.fused_layout(S, n + spare, False, True)[0]["face_owner"]
        assert owner_at == before[spare] + (before[spare] & 1) and owner_at % 2 == 0 and owner_words == 2 * (n + spare)
    exact, padded = case.sweep(True), case.sweep(True, spare=1)
    assert exact.shape == (n,) and padded.shape == (n + 1,)
    assert np.array_equal(exact, padded[:n]) and padded[n] == 0   # (the bits of 0.0)
    assert np.array_equal(exact, case.sweep(False))
    verts = case.lms[torch.as_tensor(case.simp, device=DEV)].contiguous()
    tree, _ = core._sweep_dimension_bvh(case.index, verts, case.weights, case.faces, None)
    torch.cuda.synchronize()
    assert np.array_equal(tree.cpu().numpy().view(np.int32), exact[case.slot.cpu().numpy()])


def test_closure_entry_on_hand_made_words():
    lib = _native.load()
    w, vi, fi = core.generate_grid(3, 3, DEV, torch.float32)
    keep = core.FACE_OWNER
    core.FACE_OWNER = True
    try:
        sub = core.SamplePlan(w, core._FaceTable(fi, w.shape[0], DEV)).sub_faces
    finally:
        core.FACE_OWNER = keep
    F = 15
    sub_np = sub.cpu().numpy().view(np.uint32)

    def closure(bits, slot):
        bits_t = torch.as_tensor(np.asarray(bits, np.float32).view(np.int32), device=DEV)
        slot_t = torch.as_tensor(np.asarray(slot, np.int32), device=DEV)
        out = torch.zeros(bits_t.shape[0], dtype=torch.float32, device=DEV)
        _native.check(lib.flooder_face_closure_f32(_native.ptr(bits_t), _native.ptr(slot_t), _native.ptr(sub), slot_t.shape[0], F,
                                                   _native.ptr(out), _native.current_stream_ptr(DEV)), "flooder_face_closure_f32")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def model(bits, slot):
        bits, slot = np.asarray(bits, np.float32), np.asarray(slot)
        out = np.zeros(bits.shape[0], np.float32)
        for s in range(slot.shape[0]):
            for f in range(F):
                out[slot[s, f]] = np.sqrt(max(bits[slot[s, g]] for g in range(F) if (int(sub_np[f]) >> g) & 1))
        return out

    # one tetrahedron whose own word is raised by a vertex word only (face 11 is a vertex)
    one = np.arange(F)[None, :]
    bits = np.zeros(F, np.float32)
    bits[0], bits[11] = 2.0, 9.0
    got = closure(bits, one)
    assert got[0] == 3.0 and np.array_equal(got.view(np.uint32), model(bits, one).view(np.uint32))
    assert (got[[f for f in range(F) if (int(sub_np[f]) >> 11) & 1]] == 3.0).all()      # every face that holds the vertex
    assert (got[[f for f in range(F) if not (int(sub_np[f]) >> 11) & 1]] == 0.0).all()
    # +0 words stay +0
    assert np.array_equal(closure(np.zeros(F, np.float32), one).view(np.uint32), np.zeros(F, np.uint32))
    # two tetrahedra that share a triangle (face 1 of the first = face 4 of the second, with its edges and vertices):
    # the shared slots are written by several (simplex, face) pairs, all with the same bits; a slot of no pair keeps 0
    rng = np.random.default_rng(3)
    n_slots = 24
    vsets = [frozenset(int(x) for x in row) for v in vi for row in v.cpu().numpy()]
    assert vsets[1] == {1, 2, 3} and vsets[4] == {0, 1, 2}                # cells (0 1 2 3) and (1 2 3 4)
    two = np.stack([np.arange(F), np.arange(F)])
    fresh = iter(range(F, n_slots))
    for g in range(F):
        two[1, g] = vsets.index(frozenset(i + 1 for i in vsets[g])) if vsets[g] <= vsets[4] else next(fresh)
    assert len(set(two[0]) & set(two[1])) == 7
    bits = rng.random(n_slots).astype(np.float32)
    got = closure(bits, two)
    assert np.array_equal(got.view(np.uint32), model(bits, two).view(np.uint32))
    assert got[n_slots - 1] == 0.0 and (n_slots - 1) not in two
