"""The face-plane table (csrc/flood_planes.hpp: 24 float32 words per simplex) on the GPU, word for word.

The table has two writers: the prepare launch (flooder_simplex_prepare_f32) and the stand-alone plane launch that
flooder_fused_witness / flooder_fused_cell make when the caller passes planes_ready = 0.  Both must write what the
float32 replica of tests/wit_reference.py (`plane_row`) computes - the replica on which the CPU statements about the
witness sweep's margins rest (tests/test_wit_sorted_stage_cpu.py) - bit for bit: no tolerance, signed zeros included.
The output is prefilled with a NaN pattern and has guard words on both sides.

Inputs, in 2-D and 3-D: the replica's own simplices (random, slivers, flat, axis-parallel, dyadic, offset by 1e3), the
same times 2^-20 and 2^20, a scale at which `len2 > 1e-30f` fails for every face, families that cross each of the three
terms of the kernel's `ok` (the replica must report both outcomes of each), repeated vertices, faces of lower dimension
(every plane disabled), in launches of 1, 255, 257 and 4097 simplices.  Runs on a real MI355X only (-m gpu)."""
import numpy as np
import pytest
import torch

from flooder_amd import _native, core
from helpers import get_options, set_options
from test_gpu_planes_ready import fused_chain
from wit_reference import f32, plane_words, simplices

pytestmark = pytest.mark.gpu

N_POINTS, POINTS_PER_EDGE = 20_000, 10
NAN_WORD, GUARD_WORD, N_GUARD = 0x7FC0DEAD, 0x7FC0BEEF, 64   # (two quiet NaN with different payloads)
LAUNCH_SIZES = [1, 255, 257, 4097]   # one thread per simplex in blocks of 256: a part block, a full one + 1, many blocks


# ---------------------------------------------------------------------------------------------- inputs
def _ok_families(dim):
    """Families of simplices along which ONE term of `ok` changes sides (the other two hold):
    0  len2 > 1e-30                          a simplex shrunk until its normals' squared length passes 1e-30;
    1  len2 >= 1e-8 |e1|^2 |e2|^2  (3-D)     two edges of a face at an angle around 1e-4 (in 2-D len2 and l12 are the
                                             same expression of the same edge: the term cannot fail where term 0 holds);
    2  side^2 >= 1e-8 len2 sext^2            a vertex at a height around 1e-4 of the extent over the opposite face."""
    rng = np.random.default_rng(500 + dim)
    steps = np.geomspace(0.25, 4.0, 48)
    out = []
    base = rng.standard_normal((dim + 1, dim))
    at = 1e-30 ** (0.25 if dim == 3 else 0.5)   # len2 ~ scale^4 in 3-D (a cross product), scale^2 in 2-D (an edge)
    for i, t in enumerate(steps):
        out.append((f"term 0, step {i}", (base * (at * t)).astype(f32)))
    if dim == 3:
        for i, t in enumerate(steps):
            v = np.array([[0, 0, 0], [1, 0, 0], [2, 2e-4 * t, 0], [0.3, 0.4, 1.0]]) + 0.01 * rng.standard_normal((4, 3)) * [[0], [0], [0], [1]]
            out.append((f"term 1, step {i}", v.astype(f32)))
    for i, t in enumerate(steps):
        v = rng.standard_normal((dim + 1, dim))
        normal = np.linalg.svd(v[1:dim] - v[0])[2][-1] if dim == 3 else np.array([-(v[1] - v[0])[1], (v[1] - v[0])[0]]) / np.linalg.norm(v[1] - v[0])
        ext = np.abs(v[:dim] - v[0]).max()
        v[dim] = v[:dim].mean(0) + (1e-4 * t * ext) * normal
        out.append((f"term 2, step {i}", v.astype(f32)))
    return out


def _inputs(dim):
    """[(name, (dim + 1, dim) float32)]"""
    base = simplices(dim)
    out = list(base)
    for e in (-20, 20):   # (a power of two: the scaled simplex is exact)
        out += [(f"{name}, times 2^{e}", (v * f32(2.0 ** e)).astype(f32)) for name, v in base]
    # every face's len2 below 1e-30 (but well inside float32's normal range: 2^-120)
    tiny = f32(2.0 ** (-30 if dim == 3 else -60))
    out += [(f"{name}, planes disabled by scale", (v * tiny).astype(f32)) for name, v in base[:13]]
    out += _ok_families(dim)
    rng = np.random.default_rng(600 + dim)
    for j in range(1, dim + 1):   # vertex j repeats vertex 0
        v = rng.standard_normal((dim + 1, dim)).astype(f32)
        v[j] = v[0]
        out.append((f"vertex {j} repeats vertex 0", v))
    v = rng.standard_normal((dim + 1, dim)).astype(f32)
    v[dim] = v[dim - 1]
    out.append(("last vertex repeats the one before", v))
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    _native.load()
    return torch.device("cuda:0")


_cache = {}


def _setting(dim, k1, dev):
    """(point index, sample plan, face table) of one (dim, k1): the sweeps behind the plane launch need valid inputs"""
    key = (dim, k1)
    if key not in _cache:
        if ("index", dim) not in _cache:
            pts = torch.randn(N_POINTS, dim, generator=torch.Generator().manual_seed(31 + dim)).to(dev)
            _cache["index", dim] = core.PointIndex(pts)
        weights, _, face_idxs = core.generate_grid(POINTS_PER_EDGE, k1 - 1, dev, torch.float32)
        faces = core._FaceTable(face_idxs, weights.shape[0], dev)
        plan = core.SamplePlan(weights, faces)
        assert plan.memb_all is not None and plan.wit is not None, "no witness plan for this lattice"
        _cache[key] = (_cache["index", dim], plan, faces)
    return _cache[key]


def _reference(dim):
    """(names, vertices (n, dim + 1, dim), replica rows (n, 24) as uint32, per simplex the `ok` terms of its faces)"""
    key = ("reference", dim)
    if key not in _cache:
        names, verts, rows, terms = [], [], [], []
        for name, v in _inputs(dim):
            t = []
            names.append(name)
            verts.append(v)
            rows.append(plane_words(v, t).view(np.uint32))
            terms.append(t)
        _cache[key] = (names, np.stack(verts), np.stack(rows), terms)
    return _cache[key]


def _both_writers(dim, verts_np, dev):
    """(rows of the prepare launch, rows of the sweeps' own plane launch), each (S, 24) uint32; guards checked"""
    S, k1 = verts_np.shape[:2]
    index, plan, faces = _setting(dim, k1, dev)
    lib = _native.load()
    keep = get_options(lib, b"wit_surface_pct")
    got = []
    try:
        assert lib.flooder_set_option(b"wit_surface_pct", 0) == 0
        for planes_ready in (1, 0):
            buf = torch.full((24 * S + 2 * N_GUARD,), GUARD_WORD, dtype=torch.int32, device=dev)
            planes = buf[N_GUARD:N_GUARD + 24 * S].view(torch.float32)
            planes.view(torch.int32).fill_(NAN_WORD)
            # (1: the prepare launch writes into the NaN pattern and the sweeps keep their hands off; 0: the pattern is
            # put back behind the prepare launch and the sweeps' entries write the rows)
            refill = None if planes_ready else (lambda verts, p: p.view(torch.int32).fill_(NAN_WORD))
            verts = torch.as_tensor(verts_np, device=dev).contiguous()
            _, _, out = fused_chain(index, verts, plan, faces.n_faces, planes_ready, between=refill, planes=planes)
            assert out.data_ptr() == planes.data_ptr()
            words = buf.cpu().numpy().view(np.uint32)
            assert (words[:N_GUARD] == GUARD_WORD).all() and (words[N_GUARD + 24 * S:] == GUARD_WORD).all(), \
                f"planes_ready {planes_ready}: a guard word next to the table was overwritten"
            got.append(words[N_GUARD:N_GUARD + 24 * S].reshape(S, 24).copy())
    finally:
        set_options(lib, keep)
    return got


def _differences(got, want, names):
    bad = np.argwhere(got != want)
    return [f"{names[s]}: word {w}: {got[s, w]:#010x} for {want[s, w]:#010x}" for s, w in bad[:8]]


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("dim", [2, 3])
def test_the_inputs_cross_every_term_of_ok(dim):
    """The replica reports both outcomes of every term of `ok` with the other two holding, a scale at which every plane
    is disabled, and enabled planes on the scaled simplices: the comparison below sees both branches of each."""
    names, _, rows, terms = _reference(dim)
    for term in ((0, 2) if dim == 2 else (0, 1, 2)):
        others = [t for t in range(3) if t != term]
        faces = [f for name, ts in zip(names, terms) if name.startswith(f"term {term}") for f in ts]
        holds = sum(1 for f in faces if f[term] and all(f[o] for o in others))
        fails = sum(1 for f in faces if not f[term] and all(f[o] for o in others))
        print(f"dim {dim}, term {term}: {holds} faces on the side where it holds, {fails} where it alone fails")
        assert holds > 0 and fails > 0, (dim, term, holds, fails)
    if dim == 2:   # (term 1 compares one expression with 1e-8 of itself)
        assert all(f[1] for ts in terms for f in ts if f[0])
    po = rows.view(f32)[:, 7:24:5][:, :dim + 1]
    disabled = [bool((p == f32(3.0e38)).all()) for p in po]
    assert all(d for name, d in zip(names, disabled) if "planes disabled by scale" in name)
    assert all(not d for name, d in zip(names, disabled) if name.startswith("random") and "disabled" not in name)
    assert any(any(p == f32(3.0e38)) for name, p in zip(names, po) if "repeats" in name)


@pytest.mark.parametrize("n_simplices", LAUNCH_SIZES)
@pytest.mark.parametrize("dim", [2, 3])
def test_both_writers_equal_the_replica_word_for_word(dim, n_simplices, dev, monkeypatch):
    monkeypatch.setattr(core, "WIT_MIN_ROWS", 0)   # (a lattice of 10 points per edge gets a witness plan)
    names, verts, rows, _ = _reference(dim)
    # (the launches cycle through the inputs from different starts; 4097 simplices hold every input many times over)
    pick = (np.arange(n_simplices) + 7 * n_simplices) % len(names)
    prepared, launched = _both_writers(dim, verts[pick], dev)
    want, who = rows[pick], [names[i] for i in pick]
    for what, got in (("prepare launch", prepared), ("plane launch of the sweeps", launched)):
        assert not (got == NAN_WORD).any(), f"{what}: words of the prefill left"
        diff = _differences(got, want, who)
        assert not diff, f"dim {dim}, {what}: {int((got != want).sum())} of {got.size} words differ from the replica: {diff}"
    assert np.array_equal(prepared, launched)


@pytest.mark.parametrize("dim,k1", [(3, 3), (3, 2), (2, 2)])
def test_faces_of_lower_dimension_have_every_plane_disabled(dim, k1, dev, monkeypatch):
    """k1 < dim + 1 (triangles and edges in 3-D, edges in 2-D): po = 3e38, normals and slacks 0, origin and extent as
    for a full simplex."""
    monkeypatch.setattr(core, "WIT_MIN_ROWS", 0)
    _, verts, _, _ = _reference(dim)
    verts = np.ascontiguousarray(verts[:, :k1])
    want = np.stack([plane_words(v).view(np.uint32) for v in verts])
    w = want.view(f32)
    assert (w[:, 7:24:5][:, :dim + 1] == f32(3.0e38)).all() and (w[:, 4:24:5] == 0).all() and (w[:, 8:24:5] == 0).all()
    assert (w[:, 3] > 0).sum() >= len(verts) - 2   # (extent 0: the faces whose vertices all repeat vertex 0)
    names = [f"simplex {i}" for i in range(len(verts))]
    for what, got in zip(("prepare launch", "plane launch of the sweeps"), _both_writers(dim, verts, dev)):
        diff = _differences(got, want, names)
        assert not diff, f"dim {dim}, k1 {k1}, {what}: {int((got != want).sum())} words differ from the replica: {diff}"
