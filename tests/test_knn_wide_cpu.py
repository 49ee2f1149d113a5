"""The robust filtration by mass without a device: the declaration, binding and layout of ``flooder_knn_wide_f32``'s
parameter block and everything the entry refuses before a pointer is read (the non-null "pointers" are the number
4096); ``core.mass_neighbors``; ``distance_to_measure`` and ``flood_complex(neighbor_mass=m)`` on CPU tensors against a
float64 brute force over all points at k = 40 and k = 200; the identity with ``neighbors=k`` up to 32; every Python
refusal, ``flood_complex_sharded``'s modes and the command line's pair of options included."""

import ctypes
import os

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, cli, core, distributed

import knn_wide_reference as kw
from helpers import assert_close_filtration, header_numbers, tolerances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "flooder_knn_wide_f32"
FAKE = 4096


# ------------------------------------------------------------------------------------------------ ABI
def test_entry_is_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "flooder_knn_wide_f32(const flooder_knn_wide_t* p, void* stream);" in header
    assert "typedef struct flooder_knn_wide_s" in header and "#define FLOODER_KNN_WIDE_MAX 1024" in header
    res, args = _native.SIGNATURES[ENTRY]
    assert res is ctypes.c_int and len(args) == 2 and args[0]._type_ is _native.KnnWide
    from flooder_amd import build
    assert "flood_knn_wide.hip" in build.HIP_SOURCES
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), ENTRY) and hasattr(_native.load(), ENTRY)
    assert core.KNN_WIDE_MAX == 1024 and core.KNN_MAX == 32


def test_block_has_the_layout_of_the_header(tmp_path):
    """(size and offsets against the header: test_host.py, test_parameter_block_has_the_layout_of_the_header)"""
    cls = _native.KnnWide
    assert header_numbers(tmp_path, extra={"wide_max": "FLOODER_KNN_WIDE_MAX"}) == {"wide_max": core.KNN_WIDE_MAX}
    for needed in ("size", "abi", "pts_sorted", "n_pts", "dim", "k1", "nodes", "verts", "weights", "R", "k", "n_simplices",
                   "stat", "order", "sample_order", "out_bits", "out_ids", "out_d2"):
        assert hasattr(cls, needed), needed
    assert [name for name, _ in cls._fields_][:2] == ["size", "abi"]


# ------------------------------------------------------------------------------------------------ refusals of the entry
def _call(**change):
    """The entry on a block whose pointers are all NULL but ``out_bits`` (a number that is never read), with
    ``change`` applied -> (return code, message)."""
    lib = _native.load()
    good = dict(n_pts=5000, dim=3, k1=4, R=10, n_simplices=7, k=200, stat=1)
    blk = _native.KnnWide(**{**good, **{k: v for k, v in change.items() if k not in ("size", "abi", "out_bits")}})
    blk.out_bits = change.get("out_bits", FAKE)
    if "abi" in change:
        blk.abi = change["abi"]
    if "size" in change:
        blk.size = change["size"]
    rc = lib.flooder_knn_wide_f32(ctypes.byref(blk), None)
    return rc, (lib.flooder_last_error() or b"").decode()


@pytest.mark.parametrize("change,words", [
    (dict(abi=2), "bad parameter block"),
    (dict(size=4), "bad parameter block"),
    (dict(size=ctypes.sizeof(_native.KnnWide) + 8), "bad parameter block"),
    (dict(k=0), "k must be in 1..1024"),
    (dict(k=-3), "k must be in 1..1024"),
    (dict(k=1025), "k must be in 1..1024"),
    (dict(dim=1), "dim must be in 2..8"),
    (dict(dim=9), "dim must be in 2..8"),
    (dict(stat=2), "stat must be 0 (kth) or 1 (dtm)"),
    (dict(stat=-1), "stat must be 0 (kth) or 1 (dtm)"),
    (dict(n_pts=199), "fewer points than k"),
    (dict(n_pts=1 << 31), "more than 2^31 - 1 points"),
    (dict(n_simplices=1 << 31, R=2), "n_simplices * R must be below 2^32 - 2"),
    (dict(n_simplices=(1 << 32) - 2, R=1), "n_simplices * R must be below 2^32 - 2"),
    (dict(out_bits=0), "no output"),
    (dict(out_ids=FAKE), "out_ids needs order"),
])
def test_entry_refuses_before_a_pointer_is_read(change, words):
    rc, msg = _call(**change)
    assert rc == -1 and msg.startswith(ENTRY + ":") and words in msg, (rc, msg)


def test_entry_refuses_a_null_block_and_accepts_nothing_to_do():
    lib = _native.load()
    assert lib.flooder_knn_wide_f32(None, None) == -1
    assert lib.flooder_last_error().startswith(ENTRY.encode())
    # nothing to sweep: FLOODER_OK, no pointer is looked at (they are all NULL or fake) and nothing is launched
    assert _call(n_simplices=0)[0] == 0 and _call(R=0)[0] == 0
    # (the stack encoding's limit of 2^37 points lies behind the limit of 2^31 - 1 ids and cannot be reached from here)
    # the register family's entries keep their own range
    blk = _native.KnnSorted(n_pts=100, dim=3, k1=1, R=1, n_simplices=0, k=33, stat=0)
    assert lib.flooder_sweep_knn_sorted_f32(ctypes.byref(blk), None) == -1
    assert b"k must be in 1..32" in lib.flooder_last_error()


# ------------------------------------------------------------------------------------------------ mass -> k
@pytest.mark.parametrize("mass,n,k", [(0.1, 30, 3), (1.0, 30, 30), (1.0, 1, 1), (1.0, 1_000_000, 1_000_000), (1e-9, 1000, 1),
                                      (0.001, 1_000_000, 1000), (0.5, 7, 4), (0.3, 10, 3), (0.31, 10, 4), (1, 5, 5),
                                      (np.float32(0.25), 8, 2), (0.0005, 2000, 1), (0.00051, 2000, 2)])
def test_mass_neighbors_table(mass, n, k):
    assert core.mass_neighbors(mass, n) == k and isinstance(core.mass_neighbors(mass, n), int)


def test_mass_neighbors_refusals():
    for bad in (True, False, "0.1", None, [0.1], 1j):
        with pytest.raises(TypeError, match="mass must be a real number"):
            core.mass_neighbors(bad, 100)
    for bad in (0, 0.0, -0.1, 1.0000001, 2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"mass must be in \(0, 1\]"):
            core.mass_neighbors(bad, 100)


# ------------------------------------------------------------------------------------------------ values on CPU tensors
def _cloud(dim, n, dtype, seed=0):
    """``n`` points of which a third are copies of others, 60 queries: 15 of them cloud points."""
    g = torch.Generator().manual_seed(100 * dim + seed)
    base = torch.randn(n - n // 3, dim, generator=g, dtype=torch.float64)
    pts = torch.cat([base, base[:n // 3]])[torch.randperm(n, generator=g)].to(dtype)
    qs = torch.cat([pts[:15], 1.5 * torch.randn(45, dim, generator=g, dtype=torch.float64).to(dtype)])
    return pts, qs


def _assert_close(got, want, points, what):
    rtol, atol = tolerances(points)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    assert (err <= atol + rtol * np.abs(want)).all(), (what, float(err.max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dim", [2, 3, 6])
def test_distance_to_measure_against_the_brute_force(dim, dtype):
    pts, qs = _cloud(dim, 600, dtype)
    for k in (40, 200):
        for stat in ("kth", "dtm"):
            want2 = kw.brute_statistic(pts.numpy(), qs.numpy(), k, stat)
            got = fa.distance_to_measure(pts, qs, neighbors=k, neighbor_stat=stat)
            by_mass = fa.distance_to_measure(pts, qs, k / 600, neighbor_stat=stat)
            got2 = fa.distance_to_measure(pts, qs, neighbors=k, neighbor_stat=stat, squared=True)
            assert got.dtype == dtype and got.shape == (60,) and got2.dtype == dtype and torch.equal(got, by_mass)
            _assert_close(got.numpy(), np.sqrt(want2), pts.numpy(), (dim, k, stat))
            rtol, atol = tolerances(pts.numpy())   # (squared: the tolerance of the distance carried through the square)
            d = np.sqrt(want2)
            assert (np.abs(got2.numpy().astype(np.float64) - want2) <= 3 * rtol * want2 + 3 * d * atol + atol * atol).all()
    # the default statistic is the distance to the measure; the neighbours come ascending and realise the value
    value, ids, dist = fa.distance_to_measure(pts, qs, neighbors=40, return_neighbors=True)
    assert torch.equal(value, fa.distance_to_measure(pts, qs, neighbors=40, neighbor_stat="dtm"))
    assert ids.shape == (60, 40) and ids.dtype == torch.int64 and dist.shape == (60, 40) and dist.dtype == dtype
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()) and all(len(set(row)) == 40 for row in ids.tolist())
    d_ids = (qs.double().unsqueeze(1) - pts.double()[ids]).norm(dim=2)
    _assert_close(dist.numpy(), d_ids.numpy(), pts.numpy(), "neighbour distances")
    _assert_close(value.numpy(), np.sqrt((d_ids.numpy() ** 2).mean(axis=1)), pts.numpy(), "value from neighbours")
    # own points, no queries, requires_grad inputs are used detached
    own = fa.distance_to_measure(pts.clone().requires_grad_(True), None, neighbors=40)
    assert own.shape == (600,) and not own.requires_grad
    _assert_close(own.numpy(), np.sqrt(kw.brute_statistic(pts.numpy(), pts.numpy(), 40, "dtm")), pts.numpy(), "own")
    empty = fa.distance_to_measure(pts, qs[:0], neighbors=40, return_neighbors=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 40) and empty[2].shape == (0, 40)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("stat", ["kth", "dtm"])
def test_flood_complex_by_mass_against_the_brute_force(dtype, stat):
    pts, _ = _cloud(3, 600, dtype, seed=3)
    lms = fa.generate_landmarks(pts, 12, start_idx=0)
    for k in (40, 200):
        with pytest.warns(RuntimeWarning) if dtype is torch.float64 else _no_warning():
            fc = fa.flood_complex(pts, lms, points_per_edge=5, neighbor_mass=k / 600, neighbor_stat=stat)
        ref = kw.brute_flood_reference(fc, pts.numpy(), lms.numpy(), k, stat, 5)
        keys = sorted(fc)
        assert_close_filtration([fc[key] for key in keys], [ref[key] for key in keys], pts.numpy(), (k, stat))
        # the vertex values are the statistic at the landmarks
        want = fa.distance_to_measure(pts, lms, k / 600, neighbor_stat=stat).double().numpy()
        assert np.allclose([fc[(i,)] for i in range(12)], want, rtol=1e-6, atol=0)


class _no_warning:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_up_to_32_the_mass_is_the_neighbors_call():
    pts, _ = _cloud(3, 300, torch.float32, seed=5)
    lms = fa.generate_landmarks(pts, 12, start_idx=0)
    for mass, k in ((0.1, 30), (32 / 300, 32), (1e-9, 1), (0.01, 3)):
        assert core.mass_neighbors(mass, 300) == k
        for stat in ("kth", "dtm"):
            by_mass = fa.flood_complex(pts, lms, points_per_edge=5, neighbor_mass=mass, neighbor_stat=stat)
            assert by_mass == fa.flood_complex(pts, lms, points_per_edge=5, neighbors=k, neighbor_stat=stat)
    # ... with its checks and their wording
    with pytest.raises(ValueError, match="neighbors > 1 needs the tree sweep"):
        fa.flood_complex(pts, lms, points_per_edge=5, neighbor_mass=0.1, method="ball")


def test_simplex_shards_reduce_to_the_whole_dict():
    pts, _ = _cloud(3, 600, torch.float32, seed=7)
    lms = fa.generate_landmarks(pts, 12, start_idx=0)
    whole = fa.flood_complex(pts, lms, points_per_edge=5, neighbor_mass=0.1)
    halves = []         # the hook sees one buffer per dimension pass: this rank's rows, +inf elsewhere
    for rank in (0, 1):
        got = []
        fa.flood_complex(pts, lms, points_per_edge=5, neighbor_mass=0.1, simplex_shard=(rank, 2),
                         face_reduce_hook=lambda face, got=got: got.append(face.clone()))
        halves.append(got)
    merged = iter([torch.minimum(a, b) for a, b in zip(*halves)])
    both = fa.flood_complex(pts, lms, points_per_edge=5, neighbor_mass=0.1, simplex_shard=(1, 2),
                            face_reduce_hook=lambda face: face.copy_(next(merged)))
    assert both == whole
    # flood_complex_sharded forwards the keyword in mode="simplices" (one rank: the whole result)
    assert distributed.flood_complex_sharded(pts, lms, points_per_edge=5, neighbor_mass=0.1) == whole


# ------------------------------------------------------------------------------------------------ refusals in Python
def test_flood_complex_refusals():
    pts, _ = _cloud(3, 300, torch.float32)
    lms = pts[:10].clone()
    call = lambda **kw_: fa.flood_complex(pts, lms, points_per_edge=3, **kw_)   # noqa: E731
    with pytest.raises(ValueError, match="neighbor_mass cannot be combined with neighbors=3"):
        call(neighbor_mass=0.2, neighbors=3)
    with pytest.raises(TypeError, match="mass must be a real number"):
        call(neighbor_mass="0.2")
    with pytest.raises(TypeError, match="mass must be a real number"):
        call(neighbor_mass=True)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match=r"mass must be in \(0, 1\]"):
            call(neighbor_mass=bad)
    with pytest.raises(ValueError, match="neighbor_stat must be one of"):
        call(neighbor_mass=0.5, neighbor_stat="mean")
    for method in ("cell", "ball"):
        with pytest.raises(ValueError, match=f"neighbor_mass needs the tree sweep: method '{method}'"):
            call(neighbor_mass=0.5, method=method)
    hook = lambda t: None   # noqa: E731
    with pytest.raises(ValueError, match="neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook"):
        call(neighbor_mass=0.5, reduce_hook=hook)
    with pytest.raises(ValueError, match="neighbor_mass cannot be combined with reduce_hook or neighbor_reduce_hook"):
        call(neighbor_mass=0.5, neighbor_reduce_hook=hook)
    with pytest.raises(ValueError, match="a mass is a share of the WHOLE cloud"):
        call(neighbor_mass=0.01, reduce_hook=hook)             # (k = 3: refused all the same - the share is the point)
    with pytest.raises(ValueError, match="neighbor_mass cannot be combined with shard_blocks=True"):
        call(neighbor_mass=0.5, shard_blocks=True, simplex_shard=(0, 2))
    big = torch.randn(3000, 3)
    with pytest.raises(ValueError, match=r"is 1500 neighbours of 3000 points, above KNN_WIDE_MAX = 1024 .*largest mass "
                                         r"that fits this cloud is 0\.341333"):
        fa.flood_complex(big, big[:10].clone(), points_per_edge=3, neighbor_mass=0.5)
    assert core.mass_neighbors(float("0.341333"), 3000) == 1024
    with pytest.raises(TypeError):
        fa.flood_complex(pts, lms, None, 3, None, 64, None, False, None, 0, 0.5)   # keyword-only
    # the keyword is the last one
    import inspect
    assert list(inspect.signature(fa.flood_complex).parameters)[-1] == "neighbor_mass"
    assert "neighbor_mass" not in inspect.signature(fa.flood_filtration).parameters
    assert "neighbor_mass" not in inspect.signature(fa.flood_profile).parameters


def test_distance_to_measure_refusals():
    pts, qs = _cloud(3, 300, torch.float32)
    assert "distance_to_measure" in fa.__all__
    with pytest.raises(ValueError, match="exactly one of mass and neighbors"):
        fa.distance_to_measure(pts, qs)
    with pytest.raises(ValueError, match="exactly one of mass and neighbors"):
        fa.distance_to_measure(pts, qs, 0.1, neighbors=30)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match=r"neighbors must be in 1\.\.1024"):
            fa.distance_to_measure(pts, qs, neighbors=bad)
    for bad in (True, 2.0, "3"):
        with pytest.raises(TypeError, match="neighbors must be an integer"):
            fa.distance_to_measure(pts, qs, neighbors=bad)
    with pytest.raises(ValueError, match=r"neighbors=301 exceeds the number of points \(300\)"):
        fa.distance_to_measure(pts, qs, neighbors=301)
    with pytest.raises(TypeError, match="mass must be a real number"):
        fa.distance_to_measure(pts, qs, "0.5")
    with pytest.raises(ValueError, match=r"mass must be in \(0, 1\]"):
        fa.distance_to_measure(pts, qs, 1.5)
    with pytest.raises(ValueError, match="neighbor_stat must be one of"):
        fa.distance_to_measure(pts, qs, 0.5, neighbor_stat="mean")
    big = torch.randn(3000, 3)
    with pytest.raises(ValueError, match=r"above KNN_WIDE_MAX = 1024 .*largest mass that fits this cloud is 0\.341333"):
        fa.distance_to_measure(big, None, 0.5)
    with pytest.raises(RuntimeError, match="queries must be a"):
        fa.distance_to_measure(pts, qs[:, :2], 0.1)
    with pytest.raises(RuntimeError, match="points must be a non-empty"):
        fa.distance_to_measure(pts[:0], None, 0.1)
    with pytest.raises(TypeError, match="not supported"):
        fa.distance_to_measure(pts.half(), None, 0.1)


def test_sharded_modes_and_the_command_line():
    pts, _ = _cloud(3, 300, torch.float32)
    lms = pts[:10].clone()
    for mode in ("points", "blocks"):
        with pytest.raises(ValueError, match=f"neighbor_mass cannot be combined with mode='{mode}': a mass is a share of the "
                                             "WHOLE cloud"):
            distributed.flood_complex_sharded(pts, lms, points_per_edge=3, mode=mode, neighbor_mass=0.2)
    args = cli.build_parser().parse_args(["--input-file", "in.npy", "--neighbor-mass", "0.25"])
    assert args.neighbor_mass == 0.25 and args.neighbors == 1


def test_command_line_refuses_mass_with_neighbors(tmp_path, capsys):
    src = tmp_path / "cloud.npy"
    np.save(src, np.random.default_rng(0).random((400, 2)).astype(np.float32))
    base = _cli_args(src, tmp_path / "out.pkl")
    with pytest.raises(SystemExit) as exc:
        cli.main(base + ["--neighbor-mass", "0.1", "--neighbors", "3"])
    assert exc.value.code == 2 and "--neighbor-mass cannot be combined with --neighbors" in capsys.readouterr().err
    assert cli.main(base + ["--neighbor-mass", "0.1", "--neighbor-stat", "dtm"]) == 0
    import pickle
    meta = pickle.load(open(tmp_path / "out.pkl", "rb"))["meta"]
    assert meta["neighbor_mass"] == 0.1 and meta["neighbors"] == 1 and meta["neighbor_stat"] == "dtm"


def _cli_args(src, out):
    return ["--input-file", str(src), "--device", "cpu", "--num-landmarks", "20", "--points-per-edge", "5", "--output-file", str(out)]
