"""The leaf cull of the cell sweep (csrc/flood_cell.hip: the leaves a gather has collected are tested against the
region's slabs, csrc/flood_planes.hpp: node_meets_slabs) on the GPU: a leaf it drops holds no point the classification
would keep, so every face value keeps its bits.

Per cloud, face values of flood_complex are compared BIT FOR BIT with method="bvh" - the tree sweep, which has no such
gather - with the witness sweep on and off and through all three instantiations of the cell sweep: the runs-of-four
launch ("cell_super_min_chunks" 0), the per-chunk launch, and "cell_tiles" 1.  32 top simplices per cloud (the largest
values among them) are checked against float64 brute force over ALL points, with the relative bound of
tests/test_gpu_wit_far_clouds.py (2 * 2^-23, derived there; no absolute term).

Clouds: two Gaussian clouds in 3-D (20 k points / 60 landmarks, 60 k / 150), one in 2-D, a thin slab, the needle / sliver
landmark set of test_gpu_parity.py at offsets 0 and 300, and a Gaussian cloud at offset 1e3.  12 points per edge in 3-D.

One case runs with statistics: the tiles the sweep flags for the finish are no more than with a library built with
-DFLOODER_GATHER_PLANES=0, where such a side build is present (FLOODER_GATHER_PLANES_OFF_LIB, or
flooder_amd/_diag/libflooder_hip_gather_planes_off.so); without one only the bit identity is asserted.
Runs on a real MI355X only (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF_LIB = os.environ.get("FLOODER_GATHER_PLANES_OFF_LIB") or os.path.join(ROOT, "flooder_amd", "_diag", "libflooder_hip_gather_planes_off.so")
ST_TILES_FLAGGED = 2      # word of the cell sweep's statistics (include/flooder_hip.h)
N_REFERENCE = 32
RTOL = 2.0 * 2.0 ** -23   # (tests/test_gpu_wit_far_clouds.py derives it)
CLOUDS = ["gauss_20k", "gauss_60k", "plane_2d", "thin_slab", "needles_0", "needles_300", "gauss_1e3"]
LAUNCHES = {"runs_of_four": {b"cell_super_min_chunks": 0}, "per_chunk": {}, "tiles": {b"cell_tiles": 1}}

pytestmark = pytest.mark.gpu


def _make(name):
    """-> points, landmarks (device tensors), points per edge"""
    import torch

    import flooder_amd as fa
    from oracle import flood_oracle as fo

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(19)
    if name.startswith("needles"):
        offset = float(name.split("_")[1])
        rng = np.random.default_rng(77)
        cloud = rng.normal(size=(30_000, 3)).astype(np.float64)
        t = np.linspace(-1.5, 1.5, 12)
        line = np.stack([t, 0.3 * t, -0.2 * t], axis=1) + rng.normal(size=(12, 3)) * 1e-4
        u, v = np.meshgrid(np.linspace(-1, 1, 5), np.linspace(-1, 1, 5))
        plane = np.stack([u.ravel(), v.ravel(), 0.5 + 0.1 * u.ravel()], axis=1) + rng.normal(size=(25, 3)) * 1e-4
        extra = cloud[fo.exact_fps(cloud.astype(np.float32), 20, 0)]
        lms = np.concatenate([line, plane, extra]) + offset
        pts = torch.as_tensor(np.concatenate([cloud + offset, lms]).astype(np.float32), device=dev)
        return pts, pts[-lms.shape[0]:].contiguous(), 12
    if name == "gauss_20k":
        pts, n_l, ppe = torch.randn(20_000, 3, generator=g), 60, 12
    elif name == "gauss_60k":
        pts, n_l, ppe = torch.randn(60_000, 3, generator=g), 150, 12
    elif name == "plane_2d":
        pts, n_l, ppe = torch.randn(30_000, 2, generator=g), 80, 24
    elif name == "thin_slab":
        pts, n_l, ppe = torch.randn(40_000, 3, generator=g) * torch.tensor([1.0, 1.0, 0.02]), 100, 12
    elif name == "gauss_1e3":
        pts, n_l, ppe = torch.randn(30_000, 3, generator=g) + 1000.0, 80, 12
    else:
        raise ValueError(name)
    pts = pts.contiguous().to(dev)
    return pts, fa.generate_landmarks(pts, n_l, start_idx=0), ppe


class _Setup:
    """the settings under which every simplex is offered to the witness sweep and needles are triangulated with Qhull
    (as tests/test_gpu_wit_far_clouds.py), put back on exit"""

    def __enter__(self):
        from flooder_amd import _native, core
        from flooder_amd import simplex_tree as stm
        from helpers import get_options, set_options

        self.lib = _native.load()
        self.core, self.stm, self.set_options = core, stm, set_options
        self.keep = core.WIT_MIN_SIMPLICES, core.WIT_MAX_POINTS_PER_SIMPLEX, core.CELL_WITNESS, stm.NATIVE_DELAUNAY
        self.options = get_options(self.lib, b"cell_super_min_chunks", b"cell_tiles", b"wit_surface_pct")
        core.WIT_MIN_SIMPLICES, core.WIT_MAX_POINTS_PER_SIMPLEX, stm.NATIVE_DELAUNAY = 0, 1 << 40, False
        set_options(self.lib, {b"wit_surface_pct": 0})
        return self

    def __exit__(self, *exc):
        core, stm = self.core, self.stm
        core.WIT_MIN_SIMPLICES, core.WIT_MAX_POINTS_PER_SIMPLEX, core.CELL_WITNESS, stm.NATIVE_DELAUNAY = self.keep
        self.set_options(self.lib, self.options)
        return False

    def values(self, pts, lms, ppe, method="cell", witness=True, options=None):
        import flooder_amd as fa

        self.core.CELL_WITNESS = witness
        self.set_options(self.lib, options or {})
        try:
            out = fa.flood_complex(pts, lms, points_per_edge=ppe, method=method)
        finally:
            self.core.CELL_WITNESS = True
            self.set_options(self.lib, self.options)
        keys = sorted(out)
        return keys, np.array([out[k] for k in keys], dtype=np.float32)


_cache = {}


def _cloud(name):
    """the cloud and its reference (method="bvh"), computed once and left unchanged"""
    if name not in _cache:
        pts, lms, ppe = _make(name)
        with _Setup() as su:
            ref = su.values(pts, lms, ppe, method="bvh")
        ref[1].setflags(write=False)
        _cache[name] = pts, lms, ppe, ref
    return _cache[name]


def _same(a, b):
    return a[0] == b[0] and bool((a[1].view(np.uint32) == b[1].view(np.uint32)).all())


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("name", CLOUDS)
def test_face_values_have_the_tree_sweeps_bits(name, launch):
    pts, lms, ppe, ref = _cloud(name)
    with _Setup() as su:
        before = dict(su.options)
        for witness in (True, False):
            got = su.values(pts, lms, ppe, witness=witness, options=LAUNCHES[launch])
            assert np.isfinite(got[1]).all() and got[1].size > 0
            assert _same(got, ref), f"{name}, {launch}, witness sweep {'on' if witness else 'off'}: face values differ from the tree sweep's"
    from helpers import get_options
    from flooder_amd import _native

    assert get_options(_native.load(), *before) == before      # options are back


@pytest.mark.parametrize("name", CLOUDS)
def test_top_simplices_against_float64_brute_force(name):
    import torch

    from flooder_amd import core
    from wit_reference import fma

    pts, lms, ppe, ref = _cloud(name)
    d = pts.shape[1]
    with _Setup() as su:
        got = su.values(pts, lms, ppe)
        tops = core._build_complex(lms, d)[1][d]
    assert _same(got, ref)
    lookup = dict(zip(got[0], got[1].tolist()))
    vals = np.array([lookup[tuple(sorted(int(i) for i in row))] for row in tops])
    order = np.argsort(-vals, kind="stable")
    pick = list(order[:N_REFERENCE // 2])
    rest = order[N_REFERENCE // 2:]
    pick += list(rest[np.linspace(0, len(rest) - 1, N_REFERENCE - len(pick)).astype(int)])
    pick = np.array(sorted(set(int(i) for i in pick)))
    w = core.generate_grid(ppe, d, pts.device, torch.float32)[0].cpu().numpy()
    v = lms.cpu().numpy()[tops[pick]]
    p = np.zeros((len(pick), w.shape[0], d), np.float32)
    for j in range(d + 1):   # the sample as every kernel builds it: one fma per vertex
        p = fma(w[None, :, j, None], v[:, None, j, :], p)
    P = pts.double()
    Q = torch.as_tensor(p.reshape(-1, d), device=pts.device).double()
    per, best = max(1, (1 << 26) // P.shape[0]), []
    for a in range(0, Q.shape[0], per):
        q = Q[a:a + per]
        d2 = (q[:, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for c in range(1, d):
            d2 += (q[:, c:c + 1] - P[:, c].unsqueeze(0)) ** 2
        best.append(d2.min(dim=1).values)
    exact = torch.cat(best).reshape(len(pick), -1).max(dim=1).values.sqrt().cpu().numpy()
    rel = np.abs(vals[pick].astype(np.float64) - exact) / exact
    print(f"{name}: {len(pick)} simplices, worst {rel.max() * 2 ** 23:.2f} x 2^-23 off the float64 brute force")
    assert len(pick) == N_REFERENCE and vals.max() == vals[pick].max()
    assert rel.max() <= RTOL


def _tiles_flagged(name):
    """tiles the cell sweep of the top simplices flags for the finish, and the face words it leaves"""
    import torch

    from flooder_amd import core

    pts, lms, ppe = _make(name)
    d = pts.shape[1]
    verts = lms[torch.as_tensor(core._build_complex(lms, d)[1][d], device=pts.device)].contiguous()
    weights, _, face_idxs = core.generate_grid(ppe, d, pts.device, torch.float32)
    faces = core._FaceTable(face_idxs, weights.shape[0], pts.device)
    st = torch.zeros(40, dtype=torch.int64, device=pts.device)
    out, _ = core._sweep_dimension_cell(core.PointIndex(pts), verts, weights, faces, None, stats=st)
    torch.cuda.synchronize()
    return int(st[ST_TILES_FLAGGED].item()), out.cpu().numpy().view(np.uint32)


def test_no_more_tiles_flagged_than_without_the_cull(tmp_path):
    flagged, words = _tiles_flagged("gauss_60k")
    print(f"tiles flagged: {flagged}")
    assert np.array_equal(words, _tiles_flagged("gauss_60k")[1])          # (statistics on: the same words run after run)
    if not os.path.exists(OFF_LIB):
        return   # no side build to compare with: the bit identity above and in the other tests is all there is
    out = tmp_path / "off.json"
    env = dict(os.environ, FLOODER_HIP_LIB=OFF_LIB,
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), "gauss_60k", str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    off = json.loads(out.read_text())
    print(f"tiles flagged with -DFLOODER_GATHER_PLANES=0: {off['flagged']}")
    assert flagged <= off["flagged"]
    assert off["words_crc"] == int(np.bitwise_xor.reduce(words.ravel())) and off["n_words"] == int(words.size)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    n_flagged, face_words = _tiles_flagged(sys.argv[1])
    with open(sys.argv[2], "w") as fh:
        json.dump({"flagged": n_flagged, "words_crc": int(np.bitwise_xor.reduce(face_words.ravel())), "n_words": int(face_words.size)}, fh)
