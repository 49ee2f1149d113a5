"""The cell and the witness sweep end to end under the options no other test sets: the launch sizes "cell_grid" and
"wit_grid" down to one workgroup, the queue sharding "cell_queue_block", and the thresholds between the ways a chunk
is evaluated ("cell_brute_max", "cell_density_grid", "cell_exh_*", "cell_retry_*", "cell_tiles" 2 with
"cell_tail_waves").  One option per run; every run gives the dict of the default run, which is pinned once per cloud to
the tree sweep bit for bit and to the kd-tree.  The sweep's own counters show that each cloud takes the paths the
options are about: a cloud too small for its path fails here instead of passing idly.
Runs on a real MI355X only (-m gpu)."""
import functools

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from oracle import flood_oracle as fo

import variant_cases as vc
from helpers import assert_tree_matches_kdtree
from variant_cases import INT_MAX, options

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PPE = 30
# cloud: (points, landmarks, the paths its default run must take).  The smallest of the sizes tried (30 000, 100 000
# and 300 000 points; 20 000, 60 000 and 200 000 in the plane) at which the counters of every path named are in the
# dozens at least; the witness sweep handles simplices in 3-D only.
CLOUDS = {
    "core3d": (30_000, 40, ("restaged", "exhaustive", "dense_tiles", "witness")),       # a dense Gaussian core
    "torus3d": (30_000, 100, ("given_up", "exhaustive", "dense_tiles", "witness")),     # a noisy surface: chunks near the sheet overflow
    "eight2d": (60_000, 200, ("restaged", "given_up", "exhaustive", "dense_tiles")),    # a figure eight in the plane
}
VARIANTS = {
    "cell_grid_1": dict(cell_grid=1),
    "queue_interleaved": dict(cell_queue_block=-1), "queue_block_1": dict(cell_queue_block=0),
    "queue_block_4096": dict(cell_queue_block=12),
    "no_brute": dict(cell_brute_max=0), "no_density_grid": dict(cell_density_grid=0),
    "exh_tries_0": dict(cell_exh_tries=0), "exh_tries_8": dict(cell_exh_tries=8),
    "exh_sparse_least": dict(cell_exh_sparse=480), "exh_dense_least": dict(cell_exh_dense=512),
    "retry_keep_0": dict(cell_retry_keep=0), "retry_pct_0": dict(cell_retry_pct=0), "retry_pct_never": dict(cell_retry_pct=INT_MAX),
    "tail_tiles_none": dict(cell_tiles=2, cell_tail_waves=0), "tail_tiles": dict(cell_tiles=2),
}


def test_variants_are_the_listed_values():
    seen = {"wit_grid": {1}}
    for opts in VARIANTS.values():
        for name, v in opts.items():
            seen.setdefault(name, set()).add(v)
    mine = vc.SET_BY["test_gpu_cell_variants"]
    assert {k: tuple(sorted(v)) for k, v in seen.items()} == {k: tuple(sorted(v)) for k, v in mine.items()}


@functools.lru_cache(maxsize=None)
def _cloud(name):
    n, n_lms, _ = CLOUDS[name]
    if name == "core3d":
        pts = np.random.default_rng(4).normal(size=(n, 3)).astype(np.float32) * 0.05
    elif name == "torus3d":
        pts = fo.noisy_torus(n, seed=3)
    else:
        pts = fa.generate_figure_eight_points_2d(n, noise_std=0.02, seed=3).numpy().astype(np.float32)
    tp = torch.as_tensor(pts, device=DEV)
    return pts, tp, fa.generate_landmarks(tp, n_lms, start_idx=0)


def _run(name, **kw):
    _, tp, tl = _cloud(name)
    return fa.flood_complex(tp, tl, points_per_edge=PPE, method="cell", **kw)


@functools.lru_cache(maxsize=None)
def _default(name):
    return _run(name)


def _counters(name, witness=False):
    """{path: count} of the top dimension's sweep under the options in force."""
    _, tp, tl = _cloud(name)
    d = tp.shape[1]
    _, simplices = core._build_complex(tl, d)
    verts = tl[torch.as_tensor(simplices[d], device=DEV)].contiguous()
    weights, _, face_idxs = core.generate_grid(PPE, d, DEV, torch.float32)
    st = torch.zeros(40, dtype=torch.int64, device=DEV)
    core._sweep_dimension_cell(core.PointIndex(tp), verts, weights, core._FaceTable(face_idxs, weights.shape[0], DEV), None, stats=st)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    return dict(restaged=int(s[3]), given_up=int(s[4:8].sum()), exhaustive=int(s[8]), flagged=int(s[2]),
                dense_tiles=int(core.LAST_STATS.dense_tiles), deferred=int(core.LAST_STATS.deferred_chunks),
                witness=int(s[16]) if witness else 0)


@pytest.fixture
def witness_on(monkeypatch):
    """As ``test_gpu_witness``: the product skips the witness sweep on short queues, on clouds with many points per
    simplex and on surfaces; here it has to run."""
    monkeypatch.setattr(core, "WIT_MIN_SIMPLICES", 0)
    monkeypatch.setattr(core, "WIT_MAX_POINTS_PER_SIMPLEX", 1 << 40)
    with options(wit_surface_pct=0):
        yield


@pytest.mark.parametrize("name", list(CLOUDS))
def test_default_run_is_the_tree_sweep_and_the_kdtree(name):
    pts, tp, tl = _cloud(name)
    assert _default(name) == fa.flood_complex(tp, tl, points_per_edge=PPE, method="bvh"), "differs from the tree sweep"
    st = fa.flood_complex(tp, tl, points_per_edge=PPE, method="cell", return_simplex_tree=True)
    n = assert_tree_matches_kdtree(st, pts, tl.cpu().numpy(), PPE, pts.shape[1], name, strict=True)
    assert n == len(_default(name)) - tl.shape[0]


@pytest.mark.parametrize("name", list(CLOUDS))
def test_clouds_take_their_paths(name, witness_on):
    with options(cell_tiles=2):
        tail = _counters(name, witness=True)
    plain = _counters(name, witness=True)
    print(name, "default:", plain, "| cell_tiles 2:", tail)
    seen = dict(plain, dense_tiles=tail["dense_tiles"])
    for path in CLOUDS[name][2]:
        assert seen[path] > 0, f"{name} does not reach '{path}': {seen}"


def test_every_path_is_taken_by_some_cloud():
    assert {p for _, _, paths in CLOUDS.values() for p in paths} == {"restaged", "exhaustive", "given_up", "dense_tiles", "witness"}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(CLOUDS))
def test_variant_equals_the_default(name, variant):
    with options(**VARIANTS[variant]):
        got = _run(name)
    assert got == _default(name), (name, variant)


@pytest.mark.parametrize("name", list(CLOUDS))
def test_witness_grid_of_one_workgroup(name, witness_on):
    """One workgroup works off the whole item list of the witness sweep; on the cloud that is there for it, it handles
    simplices."""
    with options(wit_grid=1):
        got = _run(name)
        handled = _counters(name, witness=True)["witness"]
    print(name, "witness simplices handled under wit_grid 1:", handled)
    assert got == _default(name), name
    if "witness" in CLOUDS[name][2]:
        assert handled > 0
