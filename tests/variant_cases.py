"""Shared by the tests that run the kernel variants behind the tuning options (csrc/flood_options.def):

* ``SET_BY`` / ``COVERED_ELSEWHERE``: which GPU test sets which option to which non-default values
  (``test_option_coverage_cpu.py`` holds the two against flood_options.def and the ranges of ``test_options_cpu.py``);
* exact kernel cases in 2-D, 3-D and 6-D (padded widths 2, 4, 8): integer clouds with a hole in the middle, simplices
  partly on cloud points and partly inside the hole, a fixed random subset of the lattice rows as weights, and the
  float64 brute force over all points as the reference - ``_kernel_case`` of ``test_gpu_top_simplices.py`` for the low
  dimensions;
* the harness of the finish tests: a hand-built list of flagged tiles whose samples all start unsettled from +inf.

Nothing here touches a device before a function is called."""
import contextlib
import functools
import math
import types

import numpy as np
import torch

import grad_reference as gr
from helpers import get_options, set_options, smallest32

INT_MAX = 2 ** 31 - 1
INF_BITS = 0x7F800000
UNWRITTEN = -1          # prefill of output words no kernel may leave behind
GUARD = 64              # words behind every output buffer that no kernel may touch

# ------------------------------------------------------------------------------------------------ option coverage
# option: the non-default values a GPU test of the named module sets (the modules parametrise from these rows)
SET_BY = {
    "test_gpu_bvh_variants": {
        "bvh_ks": (1, 2, 4, 8),
        "bvh_grid": (1, 3, 65536),
        "bvh_refine_pct": (1, INT_MAX),
        "bvh_subs": (1, 64),
        "bvh_leaf_batch": (4,),
    },
    "test_gpu_sorted_variants": {
        "sorted_ks": (2,),
        "sorted_batch_pct": (100, 100000),
        "sorted_blocks": (1,),
    },
    "test_gpu_finish_variants": {
        "finish_wide_points": (1,),
        "finish_items_cap": (1024,),
        "finish_focus_pct": (0, 100),
        "finish_refresh": (1, INT_MAX),
        "bvh_refine_pct": (1, INT_MAX),
        "bvh_grid": (1, 3, 4),
        "bvh_subs": (1,),
    },
    "test_gpu_grid_variants": {
        "bvh_grid": (1, 65536),
    },
    "test_gpu_cell_variants": {
        "cell_grid": (1,),
        "wit_grid": (1,),
        "cell_queue_block": (-1, 0, 12),
        "cell_brute_max": (0,),
        "cell_density_grid": (0,),
        "cell_exh_tries": (0, 8),
        "cell_exh_sparse": (480,),
        "cell_exh_dense": (512,),
        "cell_retry_keep": (0,),
        "cell_retry_pct": (0, INT_MAX),
        "cell_tiles": (2,),
        "cell_tail_waves": (0,),
    },
}

# options that earlier GPU tests set to a non-default value: the test that does
COVERED_ELSEWHERE = {
    "bvh_subs": "test_gpu_finish_single.py::test_tree_depths_and_partly_filled_tiles",
    "cell_chunk_major": "test_gpu_parity.py",
    "cell_chunks_per_block": "test_gpu_parity.py",
    "cell_drop": "test_gpu_parity.py",
    "cell_exh_dense": "test_gpu_finish_single.py::test_through_the_product_path",
    "cell_listed_first": "test_gpu_parity.py",
    "cell_min_grid": "test_gpu_parity.py",
    "cell_one_pass": "test_gpu_parity.py",
    "cell_split_launches": "test_gpu_parity.py",
    "cell_super_min_chunks": "test_gpu_parity.py",
    "cell_super_n0": "test_gpu_parity.py",
    "cell_super_sparse": "test_gpu_parity.py",
    "cell_super_weight": "test_gpu_parity.py",
    "cell_surface_pct": "test_gpu_parity.py",
    "cell_tiles": "test_gpu_parity.py",
    "cell_tries": "test_gpu_finish_single.py::test_through_the_product_path",
    "cell_weight_classes": "test_gpu_parity.py",
    "curve": "test_gpu_index_exact.py",
    "curve_bits": "test_gpu_index_exact.py",
    "finish_budget": "test_gpu_parity.py",
    "finish_budget_min": "test_gpu_parity.py",
    "finish_order": "test_gpu_parity.py",
    "finish_top": "test_gpu_parity.py",
    "fps_lane_best": "test_gpu_fullsize.py",
    "fps_rounds": "test_gpu_fullsize.py",
    "fps_rpl": "test_gpu_fullsize.py",
    "fps_switch": "test_gpu_entry_forms.py",
    "sort_shape": "test_gpu_parity.py",
    "sorted_refresh": "test_gpu_parity.py",
    "sweep_variant": "test_gpu_parity.py",
    "wit_adaptive": "test_gpu_witness.py",
    "wit_cmax_ext_pct": "test_gpu_witness.py",
    "wit_cmax_pct": "test_gpu_witness.py",
    "wit_flags": "test_gpu_witness.py",
    "wit_max_eval": "test_gpu_witness.py",
    "wit_max_in_pct": "test_gpu_witness.py",
    "wit_max_leaves": "test_gpu_witness.py",
    "wit_max_live_pct": "test_gpu_witness.py",
    "wit_max_open": "test_gpu_witness.py",
    "wit_min_bins": "test_gpu_witness.py",
    "wit_runs": "test_gpu_wit_runs.py",
    "wit_sorted_stage": "test_gpu_wit_sorted_stage.py",
    "wit_surface_pct": "test_gpu_witness.py",
    "wit_weight": "test_gpu_witness.py",
}


def option_values():
    """{option: sorted non-default values the new modules set}"""
    out = {}
    for rows in SET_BY.values():
        for name, values in rows.items():
            out.setdefault(name, set()).update(values)
    return {name: sorted(v) for name, v in out.items()}


@contextlib.contextmanager
def options(**values):
    """Set these options of the library for the block and put back what they were (they are process-wide)."""
    from flooder_amd import _native

    lib = _native.load()
    names = [name.encode() for name in values]
    keep = get_options(lib, *names)
    try:
        set_options(lib, {name.encode(): v for name, v in values.items()})
        yield
    finally:
        set_options(lib, keep)


# ------------------------------------------------------------------------------------------------ exact kernel cases
PPE = {2: 33, 3: 17, 6: 9}                           # lattices of 561, 969 and 3003 rows
ALL_R = (63, 64, 65, 129, 512, 513)                  # the edges of tiles of 64, 128, 256 and 512 samples
FEW_R = (65, 513)
# (dim, n points, every point doubled, simplices, the subset lengths).  n = 40: one level of the box tree; 1025: two;
# 70 001: three; none a multiple of 16.  One n per dimension runs every length.
CASES = [
    (2, 40, True, 30, FEW_R), (2, 1025, False, 16, ALL_R), (2, 70_001, True, 8, FEW_R),
    (3, 40, False, 30, FEW_R), (3, 1025, True, 16, FEW_R), (3, 70_001, False, 8, ALL_R),
    (6, 40, True, 30, ALL_R), (6, 1025, False, 16, FEW_R), (6, 70_001, False, 8, FEW_R),
]
CASE_R = [(dim, n, R) for dim, n, _, _, Rs in CASES for R in Rs]
CASE_R_IDS = [f"{dim}d-{n}-R{R}" for dim, n, R in CASE_R]
THREE_LEVEL = [(dim, n, R) for dim, n, R in CASE_R if n == 70_001]
THREE_LEVEL_IDS = [f"{dim}d-{n}-R{R}" for dim, n, R in THREE_LEVEL]


def case_row(dim, n):
    return next(c for c in CASES if c[0] == dim and c[1] == n)


def levels(n):
    leaves, lv = (n + 15) // 16, 1
    while leaves > 64:
        leaves, lv = (leaves + 63) // 64, lv + 1
    return lv


def coordinate_range(dim):
    return min(511, int(2047 / ((PPE[dim] - 1) * math.sqrt(dim))))


@functools.lru_cache(maxsize=None)
def case_inputs(dim, n):
    """(points (n, dim), vertices (S, dim + 1, dim), lattice rows (513,)) as integers / indices, on the host: integer
    coordinates in [-r, r] without the ball of radius 0.45 r around the origin; a quarter of the simplices on cloud
    points, a quarter shrunk into the hole."""
    _, _, dup, n_s, _ = case_row(dim, n)
    ppe = PPE[dim]
    rng = np.random.default_rng(1000 * dim + n % 97 + ppe)
    r = coordinate_range(dim)
    need = (n + 1) // 2 if dup else n
    rows = np.empty((0, dim), dtype=np.int64)
    while rows.shape[0] < need:
        draw = rng.integers(-r, r + 1, size=(2 * need + 64, dim))
        rows = np.concatenate([rows, draw[(draw * draw).sum(axis=1) > (0.45 * r) ** 2]])
    rows = rows[:need]
    P = np.concatenate([rows, rows])[:n][rng.permutation(n)] if dup else rows
    V = rng.integers(-r, r + 1, size=(n_s, dim + 1, dim))
    V[: n_s // 4] = P[rng.integers(0, n, size=(n_s // 4, dim + 1))]              # simplices on points of the cloud
    V[n_s // 4: n_s // 2] //= 4                                                # small ones inside the hole
    pick = rng.permutation(gr.lattice(ppe, dim).shape[0])[:max(ALL_R)]          # every R takes a prefix of these rows
    gr.assert_exact_inputs(P, V.reshape(-1, dim), ppe)
    return P, V, pick


def assert_reference_bites(d2, what):
    """From the reference alone: few exact zeros, and a good share of minima far enough away for the culling to matter."""
    zero, far = float((d2 == 0).mean()), float((d2 >= 16).mean())
    assert zero <= 0.05 and far >= 0.25, (what, zero, far)
    return zero, far


@functools.lru_cache(maxsize=None)
def kernel_base(dim, n):
    """The cloud and its index on the device, the vertices, the 513 picked lattice rows and the reference of all of them
    (computed once; every R of the case is a prefix of the picked rows, so its reference is a slice)."""
    from flooder_amd import core

    dev = torch.device("cuda:0")
    P, V, pick = case_inputs(dim, n)
    ppe, step = PPE[dim], PPE[dim] - 1
    W = gr.lattice(ppe, dim)[torch.as_tensor(pick)]
    tp = torch.as_tensor(P, dtype=torch.float32, device=dev)
    index = core.PointIndex(tp)
    assert index.pts.shape[0] % 16 == 0 and index.pts.shape[0] > n
    samples = torch.einsum("rk,skd->srd", W.to(dev), torch.as_tensor(V, dtype=torch.float64, device=dev))
    small = smallest32(tp.double(), samples.reshape(-1, dim))                 # (S * 513, min(32, n)) float64, ascending
    assert small.max() * step * step < 2 ** 24
    asc = small.astype(np.float32)
    assert np.array_equal(asc.astype(np.float64), small)                       # exact in float32
    b = types.SimpleNamespace(dim=dim, n=n, k1=dim + 1, n_s=V.shape[0], index=index, P=P, V=V, W=W,
                              asc=asc.reshape(V.shape[0], W.shape[0], -1), samples=samples)
    b.verts = torch.as_tensor(V, dtype=torch.float32, device=dev).contiguous()
    return b


@functools.lru_cache(maxsize=None)
def kernel_case(dim, n, R):
    """One case of CASE_R: the first R picked rows as the weight matrix."""
    b = kernel_base(dim, n)
    c = types.SimpleNamespace(dim=dim, n=n, k1=b.k1, R=R, n_s=b.n_s, index=b.index, verts=b.verts, base=b)
    c.asc = np.ascontiguousarray(b.asc[:, :R]).reshape(b.n_s * R, -1)
    assert_reference_bites(c.asc[:, 0], (dim, n, R))
    c.weights = b.W[:R].to(torch.float32).to(b.verts.device).contiguous()
    c.want = c.asc[:, 0].view(np.uint32)                                      # the words of the minimum
    c.common = dict(pts_sorted=b.index.pts, n_pts=b.index.n, dim=dim, k1=b.k1, nodes=b.index.nodes, verts=c.verts,
                    weights=c.weights, R=R, n_simplices=b.n_s)
    return c


def guarded(words, fill, dev):
    """`words` int32 words of `fill` and GUARD words of UNWRITTEN behind them"""
    buf = torch.full((words + GUARD,), UNWRITTEN, dtype=torch.int32, device=dev)
    buf[:words] = fill
    return buf


def read_guarded(buf, words, what):
    got = buf.cpu().numpy()
    assert (got[words:] == UNWRITTEN).all(), f"{what}: guard words behind the output were written"
    return got[:words].view(np.uint32)


def same_words(got, want, what):
    bad = np.argwhere(got != want).ravel()
    assert bad.size == 0, (what, bad.size, [(int(i), hex(got[i]), hex(want[i])) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------ finish harness
def single_tiles():
    from flooder_amd import _native

    return int(_native.load().flooder_finish_single_tiles())


class Setup:
    """A cloud, its index, the top simplices of a landmark complex and the lattice of one dimension."""

    def __init__(self, pts, dev, n_landmarks, ppe, verts=None):
        import flooder_amd as fa
        from flooder_amd import core

        self.pts = pts.to(dev).contiguous()
        self.dim = d = pts.shape[1]
        self.ppe = ppe
        self.index = core.PointIndex(self.pts)
        if verts is None:
            self.lms = fa.generate_landmarks(self.pts, n_landmarks, start_idx=0)
            self.rows = np.asarray(core._build_complex(self.lms, d)[1][d])
            verts = self.lms[torch.as_tensor(self.rows, device=dev)]
        self.verts = verts.to(dev).float().contiguous()
        self.weights, _, face_idxs = core.generate_grid(ppe, d, dev, torch.float32)
        self.faces = core._FaceTable(face_idxs, self.weights.shape[0], dev)
        self.plan = core.SamplePlan(self.weights, self.faces)
        assert self.plan.memb_all is not None
        self.R = self.weights.shape[0]
        self.tiles = (self.R + 63) // 64

    def kdtree_top(self, verts):
        """value of every simplex of `verts` (maximum over all lattice samples) by the kd-tree, as helpers does it"""
        from scipy.spatial import cKDTree
        from oracle import flood_oracle as fo

        tree = cKDTree(self.pts.cpu().numpy(), balanced_tree=False, compact_nodes=False)
        w, _, _ = fo.generate_grid(self.ppe, self.dim, np.float32)
        samples = np.matmul(w[None], verts.cpu().numpy()).astype(np.float32)
        dist, _ = tree.query(samples, workers=-1)
        return dist.max(axis=1)


def finish(su, verts, flag_tiles, subs, **more):
    """flooder_finish_faces_f32 + flooder_face_values_f32 on the tiles `flag_tiles` (simplex * tiles + tile) of `verts`,
    every sample unsettled with seed +inf, under option bvh_subs = subs (and the options `more`).
    Returns (face value bits (S, F) int32, the 7 counters, samples left over by the short-list launch)."""
    from flooder_amd import _native, core

    lib, dev = _native.load(), verts.device
    st = _native.current_stream_ptr(dev)
    S, k1, _ = verts.shape
    R, F = su.R, su.faces.n_faces
    flag_list = torch.as_tensor(np.asarray(flag_tiles, dtype=np.int32), device=dev)
    flag_count = torch.tensor([flag_list.numel()], dtype=torch.int32, device=dev)
    d2 = torch.full((S, R), INF_BITS, dtype=torch.int32, device=dev)
    face_bits = torch.zeros(S * F, dtype=torch.int32, device=dev)
    ctl = torch.zeros(_native.FINISH_CTL_WORDS, dtype=torch.int32, device=dev)
    top = torch.zeros(S, dtype=torch.int64, device=dev)
    top_list = torch.empty(S, dtype=torch.int32, device=dev)
    hard = torch.empty(4 * core.FINISH_HARD_CAP, dtype=torch.int64, device=dev)
    stats = torch.zeros(7, dtype=torch.int64, device=dev)
    out = torch.empty((S, F), dtype=torch.float32, device=dev)
    with options(bvh_subs=subs, **more):
        _native.check(lib.flooder_finish_faces_f32(
            _native.ptr(su.index.pts), su.index.n, su.dim, _native.ptr(su.index.nodes), _native.ptr(verts),
            _native.ptr(su.plan.w_perm), k1, R, S, _native.ptr(flag_list), _native.ptr(flag_count), None, None, None,
            _native.ptr(ctl), _native.ptr(top), _native.ptr(top_list), 1, _native.ptr(d2), _native.ptr(su.plan.memb_all), F,
            _native.ptr(face_bits), None, _native.ptr(hard), core.FINISH_HARD_CAP, _native.ptr(stats), st),
            "flooder_finish_faces_f32")
        _native.check(lib.flooder_face_values_f32(_native.ptr(face_bits), S * F, _native.ptr(out), st), "flooder_face_values_f32")
        torch.cuda.synchronize()
    return out.view(torch.int32).cpu().numpy(), stats.cpu().numpy(), int(ctl[_native.FINISH_CTL_SINGLE_LEFT].item())


def all_tiles(n_simplices, tiles):
    return np.arange(n_simplices * tiles, dtype=np.int32)
