"""Every GPU path on poisoned, guarded workspaces (poison_helper.py; the table of paths: gpu_paths.py).

All device memory of the library comes from the ``torch.empty`` / ``zeros`` / ``full`` of its Python drivers, and in a
test process the caching allocator hands those out as zeros of a fresh segment or as the leftovers of the same call one
test earlier.  Here every call of the shared table runs once unpatched and once under each of the byte patterns 0xFF,
0x7F and 0x01, where every ``torch.empty`` of the library holds the pattern and every allocation sits between two
512-byte guards.  Each poisoned run must equal the unpatched one BIT FOR BIT (a kernel that reads a scratch word before
any launch of the call has written it reads another value under another pattern) and no guard byte may change (a kernel
that writes a few elements past a buffer of the library lands in the allocator's 512-byte rounding in production, and in
somebody else's memory under a C caller's own allocator).  No tolerance is involved.

Shapes: N = 20 011 points (no multiple of 16, 64 or 1024: the last leaf, the last tile and every tree level are
padded), 3 001 queries, 8 003 points for the gradients, lattices whose R is no multiple of 64 (asserted), and a tiny
cloud of 1 037 points per family.  The checks the table carries (exact_fps, the driver that ran, the k of the k-nearest
cases, reached and unreached queries) are made on the unpatched result of the large cloud; the tiny cloud is compared
bit for bit (its landmark selections also with exact_fps).

Waits on the device, read before the first run.  A poisoned word that a kernel spins on would hang the GPU, so the
wait loops were looked for in the sources: the only device-side ones are the look-back of the radix sort
(csrc/flood_index.hip, ``os_sort_pairs``: rocprim's onesweep states, read until a block's prefix is published) - every
other counter below is a ticket: fetched with an atomic add and compared with a total, never waited for.  Who clears
them, for any n >= 1 (20 011 and 1 037 included: each clearing loop is a grid-stride loop over ALL words of the block
in a launch of at least one workgroup):

  buffer                                   cleared by                                where
  ---------------------------------------  ----------------------------------------  -----------------------------------
  PointIndex ``zeroed`` = density grid |    flooder_morton_zero_f32: every thread    flood_bvh.hip morton_kernel, first
  sort state (digit histograms, look-back  of the curve-code launch clears its       loop over ``zero_words`` =
  arrays, tickets, last block's offsets)   share of all n_dens + n_state words       zeroed.numel(); grid (n+255)/256 >= 1
  ... laid out by os_sort_pairs for        (the state words are sized for the        flood_index.hip os_state_words /
  os_blocks(n, shape) blocks               SMALLEST block shape: the most blocks)    os_sort_pairs
  sort state, SORT_STATE_BY_CALLER=False   flooder_index_sort: rocprim's own         rocprim::radix_sort_pairs inside
                                           memsets inside ``tmp``                    ``tmp`` (flooder_index_sort_bytes)
  k-d order (dim > 3): sort state inside   kd_key_kernel of EVERY level, before      flood_index.hip kd_key_kernel, first
  ``tmp`` behind keys and rows             that level's os_sort_pairs                loop; KdOrderOp::run
  sample sorts (sorted sweeps, queries):   core._zeroed_queue: ONE torch.zeros for   core.py _zeroed_queue (state sized
  queue heads | sort state                 QUEUE_WORDS + state words                 for 32 key bits, sorts use <= 32)
  fused sweep ``arena``: wit_queue,        flooder_simplex_prepare_f32: every        flood_finish.hip
  cell_queue, finish_ctl, top, ctl,        thread clears its share of all n_words;   simplex_weight_kernel, first loop;
  face_bits, face_owner, result            torch.zeros where CELL_SUPER or           core.py FusedWorkspace
                                           SWEEP_PREPARE_FUSED is off
  unfused cell sweep ``ctl`` (flag         torch.zeros                               core.py _sweep_dimension_cell
  counter, list length, queue heads)
  tree / k-nearest / power / float64       torch.zeros(QUEUE_WORDS) or               core.py, neighbors.py
  sweeps ``queue``                         core._zeroed_queue
  ball sweep ``cursor`` (+ sweep queue)    torch.zeros                               core.py _sweep_dimension_hip
  landmark selection ``work_best``,        ONE torch.zeros (batched); torch.zeros    core.py fps_indices,
  ``work_ctr``                             (one per launch, brute force)             _fps_bucket_one_per_launch

  None of them is left to a later launch or cleared in part; the tests below then make the rest of the scratch hostile.

Runs on a real MI355X only (-m gpu)."""
import time

import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from helpers import get_options, set_options
from oracle import flood_oracle as fo
import gpu_paths as gp
import streams_helper as sh
from poison_helper import PATTERNS, poisoned

pytestmark = pytest.mark.gpu

N, Q, GRAD_N, TINY = 20_011, 3_001, 8_003, 1_037
SIZES = {"ragged": N, "tiny": TINY}
GRAD_SIZES = {"ragged": GRAD_N, "tiny": TINY}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    assert N % 16 and N % 64 and N % 1024 and Q % 64 and GRAD_N % 16 and TINY % 16
    return _native.load()


@pytest.fixture(autouse=True)
def stop_at_a_gpu_fault():
    """A fault of the device poisons every later GPU test of the process (and the machine is shared): end the session."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # (an illegal access, a hang the runtime gave up on)
        pytest.exit(f"the GPU reported {e!s:.200} - nothing more is run on it", returncode=3)


@pytest.fixture
def options(lib):
    """set(name=value, ...) for options of the native library; put back after the test."""
    keep = get_options(lib, b"fps_switch", b"fps_rounds", b"fps_lane_best")

    def set_(**values):
        set_options(lib, {k.encode(): v for k, v in values.items()})

    yield set_
    set_options(lib, keep)


def compare(label, f, args, ref, patterns=PATTERNS):
    """``f(*args)`` under each pattern: the outputs equal ``ref`` (the unpatched outputs on the host) bit for bit and
    every guard of every allocation of the call is intact."""
    for pattern in patterns:
        t0 = time.perf_counter()
        with poisoned(pattern, "cuda") as rec:
            got = sh.to_host(f(*args))
            broken = rec.broken()
            n_alloc, n_poisoned = len(rec), sum(a.kind.startswith("empty") for a in rec.allocations)
        print(f"[poison] {label} 0x{pattern:02X}: {n_alloc} guarded allocations, {n_poisoned} of them poisoned, "
              f"{(time.perf_counter() - t0) * 1e3:.0f} ms")
        assert n_poisoned > 0, f"{label}: the call allocated nothing through torch.empty - the harness saw none of it"
        assert sh.same_bits(got, ref), (f"{label}: under pattern 0x{pattern:02X} the result differs from the unpatched run "
                                        f"(outputs {sh.differing(got, ref)}): a scratch word is read before it is written")
        assert not broken, f"{label}: under pattern 0x{pattern:02X} guard bytes changed: {broken}"


def reference_and_poisoned(label, f, args):
    """The unpatched outputs on the host (the reference), then ``compare`` under every pattern."""
    ref = sh.to_host(f(*args))
    torch.cuda.synchronize()
    compare(label, f, args, ref)
    return ref


# --------------------------------------------------------------------------------------------------- index
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("dim,by_caller", gp.INDEX_CASES)
def test_poisoned_point_index(dim, by_caller, size, lib, monkeypatch):
    monkeypatch.setattr(core, "SORT_STATE_BY_CALLER", by_caller)
    n = SIZES[size]
    cloud = gp.randn(n, dim, 10 + dim)
    assert core.PointIndex(cloud).kd == (dim == 6)
    # (index_parts leaves out the lanes [dim:8] and [8+dim:16] of the box, which no kernel defines)
    reference_and_poisoned(f"PointIndex {dim}-D, {n} points{'' if by_caller else ' (sort fills its state)'}",
                           lambda p: gp.index_parts(core.PointIndex(p)), (cloud,))


def test_poisoned_index_from_host_in_chunks(lib):
    points = torch.randn(N, 3, generator=torch.Generator().manual_seed(31)).pin_memory()

    def run(points_cpu):
        index, raw = core.index_from_host(points_cpu, gp.DEV, chunk_rows=7000)   # 3 chunks, the last one short
        return gp.index_parts(index) + [raw]

    ref = reference_and_poisoned("index_from_host, 3 chunks", run, (points,))
    assert sh.same_bits(ref[:-1], sh.to_host(gp.index_parts(core.PointIndex(points.to(gp.DEV)))))


# --------------------------------------------------------------------------------------------------- landmarks
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", list(gp.FPS_CASES))
def test_poisoned_landmark_selection(case, size, options, monkeypatch):
    dim, method, batched, opts, launches = gp.FPS_CASES[case]
    n = SIZES[size]
    monkeypatch.setattr(core, "FPS_BUCKET_MIN_POINTS", 0)
    monkeypatch.setattr(core, "FPS_BATCHED", batched)
    monkeypatch.setattr(core, "LAST_FPS_LAUNCHES", -1)
    options(**opts)
    cloud = gp.randn(n, dim, 40 + dim)
    ref = reference_and_poisoned(f"fps_indices {case}, {n} points", lambda p: core.fps_indices(p, gp.N_LMS, 5, method=method),
                                 (cloud,))
    if launches is None:
        assert core.LAST_FPS_LAUNCHES == -1, "the batched entry ran"
    elif size == "ragged":
        assert 7 < core.LAST_FPS_LAUNCHES < gp.N_LMS - 1, f"no launch selected more than one landmark ({core.LAST_FPS_LAUNCHES})"
    else:   # (1 037 points are 17 buckets: how many landmarks a launch takes there is not the point)
        assert core.LAST_FPS_LAUNCHES != -1, "the batched entry did not run"
    assert np.array_equal(ref, fo.exact_fps(cloud.cpu().numpy(), gp.N_LMS, 5))
    if case == "batched":   # the public entry on the same path
        got = reference_and_poisoned(f"generate_landmarks (batched), {n} points",
                                     lambda p: fa.generate_landmarks(p, gp.N_LMS, start_idx=5), (cloud,))
        assert np.array_equal(got, cloud.cpu().numpy()[ref])


# --------------------------------------------------------------------------------------------------- flood_complex
def assert_ragged_lattice(label):
    """The samples per simplex of the call that has just run are no multiple of the 64-sample tile."""
    R = core.LAST_STATS.samples_per_simplex
    assert R > 0 and R % 64 != 0, f"{label}: R = {R} is a multiple of 64 - no ragged last tile (take one more point per edge)"
    return R


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", list(gp.FLOOD_CASE_NAMES))
def test_poisoned_flood_complex(case, size, lib, monkeypatch):
    n = SIZES[size]
    dim, dtype, kw, driver = gp.flood_cases(n)[case]
    ran, ks = gp.watch_sweeps(monkeypatch)
    if case == "3d_mass_100":
        assert core.mass_neighbors(kw["neighbor_mass"], n) == 100 > 64
    (args,) = gp.flood_arguments(case, n, (60,))
    keys, values = reference_and_poisoned(f"flood_complex {case}, {n} points", lambda *a: gp.flood(*a, **kw), args)
    assert_ragged_lattice(case)
    assert max(len(k) for k in keys) == dim + 1 and np.isfinite(values).all() and values.max() > 0
    gp.check_flood_path(case, n, ran, ks)


# Switches of the fused 2-D / 3-D sweep (the default production path, and the one with the most scratch) that change
# which buffers exist or who clears them, one at a time; each is compared with its own unpatched run.  The lattices have
# core.WIT_MIN_ROWS rows and more, so that the witness sweep can take part where its switch asks for it.
FUSED_SWITCHES = [("SWEEP_PREPARE_FUSED", False), ("CELL_SUPER", False), ("CELL_PROBE", False), ("FACE_OWNER", False),
                  ("SHARED_FACE_SLOTS", False), ("FUSED_FACES", False), ("WIT_MIN_SIMPLICES", 0), ("FINISH_HARD_CAP", 64),
                  ("SORT_STATE_BY_CALLER", False), ("CELL_DENSITY_GRID", False)]
FUSED_CLOUDS = {3: dict(points_per_edge=14), 2: dict(points_per_edge=32)}


@pytest.fixture(scope="module")
def fused_defaults(lib):
    """{dim: the result of the fused-switch call with every switch at its default, on the host}."""
    return {dim: sh.to_host(gp.flood(gp.randn(N, dim, 150 + dim), n_lms=60, **kw)) for dim, kw in FUSED_CLOUDS.items()}


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("switch,value", FUSED_SWITCHES, ids=[f"{s}={v}" for s, v in FUSED_SWITCHES])
def test_poisoned_fused_sweep_switches(switch, value, dim, lib, fused_defaults, monkeypatch):
    assert getattr(core, switch) != value, f"core.{switch} is {value} already: the case switches nothing"
    monkeypatch.setattr(core, switch, value)
    ran, _ = gp.watch_sweeps(monkeypatch)
    witness_launches = []
    real_witness = lib.flooder_fused_witness
    monkeypatch.setattr(lib, "flooder_fused_witness", lambda *a: witness_launches.append(1) or real_witness(*a))
    cloud = gp.randn(N, dim, 150 + dim)
    kw = FUSED_CLOUDS[dim]
    keys, values = reference_and_poisoned(f"flood_complex {dim}-D with core.{switch} = {value}",
                                          lambda p: gp.flood(p, n_lms=60, **kw), (cloud,))
    assert assert_ragged_lattice(switch) >= core.WIT_MIN_ROWS
    assert ran == {"_sweep_dimension_cell"} and np.isfinite(values).all() and values.max() > 0
    # (every one of these switches chooses between ways to the same exact values)
    assert sh.same_bits([keys, values], fused_defaults[dim]), f"core.{switch} = {value} changes a filtration value"
    if switch == "WIT_MIN_SIMPLICES":
        assert len(witness_launches) == 1 + len(PATTERNS), "the witness sweep did not take part"
    else:
        assert not witness_launches


# --------------------------------------------------------------------------------------------------- neighbours
@pytest.fixture(scope="module")
def neighbour_clouds():
    return {size: gp.neighbour_clouds(n, Q if size == "ragged" else 517, seeds=(80,))[0] for size, n in SIZES.items()}


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("call", list(gp.NEIGHBOUR_CALLS))
def test_poisoned_neighbour_family(call, size, neighbour_clouds, lib):
    ref = reference_and_poisoned(f"{call}, {SIZES[size]} points", gp.NEIGHBOUR_CALLS[call], neighbour_clouds[size])
    if size == "ragged":
        gp.check_neighbour_result(call, ref)


# --------------------------------------------------------------------------------------------------- profiles
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("call", list(gp.PROFILE_CALL_NAMES))
def test_poisoned_profiles(call, size, lib):
    n = SIZES[size]
    (args,) = gp.profile_arguments(n, 1)
    ref = reference_and_poisoned(f"{call}, {n} points", gp.profile_calls(n)[call], args)
    assert all(np.isfinite(t).all() for t in ref) and ref[3].shape[1] >= 2


# --------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("size", list(GRAD_SIZES))
@pytest.mark.parametrize("call", list(gp.GRAD_CALL_NAMES))
def test_poisoned_gradients(call, size, lib):
    """Forward and backward (on autograd's worker thread: the patch is process-wide) under the patterns."""
    n = GRAD_SIZES[size]
    (cloud,) = gp.grad_clouds(n, (120,))
    ref = reference_and_poisoned(f"{call}, {n} points", gp.with_grad(gp.grad_calls(n)[call]), (cloud,))
    grad = ref[-1]
    assert np.isfinite(grad).all() and np.any(grad != 0)
    if size == "ragged":
        assert all(np.isfinite(v).all() for v in ref[:-1]), "a value is not finite (a point not reached)"


# --------------------------------------------------------------------------------------------------- the detector
def test_a_missing_fill_is_detected(lib, monkeypatch):
    """The harness can fail: ``method="ball"`` fills its (S, R) distance words with +inf by ``flooder_fill_u32`` before
    the sweep lowers them with atomic minima.  Without the fill the words hold what the allocator returned; under 0x01
    that is 2.4e-38, below every squared distance, and the result differs from the reference.  (Distance words only: no
    index or address is derived from them.)"""
    kw = dict(points_per_edge=12, method="ball")
    cloud = gp.randn(N, 3, 63)
    ref = sh.to_host(gp.flood(cloud, **kw))
    torch.cuda.synchronize()
    compare("flood_complex ball", lambda p: gp.flood(p, **kw), (cloud,), ref, patterns=(0x01,))
    monkeypatch.setattr(lib, "flooder_fill_u32", lambda *a: 0)
    with pytest.raises(AssertionError, match="a scratch word is read before it is written"):
        compare("flood_complex ball without its fill", lambda p: gp.flood(p, **kw), (cloud,), ref, patterns=(0x01,))
