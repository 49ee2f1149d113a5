"""Every GPU path on a side stream while the default stream is held (streams_helper.py: the hold and the held call).

All other GPU tests run on the default stream; here the current stream is a side stream and the default stream is
occupied by one long kernel.  A launch that lands on the default stream then sits behind the hold and its effect is
missing when the side stream reads it (the outputs differ from the default-stream reference); a device-wide wait or a
wait for the default stream outlasts the hold (``held.query()`` is True when the outputs are on the host).  Then: the
pinned progress words of the batched landmark selection on nine streams past the tag wrap, the module-level tables filled
on one stream and used on another, and the landmark selection above ``flooder_fps_batched_max_points()``.
Runs on a real MI355X only (-m gpu)."""
import numpy as np
import pytest
import torch

import flooder_amd as fa
from flooder_amd import _native, core
from helpers import get_options, set_options
from oracle import flood_oracle as fo
import streams_helper as sh
import gpu_paths
from gpu_paths import (DEV, FPS_CASES, INDEX_CASES, N_LMS, NEIGHBOUR_CALLS, check_flood_path, check_neighbour_result, flood,
                       flood_arguments, flood_cases, grad_calls, grad_clouds, index_parts, profile_arguments, profile_calls,
                       randn, watch_sweeps, with_grad)

pytestmark = pytest.mark.gpu

N = 20_000
FLOOD_CASES = flood_cases(N)
PROFILE_CALLS = profile_calls(N)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return _native.load()


@pytest.fixture(scope="module")
def free_streams(lib):
    """Side streams that run while the default stream is held, found by trying: the runtime maps all streams of a process
    onto a few hardware queues, and a pool stream that shares the default stream's queue runs BEHIND the default
    stream's kernels whatever its flags (one in eight with four queues).  Such a stream cannot tell a misplaced launch
    from its own queueing and is passed over; ``test_premise`` asserts that the chosen stream is not one of them."""
    x = torch.arange(1024, device=DEV, dtype=torch.float32)
    found, tried = [], 0
    try:
        while len(found) < 2 and tried < 12:
            s = torch.cuda.Stream()
            tried += 1
            if any(s == t for t in found):
                continue
            with torch.cuda.stream(s):
                (x + 1).cpu()          # (first use of the stream)
            torch.cuda.synchronize()
            held = sh.hold(DEV, 0.05)
            with torch.cuda.stream(s):
                (x + 1).cpu()
                free = not held.query()
            torch.cuda.synchronize()
            if free:
                found.append(s)
    finally:
        torch.cuda.synchronize()
    print(f"[streams] hold by {sh.hold_kind(DEV)}; {len(found)} free side streams among the first {tried} of the pool")
    assert len(found) == 2, (f"only {len(found)} of {tried} pool streams ran while the default stream was held: "
                             "the held tests have no side stream to run on")
    return found


@pytest.fixture(scope="module")
def side(free_streams):
    return free_streams[0]


@pytest.fixture
def options(lib):
    """set(name=value, ...) for options of the native library; put back after the test."""
    keep = get_options(lib, b"fps_switch", b"fps_rounds", b"fps_lane_best")

    def set_(**values):
        set_options(lib, {k.encode(): v for k, v in values.items()})

    yield set_
    set_options(lib, keep)


# --------------------------------------------------------------------------------------------------- 1. the premise
def test_premise_a_side_stream_does_not_wait_for_the_held_default_stream(side):
    x = torch.arange(1 << 16, device=DEV, dtype=torch.float32)
    torch.cuda.synchronize()
    try:
        held = sh.hold(DEV, 0.2)
        with torch.cuda.stream(side):
            y = (x * 2 + 1).cpu()
            still_held = not held.query()
        assert still_held, "a torch op and .cpu() on a side stream waited for the held default stream"
        assert torch.equal(y, torch.arange(1 << 16, dtype=torch.float32) * 2 + 1)
        held.synchronize()
        assert held.query()
    finally:
        torch.cuda.synchronize()


def test_the_held_call_notices_a_misplaced_launch_and_a_device_wide_wait(side, monkeypatch):
    """The detector itself: the bounding-box launch put on the default stream whenever a side stream is current fails
    step 6 (its result is not there when the side stream reads it), a device-wide wait inside the call fails step 5."""
    real, decoy = randn(N, 3, 1), randn(N, 3, 2)

    def on_a_side_stream():
        return torch.cuda.current_stream(DEV) != torch.cuda.default_stream(DEV)

    def misplaced(p):
        with monkeypatch.context() as m:
            if on_a_side_stream():
                m.setattr(_native, "current_stream_ptr", lambda device: 0)
            box = core.cloud_box(p)
            return [box[:3], box[8:11]]

    def waits(p):
        if on_a_side_stream():
            torch.cuda.synchronize()
        return p.sum(dim=0)

    with pytest.raises(AssertionError, match="differs from the default-stream reference"):
        sh.held_call("misplaced launch", misplaced, (real,), (decoy,), side)
    with pytest.raises(AssertionError, match="outlasted its hold or waited for the default stream"):
        sh.held_call("device-wide wait", waits, (real,), (decoy,), side)


# --------------------------------------------------------------------------------------------------- 2. index
@pytest.mark.parametrize("dim,by_caller", INDEX_CASES)
def test_held_point_index(dim, by_caller, side, monkeypatch):
    monkeypatch.setattr(core, "SORT_STATE_BY_CALLER", by_caller)
    real, decoy = randn(N, dim, 10 + dim), randn(N, dim, 20 + dim)
    assert core.PointIndex(real).kd == (dim == 6)
    sh.held_call(f"PointIndex {dim}-D{'' if by_caller else ' (sort fills its state)'}",
                 lambda p: index_parts(core.PointIndex(p)), (real,), (decoy,), side)


def test_held_index_from_host_in_chunks(free_streams):
    """``index_from_host`` with the side stream as its compute stream; the copy stream is the second stream known to
    run during a hold (a pool stream of its own choice may share the default stream's hardware queue: free_streams)."""
    side, copy = free_streams
    g = torch.Generator().manual_seed(31)
    real, decoy = torch.randn(N, 3, generator=g).pin_memory(), torch.randn(N, 3, generator=g).pin_memory()

    def run(points_cpu, copy_stream=copy):
        index, raw = core.index_from_host(points_cpu, DEV, chunk_rows=7000, copy_stream=copy_stream)   # 3 chunks
        lms = fa.generate_landmarks(raw, 40, start_idx=0)
        return index_parts(index) + [raw, fa.flood_complex(raw, lms, points_per_edge=10, index=index)]

    ref = sh.held_call("index_from_host, 3 chunks, + flood_complex", run, (real,), (decoy,), side)
    on_dev = real.to(DEV)
    plain = core.PointIndex(on_dev)
    lms = fa.generate_landmarks(on_dev, 40, start_idx=0)
    want = sh.to_host(index_parts(plain) + [on_dev, fa.flood_complex(on_dev, lms, points_per_edge=10)])
    assert sh.same_bits(ref, want), "index_from_host differs from PointIndex(points.to(device))"
    with torch.cuda.stream(side):   # ... and with a copy stream from the pool, not held
        pooled = sh.to_host(run(real, None))
    torch.cuda.synchronize()
    assert sh.same_bits(pooled, want)


# --------------------------------------------------------------------------------------------------- 2. landmarks
@pytest.mark.parametrize("case", list(FPS_CASES))
def test_held_landmark_selection(case, side, options, monkeypatch):
    dim, method, batched, opts, launches = FPS_CASES[case]
    monkeypatch.setattr(core, "FPS_BUCKET_MIN_POINTS", 0)
    monkeypatch.setattr(core, "FPS_BATCHED", batched)
    monkeypatch.setattr(core, "LAST_FPS_LAUNCHES", -1)
    options(**opts)
    real, decoy = randn(N, dim, 40 + dim), randn(N, dim, 50 + dim)
    ref = sh.held_call(f"fps_indices {case}", lambda p: core.fps_indices(p, N_LMS, 5, method=method),
                       (real,), (decoy,), side)
    if launches is None:
        assert core.LAST_FPS_LAUNCHES == -1, "the batched entry ran"
    else:
        assert 7 < core.LAST_FPS_LAUNCHES < N_LMS - 1, f"no launch selected more than one landmark ({core.LAST_FPS_LAUNCHES})"
    assert np.array_equal(ref, fo.exact_fps(real.cpu().numpy(), N_LMS, 5))
    if case == "batched":   # the public entry on the same path
        want = real.cpu().numpy()[ref]
        sh.held_call("generate_landmarks (batched)", lambda p: fa.generate_landmarks(p, N_LMS, start_idx=5),
                     (real,), (decoy,), side)
        assert np.array_equal(fa.generate_landmarks(real, N_LMS, start_idx=5).cpu().numpy(), want)


# --------------------------------------------------------------------------------------------------- 2. flood_complex
@pytest.mark.parametrize("case", list(FLOOD_CASES))
def test_held_flood_complex(case, side, monkeypatch):
    dim, dtype, kw, driver = FLOOD_CASES[case]
    ran, ks = watch_sweeps(monkeypatch)
    if case == "3d_mass_100":
        assert core.mass_neighbors(kw["neighbor_mass"], N) == 100 > 64
    args = flood_arguments(case, N, (60, 70))
    ref = sh.held_call(f"flood_complex {case}", lambda *a: flood(*a, **kw), args[0], args[1], side)
    keys, values = ref
    assert max(len(k) for k in keys) == dim + 1 and np.isfinite(values).all() and values.max() > 0
    check_flood_path(case, N, ran, ks)


# --------------------------------------------------------------------------------------------------- 2. neighbours
@pytest.fixture(scope="module")
def neighbour_clouds():
    return gpu_paths.neighbour_clouds(N, 3000)


@pytest.mark.parametrize("call", list(NEIGHBOUR_CALLS))
def test_held_neighbour_family(call, side, neighbour_clouds):
    real, decoy = neighbour_clouds
    ref = sh.held_call(call, NEIGHBOUR_CALLS[call], real, decoy, side)
    check_neighbour_result(call, ref)


# --------------------------------------------------------------------------------------------------- 2. profiles
@pytest.mark.parametrize("call", list(PROFILE_CALLS))
def test_held_profiles(call, side):
    args = profile_arguments(N)
    ref = sh.held_call(call, PROFILE_CALLS[call], args[0], args[1], side)
    assert all(np.isfinite(t).all() for t in ref) and ref[3].shape[1] >= 2


# --------------------------------------------------------------------------------------------------- 2. gradients
GRAD_N = 8000
GRAD_CALLS = grad_calls(GRAD_N)
# calls whose step 5 (still held when the outputs are on the host) is not asserted, with the reason (none so far)
GRAD_WITHOUT_STEP_5 = {}


@pytest.mark.parametrize("call", list(GRAD_CALLS))
def test_held_gradients(call, side):
    """Forward, ``torch.autograd.grad`` and the read of the gradient inside the side-stream context: the backward runs on
    autograd's worker thread, on the stream of its forward."""
    real, decoy = grad_clouds(GRAD_N)
    ref = sh.held_call(call, with_grad(GRAD_CALLS[call]), (real,), (decoy,), side,
                       check_hold=call not in GRAD_WITHOUT_STEP_5)
    grad = ref[-1]
    assert np.isfinite(grad).all() and np.any(grad != 0)
    assert all(np.isfinite(v).all() for v in ref[:-1]), "a value is not finite (a point not reached)"


# --------------------------------------------------------------------------------------------------- 3. progress words
# (the Gaussian cloud is the larger one: 4096 points are the 64 buckets of one workgroup, and no launch of the selection
# takes more than one landmark from them)
WORDS_N, WORDS_N_GAUSS, WORDS_LMS, WORDS_STARTS = 4096, 20_000, 96, (0, 1234)


@pytest.fixture(scope="module")
def word_cases(lib):
    """[(cloud, its PointIndex, start, exact_fps)] x 4: a permuted integer lattice (ties decided by index alone) and a
    Gaussian cloud, two start indices each; alternating from entry to entry."""
    g = torch.Generator().manual_seed(140)
    axis = torch.arange(16.0)
    lattice = torch.cartesian_prod(axis, axis, axis)[torch.randperm(WORDS_N, generator=g)].contiguous()
    gauss = torch.randn(WORDS_N_GAUSS, 3, generator=g)
    cases = []
    for start in WORDS_STARTS:
        for kind, cloud in (("lattice", lattice), ("gauss", gauss)):
            cases.append((kind, cloud.to(DEV), start, fo.exact_fps(cloud.numpy(), WORDS_LMS, start)))
    indices = {"lattice": core.PointIndex(cases[0][1]), "gauss": core.PointIndex(cases[1][1])}
    torch.cuda.synchronize()
    return [(kind, cloud, indices[kind], start, want) for kind, cloud, start, want in cases]


def select_round_robin(word_cases, streams, n_calls):
    """``n_calls`` selections, call i on stream i mod len(streams) and case i mod 4, nothing synchronised in between ->
    the calls whose result is wrong, the launches of the Gaussian calls."""
    got, launches = [], []
    try:
        for i in range(n_calls):
            kind, cloud, index, start, want = word_cases[i % 4]
            with torch.cuda.stream(streams[i % len(streams)]):
                got.append(core.fps_indices(cloud, WORDS_LMS, start, method="bucket", index=index))
            if kind == "gauss":
                launches.append(core.LAST_FPS_LAUNCHES)
    finally:
        torch.cuda.synchronize()
    wrong = [i for i, idx in enumerate(got) if not np.array_equal(idx.cpu().numpy(), word_cases[i % 4][4])]
    return wrong, launches


@pytest.fixture
def tiny_batched(options, monkeypatch):
    monkeypatch.setattr(core, "FPS_BUCKET_MIN_POINTS", 0)
    monkeypatch.setattr(core, "FPS_BATCHED", True)
    options(fps_switch=8)
    return options


def test_progress_words_shared_by_nine_streams(word_cases, tiny_batched):
    """Nine streams: one more than there are progress words per device, so two of them share a word whatever the hash;
    270 selections round-robin.  (The tags are counted per word: this spreads the 270 over up to eight words and takes
    none of them past its 255 tags - the test below does.)"""
    streams = [torch.cuda.Stream() for _ in range(9)]
    assert len({s.cuda_stream for s in streams}) == 9
    wrong, launches = select_round_robin(word_cases, streams, 270)
    assert not wrong, f"selections {wrong[:10]} of 270 over nine streams differ from exact_fps"
    assert max(launches) < WORDS_LMS, f"no launch selected more than one landmark ({max(launches)}): no batching"


def test_one_progress_word_past_its_tag_wrap(word_cases, tiny_batched):
    """A word's tag is (its own call count mod 255) + 1, so 256 calls on ONE stream take that stream's word through
    every tag and back to the first one it used here, whatever the count it started with; 264 are run, nothing
    synchronised in between, so each call also meets the late stores of the one before it - which, right after the
    wrap, carry a tag that compares as the OLDEST one.  Every result must be ``exact_fps``."""
    wrong, launches = select_round_robin(word_cases, [torch.cuda.Stream()], 264)
    assert not wrong, f"selections {wrong[:10]} of 264 on one stream differ from exact_fps"
    assert max(launches) < WORDS_LMS, f"no launch selected more than one landmark ({max(launches)}): no batching"


def test_back_to_back_selections_with_surplus_launches_in_flight(word_cases, tiny_batched):
    """A, B on the other cloud, A again on ONE side stream with nothing in between: B's progress word sees the late
    stores of A's surplus launches."""
    stream = torch.cuda.Stream()
    order = [word_cases[1], word_cases[0], word_cases[1], word_cases[2], word_cases[3], word_cases[2]]
    got = []
    try:
        with torch.cuda.stream(stream):
            for kind, cloud, index, start, want in order:
                got.append(core.fps_indices(cloud, WORDS_LMS, start, method="bucket", index=index))
    finally:
        torch.cuda.synchronize()
    for i, (idx, case) in enumerate(zip(got, order)):
        assert np.array_equal(idx.cpu().numpy(), case[4]), f"call {i} ({case[0]}, start {case[3]}) differs from exact_fps"


def test_counter_read_back_on_nine_streams(word_cases, tiny_batched):
    """The path without pinned memory (``fps_rounds``): rounds of launches and a read-back that waits for the given
    stream alone; one pass over the nine streams."""
    tiny_batched(fps_rounds=1)
    wrong, launches = select_round_robin(word_cases, [torch.cuda.Stream() for _ in range(9)], 9)
    assert not wrong, f"selections {wrong} differ from exact_fps"
    assert max(launches) < WORDS_LMS


# --------------------------------------------------------------------------------------------------- 4. module tables
def test_tables_cached_on_one_stream_serve_the_others(monkeypatch):
    """``_GRID_CACHE``, ``_SAMPLE_ORDER_CACHE`` and ``_WIT_PLAN_CACHE`` are filled by the first call - here on side
    stream A - and read by the calls behind it on stream B and on the default stream, with no synchronisation of the
    test's own in between.  Some of the tables are written by kernels on A's stream; they are complete for B because the
    call that made them brought its results to the host (a wait for its stream) before it returned.  This check can
    catch a race; it cannot prove that there is none."""
    p3, p2 = randn(N, 3, 150), randn(N, 2, 151)
    kw3, kw2 = dict(points_per_edge=14), dict(points_per_edge=32)    # (lattices of WIT_MIN_ROWS rows: a witness plan)
    monkeypatch.setattr(core, "WIT_MIN_SIMPLICES", 0)
    try:
        want = sh.to_host([fa.flood_complex(p3, 60, **kw3), fa.flood_complex(p2, 60, **kw2)])
        torch.cuda.synchronize()
        core._GRID_CACHE.clear()
        core._SAMPLE_ORDER_CACHE.clear()
        core._WIT_PLAN_CACHE.clear()
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        got = []
        for stream in (a, b, torch.cuda.default_stream(DEV)):
            with torch.cuda.stream(stream):
                got.append(sh.to_host([fa.flood_complex(p3, 60, **kw3), fa.flood_complex(p2, 60, **kw2)]))
        assert core._GRID_CACHE and core._SAMPLE_ORDER_CACHE, "the tables were not cached"
        assert any(v is not None for v in core._WIT_PLAN_CACHE.values()), "no witness plan was made and cached"
    finally:
        torch.cuda.synchronize()
    for where, g in zip(("stream A (filled the tables)", "stream B", "the default stream"), got):
        assert sh.same_bits(g, want), f"flood_complex on {where} differs from the reference"


# --------------------------------------------------------------------------------------------------- 5. largest clouds
@pytest.fixture
def small_batched_limit(lib, monkeypatch):
    """The branch of ``fps_indices`` for clouds above ``flooder_fps_batched_max_points()`` at 20 000 points."""
    monkeypatch.setattr(lib, "flooder_fps_batched_max_points", lambda: 10_000)
    monkeypatch.setattr(core, "FPS_BUCKET_MIN_POINTS", 0)
    monkeypatch.setattr(core, "FPS_BATCHED", True)
    monkeypatch.setattr(core, "LAST_FPS_LAUNCHES", -1)


@pytest.mark.parametrize("dim", [3, 5])
def test_selection_above_the_batched_limit(dim, small_batched_limit, side):
    """3-D: the one-per-launch kernels; 5-D: brute force.  Neither is the batched entry."""
    real, decoy = randn(N, dim, 160 + dim), randn(N, dim, 170 + dim)
    want = fo.exact_fps(real.cpu().numpy(), 100, 3)
    assert np.array_equal(core.fps_indices(real, 100, 3, method="bucket").cpu().numpy(), want)
    if dim == 3:
        ref = sh.held_call("fps_indices above the batched limit", lambda p: core.fps_indices(p, 100, 3, method="bucket"),
                           (real,), (decoy,), side)
        assert np.array_equal(ref, want)
    assert core.LAST_FPS_LAUNCHES == -1, "the batched entry ran"


def test_return_index_above_the_batched_limit(small_batched_limit):
    points = randn(N, 3, 180)
    lms, idx = fa.generate_landmarks(points, 100, start_idx=0, return_index=True)
    assert core.LAST_FPS_LAUNCHES == -1, "the batched entry ran"
    assert isinstance(idx, core.PointIndex), f"return_index=True gave {idx!r} for a cloud above the batched limit"
    assert np.array_equal(lms.cpu().numpy(), points.cpu().numpy()[fo.exact_fps(points.cpu().numpy(), 100, 0)])
    with_index = fa.flood_complex(points, lms, points_per_edge=10, index=idx)
    assert with_index == fa.flood_complex(points, lms, points_per_edge=10)
