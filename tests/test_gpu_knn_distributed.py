"""``flood_complex_sharded(mode="points", neighbors=k > 1)`` through real process groups on the one GPU there is: a
one-rank ``nccl`` world with the collectives forced (``all_gather_into_tensor`` over RCCL), and a two-rank gloo world
(RCCL refuses two ranks on one device), which is the gather staged through pinned host memory.  Every rank must return
the unsharded dict; k larger than the whole cloud raises on every rank."""

import os
import pickle
import socket
import sys
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN_LIMIT_S = 240            # a worker that has not ended by then is killed and the test fails
RUNS = (("kth", dict(points_per_edge=5)), ("dtm", dict(num_rand=30)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _inputs():
    g = torch.Generator().manual_seed(77)
    pts = torch.rand(1500, 3, generator=g)
    return pts, pts[:14].clone()


def _worker(rank, world, port, backend, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flooder_amd import _native, core
        from flooder_amd.distributed import flood_complex_sharded, knn_gather_hook, shard_points

        _native.load()  # no fallback: the HIP library must be there
        hook = knn_gather_hook(always=True)
        assert hook.world_size == world and hook.checks_ranks
        pts, lms = _inputs()
        pts, lms = pts.to(dev), lms.to(dev)
        mine = shard_points(pts, rank, world)
        merges = []
        orig = core._sweep_dimension_knn_sharded
        core._sweep_dimension_knn_sharded = lambda *a, **k: merges.append(1) or orig(*a, **k)
        res = {}
        for n, (stat, kw) in enumerate(RUNS):
            torch.manual_seed(5 if rank == 0 else 900 + rank)
            res[n] = flood_complex_sharded(mine, lms, mode="points", neighbors=8, neighbor_stat=stat,
                                           always_reduce=True, **kw)
        res["merges"] = len(merges)
        # more neighbours than the ranks hold together: every rank raises, none hangs
        few = shard_points(pts[:20], rank, world)
        try:
            flood_complex_sharded(few, lms, mode="points", neighbors=21, always_reduce=True, points_per_edge=5)
            res["too_many"] = "no error"
        except ValueError as e:
            res["too_many"] = str(e)
        res["just_enough"] = flood_complex_sharded(few, lms, mode="points", neighbors=20, always_reduce=True,
                                                   points_per_edge=5)
        with open(os.path.join(out_dir, f"r{rank}.pkl"), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def _spawn(world, backend, out_dir):
    ctx = mp.spawn(_worker, args=(world, _free_port(), backend, out_dir), nprocs=world, join=False)
    deadline = time.monotonic() + JOIN_LIMIT_S
    try:
        while not ctx.join(timeout=max(0.0, deadline - time.monotonic())):
            if time.monotonic() >= deadline:
                raise AssertionError(f"the workers did not end within {JOIN_LIMIT_S} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join()


def _check(world, out_dir):
    import flooder_amd as fa

    dev = torch.device("cuda:0")
    pts, lms = _inputs()
    pts, lms = pts.to(dev), lms.to(dev)
    got = [pickle.load(open(os.path.join(out_dir, f"r{r}.pkl"), "rb")) for r in range(world)]
    for n, (stat, kw) in enumerate(RUNS):
        torch.manual_seed(5)
        want = fa.flood_complex(pts, lms, neighbors=8, neighbor_stat=stat, **kw)
        for r in range(world):
            assert got[r][n] == want, (n, r)
    enough = fa.flood_complex(pts[:20].contiguous(), lms, neighbors=20, points_per_edge=5)
    for r in range(world):
        assert got[r]["merges"] >= len(RUNS)
        assert "neighbors=21 exceeds the number of points (20)" in got[r]["too_many"], got[r]["too_many"]
        assert got[r]["just_enough"] == enough


def test_rccl_world_size_one_gathers_on_the_device(tmp_path):
    assert torch.cuda.is_available()
    _spawn(1, "nccl", str(tmp_path))
    _check(1, str(tmp_path))


def test_two_ranks_one_gpu_gloo_gather_through_pinned_memory(tmp_path):
    assert torch.cuda.is_available()
    _spawn(2, "gloo", str(tmp_path))
    _check(2, str(tmp_path))
