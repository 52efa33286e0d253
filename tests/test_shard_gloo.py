"""Multi-rank path on CPU (world size 2).

* SPMD: two gloo processes call `shard.solve_batch_distributed` on a ragged batch; the solver is a
  stand-in (the oracle, test infrastructure) because there is no GPU here - partitioning, gather and
  row order are what is covered.  The same entry point with the REAL HIP solver runs under `-m gpu`
  (tests/test_gpu_sharded.py).
* single controller: `ShardedSolver` with two worker processes, shards through shared memory, the
  several-solves-per-geometry form (`sections=`) of the dataset path (reference data.py:107-114).
"""
import os
import socket

import numpy as np
import torch.multiprocessing as mp

from tests import helpers as H


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, names, out_dir):
    import torch.distributed as dist
    from python_stable_3d_truss_analysis_amd import batch, shard
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    packed = batch.pack_json([H.load_json(n) for n in names])
    # the stand-in for the HIP pipeline is patched in HERE, in the test process of this rank
    shard._solve_shard = lambda mine, device, reorder, *a, **k: H.oracle_batch_solver(mine)
    full = shard.solve_batch_distributed(packed, device="cpu")
    dist.barrier()
    np.savez(os.path.join(out_dir, f"full{rank}.npz"), u=full.displace, f=full.external, n=full.internal,
             info=full.info)
    dist.destroy_process_group()


def test_two_rank_shard_and_gather(tmp_path):
    from python_stable_3d_truss_analysis_amd import batch, shard
    names = H.data_case_names()[:8]           # ragged: 2D and 3D, 5 .. 111 free DOFs
    packed = batch.pack_json([H.load_json(n) for n in names])
    parts = shard.shard_indices(packed.n_free.astype(float) ** 3, 2)
    assert sorted(np.concatenate(parts).tolist()) == list(range(packed.B))
    assert abs(len(parts[0]) - len(parts[1])) <= 1
    big = int(np.argmax(packed.n_free))        # the two most expensive trusses land on different ranks
    second = int(np.argsort(-packed.n_free)[1])
    assert (big in parts[0]) != (second in parts[0])
    mp.spawn(_worker, args=(2, _free_port(), names, str(tmp_path)), nprocs=2, join=True)
    single = H.oracle_batch_solver(packed)
    for rank in range(2):                      # the gathered result is complete on every rank
        z = np.load(tmp_path / f"full{rank}.npz")
        np.testing.assert_array_equal(z["u"], single.displace)
        np.testing.assert_array_equal(z["f"], single.external)
        np.testing.assert_array_equal(z["n"], single.internal)
        assert not z["info"].any()


def test_sharded_solver_pool_two_workers():
    import dataclasses
    from python_stable_3d_truss_analysis_amd import batch, shard
    names = [n for n in H.data_case_names() if "942" not in n]
    packed = batch.pack_json([H.load_json(n) for n in names])
    with H.sharded_solver_class(H.oracle_worker_main)(["cpu", "cpu"]) as pool:
        assert pool.world_size == 2
        one = pool.solve(packed)
        two = pool.solve(packed, sections=[None, (1.0, 1e7, 0.1)])
        again = pool.solve(packed.take(np.arange(3)))   # the pool outlives a batch; smaller than world*2
    single = H.oracle_batch_solver(packed)
    np.testing.assert_array_equal(one.displace, single.displace)
    np.testing.assert_array_equal(one.internal, single.internal)
    np.testing.assert_array_equal(two[0].external, single.external)
    ones = np.ones_like(packed.A)
    fixed = H.oracle_batch_solver(dataclasses.replace(packed, A=ones, E=ones * 1e7, rho=ones * 0.1))
    np.testing.assert_array_equal(two[1].displace, fixed.displace)
    np.testing.assert_array_equal(two[1].internal, fixed.internal)
    np.testing.assert_array_equal(again.displace, single.displace[:3])
    assert not os.path.exists("/dev/shm") or not [f for f in os.listdir("/dev/shm") if f.startswith("psm_")]


def test_sharded_solver_reports_worker_errors():
    import pytest
    from python_stable_3d_truss_analysis_amd import batch, shard
    from python_stable_3d_truss_analysis_amd.utils import HipExtensionError
    packed = batch.pack_json([H.load_json("bar-6_input_0")])
    with H.sharded_solver_class(H.failing_worker_main)(["cpu"]) as pool:
        with pytest.raises(HipExtensionError, match="stand-in failure"):
            pool.solve(packed)


def test_eight_workers_share_the_host_cpus():
    """Eight workers (one per GPU of a node) together never start more OpenMP threads than the container has
    CPUs (one each when it has fewer than eight): `generate.host_thread_budget`."""
    from python_stable_3d_truss_analysis_amd import generate as gen
    cpus = gen.available_cpus()
    assert gen.host_thread_budget(1) == cpus and gen.host_thread_budget(8) == max(1, cpus // 8)
    assert gen.host_thread_budget(10 ** 6) == 1
    if "OMP_NUM_THREADS" in os.environ:
        return
    with H.sharded_solver_class(H.oracle_worker_main)(["cpu"] * 8) as pool:
        teams = pool.host_threads()
    assert len(teams) == 8 and all(t == max(1, cpus // 8) for t in teams), teams
    assert sum(teams) <= max(cpus, 8)


def test_rank_of_a_launch_takes_its_share(monkeypatch):
    """Under `torchrun` (LOCAL_WORLD_SIZE ranks on this host) a rank's default budget is its share."""
    from python_stable_3d_truss_analysis_amd import _hostapi, generate as gen
    monkeypatch.setattr(_hostapi, "_thread_share", None)   # (the budget's state lives with the host library's loader)
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "4")
    assert gen.host_thread_budget() == max(1, gen.available_cpus() // 4)
    monkeypatch.delenv("LOCAL_WORLD_SIZE")
    assert gen.host_thread_budget() == gen.available_cpus()


def _gather_worker(rank, world, port, total, nJ, nM, same_host, out_dir):
    import time
    import torch.distributed as dist
    from python_stable_3d_truss_analysis_amd import batch, shard
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if same_host is False:
        shard._same_host = lambda group: False       # the several-hosts path: contiguous tensors, no objects
    elif same_host == "full":
        shard._shm_files = lambda shapes, headroom=0: None   # /dev/shm without room: rank 0 says so, ALL fall back
    idx = np.arange(rank, total, world)
    if same_host == "empty" and rank == 1:
        idx = idx[:0]                                # a rank with an empty shard (fewer trusses than ranks)
        shard._same_host = lambda group: False
    elif same_host == "empty":
        idx = np.arange(total)
        shard._same_host = lambda group: False
    rng = np.random.default_rng(rank)
    # ragged widths per rank, as the shards of a real batch have them
    local = batch.BatchResult(rng.random([len(idx), nJ - rank, 3]), rng.random([len(idx), nJ - rank, 3]),
                              rng.random([len(idx), nM - 2 * rank]), (idx % 7 == 0).astype(np.int32))
    dist.barrier()
    t0 = time.perf_counter()
    full = shard.gather_results(local, idx, total, widths=(nJ, nM))
    dt = time.perf_counter() - t0
    ok = True
    for r in range(world):                       # every rank sees every rank's rows, padding zero
        ridx = np.arange(r, total, world)
        if same_host == "empty":
            ridx = np.arange(total) if r == 0 else np.arange(0)
        g = np.random.default_rng(r)
        u, f, n = g.random([len(ridx), nJ - r, 3]), g.random([len(ridx), nJ - r, 3]), g.random([len(ridx), nM - 2 * r])
        ok &= np.array_equal(full.displace[ridx, :nJ - r], u) and not full.displace[ridx, nJ - r:].any()
        ok &= np.array_equal(full.external[ridx, :nJ - r], f) and np.array_equal(full.internal[ridx, :nM - 2 * r], n)
        ok &= not full.internal[ridx, nM - 2 * r:].any() and np.array_equal(full.info[ridx], (ridx % 7 == 0).astype(np.int32))
    dist.barrier()
    # an in-place edit on one rank stays on that rank (the shared-memory path maps the files copy-on-write)
    if rank == 0 and total:
        full.displace[0, 0, 0] = -123.0
    dist.barrier()
    if rank == 1 and total:
        ok &= full.displace[0, 0, 0] != -123.0
    dist.barrier()
    with open(os.path.join(out_dir, f"g{rank}.txt"), "w") as fh:
        fh.write(f"{int(ok)} {dt}\n")
    dist.destroy_process_group()


def test_gather_results_through_shared_memory_and_as_tensors(tmp_path):
    """`gather_results` ships no Python objects: ranks of one host write their rows into memory-mapped files
    that are unlinked before the call returns (a quarter of config 3's result set here: 0.55 GB, well under a
    second), ranks of several hosts gather one contiguous tensor each."""
    # (True: memory-mapped files; False: several hosts; "full": one host whose /dev/shm has no room - decided by rank 0
    # for everybody; "empty": a rank without a single truss on the tensor path)
    for same_host, total in ((True, 16384), (False, 512), ("full", 512), ("empty", 64)):
        mp.spawn(_gather_worker, args=(2, _free_port(), total, 343, 2100, same_host, str(tmp_path)), nprocs=2, join=True)
        for rank in range(2):
            ok, dt = open(tmp_path / f"g{rank}.txt").read().split()
            assert ok == "1"
            if same_host is True:
                assert float(dt) < 6.0, f"gather of 0.55 GB took {dt} s"   # (0.3 s on a quiet box; page reclaim of a busy container can cost seconds)
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("trs_gather_")]


def _timing_group_worker(rank, world, port, out_dir, pretend_gpus):
    import json
    import torch
    import torch.distributed as dist
    import bench
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["TRS_BENCH_NO_RCCL_RANK"] = "1"          # rank 1 declines RCCL; rank 0 would be willing
    dist.init_process_group("gloo", rank=rank, world_size=world)
    name, group = bench.choose_timing_group(dist, torch, torch.device("cpu"), rank, world, pretend_gpus)
    # the chosen group works: barrier + the max of the elapsed times, as bench.py uses it
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    dist.barrier()
    with open(os.path.join(out_dir, f"tg{rank}.json"), "w") as fh:
        json.dump({"name": name, "default_group": group is None, "max": float(t.item())}, fh)
    dist.destroy_process_group()


def test_timing_group_is_chosen_collectively(tmp_path):
    """`bench.choose_timing_group`: one rank that cannot / will not use RCCL takes EVERY rank to
    gloo - decided over the gloo control plane before anybody enters an RCCL call, so no rank is left waiting in a
    collective the other never joins.  Two ranks on CPU, both pretending to own a GPU; rank 1 declines."""
    import json
    mp.spawn(_timing_group_worker, args=(2, _free_port(), str(tmp_path), 2), nprocs=2, join=True)
    for rank in range(2):
        with open(tmp_path / f"tg{rank}.json") as fh:
            rec = json.load(fh)
        assert rec == {"name": "gloo", "default_group": True, "max": 2.0}
