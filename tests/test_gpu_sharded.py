"""Multi-process / multi-GPU path with the REAL HIP solver, `-m gpu`.

World size 2 everywhere: on a box with one GPU both ranks share cuda:0 (the processes, shards,
shared-memory transport and gathers are the same as with one GPU per rank), on a box with more GPUs
rank r takes cuda:r.  Sharded results are compared BITWISE with the single-process result: a truss's
arithmetic does not depend on which batch or bucket it travels in.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _devices(n=2):
    import torch
    ndev = torch.cuda.device_count()
    assert ndev >= 1
    return [f"cuda:{i % ndev}" for i in range(n)]


def _ragged_batch():
    from python_stable_3d_truss_analysis_amd import batch
    datas = [H.load_json(n) for n in H.data_case_names()]
    datas += [d for _, d, _ in H.ragged_cube_cases()]
    return batch.pack_json(datas)


def _assert_same(a, b):
    np.testing.assert_array_equal(a.displace, b.displace)
    np.testing.assert_array_equal(a.external, b.external)
    np.testing.assert_array_equal(a.internal, b.internal)
    np.testing.assert_array_equal(a.info, b.info)


def test_sharded_solver_matches_single_process_bitwise():
    from python_stable_3d_truss_analysis_amd import batch, shard
    packed = _ragged_batch()
    single = batch.solve_batch(packed)
    single_two = batch.solve_batch(packed, sections=[None, (1.0, 1e7, 0.1)], reorder=True)
    with shard.ShardedSolver(_devices()) as pool:
        _assert_same(pool.solve(packed), single)
        both = pool.solve(packed, reorder=True, sections=[None, (1.0, 1e7, 0.1)])
    assert not single.info.any()
    for got, want in zip(both, single_two):
        _assert_same(got, want)
    # reordering changes the summation order, not the answer
    assert H.max_scaled_err(single_two[0].displace, single.displace) < 1e-8


def _spmd_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from python_stable_3d_truss_analysis_amd import shard
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["LOCAL_RANK"] = str(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = shard.solve_batch_distributed(_ragged_batch())   # real HIP solver on cuda:(rank % ndev)
    dist.barrier()
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), u=full.displace, f=full.external, n=full.internal,
             info=full.info)
    dist.destroy_process_group()


def test_spmd_two_ranks_real_solver(tmp_path):
    import torch.multiprocessing as mp
    from python_stable_3d_truss_analysis_amd import batch
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_spmd_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    single = batch.solve_batch(_ragged_batch())
    for rank in range(2):
        z = np.load(tmp_path / f"r{rank}.npz")
        np.testing.assert_array_equal(z["u"], single.displace)
        np.testing.assert_array_equal(z["f"], single.external)
        np.testing.assert_array_equal(z["n"], single.internal)
        assert not z["info"].any()


@pytest.mark.timeout(700)
def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it starts two ranks itself and rank 0 prints
    the one JSON line (n_gpus = the devices really used: 2 on a multi-GPU box, 1 when shared)."""
    import torch
    ndev = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "256", "--no-cpu-baseline", "--no-pcie", "--cube-batch", "384", "--cube-steps", "2",
           "--dataset-samples", "512", "--no-dense-ref", "--cube-total", "600", "--dataset-total", "700", "--full"]
    if ndev < 2:
        cmd.append("--oversubscribe")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["ranks"] == 2 and line["n_gpus"] == min(2, ndev)
    assert line["info_nonzero"] == 0 and line["value"] > 0
    assert line["scaling"] == "weak" and line["config"]["batch_per_gpu"] == 256
    # the ragged cube-truss leg (BASELINE config 3) runs on every rank too: whole-job rate, roofline fractions
    cube = line["cube_batch"]
    assert "error" not in cube, cube
    assert cube["batch_per_gpu"] == 384 and cube["info_nonzero"] == 0 and cube["value"] > 0
    assert 0 < cube["roofline"]["hbm"]["frac"] < 1 and 0 < cube["roofline"]["mfma"]["frac"] < 1
    assert set(cube["stages_ms"]) >= {"order", "solve"}   # (gather / scatter launches only for the small-system bucket)
    assert line["dataset"]["value"] > 0 and line["dataset"]["info_nonzero_rank0"] == 0
    assert line["dataset"]["rank0_samples"] == 512
    assert line["timing_group"] in ("nccl", "gloo")
    _check_scaling_record(line, ranks=2, batch=256, cube_total=600, dataset_total=700)


@pytest.mark.timeout(500)
def test_bench_two_ranks_one_declines_rccl():
    """The RCCL-failure branch of the timing group: rank 1 is made to decline RCCL
    (`TRS_BENCH_NO_RCCL_RANK=1`); both ranks must end up on gloo - chosen collectively, nobody waits in an RCCL
    collective - and the run must finish with its one line."""
    import torch
    ndev = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["TRS_BENCH_NO_RCCL_RANK"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "128", "--no-cpu-baseline", "--no-pcie", "--cube-batch", "0", "--dataset-samples", "0",
           "--no-dense-ref", "--cube-total", "0", "--dataset-total", "0"]
    if ndev < 2:
        cmd.append("--oversubscribe")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["ranks"] == 2 and line["timing_group"] == "gloo" and line["value"] > 0 and line["info_nonzero"] == 0


@pytest.mark.timeout(1000)
def test_bench_eight_ranks_smoke():
    """What the driver's scaling run does at N = 8, made boring beforehand: `bench.py --gpus 8` (ranks sharing the
    box's GPU(s) where there are fewer than eight: --oversubscribe) with tiny workloads - eight processes come up,
    rendezvous, run every leg, and rank 0 prints ONE JSON line; every rank's native host helpers are limited to its
    share of the host CPUs."""
    import torch
    from python_stable_3d_truss_analysis_amd.generate import available_cpus
    ndev = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
           "--batch", "128", "--no-cpu-baseline", "--no-pcie", "--cube-batch", "256", "--cube-steps", "1",
           "--dataset-samples", "256", "--no-dense-ref", "--cube-total", "2000", "--dataset-total", "3000", "--full"]
    if ndev < 8:
        cmd.append("--oversubscribe")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["ranks"] == 8 and line["n_gpus"] == min(8, ndev)
    assert line["info_nonzero"] == 0 and line["value"] > 0
    assert line["rank_ms_per_step"]["min"] <= line["rank_ms_per_step"]["max"]
    # (its share of the CPUs at most; torchrun's OMP_NUM_THREADS=1 for multi-process jobs wins where it is set, and an
    # OMP_NUM_THREADS of the caller's environment wins over both in every rank: generate.set_host_thread_share)
    omp = os.environ.get("OMP_NUM_THREADS")
    if omp:
        assert line["host_threads_per_rank"] == int(omp)
    else:
        assert 1 <= line["host_threads_per_rank"] <= max(1, available_cpus() // 8)
    cube = line["cube_batch"]
    assert "error" not in cube and cube["info_nonzero"] == 0 and cube["batch_per_gpu"] == 256
    assert cube["value"] > 0 and cube["rank_ms_per_step"]["min"] <= cube["rank_ms_per_step"]["max"]
    assert line["dataset"]["value"] > 0 and line["dataset"]["rank0_samples"] == 256
    _check_scaling_record(line, ranks=8, batch=128, cube_total=2000, dataset_total=3000)


def _check_scaling_record(line, ranks, batch, cube_total, dataset_total):
    """`north_star_scaling` of a bench line: the three per-N entries north_star asks for are present - config 2
    weak-scaled, config 3 and config 5 strong-scaled - each with the spread over the ranks, and the shards of the two
    strong-scaled entries, keyed by GLOBAL index, are disjoint, cover the whole dataset and hold the trusses a single
    process generates for those indices (joint / member totals of the regenerated dataset)."""
    import torch
    import bench
    from python_stable_3d_truss_analysis_amd import generate as gen
    from python_stable_3d_truss_analysis_amd.data import dataset_sizes
    rec = line["north_star_scaling"]
    assert rec["ranks"] == ranks and set(rec) >= {"config2_weak", "config3_strong", "config5_strong"}
    c2, c3, c5 = rec["config2_weak"], rec["config3_strong"], rec["config5_strong"]
    assert c2["scaling"] == "weak" and c2["value"] == line["value"] > 0
    assert c2["rank_ms_per_step"]["min"] <= c2["rank_ms_per_step"]["max"]
    # config 3: contiguous global-index shards
    assert c3["scaling"] == "strong" and c3["total_trusses"] == cube_total and c3["value"] > 0 and c3["info_nonzero"] == 0
    assert c3["rank_ms_per_step"]["min"] <= c3["rank_ms_per_step"]["max"]
    assert [sh["rank"] for sh in c3["shards"]] == list(range(ranks))
    covered = sorted((sh["first"], sh["first"] + sh["count"]) for sh in c3["shards"] if sh["count"])
    assert covered[0][0] == 0 and covered[-1][1] == cube_total
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    whole, _ = bench.cube_workload(cube_total, 0, device="cuda:0", first=0)
    assert sum(sh["members"] for sh in c3["shards"]) == int(whole.nM.astype(np.int64).sum())
    assert sum(sh["joints"] for sh in c3["shards"]) == int(whole.nJ.astype(np.int64).sum())
    # config 5: rank r owns the chunks r, r + ranks, ... of the globally indexed dataset
    assert c5["scaling"] == "strong" and c5["total_samples"] == dataset_total and c5["value"] > 0
    assert c5["info_nonzero"] == 0 and c5["solves_per_sample"] == 2
    assert c5["rank_seconds"]["min"] <= c5["rank_seconds"]["max"]
    spans = sorted((first, first + count) for sh in c5["shards"] for first, count in sh["chunks"])
    assert spans[0][0] == 0 and spans[-1][1] == dataset_total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert sum(sh["samples"] for sh in c5["shards"]) == dataset_total
    sizes = dataset_sizes(11, 0, dataset_total, (8, 190))
    whole, _ = gen.generate_cube_batch_device(sizes, gridRange=(6, 6, 6), seed=11, first_index=0, device="cuda:0")
    assert sum(sh["joints"] for sh in c5["shards"]) == int(whole.nJ.astype(np.int64).sum())
    torch.cuda.empty_cache()


def test_ga_population_sharded_over_two_workers():
    """Config 4 in its sharded form: the population split over two workers gives the same fitness
    triples as the single-device evaluation."""
    import random
    from python_stable_3d_truss_analysis_amd import Truss, MemberType
    from python_stable_3d_truss_analysis_amd.ga import GA
    truss = Truss(3).LoadFromJSON(data=H.load_json("bar-120_input_0"))
    types = [MemberType(0.5 + 0.5 * i, 1e7, 0.1) for i in range(6)]
    random.seed(3)
    one = GA(truss.Copy(), types, nPop=64, nElite=16)
    genes = one.Initialize()
    two = GA(truss.Copy(), types, nPop=64, nElite=16, devices=_devices())
    try:
        a, b = one.GetFitnessBatch(genes), two.GetFitnessBatch(genes)
        b2 = two.GetFitnessBatch(genes[::-1])   # second generation: geometry already resident
    finally:
        two.close()
    assert a == b and b2 == a[::-1]


def test_fitness_without_a_geometry_key_never_reuses_a_resident_batch():
    """Two geometries of the SAME padded shapes through `ShardedSolver.fitness` back to back: without a
    `geometry_key` every call uploads its own batch (round 2 reused the first one's geometry and returned the
    fitness of the wrong trusses); with a key the geometry stays and only the sections change."""
    import dataclasses
    from python_stable_3d_truss_analysis_amd import batch, shard
    base = batch.pack_json([H.load_json("bar-120_input_0")]).replicate(8)
    stretched = dataclasses.replace(base, xyz=base.xyz * 1.5)

    def single(packed):
        dev = batch.DeviceBatch(packed, "cuda:0")
        w, sv, dv = dev.solve_fitness(30000., 10.)
        return np.stack([w.cpu().numpy(), sv.cpu().numpy(), dv.cpu().numpy()], axis=1)

    want_a, want_b = single(base), single(stretched)
    assert not np.array_equal(want_a, want_b)
    with shard.ShardedSolver(_devices()) as pool:
        got_a, _ = pool.fitness(base, 30000., 10.)
        got_b, _ = pool.fitness(stretched, 30000., 10.)
        keyed_a, _ = pool.fitness(base, 30000., 10., geometry_key="a")
        thicker = dataclasses.replace(base, A=base.A * 2.0)
        keyed_a2, _ = pool.fitness(thicker, 30000., 10., geometry_key="a")   # sections only
        keyed_b, _ = pool.fitness(stretched, 30000., 10., geometry_key="b")  # another key: re-uploaded
    np.testing.assert_array_equal(got_a, want_a)
    np.testing.assert_array_equal(got_b, want_b)
    np.testing.assert_array_equal(keyed_a, want_a)
    np.testing.assert_array_equal(keyed_a2, single(thicker))
    np.testing.assert_array_equal(keyed_b, want_b)
