"""Multi-process (gloo, world_size 2, CPU) tests of the sharding helpers used for N>1."""
import os
import socket

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from lsm_amd import shard


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # block-parallel: timing max-reduce
        t = shard.max_over_ranks(1.0 + rank)
        # compaction-shaped: each rank holds an overlapping sorted run of block first keys
        first_keys = [b"key%06d" % i for i in range(rank * 500, rank * 500 + 1500, 3)]
        spl = shard.exchange_splitters(first_keys, samples=32)
        q.put((rank, t, spl))
    finally:
        dist.destroy_process_group()


def test_block_ranges_cover():
    for n in (0, 1, 7, 1 << 20):
        for w in (1, 2, 3, 8):
            r = shard.block_ranges(n, w)
            assert r[0][0] == 0 and r[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
            assert max(h - l for l, h in r) - min(h - l for l, h in r) <= 1


def test_choose_splitters_and_owner():
    keys = [b"%04d" % i for i in range(100)]
    spl = shard.choose_splitters(keys, 4)
    assert spl == [b"0025", b"0050", b"0075"]
    assert [shard.owner_of(k, spl) for k in (b"0000", b"0025", b"0049", b"0099")] == [0, 1, 1, 3]


@pytest.mark.timeout(120)
def test_gloo_world2_exchange():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=100) for _ in range(2))
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    (r0, t0, s0), (r1, t1, s1) = res
    assert t0 == t1 == 2.0
    assert s0 == s1 and len(s0) == 1
    # the splitter lies inside the union of both runs
    assert b"key000000" < s0[0] < b"key002000"


@pytest.mark.timeout(180)
@pytest.mark.parametrize("world", [2, 4])
def test_bench_launcher_starts_world_ranks(world):
    """`bench.py --gpus N` without torchrun starts N rank processes itself (the parent touches no
    GPU); in --dry-run every rank joins one gloo group and rank 0 reports what it saw."""
    _dry_run(world)


def _dry_run(world):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--dry-run"],
                       capture_output=True, text=True, timeout=170, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == world and line["collective_world"] == world
    assert line["rank_mask"] == (1 << world) - 1
    return line


@pytest.mark.timeout(240)
def test_bench_default_c_extra_at_8_gpus_is_configs4_shape():
    """At N = 8 the default --full run's compaction extra is SURVEY.md section 8(d) config 5: 3 key ranges
    of 1 Mi input blocks per GPU, 12.7 GB of L0 input per GPU, ~100 GB on 8 (VERDICT round 4,
    missing item 3) -- shown by the launcher's dry run, 8 gloo ranks (no GPU)."""
    line = _dry_run(8)
    plan = line["c_extra_plan"]
    assert plan["ranges_per_gpu"] == 3 and plan["input_blocks_per_gpu"] == 3 << 20
    assert 12.0 < plan["input_gb_per_gpu"] < 13.0 and 95 < plan["total_input_gb"] < 105


def test_bench_refuses_world_mismatch():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and r.stdout == ""


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world,fail", [(2, 1), (3, 0)])
def test_bench_launcher_fails_fast_when_a_rank_dies(world, fail):
    """One rank exits early (before joining the gloo group, so the others block in the
    rendezvous): the launcher terminates the rest and returns non-zero within seconds, printing
    no bench line."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--dry-run",
                        "--dry-run-fail-rank", str(fail)], capture_output=True, text=True, timeout=100, env=env)
    dt = time.time() - t0
    assert r.returncode != 0 and r.stdout.strip() == "", (r.returncode, r.stdout)
    assert f"rank {fail} exited with status 3" in r.stderr
    assert dt < 60, dt


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world,fail", [(2, 1), (3, 0)])
def test_bench_extra_failure_inside_compact_dist_ends_the_job(world, fail):
    """A rank that raises inside shard.compact_dist during the N>1 extra config exits at once
    (extra_or_exit) while its peers block in the head all-gather: the launcher tears the job down
    and returns non-zero within seconds, printing no bench line."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--dry-run",
                        "--dry-run-fail-extra", str(fail)], capture_output=True, text=True, timeout=100, env=env)
    dt = time.time() - t0
    assert r.returncode != 0 and r.stdout.strip() == "", (r.returncode, r.stdout)
    assert f"[rank {fail}] extra config C failed" in r.stderr and "merge failed as asked" in r.stderr
    assert f"rank {fail} exited with status 1" in r.stderr
    assert dt < 60, dt
