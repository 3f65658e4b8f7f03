"""Measure batched SST point lookups (lsmblk_sst_open_batch / lsmblk_sst_get_batch) on the GPU.

Workload (defaults): 16 SSTs of 64 MiB at block_size 4096 -- 1 GiB of files, past the Infinity Cache --
written on the device (encode_sst + sst_files), 1 Mi uniformly random lookups, half present keys and
half absent keys inside the SSTs' ranges.  Reported, one JSON line each, to stdout and OUT:

  open        ms per lsmblk_sst_open_batch call, and per SST
  get         lookups/s of the default mode, of no_filter, and of the default mode with the value gather
  kernels     per-kernel ms (LSMBLK_DEBUG_KERNEL_TIMING / lsmblk_ctx_kernel_log), in a pass of its own
  baseline    the composition that existed before these calls, on the first 64 Ki of the same lookups:
              host SsTable.may_contain + find_block_idx per lookup, then batch.seek_blocks; and
              batch.seek_blocks alone with the block indices precomputed (its seek_kernel time from the
              kernel log isolates the old kernel); its landings are compared with no_filter's

Every timed figure: 2 warm-up runs, then RUNS runs between device events; median, min and max.  Every
GPU step runs under its own time limit (SIGALRM ends the process).
usage: python tools/get_probe.py [OUT_JSON] [--ssts N] [--sst-mib M] [--queries Q] [--base-queries B] [--runs R]
"""
import argparse
import ctypes
import json
import os
import signal
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lsm_amd import batch, sst  # noqa: E402
from lsm_amd._build import src_sha  # noqa: E402
from lsm_amd._lib import LSMBLK_GET_NO_FILTER, GetResultC, kernel_timing  # noqa: E402

KLEN, VLEN, ENTRY = 16, 100, 4 + 10 + 8 + 2 + 100 + 2  # ~ bytes per entry in a block (6 key bytes shared)
LINES = []


def step(name, seconds):
    """The time limit of the GPU step that starts here."""
    signal.alarm(seconds)
    print(f"# {name} (limit {seconds} s)", file=sys.stderr, flush=True)


def emit(**kw):
    LINES.append(kw)
    print(json.dumps(kw), flush=True)


def key_bytes(ids):
    """16-byte keys: the id as a big-endian u64, then 8 bytes derived from it."""
    k = np.empty((len(ids), KLEN), np.uint8)
    k[:, :8] = ids.astype(">u8").view(np.uint8).reshape(-1, 8)
    k[:, 8:] = (ids * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(-1, 8)
    return k


def spread(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), runs=len(ms))


def timed(fn, runs):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "get_probe.json"))
    ap.add_argument("--ssts", type=int, default=16)
    ap.add_argument("--sst-mib", type=int, default=64)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--base-queries", type=int, default=1 << 16)
    ap.add_argument("--runs", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("get_probe needs a ROCm device")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(1)
    per = (a.sst_mib << 20) // ENTRY
    n = per * a.ssts

    step("write the SST files on the device", 300)
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)  # present keys: even ids; SST s = ids [2 s per, 2 (s + 1) per)
    keys = key_bytes(ids).reshape(-1)
    vals = rng.integers(0, 256, n * VLEN, dtype=np.uint8)
    kv = batch.KVStream.from_numpy(keys, np.arange(n + 1, dtype=np.uint64) * KLEN, vals,
                                   np.arange(n + 1, dtype=np.uint64) * VLEN, np.full(n, 7, np.uint64), device=dev)
    seg = (np.arange(a.ssts + 1, dtype=np.uint64) * per).astype(np.uint32)
    r = batch.encode_sst(kv, seg, 4096)
    files, file_off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, kv)
    del r, kv, keys, vals
    torch.cuda.empty_cache()

    step("open", 120)
    ss = sst.SstSet(files, file_off)
    assert not ss.err.any(), ss.err
    cap = len(ss.index)
    open_ms = timed(lambda: ss._open(cap), a.runs)  # (each call ends in a synchronize)
    emit(what="open", ssts=a.ssts, sst_mib=a.sst_mib, file_bytes=int(files.numel()), blocks=cap, entries=n,
         per_sst_ms=round(sorted(open_ms)[len(open_ms) // 2] / a.ssts, 4), **spread(open_ms))

    nq = a.queries
    q_sst = rng.integers(0, a.ssts, nq).astype(np.uint64)
    qid = (q_sst * np.uint64(per) + rng.integers(0, per, nq).astype(np.uint64)) * np.uint64(2)
    qid += (rng.random(nq) < 0.5).astype(np.uint64)  # odd ids: absent, inside the SST's range
    qk = torch.from_numpy(key_bytes(qid).reshape(-1)).to(dev)
    qo = batch._u32_table(np.arange(nq + 1, dtype=np.uint64) * KLEN, dev)
    qs = batch._u32_table(q_sst, dev)
    qt = torch.full((nq,), 1 << 40, dtype=torch.int64, device=dev)
    res = torch.zeros(nq * ctypes.sizeof(GetResultC), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    vo = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
    vbuf = batch._aligned_empty(nq * VLEN, dev)

    def run(flags, gather=False):
        ss.get_into(qs, qk, qo, qt, nq, flags, res, stats, vbuf if gather else None, nq * VLEN, vo if gather else None)

    for name, flags, gather in (("default", 0, False), ("no_filter", LSMBLK_GET_NO_FILTER, False),
                                ("default+values", 0, True)):
        step("get " + name, 120)
        ms = timed(lambda: run(flags, gather), a.runs)
        st = stats.cpu().tolist()
        assert st[3] == 0, st
        med = sorted(ms)[len(ms) // 2]
        emit(what="get", mode=name, lookups=nq, found=st[1], value_bytes=st[2],
             mlookups_per_s=round(nq / med / 1e3, 2), **spread(ms))
    run(LSMBLK_GET_NO_FILTER)
    torch.cuda.synchronize()
    nof = res.cpu().numpy().view(np.dtype(GetResultC))[:nq].copy()

    step("per-kernel times", 120)
    ctx = batch._ctx(dev.index)
    with kernel_timing(ctx) as kl:
        for _ in range(3):
            ss._open(cap)
            run(0, True)
            run(LSMBLK_GET_NO_FILTER)
    emit(what="kernels", note="ms per launch; sst_get_kernel averages one default and one no_filter launch",
         **{k: round(ms / ln, 4) for k, (ln, ms) in kl.items()})

    # ---- the composition that existed before: host filters and block search, then lsmblk_seek_batch
    nb = min(a.base_queries, nq)
    step("baseline: host SsTable objects", 600)
    host = files.cpu().numpy()
    fo = file_off.cpu().tolist()
    t0 = time.perf_counter()
    tabs = [sst.SsTable(host[fo[s]:fo[s + 1]].tobytes()) for s in range(a.ssts)]
    emit(what="baseline_open", note="host SsTable.__init__ of every SST", ms=round((time.perf_counter() - t0) * 1e3, 1))
    # one offset table for lsmblk_seek_batch over the whole buffer: per SST its block offsets and its
    # meta_offset (the range between two SSTs' tables is a block nobody seeks)
    offs, base = [], [0]
    for s, t in enumerate(tabs):
        o = t.block_offsets().astype(np.int64) + fo[s]
        offs.append(o)
        base.append(base[-1] + len(o))
    blk_off = torch.from_numpy(np.concatenate(offs + [np.array([fo[-1]], np.int64)])).to(dev)
    bkeys = [bytes(x) for x in key_bytes(qid[:nb])]
    bs = q_sst[:nb].astype(np.int64)
    step("baseline: host filter + block search, then seek_blocks", 600)
    t0 = time.perf_counter()
    cand = [i for i in range(nb) if tabs[bs[i]].first_key <= bkeys[i] <= tabs[bs[i]].last_key and tabs[bs[i]].may_contain(bkeys[i])]
    qb = [base[bs[i]] + tabs[bs[i]].find_block_idx(bkeys[i]) for i in cand]
    t1 = time.perf_counter()
    batch.seek_blocks(files, blk_off, qb, [bkeys[i] for i in cand], tail=4)
    t2 = time.perf_counter()
    emit(what="baseline", mode="default", lookups=nb, candidates=len(cand), host_ms=round((t1 - t0) * 1e3, 1),
         seek_blocks_ms=round((t2 - t1) * 1e3, 1), mlookups_per_s=round(nb / (t2 - t0) / 1e6, 4))
    step("baseline: seek_blocks alone", 300)
    qb_all = [base[bs[i]] + tabs[bs[i]].find_block_idx(bkeys[i]) for i in range(nb)]
    walls = []
    with kernel_timing(ctx) as kl:
        for _ in range(5):
            t0 = time.perf_counter()
            idx = batch.seek_blocks(files, blk_off, qb_all, bkeys, tail=4)
            walls.append((time.perf_counter() - t0) * 1e3)
    seek_ms = kl["seek_kernel"][1] / kl["seek_kernel"][0]
    # the same lookups through the new kernel, timed the same way (kernel log)
    sub = lambda t, k: t[:k].contiguous()
    with kernel_timing(ctx) as kl:
        for _ in range(5):
            ss.get_into(sub(qs, nb), qk, sub(qo, nb + 1), sub(qt, nb), nb, LSMBLK_GET_NO_FILTER, res, stats)
    get_ms = kl["sst_get_kernel"][1] / kl["sst_get_kernel"][0]
    # landings: seek_blocks' entry index (+ the spill) against no_filter's (blk, ent)
    bad = 0
    for i in range(nb):
        b = qb_all[i] - base[bs[i]]
        e = int(idx[i])
        gb, ge = int(nof["blk"][i]), int(nof["ent"][i])
        if (gb, ge) != (b, e) and not (ge == 0 and gb == b + 1):
            bad += 1
    emit(what="baseline", mode="seek_blocks alone (block indices precomputed on the host)", lookups=nb,
         wall_ms_median=round(sorted(walls)[2], 2), seek_kernel_ms=round(seek_ms, 4),
         sst_get_kernel_no_filter_ms=round(get_ms, 4), seek_kernel_mlookups_per_s=round(nb / seek_ms / 1e3, 2),
         sst_get_kernel_mlookups_per_s=round(nb / get_ms / 1e3, 2), landing_mismatches=bad)
    signal.alarm(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"src_sha256": src_sha(), "device": torch.cuda.get_device_name(dev), "lines": LINES}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
