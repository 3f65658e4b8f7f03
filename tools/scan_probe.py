"""Measure batched SST range scans (lsmblk_sst_scan_batch, lsmblk_read_filter_batch) on the GPU.

Workload (defaults): the SST set of get_probe.py -- 16 SSTs of 64 MiB at block_size 4096, 1 GiB of
files written on the device, 16-byte keys, 100-byte values, one version per key -- and three range
batches, each range Included(lower) .. Excluded(upper) inside one SST:

  short    64 Ki ranges of 10 entries
  medium   4 Ki ranges of 1 000 entries
  whole    16 unbounded scans, one whole SST each

Reported per batch, one JSON line each, to stdout and OUT:

  scan        the raw scan into an exactly sized output (the sizing call, out = NULL, timed separately)
  scan+filter the raw scan followed by the read filter over its output (read_ts above every version)
  kernels     per-kernel ms (LSMBLK_DEBUG_KERNEL_TIMING / lsmblk_ctx_kernel_log), in a pass of its own
  baseline    the composition that existed before these calls, on the first BASE ranges of the batch:
              host SsTable.find_block_idx for both ends, SsTable.decode_blocks(lo, hi) (upload of the
              framed blocks, CRC-verified device decode), then a host slice of the KV stream by key
  decode      whole only: lsmblk_decode_batch_ex(tail = 4) of the same 16 data sections, the existing
              device route to those bytes

Every timed device figure: 2 warm-up runs, then RUNS runs between device events; median, min and max.
Every GPU step runs under its own time limit (SIGALRM ends the process).
usage: python tools/scan_probe.py [OUT_JSON] [--ssts N] [--sst-mib M] [--runs R] [--base B]
"""
import argparse
import bisect
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
from lsm_amd._lib import ScanResultC, kernel_timing  # noqa: E402
from tools.get_probe import ENTRY, KLEN, VLEN, key_bytes, spread, timed  # noqa: E402

LINES = []
INCL_EXCL = 1 | (2 << 2)


def step(name, seconds):
    signal.alarm(seconds)
    print(f"# {name} (limit {seconds} s)", file=sys.stderr, flush=True)


def emit(**kw):
    LINES.append(kw)
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "scan_probe.json"))
    ap.add_argument("--ssts", type=int, default=16)
    ap.add_argument("--sst-mib", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--base", type=int, default=256, help="ranges of each batch the host baseline runs")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scan_probe needs a ROCm device")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(2)
    per = (a.sst_mib << 20) // ENTRY
    n = per * a.ssts

    step("write the SST files on the device", 300)
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2)  # SST s = ids [2 s per, 2 (s + 1) per)
    vals = rng.integers(0, 256, n * VLEN, dtype=np.uint8)
    kv = batch.KVStream.from_numpy(key_bytes(ids).reshape(-1), np.arange(n + 1, dtype=np.uint64) * KLEN, vals,
                                   np.arange(n + 1, dtype=np.uint64) * VLEN, np.full(n, 7, np.uint64), device=dev)
    seg = (np.arange(a.ssts + 1, dtype=np.uint64) * per).astype(np.uint32)
    r = batch.encode_sst(kv, seg, 4096)
    files, file_off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, kv)
    del r, kv, vals
    torch.cuda.empty_cache()
    ss = sst.SstSet(files, file_off)
    assert not ss.err.any(), ss.err
    ctx = batch._ctx(dev.index)
    host = files.cpu().numpy()
    fo = file_off.cpu().tolist()
    tabs = {}

    def table(s):
        if s not in tabs:
            tabs[s] = sst.SsTable(host[fo[s]:fo[s + 1]].tobytes(), device=dev)
        return tabs[s]

    def batch_of(name, nq, length):
        """nq ranges of `length` entries: (q_sst, first entry index in the SST, tensors of scan_into)."""
        if length is None:
            q_sst = np.arange(nq, dtype=np.uint64) % np.uint64(a.ssts)
            first = np.zeros(nq, np.uint64)
            z = torch.zeros(16, dtype=torch.uint8, device=dev)
            zo = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
            return q_sst, first, (batch._u32_table(q_sst, dev), z, zo, z, zo, torch.zeros(nq, dtype=torch.int32, device=dev))
        q_sst = rng.integers(0, a.ssts, nq).astype(np.uint64)
        first = rng.integers(0, per - length, nq).astype(np.uint64)
        lo = (q_sst * np.uint64(per) + first) * np.uint64(2)
        off = batch._u32_table(np.arange(nq + 1, dtype=np.uint64) * KLEN, dev)
        lk = torch.from_numpy(key_bytes(lo).reshape(-1)).to(dev)
        uk = torch.from_numpy(key_bytes(lo + np.uint64(2 * length)).reshape(-1)).to(dev)
        return q_sst, first, (batch._u32_table(q_sst, dev), lk, off, uk, off,
                              torch.full((nq,), INCL_EXCL, dtype=torch.int32, device=dev))

    for name, nq, length in (("short", 1 << 16, 10), ("medium", 1 << 12, 1000), ("whole", a.ssts, None)):
        q_sst, first, t = batch_of(name, nq, length)
        res = torch.zeros(nq * ctypes.sizeof(ScanResultC), dtype=torch.uint8, device=dev)
        sseg = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        step(f"{name}: sizing call", 120)
        size_ms = timed(lambda: ss.scan_into(*t, nq, 0, res, sseg, stats), a.runs)
        ne, kb, vb, err = stats.cpu().tolist()
        assert err == 0 and ne == (nq * length if length else n), (ne, err)
        out = batch.KVStream.empty(ne, kb, vb, dev)
        flt = batch.KVStream.empty(ne, kb, vb, dev)
        fseg = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        fts = torch.full((nq,), 1 << 40, dtype=torch.int64, device=dev)
        fstats = torch.zeros(4, dtype=torch.int64, device=dev)
        out.n = ne

        def scan():
            ss.scan_into(*t, nq, 0, res, sseg, stats, out, (ne, kb, vb))

        def scan_filter():
            scan()
            batch.read_filter_into(out, sseg, fts, nq, flt, fseg, fstats, caps=(ne, kb, vb))

        step(f"{name}: scan", 120)
        ms = timed(scan, a.runs)
        assert stats.cpu().tolist() == [ne, kb, vb, 0]
        med = sorted(ms)[len(ms) // 2]
        emit(what="scan", batch=name, ranges=nq, entries=ne, key_bytes=kb, value_bytes=vb,
             out_gib_per_s=round((kb + vb + 16 * ne) / med / 2**30 * 1e3, 1), sizing_call=spread(size_ms), **spread(ms))
        step(f"{name}: scan + read filter", 120)
        ms = timed(scan_filter, a.runs)
        assert fstats.cpu().tolist() == [ne, kb, vb, 0], fstats
        emit(what="scan+filter", batch=name, ranges=nq, kept=ne, **spread(ms))
        step(f"{name}: per-kernel times", 120)
        with kernel_timing(ctx) as kl:
            for _ in range(3):
                scan_filter()
        emit(what="kernels", batch=name, note="ms per launch", **{k: round(ms_ / ln, 4) for k, (ln, ms_) in kl.items()})

        # ---- the parent's composition on the first ranges of the batch
        nb = min(a.base, nq)
        step(f"{name}: baseline (host block search, decode_blocks, host slice)", 900)
        for s in sorted(set(int(x) for x in q_sst[:nb])):
            table(s)  # (opening the tables is not part of the timed composition)
        t0 = time.perf_counter()
        got = 0
        for i in range(nb):
            s, tb = int(q_sst[i]), table(int(q_sst[i]))
            if length is None:
                b0, b1, lo_k, up_k = 0, tb.num_of_blocks() - 1, None, None
            else:
                base_id = (int(q_sst[i]) * per + int(first[i])) * 2
                lo_k, up_k = (bytes(x) for x in key_bytes(np.array([base_id, base_id + 2 * length], np.uint64)))
                b0, b1 = tb.find_block_idx(lo_k), tb.find_block_idx(up_k)
            keys, ko, _, _, _ = tb.decode_blocks(b0, b1 + 1).to_numpy()
            kl = keys.reshape(-1, KLEN).view(f"S{KLEN}").reshape(-1)  # fixed-width keys: a sorted byte-string column
            e0 = 0 if lo_k is None else int(np.searchsorted(kl, np.bytes_(lo_k)))
            e1 = len(kl) if up_k is None else int(np.searchsorted(kl, np.bytes_(up_k)))
            got += e1 - e0
        wall = (time.perf_counter() - t0) * 1e3
        assert got == (nb * length if length else nb * per), got
        emit(what="baseline", batch=name, ranges=nb, wall_ms=round(wall, 1), ms_per_range=round(wall / nb, 3),
             whole_batch_ms_extrapolated=round(wall / nb * nq, 1))
        del out, flt
        torch.cuda.empty_cache()

    # ---- the framed decode of the same data sections (the existing device route to the whole-SST bytes)
    step("whole: lsmblk_decode_batch_ex(tail = 4) of every data section", 300)
    offs = [torch.from_numpy(ss.block_offsets(s).astype(np.int64) + fo[s]).to(dev) for s in range(a.ssts)]
    dout = batch.KVStream.empty(per, per * KLEN, per * VLEN, dev)
    dstats = torch.zeros(4, dtype=torch.int64, device=dev)

    def decode_all():
        for s in range(a.ssts):
            batch.decode_ex_into(files, offs[s], offs[s].numel() - 1, dout, dstats, per, per * KLEN + 16,
                                 per * VLEN + 16, tail=4)

    ms = timed(decode_all, a.runs)
    assert dstats.cpu().tolist()[3] == 0 and dstats.cpu().tolist()[0] == per
    emit(what="decode", batch="whole", note="16 lsmblk_decode_batch_ex(tail=4) calls, one per data section, no CRC check",
         entries=n, **spread(ms))
    signal.alarm(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"src_sha256": src_sha(), "device": torch.cuda.get_device_name(dev), "lines": LINES}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
