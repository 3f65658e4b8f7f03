"""Measure range scans over an LSM view (lsmblk_lsm_scan_batch) against the composition a caller had before.

Workload (defaults): SSTs of 8 MiB at block_size 4096, written on the device, as a view of 4 L0 tables
that each span the whole key space and 3 levels of 4 non-overlapping tables (16 sources, so that the
composition's merge, limited to 64 runs, can run).  Key id = C n + c with C = 7 classes: L0 table c
holds n = 4 m, table j of level l holds class 4 + l, n in [j per, (j + 1) per).  One version per key
(ts 7), values of 100 bytes.  RANGES ranges [Included(key(C n0)), Excluded(key(C (n0 + SPAN)))) at
uniformly random n0, read_ts above every ts.  One JSON line to stdout and OUT:

  lsm_scan     the new call into exactly sized streams: wall ms per batch (call + synchronize), ranges/s,
               output GB/s (keys, values, ts and both offsets of the kept entries), the per-kernel split
               (LSMBLK_DEBUG_KERNEL_TIMING, a pass of its own)
  composition  the parent commit's calls only, same build, same ranges: the host expands every range
               into its tables (first / last ids), ONE lsmblk_sst_scan_batch over them, the host reads
               the run boundaries back, then per range a 16-byte aligned copy of its runs, one
               lsmblk_merge_batch (a round trip to size its output) and one lsmblk_read_filter_batch
  equal        kept entries and key bytes of both routes agree
  modes        the same batch with LSMBLK_SCAN_MVCC and with LSMBLK_LSM_SCAN_NEWEST (--modes): wall ms per
               batch and the rank kernel's ms from the kernel log, and newest_over_mvcc, the ratio of both
  rank70       separately: a view of 70 L0 tables of 1 MiB that every range crosses -- 69 searches per
               raw entry -- and lsm_scan_rank_kernel's ms from the kernel log: entries/s, searches/s; the
               rank kernel's ms in every mode of --modes

Every timed figure: 1 warm-up run, then RUNS runs; median, min and max.  Every GPU step runs under
its own time limit (SIGALRM ends the process).
usage: python tools/lsm_scan_probe.py [OUT_JSON] [--sst-mib M] [--ranges Q] [--span S] [--runs R]
                                     [--modes mvcc,newest] [--no-composition]
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from get_probe import ENTRY, KLEN, VLEN, key_bytes, spread  # noqa: E402
from lsm_amd import batch, sst  # noqa: E402
from lsm_amd._build import src_sha  # noqa: E402
from lsm_amd._lib import LSMBLK_LSM_SCAN_STATS_WORDS, LsmScanResultC, ScanResultC, kernel_timing  # noqa: E402

INCL_EXCL = 1 | (2 << 2)
MODE_FLAGS = {"default": 0, "mvcc": 2, "newest": 4}  # LSMBLK_SCAN_MVCC, LSMBLK_LSM_SCAN_NEWEST
RANK_KERNELS = ("lsm_scan_rank_kernel", "lsm_scan_rank_newest_kernel")


def step(name, seconds):
    signal.alarm(seconds)
    print(f"# {name} (limit {seconds} s)", file=sys.stderr, flush=True)


def wall(fn, runs):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


class Set:
    """nl0 L0 tables over the whole key space, nlevel levels of per_level tables, `per` entries each."""

    def __init__(self, nl0, nlevel, per_level, per, dev, rng):
        self.nl0, self.nlevel, self.per_level, self.per, self.dev = nl0, nlevel, per_level, per, dev
        self.C, self.nsst = nl0 + nlevel, nl0 + nlevel * per_level
        self.nmax = per * per_level
        n = per * self.nsst
        ids = np.concatenate([self.table_ids(t) for t in range(self.nsst)])
        vals = rng.integers(0, 256, n * VLEN, dtype=np.uint8)
        kv = batch.KVStream.from_numpy(key_bytes(ids).reshape(-1), np.arange(n + 1, dtype=np.uint64) * KLEN, vals,
                                       np.arange(n + 1, dtype=np.uint64) * VLEN, np.full(n, 7, np.uint64), device=dev)
        seg = (np.arange(self.nsst + 1, dtype=np.uint64) * per).astype(np.uint32)
        r = batch.encode_sst(kv, seg, 4096)
        files, file_off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, kv)
        del r, kv, vals, ids
        torch.cuda.empty_cache()
        self.ss = sst.SstSet(files, file_off)
        assert not self.ss.err.any(), self.ss.err
        self.l0 = list(range(nl0))
        self.levels = [[nl0 + l * per_level + j for j in range(per_level)] for l in range(nlevel)]
        self.view = self.ss.view(self.l0, self.levels)
        self.first = np.array([int(self.table_ids(t)[0]) for t in range(self.nsst)], np.uint64)
        self.last = np.array([int(self.table_ids(t)[-1]) for t in range(self.nsst)], np.uint64)

    def table_ids(self, t):
        m = np.arange(self.per, dtype=np.uint64)
        if t < self.nl0:
            return np.uint64(self.C) * (np.uint64(self.per_level) * m) + np.uint64(t)
        l, j = divmod(t - self.nl0, self.per_level)
        return np.uint64(self.C) * (np.uint64(j * self.per) + m) + np.uint64(self.nl0 + l)

    def ranges(self, nq, span, rng):
        n0 = rng.integers(0, self.nmax - span, nq).astype(np.uint64)
        return np.uint64(self.C) * n0, np.uint64(self.C) * (n0 + np.uint64(span))


class LsmScan:
    """The new call over one batch of ranges, into streams sized by two sizing calls."""

    def __init__(self, s, lo_id, hi_id, flags=0):
        ss, dev, nq = s.ss, s.dev, len(lo_id)
        self.s, self.nq, self.flags = s, nq, flags
        self.lk = torch.from_numpy(key_bytes(lo_id).reshape(-1)).to(dev)
        self.uk = torch.from_numpy(key_bytes(hi_id).reshape(-1)).to(dev)
        self.off = batch._u32_table(np.arange(nq + 1, dtype=np.uint64) * KLEN, dev)
        self.bnd = batch._u32_table(np.full(nq, INCL_EXCL, np.uint32), dev)
        self.ts = torch.full((nq,), 1 << 40, dtype=torch.int64, device=dev)
        self.res = torch.zeros(nq * ctypes.sizeof(LsmScanResultC), dtype=torch.uint8, device=dev)
        self.seg = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(LSMBLK_LSM_SCAN_STATS_WORDS, dtype=torch.int64, device=dev)
        self.sub_cap = sst.view_sub_cap(s.view, nq)
        self.raw = self.out = None
        st = self.call()
        self.raw = batch.KVStream.empty(st[4], st[5], st[6], dev)
        st = self.call()
        self.out = batch.KVStream.empty(st[0], st[1], st[2], dev)
        self.st = self.call()
        assert self.st[3] == 0, self.st

    def run(self):
        self.s.ss.lsm_scan_into(self.s.view, self.lk, self.off, self.uk, self.off, self.bnd, self.ts, self.nq, self.flags, self.sub_cap,
                                self.res, self.seg, self.stats, self.raw, self.out)

    def call(self):
        self.run()
        torch.cuda.synchronize()
        return batch._stats_words(self.stats)


def composition(s, lo_id, hi_id, caps):
    """The parent commit's calls for the same ranges -> (kept entries, kept key bytes)."""
    ss, dev, nq = s.ss, s.dev, len(lo_id)
    # host expansion: table t passes range_overlap(Included lo, Excluded hi) iff hi > first and lo <= last
    order = np.array(s.l0 + [t for lv in s.levels for t in lv])
    ok = (hi_id[:, None] > s.first[order][None, :]) & (lo_id[:, None] <= s.last[order][None, :])
    e_q, e_j = np.nonzero(ok)
    ne = len(e_q)
    sbase = np.concatenate([[0], np.cumsum(ok.sum(1))])
    qs = batch._u32_table(order[e_j].astype(np.uint32), dev)
    lk = torch.from_numpy(key_bytes(lo_id[e_q]).reshape(-1)).to(dev)
    uk = torch.from_numpy(key_bytes(hi_id[e_q]).reshape(-1)).to(dev)
    off = batch._u32_table(np.arange(ne + 1, dtype=np.uint64) * KLEN, dev)
    bnd = batch._u32_table(np.full(ne, INCL_EXCL, np.uint32), dev)
    res = torch.zeros(ne * ctypes.sizeof(ScanResultC), dtype=torch.uint8, device=dev)
    seg = torch.zeros(ne + 1, dtype=torch.int32, device=dev)
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=dev)
    kv = batch.KVStream.empty(*caps, dev)
    ss.scan_into(qs, lk, off, uk, off, bnd, ne, 1, res, seg, stats, kv)  # (NO_FILTER: the host filtered)
    torch.cuda.synchronize(dev)
    assert stats[3].item() == 0
    kv.n = int(stats[0].item())
    hseg = seg.cpu().numpy().view(np.uint32).astype(np.int64)
    ko, vo = kv.key_off.cpu().numpy().view(np.uint32).astype(np.int64), kv.val_off.cpu().numpy().view(np.uint32).astype(np.int64)
    kept = kbytes = 0
    for q in range(nq):
        a, b = int(hseg[sbase[q]]), int(hseg[sbase[q + 1]])
        if b == a:
            continue
        k0, k1, v0, v1 = int(ko[a]), int(ko[b]), int(vo[a]), int(vo[b])
        keys, vals = batch._aligned_empty(k1 - k0, dev), batch._aligned_empty(v1 - v0, dev)
        keys[:k1 - k0].copy_(kv.keys[k0:k1])
        vals[:v1 - v0].copy_(kv.vals[v0:v1])
        sub = batch.KVStream(keys, (kv.key_off[a:b + 1] - k0).contiguous(), vals, (kv.val_off[a:b + 1] - v0).contiguous(),
                             kv.ts[a:b].contiguous(), b - a)
        m = batch.merge_runs(sub, (hseg[sbase[q]:sbase[q + 1] + 1] - a).astype(np.uint32))
        f, _ = batch.read_filter(m, [0, m.n], 1 << 40)
        kept += f.n
        kbytes += f.byte_sizes()[0]
    return kept, kbytes


def kernel_times(ctx, scan, calls=3):
    """ms per launch of every kernel of `calls` calls (LSMBLK_DEBUG_KERNEL_TIMING, a pass of its own)."""
    with kernel_timing(ctx) as log:
        for _ in range(calls):
            scan.call()
    return {k: ms_ / ln for k, (ln, ms_) in log.items()}


def mode_legs(ctx, s, lo_id, hi_id, modes, runs, want):
    """Per mode: the batch's wall ms and its rank kernel's ms; the sizes must be `want`'s (one version
    per key and no key in two tables: every mode keeps every entry)."""
    out = {}
    for m in modes:
        scan = LsmScan(s, lo_id, hi_id, MODE_FLAGS[m])
        assert scan.st[:3] == want[:3] and scan.st[4:] == want[4:], (m, scan.st, want)
        ms = wall(scan.run, runs)
        kern = kernel_times(ctx, scan, 5)
        out[m] = dict(rank_kernel_ms=round(sum(kern.get(k, 0.0) for k in RANK_KERNELS), 4), **spread(ms))
        del scan
    if "mvcc" in out and "newest" in out:
        out["newest_over_mvcc"] = dict(wall=round(out["newest"]["median_ms"] / out["mvcc"]["median_ms"], 3),
                                       rank_kernel=round(out["newest"]["rank_kernel_ms"] / out["mvcc"]["rank_kernel_ms"], 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "lsm_scan_probe.json"))
    ap.add_argument("--sst-mib", type=int, default=8)
    ap.add_argument("--ranges", type=int, default=1024)
    ap.add_argument("--span", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rank-ranges", type=int, default=256)
    ap.add_argument("--modes", default="mvcc,newest", help="comma list of mvcc, newest (empty: none)")
    ap.add_argument("--no-composition", action="store_true")
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    if not torch.cuda.is_available():
        sys.exit("lsm_scan_probe needs a ROCm device")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(1)
    ctx = batch._ctx(dev.index)
    line = {"src_sha256": src_sha(), "device": torch.cuda.get_device_name(dev)}

    step("write and open the 16-source view", 300)
    s = Set(4, 3, 4, (a.sst_mib << 20) // ENTRY, dev, rng)
    lo_id, hi_id = s.ranges(a.ranges, a.span, rng)
    step("lsm_scan: sizing and timed runs", 300)
    new = LsmScan(s, lo_id, hi_id)
    st = new.st
    ms = wall(new.run, a.runs)
    med = sorted(ms)[len(ms) // 2]
    out_bytes = st[1] + st[2] + 16 * st[0]
    step("lsm_scan: per-kernel times", 120)
    kern = {k: round(v, 4) for k, v in kernel_times(ctx, new).items()}
    line["view"] = dict(ssts=s.nsst, sst_mib=a.sst_mib, l0=s.nl0, levels=s.nlevel, tables_per_level=s.per_level)
    line["lsm_scan"] = dict(ranges=a.ranges, span=a.span, table_scans=st[7], raw_entries=st[4], out_entries=st[0],
                            out_bytes=out_bytes, ranges_per_s=round(a.ranges / med * 1e3), out_gb_per_s=round(out_bytes / med / 1e6, 3),
                            kernels_ms_per_launch=kern, **spread(ms))

    if modes:
        step("modes: the same batch with " + ", ".join(modes), 300)
        line["modes"] = mode_legs(ctx, s, lo_id, hi_id, modes, a.runs, st)
    if not a.no_composition:
        step("composition: scan, merge per range, read filter", 900)
        caps = (st[4], st[5], st[6])
        kept = composition(s, lo_id, hi_id, caps)
        cms = wall(lambda: composition(s, lo_id, hi_id, caps), max(1, a.runs // 2))
        cmed = sorted(cms)[len(cms) // 2]
        line["composition"] = dict(ranges=a.ranges, kept=kept[0], ranges_per_s=round(a.ranges / cmed * 1e3),
                                   out_gb_per_s=round(out_bytes / cmed / 1e6, 3), **spread(cms))
        line["equal"] = bool(kept == (st[0], st[1]))
        line["speedup"] = round(cmed / med, 2)
    del new, s
    torch.cuda.empty_cache()

    step("rank70: write and open 70 L0 tables", 300)
    s = Set(70, 0, 1, (1 << 20) // ENTRY, dev, rng)
    lo_id, hi_id = s.ranges(a.rank_ranges, 16, rng)
    step("rank70: lsm_scan and its kernel log", 300)
    new = LsmScan(s, lo_id, hi_id)
    kern = kernel_times(ctx, new)
    rk, raw = kern["lsm_scan_rank_kernel"], new.st[4]
    line["rank70"] = dict(ranges=a.rank_ranges, runs_per_range=70, raw_entries=raw, rank_kernel_ms=round(rk, 4),
                          entries_per_s=round(raw / rk * 1e3), searches_per_s=round(raw * 69 / rk * 1e3),
                          all_kernels_ms={k: round(v, 4) for k, v in kern.items()})
    if modes:
        step("rank70: modes", 300)
        line["rank70"]["modes"] = mode_legs(ctx, s, lo_id, hi_id, modes, a.runs, new.st)
    signal.alarm(0)
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(line, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
