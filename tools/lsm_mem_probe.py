"""Measure memtable runs as sources of the LSM reads (lsmblk_lsm_view.mem) on the GPU.

Workload (defaults): lsm_scan_probe.py's view -- SSTs of 8 MiB at block_size 4096 as 4 L0 tables that
each span the whole key space and 3 levels of 4 non-overlapping tables, key id = 7 n + c -- and 4 runs
of MEM entries each (run r: class r, n = 4 k m + 1, keys no table holds; ts 9, values of 100 bytes).
One JSON document to stdout and OUT:

  mem_vs_flushed  (a) the same batches over two views of one opened set: `mem`, the 16 tables under the
                  4 runs as memtable runs, and `flushed`, the same entries written as 4 more L0 tables
                  in the runs' place (the only route without the runs in the view).  A point-read batch
                  (a third of the keys in a run, a third in a table, a third nowhere; LSMBLK_GET_MVCC,
                  values gathered) and a scan batch (RANGES ranges of SPAN ids, LSMBLK_SCAN_MVCC): wall
                  ms (device events) and ms per launch of every kernel (LSMBLK_DEBUG_KERNEL_TIMING, a
                  pass of its own); the answers of both views are compared
  nmem0           (b) what the runs cost a caller without any: the batches of get_probe.py
                  (lsmblk_sst_get_batch), lsm_get_probe.py (lsmblk_lsm_get_batch) and lsm_scan_probe.py
                  (lsmblk_lsm_scan_batch) over the 16-table view with nmem == 0, ms per launch of every
                  kernel, in NMEM0_RUNS fresh processes per library, alternating this build and the one
                  given with --parent-so (a liblsmblk.so built from the parent commit); per kernel the
                  parent's spread (max - min of its runs' medians) and this build's excess over the
                  parent's slowest run

Every timed figure: 2 warm-up runs, then RUNS runs; median, min and max.  Every GPU step runs under
its own time limit (SIGALRM ends the process); a child process that fails ends the probe.
usage: python tools/lsm_mem_probe.py [OUT_JSON] [--sst-mib M] [--mem-entries E] [--queries Q] [--ranges R]
                                    [--span S] [--runs N] [--parent-so PATH] [--nmem0-runs K]
"""
import argparse
import ctypes
import json
import os
import signal
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from get_probe import ENTRY, KLEN, VLEN, key_bytes, spread, timed  # noqa: E402
from lsm_amd import batch, sst  # noqa: E402
from lsm_amd._build import src_sha  # noqa: E402
from lsm_amd._lib import (LSMBLK_GET_MVCC, LSMBLK_LSM_SCAN_STATS_WORDS, LSMBLK_SCAN_MVCC, GetResultC, LsmGetResultC,  # noqa: E402
                          LsmScanResultC, kernel_timing)

NL0, NLEVEL, PER_LEVEL, NMEM = 4, 3, 4, 4
C = NL0 + NLEVEL
NSST = NL0 + NLEVEL * PER_LEVEL
INCL_EXCL = 1 | (2 << 2)


def step(name, seconds):
    signal.alarm(seconds)
    print(f"# {name} (limit {seconds} s)", file=sys.stderr, flush=True)


def table_ids(t, per):
    """The ids SST t holds, ascending (lsm_scan_probe.Set's layout)."""
    m = np.arange(per, dtype=np.uint64)
    if t < NL0:
        return np.uint64(C) * (np.uint64(PER_LEVEL) * m) + np.uint64(t)
    l, j = divmod(t - NL0, PER_LEVEL)
    return np.uint64(C) * (np.uint64(j * per) + m) + np.uint64(NL0 + l)


def run_ids(r, per, mem):
    """Run r's ids, ascending: class r, n = 4 k m + 1 spread over the key space -- no table's key."""
    k = max(per * PER_LEVEL // (4 * mem), 1)
    return np.uint64(C) * (np.uint64(4 * k) * np.arange(mem, dtype=np.uint64) + np.uint64(1)) + np.uint64(r)


def stream_of(ids, ts, rng, dev):
    n = len(ids)
    return batch.KVStream.from_numpy(key_bytes(ids).reshape(-1), np.arange(n + 1, dtype=np.uint64) * KLEN,
                                     rng.integers(0, 256, n * VLEN, dtype=np.uint8), np.arange(n + 1, dtype=np.uint64) * VLEN,
                                     np.asarray(ts, np.uint64), device=dev)


class Set:
    """The 16 tables (and, with mem > 0, the runs' entries as 4 more SSTs) written and opened on the device."""

    def __init__(self, per, mem, dev, rng):
        self.per, self.mem, self.dev = per, mem, dev
        ids = [table_ids(t, per) for t in range(NSST)] + ([run_ids(r, per, mem) for r in range(NMEM)] if mem else [])
        ts = np.concatenate([np.full(len(x), 7 if t < NSST else 9, np.uint64) for t, x in enumerate(ids)])
        kv = stream_of(np.concatenate(ids), ts, rng, dev)
        seg = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.uint32)
        r = batch.encode_sst(kv, seg, 4096)
        files, file_off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, kv)
        self.ss = sst.SstSet(files, file_off)
        assert not self.ss.err.any(), self.ss.err
        self.l0 = list(range(NL0))
        self.levels = [[NL0 + l * PER_LEVEL + j for j in range(PER_LEVEL)] for l in range(NLEVEL)]
        self.view = self.ss.view(self.l0, self.levels)
        if mem:  # the runs: the same entries (keys, values, ts) as the four SSTs after the tables
            a = int(seg[NSST])
            keys, ko, vals, vo, t = kv.to_numpy()
            runs = batch.KVStream.from_numpy(keys[int(ko[a]):], ko[a:] - ko[a], vals[int(vo[a]):], vo[a:] - vo[a], t[a:], device=dev)
            start = batch._u32_table((seg[NSST:] - seg[NSST]).astype(np.uint32), dev)
            self.view_mem = self.ss.view(self.l0, self.levels, mem=(runs, start))
            self.view_flushed = self.ss.view(list(range(NSST, NSST + NMEM)) + self.l0, self.levels)
        del r, kv
        torch.cuda.empty_cache()

    def keys(self, nq, rng):
        """A third of the keys in a run (with runs), a third in a table, the others nowhere."""
        kind = rng.integers(0, 3, nq)
        qid = np.uint64(C) * (np.uint64(4) * rng.integers(0, self.per, nq).astype(np.uint64) + np.uint64(2))  # n = 4 m + 2, class 0
        m = rng.integers(0, self.per, nq)
        tab = rng.integers(0, NSST, nq)
        for t in range(NSST):
            sel = (kind == 1) & (tab == t)
            qid[sel] = table_ids(t, self.per)[m[sel]]
        if self.mem:
            run = rng.integers(0, NMEM, nq)
            for r in range(NMEM):
                sel = (kind == 0) & (run == r)
                qid[sel] = run_ids(r, self.per, self.mem)[m[sel] % self.mem]
        return qid

    def ranges(self, nq, span, rng):
        n0 = rng.integers(0, self.per * PER_LEVEL - span, nq).astype(np.uint64)
        return np.uint64(C) * n0, np.uint64(C) * (n0 + np.uint64(span))


class Get:
    """One lsmblk_lsm_get_batch batch with the values gathered."""

    def __init__(self, s, qid, flags):
        dev, nq = s.dev, len(qid)
        self.s, self.nq, self.flags = s, nq, flags
        self.qk = torch.from_numpy(key_bytes(qid).reshape(-1)).to(dev)
        self.qo = batch._u32_table(np.arange(nq + 1, dtype=np.uint64) * KLEN, dev)
        self.qt = torch.full((nq,), 1 << 40, dtype=torch.int64, device=dev)
        self.res = torch.zeros(nq * ctypes.sizeof(LsmGetResultC), dtype=torch.uint8, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int64, device=dev)
        self.vo = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        self.vbuf = batch._aligned_empty(nq * VLEN, dev)

    def run(self, view):
        self.s.ss.lsm_get_into(view, self.qk, self.qo, self.qt, self.nq, self.flags, self.res, self.stats, self.vbuf, self.nq * VLEN,
                               self.vo)

    def answer(self, view):
        self.run(view)
        torch.cuda.synchronize()
        st = self.stats.cpu().tolist()
        assert st[3] == 0, st
        r = self.res.cpu().numpy().view(np.dtype(LsmGetResultC))[:self.nq]
        return st, r.copy(), self.vbuf[:st[2]].cpu().numpy().tobytes()


class Scan:
    """One lsmblk_lsm_scan_batch batch into streams sized by two sizing calls."""

    def __init__(self, s, view, lo_id, hi_id, flags):
        dev, nq = s.dev, len(lo_id)
        self.s, self.view, self.nq, self.flags = s, view, nq, flags
        self.lk = torch.from_numpy(key_bytes(lo_id).reshape(-1)).to(dev)
        self.uk = torch.from_numpy(key_bytes(hi_id).reshape(-1)).to(dev)
        self.off = batch._u32_table(np.arange(nq + 1, dtype=np.uint64) * KLEN, dev)
        self.bnd = batch._u32_table(np.full(nq, INCL_EXCL, np.uint32), dev)
        self.ts = torch.full((nq,), 1 << 40, dtype=torch.int64, device=dev)
        self.res = torch.zeros(nq * ctypes.sizeof(LsmScanResultC), dtype=torch.uint8, device=dev)
        self.seg = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(LSMBLK_LSM_SCAN_STATS_WORDS, dtype=torch.int64, device=dev)
        self.sub_cap = sst.view_sub_cap(view, nq)
        self.raw = self.out = None
        st = self.call()
        self.raw = batch.KVStream.empty(st[4], st[5], st[6], dev)
        st = self.call()
        self.out = batch.KVStream.empty(st[0], st[1], st[2], dev)
        self.st = self.call()
        assert self.st[3] == 0, self.st
        self.out.n = self.st[0]

    def run(self):
        self.s.ss.lsm_scan_into(self.view, self.lk, self.off, self.uk, self.off, self.bnd, self.ts, self.nq, self.flags, self.sub_cap,
                                self.res, self.seg, self.stats, self.raw, self.out)

    def call(self):
        self.run()
        torch.cuda.synchronize()
        return batch._stats_words(self.stats)


def kernel_ms(ctx, fn, calls=5):
    """ms per launch of every kernel of `calls` calls of fn (a pass of its own, after a warm-up call)."""
    fn()
    with kernel_timing(ctx) as log:
        for _ in range(calls):
            fn()
    return {k: round(ms / ln, 4) for k, (ln, ms) in log.items()}


def leg_nmem0(a, dev, rng, ctx):
    """(b) in this process, with the library this process loaded: the three batches without a run."""
    step("nmem0: write and open the 16-table view", 300)
    s = Set((a.sst_mib << 20) // ENTRY, 0, dev, rng)
    nq = a.queries
    qid = s.keys(nq, rng)
    out = {}
    step("nmem0: sst_get batch", 120)
    qs = batch._u32_table(rng.integers(0, NSST, nq).astype(np.uint32), dev)
    g = Get(s, qid, 0)
    res = torch.zeros(nq * ctypes.sizeof(GetResultC), dtype=torch.uint8, device=dev)
    sget = lambda: s.ss.get_into(qs, g.qk, g.qo, g.qt, nq, 0, res, g.stats, g.vbuf, nq * VLEN, g.vo)
    out["sst_get"] = dict(kernels=kernel_ms(ctx, sget), **spread(timed(sget, a.runs)))
    step("nmem0: lsm_get batch", 120)
    lget = lambda: g.run(s.view)
    out["lsm_get"] = dict(kernels=kernel_ms(ctx, lget), **spread(timed(lget, a.runs)))
    step("nmem0: lsm_scan batch", 300)
    sc = Scan(s, s.view, *s.ranges(a.ranges, a.span, rng), 0)
    out["lsm_scan"] = dict(kernels=kernel_ms(ctx, sc.run), **spread(timed(sc.run, a.runs)))
    return out


def summary(parent, this):
    """Per batch and kernel: the medians' lists, the parent's spread, this build's worst excess over the parent's slowest."""
    out = {}
    for b in this[0]:
        rows = {}
        for k in this[0][b]["kernels"]:
            p = [r[b]["kernels"].get(k) for r in parent if r[b]["kernels"].get(k) is not None]
            t = [r[b]["kernels"][k] for r in this]
            if not p:
                continue
            rows[k] = dict(parent_ms=p, this_ms=t, parent_spread_ms=round(max(p) - min(p), 4),
                           excess_over_parent_max_ms=round(max(t) - max(p), 4),
                           within_parent_spread=bool(sorted(t)[len(t) // 2] - sorted(p)[len(p) // 2] <= max(p) - min(p)))
        out[b] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "lsm_mem_probe.json"))
    ap.add_argument("--sst-mib", type=int, default=8)
    ap.add_argument("--mem-entries", type=int, default=16384)
    ap.add_argument("--queries", type=int, default=1 << 18)
    ap.add_argument("--ranges", type=int, default=1024)
    ap.add_argument("--span", type=int, default=32)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--parent-so", default=None, help="liblsmblk.so built from the parent commit: measure (b) against it")
    ap.add_argument("--nmem0-runs", type=int, default=3)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)  # nmem0: a child's run of (b), one JSON line
    a = ap.parse_args()

    if a.leg is None and a.parent_so:  # (b): fresh processes, before this one opens the device
        legs = {"parent": [], "this": []}
        for i in range(a.nmem0_runs):
            for who in ("parent", "this"):
                env = dict(os.environ)
                env.pop("LSMBLK_SO_OVERRIDE", None)
                if who == "parent":
                    env["LSMBLK_SO_OVERRIDE"] = os.path.abspath(a.parent_so)
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", "nmem0", "--sst-mib", str(a.sst_mib), "--queries",
                       str(a.queries), "--ranges", str(a.ranges), "--span", str(a.span), "--runs", str(a.runs)]
                print(f"# nmem0 run {i} with the {who} library", file=sys.stderr, flush=True)
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=900)
                if p.returncode != 0:
                    sys.exit(f"lsm_mem_probe: the {who} leg ended with {p.returncode}")
                legs[who].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    else:
        legs = None

    if not torch.cuda.is_available():
        sys.exit("lsm_mem_probe needs a ROCm device")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(1)
    ctx = batch._ctx(dev.index)
    if a.leg == "nmem0":
        out = leg_nmem0(a, dev, rng, ctx)
        signal.alarm(0)
        print(json.dumps(out), flush=True)
        return

    doc = {"src_sha256": src_sha(), "device": torch.cuda.get_device_name(dev)}
    step("write and open the 20 SSTs, upload the runs", 300)
    s = Set((a.sst_mib << 20) // ENTRY, a.mem_entries, dev, rng)
    qid = s.keys(a.queries, rng)
    lo_id, hi_id = s.ranges(a.ranges, a.span, rng)
    cmp = dict(view=dict(ssts=NSST, sst_mib=a.sst_mib, l0=NL0, levels=NLEVEL, tables_per_level=PER_LEVEL, runs=NMEM,
                         entries_per_run=a.mem_entries), queries=a.queries, ranges=a.ranges, span=a.span)
    g = Get(s, qid, LSMBLK_GET_MVCC)
    answers = {}
    for name, view in (("mem", s.view_mem), ("flushed", s.view_flushed)):
        step(f"point reads over the {name} view", 180)
        st, r, vals = g.answer(view)
        answers[name] = (r, vals)
        ms = timed(lambda: g.run(view), a.runs)
        cmp.setdefault("get", {})[name] = dict(found=st[1], value_bytes=st[2], seeks_per_key=round(float(r["seeks"].mean()), 3),
                                               kernels=kernel_ms(ctx, lambda: g.run(view)), **spread(ms))
        step(f"scans over the {name} view", 300)
        sc = Scan(s, view, lo_id, hi_id, LSMBLK_SCAN_MVCC)
        ms = timed(sc.run, a.runs)
        answers[name] += (sc.st, [x.tobytes() for x in sc.out.to_numpy()])
        cmp.setdefault("scan", {})[name] = dict(table_scans=sc.st[7], raw_entries=sc.st[4], out_entries=sc.st[0],
                                                kernels=kernel_ms(ctx, sc.run), **spread(ms))
        del sc
    (r0, v0, s0, o0), (r1, v1, s1, o1) = answers["mem"], answers["flushed"]
    cmp["equal"] = dict(get=bool(all((r0[f] == r1[f]).all() for f in ("status", "src", "ts", "vlen")) and v0 == v1),
                        scan=bool(s0[:3] == s1[:3] and s0[4:] == s1[4:] and o0 == o1))
    doc["mem_vs_flushed"] = cmp
    if legs:
        doc["nmem0"] = dict(runs=legs, by_kernel=summary(legs["parent"], legs["this"]))
    signal.alarm(0)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
