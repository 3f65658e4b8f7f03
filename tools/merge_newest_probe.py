#!/usr/bin/env python3
"""Per-kernel times of one compaction in LSMBLK_MERGE_RUNS and in LSMBLK_MERGE_NEWEST.

One synthetic compaction input from lsm_amd/synth.py -- config C's shape (8 overlapping sorted runs
of 16-byte keys and 100-byte values) cut to a size that runs in seconds, with a share of the keys
present in two runs and two versions per key and run -- through lsmblk_compact_batch in each mode of
--modes, with LSMBLK_DEBUG_KERNEL_TIMING on.  Per mode: a warm-up, then --reps timed repetitions,
each read from lsmblk_ctx_kernel_log.  Prints one JSON line: the input's metadata (entries, runs,
share of multi-run keys), and per mode the merged and kept counts, every kernel's median ms, and
per repetition the summed ms of the two tile kernels and of the whole call's kernels.

    python tools/merge_newest_probe.py --label this --modes runs,newest --out profiles/merge_newest_probe.json

--out appends the line to a JSON list.  The modes are given by number where this checkout's
lsm_amd._lib does not name them, so the same file measures an older commit's RUNS path.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lsm_amd import _lib, batch, synth  # noqa: E402
from lsm_amd._lib import kernel_log, kernel_timing  # noqa: E402

MODES = {"runs": getattr(_lib, "LSMBLK_MERGE_RUNS", 0), "newest": getattr(_lib, "LSMBLK_MERGE_NEWEST", 2)}
TILE_KERNELS = ("merge_tile_kernel", "merge_big_kernel")


def is_tile_kernel(name):
    return name.split("<")[0] in TILE_KERNELS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=600_000)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--overwrite", type=float, default=0.25, help="share of keys that also live in a second run")
    ap.add_argument("--versions", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="runs,newest")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("merge_newest_probe: needs a ROCm device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    keys, ko, vals, vo, ts, rs = synth.gen_runs(a.keys, nrun=a.runs, overwrite=a.overwrite, seed=45, versions=a.versions)
    n = len(ts)
    k16 = np.ascontiguousarray(keys).reshape(n, 16).view("V16").reshape(n)
    run = np.searchsorted(rs.astype(np.int64), np.arange(n), "right") - 1
    uk, inv = np.unique(k16, return_inverse=True)
    pairs = np.unique(inv.astype(np.int64) * a.runs + run)
    multi = float((np.bincount(pairs // a.runs, minlength=len(uk)) > 1).mean())
    line = dict(label=a.label, entries=n, runs=a.runs, versions=a.versions, keys=int(len(uk)),
                multi_run_key_share=round(multi, 4), key_bytes=int(ko[-1]), value_bytes=int(vo[-1]),
                device=torch.cuda.get_device_name(dev), reps=a.reps, modes={})

    kv = batch.KVStream.from_numpy(keys, ko, vals, vo, ts, device=dev)
    rt = batch._u32_table(rs, dev)
    wm = int(np.median(ts))
    buf = batch.CompactBuffers(n, int(ko[-1]), int(vo[-1]), dev, target_sst_size=2 << 20)
    ctx = batch._ctx(dev.index)
    for name in a.modes.split(","):
        opts = batch.compact_opts(wm, True, (), 4096, 2 << 20, dev, merge_mode=MODES[name])
        for _ in range(a.warmup):
            batch.compact_into(kv, rt, a.runs, opts, buf)
        torch.cuda.synchronize(dev)
        s = buf.stats.cpu().tolist()
        if s[3]:
            sys.exit(f"merge_newest_probe: mode {name} failed with error flags {s[3]}")
        reps = []
        with kernel_timing(ctx):
            for _ in range(a.reps):  # (the log is read, and so emptied, per repetition)
                batch.compact_into(kv, rt, a.runs, opts, buf)
                torch.cuda.synchronize(dev)
                reps.append({k: ms for k, (_, ms) in kernel_log(ctx).items()})
        names = sorted(set().union(*reps))
        line["modes"][name] = dict(
            merged=s[4], kept=s[5], blocks=s[0], ssts=s[2],
            kernel_ms_median={k: round(float(np.median([r.get(k, 0.0) for r in reps])), 4) for k in names},
            tile_kernels_ms=[round(sum(ms for k, ms in r.items() if is_tile_kernel(k)), 4) for r in reps],
            all_kernels_ms=[round(sum(r.values()), 4) for r in reps])
    print(json.dumps(line), flush=True)
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        with open(a.out, "w") as f:
            json.dump(old + [line], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
