"""Measure point reads over an LSM view (lsmblk_lsm_get_batch) against the composition it replaces.

Workload (defaults): get_probe.py's set -- 16 SSTs of 64 MiB at block_size 4096, written on the device --
arranged as a view of 4 L0 tables with overlapping key ranges and 3 levels of 4 non-overlapping tables.
Key id = 8 n + c: L0 table c (0..3) holds n = 4 m, so it spans the whole key space; table j of level l
holds c = 4 + l, n in [j per, (j + 1) per); c = 7 is absent everywhere.  One version per key (ts 7),
values of 100 bytes.  1 Mi uniformly random keys, half present (a random entry of a random table),
half absent, read_ts above every ts.  Reported, one JSON line each, to stdout and OUT:

  lsm_get     per mode (default, mvcc, newest): ms of the new call without and with the value gather,
              the sources searched per key (seeks summed), FOUND
  baseline    per mode, on the same box and the same queries: the host builds the (table, key)
              expansion (every L0 table, per level the table bisected from the level's first keys;
              numpy), ONE lsmblk_sst_get_batch runs over it (device ms), the host folds the results
              (numpy).  With one visible version per key a source's landing is on the key exactly
              when its lookup is FOUND, which is what the fold uses for the decider rule.
  compare     every field of every result of the new call against the folded baseline: mismatches
  accept      per mode: the new call's median device ms <= that single lsmblk_sst_get_batch's

Every timed figure: 2 warm-up runs, then RUNS runs between device events; median, min and max.  Every
GPU step runs under its own time limit (SIGALRM ends the process).
usage: python tools/lsm_get_probe.py [OUT_JSON] [--sst-mib M] [--queries Q] [--runs R]
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
from get_probe import KLEN, VLEN, ENTRY, key_bytes, spread, timed  # noqa: E402
from lsm_amd import batch, sst  # noqa: E402
from lsm_amd._build import src_sha  # noqa: E402
from lsm_amd._lib import LSMBLK_GET_MVCC, LSMBLK_LSM_GET_NEWEST, GetResultC, LsmGetResultC  # noqa: E402

NL0, NLEVEL, PER_LEVEL = 4, 3, 4
NSST = NL0 + NLEVEL * PER_LEVEL
NSRC = NL0 + NLEVEL
ABSENT, FOUND, RANGE_OUT, BLOOM_OUT, NONE = 0, 1, 3, 4, 0xFFFFFFFF
LINES = []


def step(name, seconds):
    signal.alarm(seconds)
    print(f"# {name} (limit {seconds} s)", file=sys.stderr, flush=True)


def emit(**kw):
    LINES.append(kw)
    print(json.dumps(kw), flush=True)


def table_ids(t, per):
    """The ids SST t holds, ascending (t < NL0: L0 table t; else level (t - NL0) // 4, table (t - NL0) % 4)."""
    m = np.arange(per, dtype=np.uint64)
    if t < NL0:
        return np.uint64(8) * (np.uint64(4) * m) + np.uint64(t)
    l, j = divmod(t - NL0, PER_LEVEL)
    return np.uint64(8) * (np.uint64(j * per) + m) + np.uint64(4 + l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "lsm_get_probe.json"))
    ap.add_argument("--sst-mib", type=int, default=64)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lsm_get_probe needs a ROCm device")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(1)
    per = (a.sst_mib << 20) // ENTRY
    n = per * NSST

    step("write the SST files on the device", 300)
    ids = np.concatenate([table_ids(t, per) for t in range(NSST)])
    vals = rng.integers(0, 256, n * VLEN, dtype=np.uint8)
    kv = batch.KVStream.from_numpy(key_bytes(ids).reshape(-1), np.arange(n + 1, dtype=np.uint64) * KLEN, vals,
                                   np.arange(n + 1, dtype=np.uint64) * VLEN, np.full(n, 7, np.uint64), device=dev)
    seg = (np.arange(NSST + 1, dtype=np.uint64) * per).astype(np.uint32)
    r = batch.encode_sst(kv, seg, 4096)
    files, file_off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, kv)
    del r, kv, vals, ids
    torch.cuda.empty_cache()

    step("open", 120)
    ss = sst.SstSet(files, file_off)
    assert not ss.err.any(), ss.err
    l0 = list(range(NL0))
    levels = [[NL0 + l * PER_LEVEL + j for j in range(PER_LEVEL)] for l in range(NLEVEL)]
    view = ss.view(l0, levels)
    emit(what="set", ssts=NSST, sst_mib=a.sst_mib, file_bytes=int(files.numel()), blocks=len(ss.index), entries=n,
         l0=NL0, levels=NLEVEL, tables_per_level=PER_LEVEL)

    nq = a.queries
    present = rng.random(nq) < 0.5
    qt_tab = rng.integers(0, NSST, nq)
    qm = rng.integers(0, per, nq).astype(np.uint64)
    qid = np.uint64(8) * rng.integers(0, 4 * per, nq).astype(np.uint64) + np.uint64(7)
    for t in range(NSST):
        sel = present & (qt_tab == t)
        qid[sel] = table_ids(t, per)[qm[sel]]
    qkeys = key_bytes(qid)
    qk = torch.from_numpy(qkeys.reshape(-1)).to(dev)
    qo = batch._u32_table(np.arange(nq + 1, dtype=np.uint64) * KLEN, dev)
    qts = torch.full((nq,), 1 << 40, dtype=torch.int64, device=dev)
    res = torch.zeros(nq * ctypes.sizeof(LsmGetResultC), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    vo = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
    vbuf = batch._aligned_empty(nq * VLEN, dev)

    # ---- the expansion of the composition it replaces (host, numpy): per key every L0 table, per level
    # the table bisected from the level's first keys
    step("baseline: host expansion", 300)
    t0 = time.perf_counter()
    cols = [np.full(nq, t, np.int64) for t in l0]
    for lv in levels:
        # (a key's first 8 bytes are its id, big-endian, and decide every comparison of this set)
        firsts = np.array([int.from_bytes(ss.first_key(t)[:8], "big") for t in lv], np.uint64)
        p = np.searchsorted(firsts, qid, side="right")
        cols.append(np.where(p > 0, np.array(lv, np.int64)[np.maximum(p, 1) - 1], -1))
    tab = np.stack(cols, 1)                       # [nq, NSRC], -1: below the level
    keep = tab >= 0
    e_q, e_src = np.nonzero(keep)
    e_sst = tab[keep]
    ne = len(e_q)
    e_keys = qkeys[e_q]
    expand_ms = (time.perf_counter() - t0) * 1e3
    eq_k = torch.from_numpy(e_keys.reshape(-1)).to(dev)
    eq_o = batch._u32_table(np.arange(ne + 1, dtype=np.uint64) * KLEN, dev)
    eq_s = batch._u32_table(e_sst.astype(np.uint32), dev)
    eq_t = torch.full((ne,), 1 << 40, dtype=torch.int64, device=dev)
    eres = torch.zeros(ne * ctypes.sizeof(GetResultC), dtype=torch.uint8, device=dev)
    estats = torch.zeros(4, dtype=torch.int64, device=dev)
    emit(what="baseline_expansion", lookups=ne, per_key=round(ne / nq, 3), host_ms=round(expand_ms, 1))

    accept = {}
    for mode, flags in (("default", 0), ("mvcc", LSMBLK_GET_MVCC), ("newest", LSMBLK_LSM_GET_NEWEST)):
        step("lsm_get " + mode, 120)
        run = lambda gather: ss.lsm_get_into(view, qk, qo, qts, nq, flags, res, stats, vbuf if gather else None,
                                             nq * VLEN, vo if gather else None)
        ms_g = timed(lambda: run(True), a.runs)
        ms = timed(lambda: run(False), a.runs)
        st = stats.cpu().tolist()
        assert st[3] == 0, st
        new = res.cpu().numpy().view(np.dtype(LsmGetResultC))[:nq].copy()
        emit(what="lsm_get", mode=mode, keys=nq, found=st[1], seeks=int(new["seeks"].sum()),
             seeks_per_key=round(float(new["seeks"].mean()), 3), bloom_out=int(new["bloom_out"].sum()),
             mkeys_per_s=round(nq / sorted(ms)[len(ms) // 2] / 1e3, 2), **spread(ms),
             with_values={"value_bytes": int(new["vlen"][new["status"] == FOUND].sum()), **spread(ms_g)})

        step("baseline " + mode, 180)
        bflags = 0 if mode == "default" else LSMBLK_GET_MVCC
        bms = timed(lambda: ss.get_into(eq_s, eq_k, eq_o, eq_t, ne, bflags, eres, estats), a.runs)
        assert estats.cpu().tolist()[3] == 0
        g = eres.cpu().numpy().view(np.dtype(GetResultC))[:ne].copy()
        t0 = time.perf_counter()
        status = np.full((nq, NSRC), RANGE_OUT, np.uint32)
        status[e_q, e_src] = g["status"]
        row = np.full((nq, NSRC), -1, np.int64)
        row[e_q, e_src] = np.arange(ne)
        found = status == FOUND
        has = found.any(1)
        dec = np.where(has, found.argmax(1), NSRC - 1)  # (every ts is equal: NEWEST keeps the lowest ordinal too)
        upto = np.arange(NSRC)[None, :] <= (dec[:, None] if mode != "newest" else NSRC)
        searched = (status != RANGE_OUT) & (status != BLOOM_OUT) & upto
        fold = dict(seeks=searched.sum(1), bloom_out=((status == BLOOM_OUT) & upto).sum(1))
        pick = row[np.arange(nq), dec]
        fold["status"] = np.where(has, FOUND, ABSENT)
        fold["src"] = np.where(has, dec, NONE)
        fold["sst"] = np.where(has, tab[np.arange(nq), dec], NONE)
        for f in ("hit_blk", "hit_ent"):
            fold[f] = np.where(has, g[f][pick], NONE)
        for f in ("vlen", "ts", "val_pos"):
            fold[f] = np.where(has, g[f][pick], 0)
        fold_ms = (time.perf_counter() - t0) * 1e3
        bad = {f: int((new[f].astype(np.uint64) != np.asarray(fold[f]).astype(np.uint64)).sum()) for f in fold}
        emit(what="baseline", mode=mode, lookups=ne, expansion_host_ms=round(expand_ms, 1), fold_host_ms=round(fold_ms, 1),
             get_batch=spread(bms))
        emit(what="compare", mode=mode, mismatches=sum(bad.values()), by_field=bad)
        new_med, base_med = spread(ms)["median_ms"], spread(bms)["median_ms"]
        accept[mode] = new_med <= base_med
        emit(what="accept", mode=mode, lsm_get_median_ms=new_med, sst_get_batch_median_ms=base_med, ok=bool(accept[mode]))
    signal.alarm(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"src_sha256": src_sha(), "device": torch.cuda.get_device_name(dev), "lines": LINES}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
