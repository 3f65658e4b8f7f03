"""bench.py -- device-resident SSTable block decode + re-encode throughput (BASELINE.json metric).

One step = decode the whole resident batch of encoded blocks into the SoA KV stream, then
re-encode that stream into blocks from the segment (SST) starts alone (the anti-shortcut
rule of SURVEY.md section 8(d)): the reference's Block::decode + BlockIterator walk
followed by SsTableBuilder::add / BlockBuilder over every SST.

A plain run does only what the headline figure needs: set up the workload, warm up, time
--steps steps, read the calls' status words, write --dump-outputs, print the line.  --full adds
everything else, after the timed region: the re-encoded bytes are checked equal to the input,
and the whole batch is checked against the C oracle (oracle/lsmblk_oracle.c): oracle encode of
the synthetic KV == the input blocks, oracle decode == the GPU decode, oracle re-encode == the
GPU re-encode (oracle_checked_blocks); then the per-kernel roofline, the framing / filter / slot
encode legs, the CPU baseline, the PCIe-inclusive rate and the extra configs.

--dump-outputs DIR writes what the last timed step returned to its caller (the decoded KV
stream, the re-encoded blocks and their offsets, the calls' status words; for config C the
compaction's outputs) as DIR/<name>.npy, float32 for bytes and float64 for offsets and
timestamps: whole arrays when small, else a fixed seeded sample of their elements (the same
indices on every run, DUMP_BYTES in all).  The inputs are seeded, so two builds can be compared
file by file.

Default workload (configs[1]): 1,048,576 x 4 KiB blocks per GPU, uniform sorted 16-B keys,
100-B values, 40-bit ts, 2 MiB segments.  --config Z / M / C select the other configs:
  Z  Zipf shared-prefix keys, 4 KiB blocks (configs[2])
  M  8 B - 4 KiB values, 64 KiB blocks (configs[3])
  C  compaction-shaped (configs[4] at one-GPU scale): 8 overlapping sorted runs of 2 MiB SSTs,
     one step = decode every input block + MergeIterator merge + compaction rules + SST
     rotation + block packing (lsmblk_compact_batch), checked against compact_generate_sst
With --full, N=1 and the default config, Z, M and C also run (fewer steps) and are reported
under "extra_configs".

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N>1: started by torchrun (RANK/WORLD_SIZE/LOCAL_RANK in the environment), or, without those,
this script starts the N rank processes itself (the parent never touches a GPU).  Prints ONE
JSON line on rank 0.  `value` = encoded-block GiB processed per second by all ranks (weak
scaling: every rank owns its own batch; no collective on the data path, only the timing
barrier / max-reduce).
"""
import argparse
import gc
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from lsm_amd import batch, synth  # noqa: E402
from lsm_amd._lib import check, lib  # noqa: E402

METRIC = "GiB/s device-resident SSTable block encode+decode, 4 KiB blocks, 1/2/4/8 GPU"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
GiB = float(1 << 30)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--config", default="U", choices=["U", "Z", "M", "C"])
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the checks (round trip, C oracle), the per-kernel roofline, "
                        "the side legs, the CPU baseline, the PCIe-inclusive rate and the extra configs "
                        "(the --no-* options below trim a --full run)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64; large arrays "
                        "as a fixed seeded sample)")
    p.add_argument("--blocks", type=int, default=None, help="blocks per GPU (default 1 Mi for U/Z/C, 64 Ki for M)")
    p.add_argument("--segment-bytes", type=int, default=2 << 20)
    p.add_argument("--ranges-per-gpu", type=int, default=None,
                   help="config C: key ranges per GPU (each under one call's 4 GiB KV arenas; default 1 at "
                        "N=1, and at N>1 3 ranges of 1 Mi blocks = 12.5 GiB of input per GPU, 100 GiB on 8: "
                        "SURVEY.md section 8(d) config 5)")
    p.add_argument("--cpu-seconds", type=float, default=10.0, help="CPU baseline budget (rank 0, N=1)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-extras", action="store_true", help="skip the Z / M / C extra configs at N=1")
    p.add_argument("--no-oracle-check", action="store_true")
    p.add_argument("--no-pcie", action="store_true", help="skip the H2D+D2H-inclusive rate (DESIGN.md)")
    p.add_argument("--dry-run", action="store_true",
                   help="launcher self-test: ranks join a gloo group and report the world, no GPU work")
    p.add_argument("--dry-run-fail-extra", type=int, default=None,
                   help="diagnostics: in --dry-run, this rank raises inside compact_dist (the N>1 extra's path)")
    p.add_argument("--dry-run-fail-rank", type=int, default=None,
                   help="launcher self-test: this rank exits with status 3 before joining the group")
    p.add_argument("--encode-mode", default="packed", choices=["packed", "slots", "slots-fused"],
                   help="re-encode output: all segments packed (lsmblk_encode_batch), per-segment slots "
                        "(LSMBLK_ENCODE_SEG_SLOTS), or slots through the fused walk + emit launch (A/B)")
    p.add_argument("--plan-pipe", type=int, default=None, choices=[0, 1],
                   help="A/B: the plan walk's helper pipelined over batches (1, the default) or not (0)")
    p.add_argument("--decode-two-pass", action="store_true",
                   help="diagnostics (A/B): count + tile scan + decode (three launches) instead of the lagged decode")
    p.add_argument("--decode-lag", type=int, default=None,
                   help="diagnostics (A/B): blocks the lagged decode counts ahead of its decodes (default 10240)")
    p.add_argument("--ablate-lag", action="store_true", help="diagnostics: the lagged decode's ablation masks")
    p.add_argument("--trace-plan", action="store_true", help="diagnostics: the plan walk's per-segment trace")
    p.add_argument("--trace-fused", action="store_true",
                   help="diagnostics: the fused walk + emit launch's per-walker trace and emitter record waits")
    p.add_argument("--ablate-only", action="store_true", help="diagnostics: time only mask 0 and --ablate")
    p.add_argument("--ablate-decode", action="store_true", help="diagnostics: --ablate is a decode mask")
    p.add_argument("--ablate", type=int, default=None,
                   help="diagnostics: time decode alone with this skip mask (prints a non-bench line)")
    return p.parse_args(argv)


# ---------------------------------------------------------------------------------------------
# launcher: N rank processes from a parent that never initialises a GPU
def launch(args, argv):
    """Start the N ranks and wait for them, failing fast: the first rank that exits non-zero
    gets the others terminated (a rank blocked in a collective with a dead peer would otherwise
    hang until the driver's time limit), and the launcher exits non-zero."""
    import socket
    import threading
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_RANK=str(r),
                   LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr))
    out = []  # rank 0's stdout, read on a thread so the poll loop never blocks on a full pipe
    reader = threading.Thread(target=lambda: out.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    failed = None
    while failed is None:
        rcs = [p.poll() for p in procs]
        failed = next(((r, rc) for r, rc in enumerate(rcs) if rc not in (None, 0)), None)
        if all(rc == 0 for rc in rcs):
            break
        time.sleep(0.1)
    if failed is not None:
        log(f"[launcher] rank {failed[0]} exited with status {failed[1]}: terminating the other ranks")
        for p in procs:
            if p.poll() is None:
                p.terminate()
        deadline = time.time() + 10
        for p in procs:
            try:
                p.wait(timeout=max(deadline - time.time(), 0.1))
            except subprocess.TimeoutExpired:
                p.kill()
    rcs = [p.wait() for p in procs]
    reader.join(timeout=10)
    if failed is None and out and out[0]:
        sys.stdout.write(out[0].decode())
        sys.stdout.flush()
    return max(max(abs(rc) for rc in rcs), 1 if failed is not None else 0)


def dist_env():
    return int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))


# ---------------------------------------------------------------------------------------------
def build_workload(cfg, nblk, seg_bytes, seed, dev):
    """Synthetic KV stream -> GPU-encoded blocks truncated to exactly nblk blocks.  Also returns
    the host KV of exactly those entries and their segment table (for the oracle check)."""
    bs = synth.BLOCK_SIZE[cfg]
    per_block = {"U": 31.0, "Z": 34.5, "M": 95.0}[cfg]
    n = int(nblk * per_block * 1.03) + 1024
    t = time.time()
    keys, ko, vals, vo, ts = synth.GENERATORS[cfg](n, seed=seed)
    seg = synth.segments_by_bytes(ko, vo, seg_bytes)
    d = batch.KVStream.from_numpy(keys, ko, vals, vo, ts, device=dev)
    blocks, blk_off = batch.encode_kv(d, seg, bs)
    del d
    total_blocks = blk_off.numel() - 1
    if total_blocks < nblk:
        raise RuntimeError(f"generated {total_blocks} < {nblk} blocks; raise per_block estimate")
    end = int(blk_off[nblk].item())
    blocks = blocks[:end].clone()
    blk_off = blk_off[:nblk + 1].clone()
    kv = batch.decode_blocks(blocks, blk_off)            # exactly the entries of the kept blocks
    seg = seg[seg < kv.n]
    seg = np.concatenate([seg, [kv.n]]).astype(np.uint32)
    host = (keys[:int(ko[kv.n])], ko[:kv.n + 1], vals[:int(vo[kv.n])], vo[:kv.n + 1], ts[:kv.n])
    log(f"[rank] workload {cfg}: {nblk} blocks, {kv.n} entries, {end / GiB:.3f} GiB encoded, "
        f"{len(seg) - 1} segments, setup {time.time() - t:.1f}s")
    return blocks, blk_off, kv, seg, bs, host


def oracle_check_blocks(host, seg, bs, blocks, blk_off, out_kv, n, out_blocks, out_off, nblk):
    """The whole batch against the C oracle: the oracle's encode of the synthetic KV must equal
    the input blocks (so the GPU-made input is independently pinned), the oracle's decode of the
    input must equal the GPU decode, and the GPU re-encode must equal both.  Returns the number
    of blocks checked (0 on any mismatch)."""
    from oracle import oracle as O
    t = time.time()
    kv = O.KV(*host)
    rc, ref_blocks, ref_off = O.encode_segments(kv, seg, bs)
    hb = blocks.cpu().numpy()
    ok = rc == 0 and len(ref_off) == nblk + 1 and np.array_equal(ref_blocks, hb)
    ok = ok and np.array_equal(ref_off, blk_off.cpu().numpy().view(np.uint64))
    ok = ok and np.array_equal(out_blocks[:len(hb)].cpu().numpy(), ref_blocks)
    ok = ok and np.array_equal(out_off[:nblk + 1].cpu().numpy().view(np.uint64), ref_off)
    if ok:
        rc, dkv = O.decode_blocks(ref_blocks, ref_off)
        keys, ko, vals, vo, ts = batch.KVStream(out_kv.keys, out_kv.key_off, out_kv.vals, out_kv.val_off,
                                                out_kv.ts, n).to_numpy()
        ok = rc == 0 and dkv.n == n and np.array_equal(ko, dkv.key_off) and np.array_equal(vo, dkv.val_off)
        ok = ok and np.array_equal(ts, dkv.ts) and np.array_equal(keys, dkv.keys) and np.array_equal(vals, dkv.vals)
    log(f"[rank] oracle check of {nblk} blocks: {'ok' if ok else 'MISMATCH'} ({time.time() - t:.1f}s)")
    return nblk if ok else 0


def run_blocks(args, cfg, steps, warmup, rank, world, local, dev, extra=False):
    """U / Z / M: decode + re-encode of the resident batch.  Returns the result dict (rank 0)."""
    nblk = args.blocks or (65536 if cfg == "M" else 1 << 20)
    blocks, blk_off, kv, seg, bs, host = build_workload(cfg, nblk, args.segment_bytes, 1000 + rank, dev)
    E = int(blocks.numel())
    K, V = kv.byte_sizes()
    n = kv.n
    D = K + V + 16 * n  # decoded SoA bytes: key + value + u64 ts + u32 key_off + u32 val_off

    # preallocated buffers, workspace reserved: the timed region does no allocation
    out_kv = batch.KVStream(batch._aligned_empty(K + 16, dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                            batch._aligned_empty(V + 16, dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                            torch.empty(n, dtype=torch.int64, device=dev), n)
    slots = args.encode_mode != "packed"
    # per-segment slots need the closed-form bound (include/lsmblk.h): keys + values + 18 B per entry
    out_cap, blk_cap = (K + V + 18 * n + 16 if slots else E + 16), nblk + 2
    out_blocks = batch._aligned_empty(out_cap, dev)
    out_off = torch.zeros(blk_cap, dtype=torch.int64, device=dev)
    seg_t = torch.from_numpy(seg.view(np.int32)).to(dev)
    seg_out = torch.zeros(2 * (len(seg) - 1), dtype=torch.int64, device=dev) if slots else None
    st_dec = torch.zeros(4, dtype=torch.int64, device=dev)
    st_enc = torch.zeros(4, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    ctx = batch._ctx(local, stream)
    check(lib().lsmblk_ctx_reserve(ctx, nblk + 1, n + 1, len(seg)))
    check(lib().lsmblk_debug_set(ctx, 3, 1 if args.decode_two_pass else 0))
    if args.encode_mode == "slots-fused" or args.trace_fused:
        check(lib().lsmblk_debug_set(ctx, 8, 1))
    if args.plan_pipe is not None:
        check(lib().lsmblk_debug_set(ctx, 9, args.plan_pipe))
    if args.decode_lag is not None:
        check(lib().lsmblk_debug_set(ctx, 4, args.decode_lag))

    def step(ev=None):
        if ev is not None:
            ev[0].record(stream)
        batch.decode_into(blocks, blk_off, nblk, out_kv, st_dec, n, K + 16, V + 16)
        if ev is not None:
            ev[1].record(stream)
        batch.encode_into(out_kv, seg_t, len(seg) - 1, bs, out_blocks, out_cap, out_off, blk_cap, st_enc,
                          seg_out=seg_out)
        if ev is not None:
            ev[2].record(stream)

    if args.trace_plan and not extra:  # the plan walk's per-segment realtime trace over one encode
        import ctypes
        step()
        torch.cuda.synchronize()
        check(lib().lsmblk_debug_set(ctx, 5, 1))
        batch.encode_into(out_kv, seg_t, len(seg) - 1, bs, out_blocks, out_cap, out_off, blk_cap, st_enc)
        NW = 16 + 8 * 32768
        w = (ctypes.c_uint64 * NW)()
        check(lib().lsmblk_debug_counters(ctx, w, NW))
        check(lib().lsmblk_debug_set(ctx, 5, 0))
        tr = np.frombuffer(w, dtype=np.uint64)[16:].reshape(-1, 8).astype(np.int64)[:len(seg) - 1]
        t0 = tr[:, 0].min()
        q = lambda x: {p: round(float(np.percentile(x, p)), 2) for p in (10, 50, 90, 100)}
        print(json.dumps({"plan_trace": {
            "walk_start_us": q((tr[:, 0] - t0) / 100), "walk_us": q((tr[:, 1] - tr[:, 0]) / 100),
            "walk_wait_frac": q(tr[:, 2] / np.maximum(1, tr[:, 1] - tr[:, 0])),
            "windows": q(tr[:, 3]), "blocks": q(tr[:, 7]),
            "helper_us": q((tr[:, 5] - tr[:, 4]) / 100), "helper_wait_frac": q(tr[:, 6] / np.maximum(1, tr[:, 5] - tr[:, 4])),
            "walk_end_us": q((tr[:, 1] - t0) / 100)}}), flush=True)
        # where the slow walkers ran: walk time by XCD, by SE, by SIMD (HW_ID / XCC_ID in word 7)
        walk = (tr[:, 1] - tr[:, 0]) / 100
        hw = (tr[:, 7] >> 32) & 0xFFFFFF
        xcc = (tr[:, 7] >> 56) & 0xF
        groups = {"xcc": xcc, "se": (hw >> 13) & 3, "simd": (hw >> 4) & 3, "cu": (hw >> 8) & 0xF}
        print(json.dumps({"plan_walk_us_by": {g: {int(v): [int((key == v).sum()), round(float(np.median(walk[key == v])), 1)]
                                                  for v in np.unique(key)} for g, key in groups.items()}}), flush=True)
        return None
    if args.trace_fused and not extra:  # the fused walk + emit launch: per-walker trace, emitter waits
        import ctypes
        step()
        torch.cuda.synchronize()
        check(lib().lsmblk_debug_set(ctx, 5, 1))
        t0 = time.time()
        batch.encode_into(out_kv, seg_t, len(seg) - 1, bs, out_blocks, out_cap, out_off, blk_cap, st_enc,
                          seg_out=seg_out)
        NW = 16 + 8 * 32768
        w = (ctypes.c_uint64 * NW)()
        check(lib().lsmblk_debug_counters(ctx, w, NW))
        check(lib().lsmblk_debug_set(ctx, 5, 0))
        a = np.frombuffer(w, dtype=np.uint64).astype(np.int64)
        tr = a[16:].reshape(-1, 8)
        tr = tr[tr[:, 0] > 0]
        t_0 = tr[:, 0].min()
        q = lambda x: {p: round(float(np.percentile(x, p)), 2) for p in (0, 10, 50, 90, 100)}
        print(json.dumps({"fused_trace": {
            "walkers": int(len(tr)), "walk_start_us": q((tr[:, 0] - t_0) / 100), "walk_us": q((tr[:, 1] - tr[:, 0]) / 100),
            "walk_end_us": q((tr[:, 1] - t_0) / 100), "walker_helper_wait_frac": q(tr[:, 2] / np.maximum(1, tr[:, 1] - tr[:, 0])),
            "windows": q(tr[:, 3]), "blocks": q(tr[:, 4]),
            "us_per_window": q((tr[:, 1] - tr[:, 0]) / 100 / np.maximum(1, tr[:, 3])),
            "emit_items": int(a[2]), "emit_waited_items": int(a[1]), "emit_wait_us_total": round(a[0] / 100, 1),
            "emit_wait_us_per_item": round(a[0] / 100 / max(1, a[2]), 3),
            "last_emitter_end_us": round((a[3] - t_0) / 100, 1)}}), flush=True)
        return None
    if args.ablate is not None and not extra:
        if args.ablate >= 65536:  # plan masks: the plan kernel alone (emit not launched)
            res = {}
            for mask in (0, 1 << 16, 1 << 17, 3 << 16):
                check(lib().lsmblk_debug_set(ctx, 1, mask))
                step()
                res[mask] = kernel_times(ctx, step, dev, reps=2)["plan"]
            check(lib().lsmblk_debug_set(ctx, 1, 0))
            print(json.dumps({"ablation_plan_ms_by_skip_mask": res}), flush=True)
            return None
        if (16 <= args.ablate < 256 or args.ablate == 1) and not args.ablate_decode:  # encode-side masks
            res = {}
            for mask in (0, 1, 16, 32, 64, 112, 128, 240):
                check(lib().lsmblk_debug_set(ctx, 1, mask))
                step()
                res[mask] = kernel_times(ctx, step, dev, reps=2)["emit"]
            check(lib().lsmblk_debug_set(ctx, 1, 0))
            print(json.dumps({"ablation_emit_ms_by_skip_mask": res}), flush=True)
            return None
        ablate(args, ctx, blocks, blk_off, nblk, out_kv, st_dec, n, K, V, stream)
        return None
    elapsed, (dec_ms, enc_ms) = timed(step, steps, warmup, world, dev)

    # the last step's status words (what its caller reads): no error, every entry and block counted
    sd, se = st_dec.cpu().tolist(), st_enc.cpu().tolist()
    ok = sd[3] == 0 and se[3] == 0 and sd[0] == n and se[0] == nblk and se[1] == E
    pk_blocks, pk_off = out_blocks, out_off  # (step() keeps writing out_blocks: never rebound)
    if slots and ok and (args.full or args.dump_outputs):
        pk_blocks, pk_off = batch.slots_to_packed(out_blocks, out_off[:nblk + 1], seg_out)
    if args.dump_outputs and ok and not extra:
        dump_outputs(args.dump_outputs, rank, world, [
            ("keys", out_kv.keys[:K]), ("key_off", out_kv.key_off[:n + 1]), ("vals", out_kv.vals[:V]),
            ("val_off", out_kv.val_off[:n + 1]), ("ts", out_kv.ts[:n]), ("decode_stats", st_dec),
            ("blocks", pk_blocks[:E]), ("blk_off", pk_off[:nblk + 1]), ("encode_stats", st_enc)])
    checked = 0
    if args.full:
        # correctness of the last step: re-encoded bytes == input bytes (the slots packed first)
        ok = ok and torch.equal(pk_blocks[:E], blocks) and torch.equal(pk_off[:nblk + 1], blk_off)
        if ok and not args.no_oracle_check:
            checked = oracle_check_blocks(host, seg, bs, blocks, blk_off, out_kv, n, pk_blocks, pk_off, nblk)
            ok = checked == nblk
    if not ok:
        log(f"ROUND TRIP MISMATCH dec_stats={sd} enc_stats={se}")
    t_max, ok_all, checked_all = reduce_ranks(elapsed, ok, checked, world, dev)

    # per-kernel durations: a short profiling pass after the timed region, each kernel launched
    # by liblsmblk.so with dispatch start/stop events (diagnostics only, not timed)
    kms = kernel_times(ctx, step, dev, reps=3) if args.full else None
    if rank != 0:
        return None
    value = world * E * steps / t_max / GiB
    ms_per_step = t_max / steps * 1e3
    desc = {"U": "16-B uniform keys, 100-B values", "Z": "Zipf 12-B prefixes, 100-B values",
            "M": "16-B keys, 8 B-4 KiB values"}[cfg]
    result = {
        "metric": METRIC, "value": round(value, 3), "unit": "GiB/s", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8",
        "data": "synthetic", "full": bool(args.full), "status_ok": bool(ok_all),
        "config": {"workload": f"{cfg}: {nblk} blocks/GPU x block_size {bs}, decode + re-encode ({desc})",
                   "blocks_per_gpu": nblk, "entries_per_gpu": n, "encoded_bytes_per_gpu": E,
                   "decoded_bytes_per_gpu": D, "block_size": bs, "segments_per_gpu": len(seg) - 1,
                   "parallelism": f"block-sharded x{world} (no data-path collective)",
                   "encode_output": {"packed": "segments packed (lsmblk_encode_batch)",
                                     "slots": "per-segment slots (LSMBLK_ENCODE_SEG_SLOTS)",
                                     "slots-fused": "per-segment slots, fused walk + emit launch"}[args.encode_mode],
                   "rccl_world": world},
    }
    if not args.full:  # the checks, the roofline and the side legs are --full's
        result["stage_ms"] = {"decode": round(dec_ms, 4), "encode": round(enc_ms, 4)}
        return result
    result["config"].update({"roundtrip_bit_exact": bool(ok_all), "oracle_checked_blocks": int(checked_all)})
    # algorithmic bytes per launch of each kernel (DESIGN.md "Kernels")
    cnt = E + 8 * (nblk + 1) + 12 * nblk             # count: streams every block, agg
    algo = {"dec_count": cnt, "dec_scan": 0, "decode": E + D + 8 * (nblk + 1) + 12 * nblk,
            "plan": 8 * (n + 1) + K + 8 * nblk, "emit": D + E + 16 * (nblk + 1)}
    dom = max(kms, key=lambda k: kms[k])
    achieved = algo[dom] / (kms[dom] * 1e-3) / 1e9
    traffic, why = measured_traffic(cfg, dom, default_size=args.blocks is None)
    result["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                          "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                          **({"traffic_reason": why} if why else {}),
                          "bytes_per_launch": algo[dom], "launch_ms": round(kms[dom], 4),
                          "kernels_ms": {k: round(v, 4) for k, v in kms.items()},
                          "stage_ms": {"decode": round(dec_ms, 4), "encode": round(enc_ms, 4)},
                          "step_algorithmic_bytes": algo["decode"] + algo["emit"],
                          "step_frac": round((algo["decode"] + algo["emit"]) / (ms_per_step * 1e-3) / 1e9
                                             / HBM_PEAK_GBS, 4)}
    result["cpu_baseline"] = None
    if extra or not ok_all:  # (the side legs read the step's outputs; a failed round trip ends the run)
        return result
    result["framing_crc32"] = framing_crc32(blocks, blk_off, nblk, E, dev, stream)
    result["read_path_verify"] = read_path_verify(blocks, blk_off, nblk, out_kv, n, K, V, st_dec, dev, stream)
    result["framing_meta"] = framing_meta(pk_blocks, pk_off, nblk, seg_t, st_enc, dev, stream)
    result["compaction_filter"] = compaction_filter(out_kv, n, K, V, dev, stream)
    result["encode_slots"] = encode_slots(out_kv, seg_t, len(seg) - 1, bs, blocks, blk_off, dev, stream)
    result["encode_framed"] = encode_framed(out_kv, seg_t, len(seg) - 1, bs, blocks, blk_off, dev, stream,
                                            round(enc_ms, 4))
    if world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(blocks, blk_off, seg, bs, args.cpu_seconds)
    if not args.no_pcie and world == 1:
        del out_kv, out_blocks, pk_blocks, pk_off
        torch.cuda.empty_cache()
        result["pcie_inclusive"] = pcie_inclusive(blocks, blk_off, nblk, kv, seg, bs, dev)
    return result


def timed(step, steps, warmup, world, dev):
    """warmup, barrier + sync, exactly `steps` timed steps, barrier + sync.  Returns the elapsed
    seconds and the mean (first-stage, second-stage) ms from HIP events on the launch stream."""
    import torch.distributed as dist
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    t0 = time.perf_counter()
    for i in range(steps):
        step(evs[i])
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    a = float(np.mean([e[0].elapsed_time(e[1]) for e in evs]))
    b = float(np.mean([e[1].elapsed_time(e[2]) for e in evs]))
    return elapsed, (a, b)


def reduce_ranks(elapsed, ok, checked, world, dev):
    """max elapsed, all-ok, and the sum of oracle-checked units over the ranks."""
    if world == 1:
        return elapsed, ok, checked
    import torch.distributed as dist
    from lsm_amd.shard import comm_device
    dev = comm_device(dev)
    tt = torch.tensor([elapsed, 0.0 if ok else 1.0], dtype=torch.float64, device=dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    cc = torch.tensor([checked], dtype=torch.int64, device=dev)
    dist.all_reduce(cc, op=dist.ReduceOp.SUM)
    return float(tt[0].item()), tt[1].item() == 0.0, int(cc.item())


DUMP_BYTES = 56 << 20  # --dump-outputs: array bytes written by all ranks together (under 64 MB with the headers)


def dump_outputs(dirpath, rank, world, arrays):
    """--dump-outputs: write every (name, array) of `arrays` -- device tensors or host arrays, trimmed
    to what the call returned -- as dirpath/<name>.npy (rank<r>_<name>.npy at N > 1).  u8 arrays are
    written as float32, the u32 / u64 ones (held in int32 / int64 tensors) as float64: offsets and the
    40-bit timestamps are exact in it.  Every array gets the same element budget, DUMP_BYTES / N over
    the arrays' item sizes; a longer array is written as a sample of its elements at sorted indices
    drawn from a generator seeded by the array's name and length, so two runs sample the same places."""
    import zlib
    os.makedirs(dirpath, exist_ok=True)
    wide = lambda a: a.dtype not in (torch.uint8, np.dtype(np.uint8))
    cap = (DUMP_BYTES // world) // sum(8 if wide(a) else 4 for _, a in arrays)
    for name, a in arrays:
        L = int(a.numel() if isinstance(a, torch.Tensor) else a.size)
        if L > cap:
            rng = np.random.default_rng([zlib.crc32(name.encode()), L])
            idx = np.sort(rng.integers(0, L, size=cap))
            a = a[torch.from_numpy(idx).to(a.device)] if isinstance(a, torch.Tensor) else a[idx]
        h = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if h.dtype.kind == "i":  # the library's unsigned words in torch's signed tensors
            h = h.view({4: np.uint32, 8: np.uint64}[h.dtype.itemsize])
        h = h.astype(np.float64 if wide(a) else np.float32)
        np.save(os.path.join(dirpath, (f"rank{rank}_" if world > 1 else "") + name + ".npy"), h)
    log(f"[rank {rank}] wrote {len(arrays)} arrays (at most {cap} elements each) to {dirpath}")


# ---------------------------------------------------------------------------------------------
# config C: compaction-shaped decode -> merge -> rules -> rotation -> encode
def build_runs(nblk, nrun, seg_bytes, seed, dev, key_slice=(0, 1), with_run_blk=False):
    """nrun overlapping sorted runs (L0 SSTs of seg_bytes each), about nblk 4 KiB blocks in all,
    encoded on the device; returns the concatenated input blocks, their offsets, the per-run
    entry starts, and the host KV (for the oracle).  key_slice = (s, w): this rank's storage holds
    slice s of w of the key space."""
    t = time.time()
    n_keys = int(nblk * 31.0 / 1.1)
    keys, ko, vals, vo, ts, rs = synth.gen_runs(n_keys, nrun=nrun, seed=seed, key_slice=key_slice)
    parts, offs, base, run_blk = [], [], 0, [0]
    for r in range(nrun):
        a, b = int(rs[r]), int(rs[r + 1])
        rk = keys[int(ko[a]):int(ko[b])]
        rv = vals[int(vo[a]):int(vo[b])]
        rko, rvo = ko[a:b + 1] - ko[a], vo[a:b + 1] - vo[a]
        seg = synth.segments_by_bytes(rko, rvo, seg_bytes)
        d = batch.KVStream.from_numpy(rk, rko, rv, rvo, ts[a:b], device=dev)
        blk, off = batch.encode_kv(d, seg, 4096)
        parts.append(blk)
        offs.append(off[:-1] + base if r < nrun - 1 else off + base)
        base += int(blk.numel())
        run_blk.append(run_blk[-1] + off.numel() - 1)
        del d
    blocks = torch.cat(parts)
    blk_off = torch.cat(offs)
    log(f"[rank] workload C: {nrun} runs, {len(ts)} entries, {blk_off.numel() - 1} blocks, "
        f"{blocks.numel() / GiB:.3f} GiB encoded, setup {time.time() - t:.1f}s")
    if with_run_blk:
        return blocks, blk_off, rs, (keys, ko, vals, vo, ts), np.array(run_blk, np.int64)
    return blocks, blk_off, rs, (keys, ko, vals, vo, ts)


def oracle_check_compaction(host, rs, opts, buf, stats):
    """GPU compaction == compact_generate_sst restated in C (orc_merge_runs + orc_compact) over the
    whole batch: blocks, block offsets, SST first entries / first blocks, kept entries."""
    from oracle import oracle as O
    t = time.time()
    kv = O.KV(*host)
    src = O.merge_runs(kv, rs)
    want = O.compact(kv, src, opts["watermark"], opts["bottom_level"], (), opts["block_size"],
                     opts["target_sst_size"])
    nblk, nbytes, nsst = stats[0], stats[1], stats[2]
    ok = (stats[4] == len(src) and stats[5] == len(want["kept"]) and nblk == len(want["blk_off"]) - 1
          and nsst == len(want["sst_blk"]) - 1)
    ok = ok and np.array_equal(buf.out[:nbytes].cpu().numpy(), want["blocks"])
    ok = ok and np.array_equal(buf.blk_off[:nblk + 1].cpu().numpy().view(np.uint64), want["blk_off"])
    ok = ok and np.array_equal(buf.sst_start[:nsst + 1].cpu().numpy().view(np.uint32), want["sst_ent"])
    ok = ok and np.array_equal(buf.sst_blk[:nsst + 1].cpu().numpy().view(np.uint32), want["sst_blk"])
    log(f"[rank] oracle check of the compaction ({nblk} output blocks, {nsst} SSTs): "
        f"{'ok' if ok else 'MISMATCH'} ({time.time() - t:.1f}s)")
    return nblk if ok else 0


def oracle_check_range(blocks_dev, off_dev, rs, opts, sh, res, lo=None, hi=None):
    """One range of the sharded compaction against the C oracle: the range's kept stream ==
    the oracle's decode of the range's input blocks + orc_merge_runs + compact_generate_sst's rules,
    restricted to the range's keys [lo, hi); its segments, carry-out and blocks ==
    compact_generate_sst resumed at the received carry-in (orc_shard_rotation) over that stream +
    the received halo.  Chained over the ranks (carry-out r == carry-in r+1, checked by the caller)
    this is the whole single-stream compaction.  Host memory: one range at a time, every
    intermediate dropped as soon as the next one exists (a few copies of the range's KV at most)."""
    from oracle import oracle as O
    t = time.time()
    rc, kv = O.decode_blocks(blocks_dev.cpu().numpy(), off_dev.cpu().numpy().view(np.uint64))
    assert rc == 0 and kv.n == int(rs[-1])
    src = O.merge_runs(kv, rs)
    idx = src[O.compact(kv, src, opts["watermark"], opts["bottom_level"], (), opts["block_size"], 1 << 62,
                        kept_only=True)["kept"]].astype(np.int64)
    del src
    if lo is not None or hi is not None:  # the kept stream is sorted: [lo, hi) is an index interval
        ko = kv.key_off

        def first_at_least(bound):
            a, b = 0, len(idx)
            while a < b:
                m = (a + b) // 2
                if bytes(kv.keys[ko[idx[m]]:ko[idx[m] + 1]]) < bound:
                    a = m + 1
                else:
                    b = m
            return a
        idx = idx[0 if lo is None else first_at_least(lo):len(idx) if hi is None else first_at_least(hi)]
    kept = O.gather(kv, idx)
    del kv, idx
    m = sh.m
    ok = kept.n == m
    ek, eko, ev, evo, ets = batch.KVStream(sh.ext.keys, sh.ext.key_off, sh.ext.vals, sh.ext.val_off, sh.ext.ts,
                                           sh.ext.n).to_numpy()
    ok = ok and np.array_equal(eko[:m + 1], kept.key_off) and np.array_equal(evo[:m + 1], kept.val_off)
    ok = ok and np.array_equal(ets[:m], kept.ts) and np.array_equal(ek[:kept.key_off[-1]], kept.keys)
    ok = ok and np.array_equal(ev[:kept.val_off[-1]], kept.vals)
    del kept
    if ok:
        ext = O.KV(ek, eko, ev, evo, ets)
        rc, seg, cout = O.shard_rotation(ext, m, sh.last, *res["carry_in"], opts["block_size"], opts["target_sst_size"])
        ok = rc == 0 and cout == res["carry_out"] and seg.tolist() == res["seg_start"].tolist()
        if ok and len(seg):
            rc, blk, off = O.encode_span(ext, seg, opts["block_size"])
            del ext, ek, ev
            ok = rc == 0 and np.array_equal(blk, res["blocks"].cpu().numpy())
            ok = ok and np.array_equal(off, res["blk_off"].cpu().numpy().view(np.uint64))
    log(f"[rank] oracle check of the range ({res['nblk']} output blocks, {res['nseg']} segments, carry "
        f"{res['carry_in']} -> {res['carry_out']}): {'ok' if ok else 'MISMATCH'} ({time.time() - t:.1f}s)")
    return res["nblk"] if ok else 0


C_RANGES_NGPU = 3          # config C at N > 1: key ranges per GPU by default ...
C_RANGE_BLOCKS = 1 << 20   # ... of 1 Mi input blocks each (12.5 GiB per GPU: configs[4]'s 100 GiB on 8)
C_BLOCK_BYTES = 4033       # mean encoded 4 KiB input block (SURVEY.md section 8 table, U-shaped data)


def c_plan(args, world):
    """(ranges per GPU, input blocks per GPU) of config C: as given, else 1 x 1 Mi at N = 1 and
    C_RANGES_NGPU x C_RANGE_BLOCKS at N > 1 (the north star's 100 GiB compaction on 8 GPUs)."""
    R = args.ranges_per_gpu or (C_RANGES_NGPU if world > 1 else 1)
    blocks = args.blocks or (R * C_RANGE_BLOCKS if world > 1 and args.ranges_per_gpu is None else 1 << 20)
    return R, blocks


def c_plan_summary(args, world):
    R, blocks = c_plan(args, world)
    per = blocks * C_BLOCK_BYTES
    return {"ranges_per_gpu": R, "input_blocks_per_gpu": blocks, "blocks_per_range": blocks // R,
            "input_gb_per_gpu": round(per / 1e9, 2), "input_gib_per_gpu": round(per / GiB, 2),
            "total_input_gb": round(world * per / 1e9, 1)}


def host_rss_gib():
    """This process's peak resident host memory (GiB)."""
    import resource
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / (1 << 20)


def run_compaction(args, steps, warmup, rank, world, local, dev, extra=False):
    if world > 1 or c_plan(args, world)[0] > 1:
        return run_compaction_sharded(args, steps, warmup, rank, world, local, dev, extra)
    nblk_in = args.blocks or (1 << 20)
    nrun = 8
    blocks, blk_off, rs, host = build_runs(nblk_in, nrun, args.segment_bytes, 2000 + rank, dev)
    nblk = blk_off.numel() - 1
    E = int(blocks.numel())
    n = int(rs[-1])
    K, V = len(host[0]), len(host[2])
    kv = batch.KVStream.empty(n, K, V, dev)
    st_dec = torch.zeros(4, dtype=torch.int64, device=dev)
    rs_t = torch.from_numpy(rs.view(np.int32)).to(dev)
    buf = batch.CompactBuffers(n, K, V, dev, target_sst_size=args.segment_bytes)
    ts = host[4]
    opts = batch.compact_opts(watermark=int(ts.max()) // 2, bottom_level=True, block_size=4096,
                              target_sst_size=args.segment_bytes, device=dev)
    stream = torch.cuda.current_stream(dev)
    ctx = batch._ctx(local, stream)
    check(lib().lsmblk_ctx_reserve(ctx, nblk + 1, n + 1, buf.sst_cap))

    def step(ev=None):
        if ev is not None:
            ev[0].record(stream)
        batch.decode_into(blocks, blk_off, nblk, kv, st_dec, n, K + 16, V + 16)
        kv.n = n
        if ev is not None:
            ev[1].record(stream)
        batch.compact_into(kv, rs_t, nrun, opts, buf)
        if ev is not None:
            ev[2].record(stream)

    elapsed, (dec_ms, cmp_ms) = timed(step, steps, warmup, world, dev)
    s = buf.stats.cpu().tolist()
    sd = st_dec.cpu().tolist()
    ok = sd[3] == 0 and s[3] == 0 and sd[0] == n
    if not ok:
        log(f"COMPACTION FAILED dec_stats={sd} stats={s}")
    if args.dump_outputs and ok and not extra:
        kept = buf.kept
        dump_outputs(args.dump_outputs, rank, world, [
            ("kept_keys", kept.keys[:s[6]]), ("kept_key_off", kept.key_off[:s[5] + 1]), ("kept_vals", kept.vals[:s[7]]),
            ("kept_val_off", kept.val_off[:s[5] + 1]), ("kept_ts", kept.ts[:s[5]]),
            ("blocks", buf.out[:s[1]]), ("blk_off", buf.blk_off[:s[0] + 1]), ("sst_start", buf.sst_start[:s[2] + 1]),
            ("sst_blk", buf.sst_blk[:s[2] + 1]), ("compact_stats", buf.stats)])
    checked = 0
    if args.full and ok and not args.no_oracle_check:
        checked = oracle_check_compaction(host, rs, opts, buf, s)
        ok = checked == s[0]
    t_max, ok_all, checked_all = reduce_ranks(elapsed, ok, checked, world, dev)
    if rank != 0:
        return None
    ms = t_max / steps * 1e3
    Dk = s[6] + s[7] + 16 * s[5]
    D = K + V + 16 * n
    step_bytes = {"decode": E + D, "merge_gather": 2 * D + 4 * n, "encode": Dk + s[1]}
    roofline = None
    if args.full:
        roofline = compaction_roofline(ctx, step, dev, E, D, Dk, n, nblk, s, sum(step_bytes.values()), ms,
                                       default_size=args.blocks is None)
    return {
        "metric": METRIC, "value": round(world * E * steps / t_max / GiB, 3), "unit": "GiB/s", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "full": bool(args.full), "status_ok": bool(ok_all),
        "config": {"workload": f"C: compaction-shaped, {nrun} overlapping sorted runs of {args.segment_bytes >> 20} MiB "
                               f"SSTs ({nblk} x 4 KiB input blocks/GPU, ~10% overwrites, 2% tombstones): decode + "
                               "MergeIterator merge + compaction rules (bottom level, watermark) + SST rotation + "
                               "block packing", "input_blocks_per_gpu": nblk, "input_entries_per_gpu": n,
                   "encoded_bytes_per_gpu": E, "merged_entries": s[4], "kept_entries": s[5],
                   "output_blocks": s[0], "output_bytes": s[1], "output_ssts": s[2],
                   "target_sst_size": args.segment_bytes, "parallelism": f"key-range sharded x{world}",
                   "rccl_world": world, "compaction_bit_exact": bool(ok_all) if args.full else None,
                   "oracle_checked_blocks": int(checked_all)},
        "stage_ms": {"decode": round(dec_ms, 4), "compact": round(cmp_ms, 4)},
        "step_algorithmic_bytes": step_bytes,
        "roofline": roofline,
    }


def compaction_roofline(ctx, step, dev, E, D, Dk, n, nblk, s, step_bytes, ms, default_size=True):
    """Config C's roofline: every kernel of a step timed from its dispatch events (kernel log), the
    dominant one priced by its algorithmic bytes and its measured traffic."""
    prof = kernel_log_profile(ctx, step, dev)
    per = {k: v[1] for k, v in prof.items()}
    dom = max(per, key=per.get)
    kept, merged = s[5], s[4]
    # algorithmic bytes per step of the kernels that can dominate
    algo = {"decode_lag_kernel": E + D + 20 * nblk,          # blocks in, decoded stream out
            "merge_tile_kernel": 24 * n,                      # key_off + 16-B key prefix in, merged rank out
            "mwrite_kernel": 2 * Dk + 4 * merged,             # kept entries gathered in merged order
            "mflag_kernel": s[6] + 12 * merged,               # keys + ts + order in, keep flags out
            "emit_kernel": Dk + s[1], "plan_walk_kernel": 8 * (kept + 1) + s[6] + 8 * s[0]}
    b = algo.get(dom.split("<")[0])  # (templates log as name<args>)
    achieved = b / (per[dom] * 1e-3) / 1e9 if b else None
    traffic, why = measured_traffic("C", dom, launches=prof[dom][0], default_size=default_size)
    top = sorted(per.items(), key=lambda kv: -kv[1])[:10]
    return {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1) if achieved else None, "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None, "traffic": traffic,
            **({"traffic_reason": why} if why else {}),
            "bytes_per_launch": b, "launch_ms": round(per[dom], 4),
            "kernels_ms": {k: round(v, 4) for k, v in top},
            "launches_per_step": {k: round(prof[k][0], 2) for k, _ in top},
            "step_algorithmic_bytes": step_bytes,
            "step_frac": round(step_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def storage_slice(k, WR, nblk_range, nrun, seg_bytes, dev):
    """Storage slice k (0 <= k <= WR) of a compaction split into WR key ranges: the L0 SSTs (nrun
    overlapping runs of seg_bytes SSTs) holding half-slices 2k-1 and 2k of the key space cut into
    2 WR (the first and the last storage slice hold one half-slice).  Deterministic in k, so
    every rank that reads a slice builds the same blocks.  Returns the blocks, their offsets,
    each run's first block, every block's first / last key and first entry, and the largest ts
    (the host KV is dropped: the oracle check reads the range inputs back from the device)."""
    h0, h1 = max(2 * k - 1, 0), min(2 * k + 1, 2 * WR)
    blocks, off, rs, host, run_blk = build_runs(nblk_range * (h1 - h0) // 2, nrun, seg_bytes, 3000 + k, dev,
                                                key_slice=(h0, 2 * WR, h1 - h0), with_run_blk=True)
    _, ent = batch.decode_blocks(blocks, off, with_blk_ent=True)
    ent = ent.cpu().numpy().view(np.uint64).astype(np.int64)
    keys, ko = host[0], host[1]
    first = [bytes(keys[ko[ent[b]]:ko[ent[b] + 1]]) for b in range(len(ent) - 1)]
    last = [bytes(keys[ko[ent[b + 1] - 1]:ko[ent[b + 1]]]) for b in range(len(ent) - 1)]
    ts_max = int(host[4].max())
    del host, keys, ko
    return dict(blocks=blocks, off=off.cpu().numpy().view(np.uint64).astype(np.int64), run_blk=run_blk,
                first=first, last=last, ent=ent, ts_max=ts_max)


def range_input(sl_lo, sl_hi, lo, hi, nrun, dev):
    """The input of key range [lo, hi) (None: unbounded): from storage slices sl_lo (holding the
    range's lower half) and sl_hi (its upper half), every block of every run whose keys meet the
    range -- BlockMeta first / last keys decide, no decode -- so a block straddling a splitter is
    read by both ranges.  Runs keep their order (run r = slice sl_lo's selected run-r blocks, then
    sl_hi's).  Returns the device blocks, offsets and run entry starts (the oracle check reads the
    blocks back from the device, one range at a time)."""
    pieces, run_start, nent = [], [0], 0
    for r in range(nrun):
        for sl, cond in ((sl_lo, lambda b, s: lo is None or s["last"][b] >= lo),
                         (sl_hi, lambda b, s: hi is None or s["first"][b] < hi)):
            b0, b1 = int(sl["run_blk"][r]), int(sl["run_blk"][r + 1])
            sel = [b for b in range(b0, b1) if cond(b, sl)]
            if sel:
                a, z = sel[0], sel[-1] + 1
                assert sel == list(range(a, z))  # a run's blocks meeting a range are contiguous
                pieces.append((sl, a, z))
                nent += int(sl["ent"][z] - sl["ent"][a])
        run_start.append(nent)
    parts, offs, base = [], [], 0
    for sl, a, z in pieces:
        o = sl["off"]
        parts.append(sl["blocks"][int(o[a]):int(o[z])])
        offs.append(o[a:z] - o[a] + base)
        base += int(o[z] - o[a])
    offs.append(np.array([base], np.int64))
    blocks = torch.cat(parts) if parts else torch.zeros(16, dtype=torch.uint8, device=dev)
    off = np.concatenate(offs)
    return blocks.contiguous(), torch.from_numpy(off.copy()).to(dev), np.array(run_start, np.uint32)


def run_compaction_sharded(args, steps, warmup, rank, world, local, dev, extra=False):
    """Config C over N GPUs, split by key range.  The key space holds
    W = N x R ranges (R = --ranges-per-gpu); the input L0 SSTs are stored in W + 1 storage slices
    whose boundaries sit in the MIDDLE of the ranges (storage_slice), and the splitters are the
    median BlockMeta first key of each storage slice, so every range reads, from two slices, the
    blocks that meet its keys (range_input): blocks straddling a splitter are decoded by both
    neighbouring ranges.  One step = decode of the range inputs + merge / rules (range-restricted)
    + halo all-gather + rotation + carry (through the rank's ranges, then send/recv to the next
    rank) + block packing (shard.compact_dist, or shard.compact_local on one GPU): together the
    outputs are the single-stream compaction of the whole input, byte for byte, SST boundaries
    included (checked per range against the oracle)."""
    import torch.distributed as dist
    from lsm_amd import shard
    R, blocks_gpu = c_plan(args, world)
    WR = world * R
    nblk_range = blocks_gpu // R
    nrun = 8
    t0 = time.time()
    # this rank's ranges g = rank*R .. rank*R+R-1 read storage slices g and g+1; slices are built
    # one ahead and freed once their second range has its input, so the host holds at most two
    # slices' KV at a time (the oracle check later reads the range inputs back from the device)
    slices, parts, wm_local = {}, [], 0

    def get_slice(k):
        nonlocal wm_local
        if k not in slices:
            sl = storage_slice(k, WR, nblk_range, nrun, args.segment_bytes, dev)
            f = sorted(sl["first"])
            sl["splitter"] = f[len(f) // 2]  # the median BlockMeta first key (k = 1 .. WR-1)
            wm_local = max(wm_local, sl["ts_max"])
            slices[k] = sl
        return slices[k]
    for i in range(R):
        g = rank * R + i
        a, b = get_slice(g), get_slice(g + 1)
        lo = a["splitter"] if g > 0 else None
        hi = b["splitter"] if g + 1 < WR else None
        blocks_i, off_i, rs = range_input(a, b, lo, hi, nrun, dev)
        parts.append((blocks_i, off_i, rs, lo, hi))
        del slices[g], a
        gc.collect()
    straddling = sum(int(p[1].numel() - 1) for p in parts)
    # one wm for the whole job (the reference's LsmMvccInner::watermark is global)
    wm_local //= 2
    if world > 1:
        cdev = shard.comm_device(dev)
        wm = torch.tensor([wm_local], dtype=torch.int64, device=cdev)
        dist.all_reduce(wm, op=dist.ReduceOp.MAX)
        wm = int(wm.item())
    else:
        cdev = torch.device("cpu")
        wm = wm_local
    del slices
    torch.cuda.empty_cache()
    log(f"[rank {rank}] {R} range inputs ({straddling} blocks incl. the straddling ones) in {time.time() - t0:.1f}s")
    opts = batch.compact_opts(watermark=wm, bottom_level=True, block_size=4096,
                              target_sst_size=args.segment_bytes, device=dev)
    stream = torch.cuda.current_stream(dev)
    kvs, decs, shards, sizes = [], [], [], []
    for i, (blocks_i, off_i, rs, lo, hi) in enumerate(parts):
        # decoded sizes bound by the encoded bytes (every entry >= 16 B encoded)
        E_i = int(blocks_i.numel())
        n, K, V = int(rs[-1]), E_i + 16, E_i + 16
        kvs.append(batch.KVStream.empty(n, K, V, dev))
        decs.append(torch.zeros(4, dtype=torch.int64, device=dev))
        sizes.append((n, K, V))
        shards.append(shard.RangeShard(kvs[-1], rs, opts, lo, hi, stream=stream))
    E = sum(int(p[0].numel()) for p in parts)
    nblk = sum(p[1].numel() - 1 for p in parts)
    n_all = sum(int(p[2][-1]) for p in parts)
    res = []

    def step(ev=None):
        if ev is not None:
            ev[0].record(stream)
        for (blocks_i, off_i, rs, lo, hi), kv, sd, (n, K, V) in zip(parts, kvs, decs, sizes):
            batch.decode_into(blocks_i, off_i, off_i.numel() - 1, kv, sd, n, K, V)
            kv.n = n
        if ev is not None:
            ev[1].record(stream)
        res[:] = shard.compact_dist(shards) if world > 1 else shard.compact_local(shards)
        if ev is not None:
            ev[2].record(stream)

    elapsed, (dec_ms, cmp_ms) = timed(step, steps, warmup, world, dev)
    ok = all(sd.cpu().tolist()[3] == 0 and sd.cpu().tolist()[0] == int(p[2][-1]) for sd, p in zip(decs, parts))
    if args.dump_outputs and ok and not extra:
        dump_outputs(args.dump_outputs, rank, world, [
            (f"range{rank * R + i}_{name}", r[name]) for i, r in enumerate(res)
            for name in ("blocks", "blk_off", "seg_start", "seg_blk")])
    checked = 0
    if args.full and ok and not args.no_oracle_check:
        for (blocks_i, off_i, rs, lo, hi), sh, r in zip(parts, shards, res):
            # range by range: its input read back from the device, every host copy freed before
            # the next range (host RSS bounded by one range's check, not by the rank's input)
            c = oracle_check_range(blocks_i, off_i, rs, opts, sh, r, lo, hi)
            gc.collect()
            ok = ok and c == r["nblk"]
            checked += c
    # the carries chain through every range: carry-out of range g == carry-in of range g + 1
    cc = torch.tensor([x for r in res for x in list(r["carry_in"]) + list(r["carry_out"])], dtype=torch.int64,
                      device=cdev)
    if world > 1:
        allc = [torch.zeros_like(cc) for _ in range(world)]
        dist.all_gather(allc, cc)
        flat = [x for c in allc for x in c.cpu().tolist()]
    else:
        flat = cc.cpu().tolist()
    chain = [flat[4 * g:4 * g + 4] for g in range(world * R)]
    chain_ok = chain[0][:2] == [0, 0] and all(chain[g][2:] == chain[g + 1][:2] for g in range(world * R - 1))
    tot = torch.tensor([sum(r["nblk"] for r in res), sum(r["nbytes"] for r in res),
                        sum(r["nseg"] - int(r["first_continues"]) for r in res), sum(r["m"] for r in res),
                        sum(r["merged"] for r in res)], dtype=torch.int64, device=cdev)
    rss = torch.tensor([host_rss_gib(), time.time() - t0], dtype=torch.float64, device=cdev)
    if world > 1:
        dist.all_reduce(tot)
        dist.all_reduce(rss, op=dist.ReduceOp.MAX)
    t_max, ok_all, checked_all = reduce_ranks(elapsed, ok and chain_ok, checked, world, dev)
    if rank != 0:
        return None
    ms = t_max / steps * 1e3
    tot = tot.cpu().tolist()
    backend = ("RCCL" if dist.get_backend() == "nccl" else "gloo") if world > 1 else "in-process"
    return {
        "metric": METRIC, "value": round(world * E * steps / t_max / GiB, 3), "unit": "GiB/s", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "full": bool(args.full), "status_ok": bool(ok_all),
        "config": {"workload": f"C: compaction-shaped, {nrun} overlapping sorted runs of {args.segment_bytes >> 20} MiB "
                               f"SSTs ({nblk} x 4 KiB input blocks/GPU, {E / GiB:.2f} GiB/GPU, ~10% overwrites, 2% "
                               f"tombstones), split by key range into {world} GPUs x {R} ranges whose splitters fall "
                               "inside the input SSTs (each range decodes the blocks meeting its keys, straddling "
                               "blocks by both neighbours): decode + range merge + compaction rules + halo all-gather "
                               "+ SST rotation with range-to-range carry + block packing",
                   "input_blocks_per_gpu": nblk, "input_entries_per_gpu": n_all, "encoded_bytes_per_gpu": E,
                   "ranges_per_gpu": R, "total_input_gib": round(world * E / GiB, 2),
                   "host_peak_rss_gib_max_rank": round(float(rss[0].item()), 2),
                   "wall_s_max_rank": round(float(rss[1].item()), 1),
                   "merged_entries": tot[4], "kept_entries": tot[3], "output_blocks": tot[0], "output_bytes": tot[1],
                   "output_ssts": tot[2], "target_sst_size": args.segment_bytes,
                   "parallelism": f"key-range sharded x{world}x{R} ({backend}: splitter + halo all-gather, "
                                  "carry send/recv)",
                   "rccl_world": world, "compaction_bit_exact": bool(ok_all) if args.full else None,
                   "carry_chain_ok": bool(chain_ok),
                   "oracle_checked_blocks": int(checked_all)},
        "stage_ms": {"decode": round(dec_ms, 4), "compact": round(cmp_ms, 4)},
    }


def extra_or_exit(rank, fn):
    """An N>1 extra config: a rank whose part raises exits at once with status 1 (no cleanup that
    could block on its peers), so the launcher -- bench.py's own or torch.distributed.run --
    tears the job down instead of the peers hanging in a collective with it."""
    try:
        return fn()
    except Exception as e:
        log(f"[rank {rank}] extra config C failed: {e!r}")
        sys.stderr.flush()
        os._exit(1)


class _DryShard:
    """--dry-run-fail-extra: a CPU stand-in for shard.RangeShard whose merge raises on one rank,
    while the other ranks go on into compact_dist's head all-gather (and block there)."""

    def __init__(self, fail):
        self.fail, self.dev, self.W = fail, torch.device("cpu"), 2

    def merge(self):
        if self.fail:
            raise RuntimeError("dry run: merge failed as asked")
        return 0

    def head(self):
        from lsm_amd import shard
        z = torch.zeros(1, dtype=torch.int64)
        return shard.Head(0, z, z.clone(), z[:0], torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8))


def dry_run(args, rank, world, local):
    """The launcher's contract without a GPU: every rank joins one gloo group; rank 0 reports the
    world size the collective saw and the ranks it heard from."""
    import torch.distributed as dist
    seen = world
    if args.dry_run_fail_rank == rank:
        log(f"[rank {rank}] dry run: exiting early as asked")
        return 3
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([1 << rank], dtype=torch.int64)
        dist.all_reduce(t)
        seen = dist.get_world_size()
        mask = int(t.item())
        if args.dry_run_fail_extra is not None:  # the N>1 extra's failure path, through compact_dist
            from lsm_amd import shard
            extra_or_exit(rank, lambda: shard.compact_dist(_DryShard(rank == args.dry_run_fail_extra)))
        dist.destroy_process_group()
    else:
        mask = 1
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "collective_world": seen, "rank_mask": mask,
                          "local_rank": local, "c_extra_plan": c_plan_summary(args, world)}), flush=True)
    return 0


# ---------------------------------------------------------------------------------------------
def main(argv=None):
    args = parse(argv)
    if args.ablate is not None or args.trace_plan or args.trace_fused:  # ablation masks, traces: diagnostics build
        from lsm_amd import _build
        os.environ.setdefault("LSMBLK_SO_OVERRIDE", _build.DIAG_SO)
    if "RANK" not in os.environ and args.gpus > 1:
        return launch(args, sys.argv[1:] if argv is None else list(argv))
    rank, world, local = dist_env()
    if world != args.gpus:
        log(f"refusing to run: WORLD_SIZE={world} but --gpus {args.gpus}")
        return 2
    if args.dry_run:
        return dry_run(args, rank, world, local)
    # diagnostics only: LSMBLK_BENCH_BACKEND=gloo runs the N-rank logic with host-side collectives,
    # e.g. several ranks sharing the one GPU of a test box
    backend = os.environ.get("LSMBLK_BENCH_BACKEND", "nccl")
    if backend == "gloo":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        if dist.get_world_size() != args.gpus:
            log(f"refusing to run: RCCL world {dist.get_world_size()} != --gpus {args.gpus}")
            return 2
    if args.config == "C":
        result = run_compaction(args, args.steps, args.warmup, rank, world, local, dev)
    else:
        result = run_blocks(args, args.config, args.steps, args.warmup, rank, world, local, dev)
    if args.ablate is not None:
        return 0
    if not args.full:  # a plain run: the headline line alone
        pass
    elif world == 1 and args.config == "U" and not args.no_extras and args.blocks is None:
        extras = {}
        for cfg in ("Z", "M"):
            torch.cuda.empty_cache()
            extras[cfg] = run_blocks(args, cfg, 5, 2, rank, world, local, dev, extra=True)
        torch.cuda.empty_cache()
        extras["C"] = run_compaction(args, 3, 1, rank, world, local, dev, extra=True)
        result["extra_configs"] = extras
    elif world > 1 and args.config == "U" and not args.no_extras and args.blocks is None:
        # the compaction-shaped config split by key range over the same N GPUs (one extra line).
        # A rank that fails here exits at once, non-zero: its peers, blocked in a collective with
        # it, are then torn down by the launcher (bench.py's own or torch.distributed.run)
        # instead of hanging until the driver's time limit.
        torch.cuda.empty_cache()
        c = extra_or_exit(rank, lambda: run_compaction(args, 3, 1, rank, world, local, dev, extra=True))
        if result is not None:
            result["extra_configs"] = {"C": c}
    ok = True
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if result is not None:
        ok = result["status_ok"]  # (--full: the round trip and the oracle check included)
        print(json.dumps(result), flush=True)
    return 0 if ok else 1


KERNELS = ["dec_count", "dec_scan", "decode", "plan", "emit"]


def framing_crc32(blocks, blk_off, nblk, E, dev, stream, reps=5):
    """SST framing row: per-block crc32fast of the resident blocks, one
    lsmblk_crc32_batch launch (crc_stream_kernel) per rep, HIP events on the launch stream.  Not part
    of `value`; reported beside it with its own HBM roofline (E bytes read per launch)."""
    import zlib
    crc = torch.zeros(nblk, dtype=torch.int32, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    batch.crc32_into(blocks, blk_off, nblk, crc, st)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for _ in range(reps):
        batch.crc32_into(blocks, blk_off, nblk, crc, st)
    ev[1].record(stream)
    torch.cuda.synchronize(dev)
    ms = ev[0].elapsed_time(ev[1]) / reps
    # spot check against zlib (== crc32fast) on a sample of blocks
    off = blk_off.cpu().numpy().view(np.uint64)
    got = crc.cpu().numpy().view(np.uint32)
    idx = np.linspace(0, nblk - 1, 64).astype(np.int64)
    host = blocks.cpu().numpy() if E < (1 << 33) else None
    ok = host is not None and all(
        int(got[i]) == zlib.crc32(host[int(off[i]):int(off[i + 1])].tobytes()) for i in idx) and st[3].item() == 0
    gbs = E / (ms * 1e-3) / 1e9
    return {"kernel": "crc_stream_kernel", "ms": round(ms, 4), "gib_s": round(E / (ms * 1e-3) / GiB, 2),
            "achieved_gbs": round(gbs, 1), "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 4),
            "bytes_per_launch": E, "checked_vs_zlib": int(len(idx)) if ok else 0, "ok": bool(ok)}


def read_path_verify(blocks, blk_off, nblk, out_kv, n, K, V, st_dec, dev, stream, reps=5):
    """read_block over a framed SST data section (src/table.rs:213-233): every
    block followed by its BE crc32fast, decoded with verify=True -- the streaming CRC pass over E,
    the checksum test, then the lagged decode (one launch).  Timed
    beside the plain decode of the same blocks; the KV stream must be identical.  Not part of
    `value`."""
    E = int(blk_off[nblk].item())
    if E >= (1 << 33):
        return None
    crc = torch.zeros(nblk, dtype=torch.int32, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    batch.crc32_into(blocks, blk_off, nblk, crc, st)
    off = blk_off.cpu().numpy()
    be = crc.cpu().numpy().view(np.uint32).byteswap().view(np.uint8)
    framed_h = np.insert(blocks.cpu().numpy(), np.repeat(off[1:], 4), be)
    framed = torch.from_numpy(framed_h).to(dev)
    del framed_h
    foff = blk_off + 4 * torch.arange(nblk + 1, dtype=torch.int64, device=dev)
    vkv = batch.KVStream(batch._aligned_empty(K + 16, dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                         batch._aligned_empty(V + 16, dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                         torch.empty(n, dtype=torch.int64, device=dev), n)
    sv = torch.zeros(4, dtype=torch.int64, device=dev)

    def run(verify):
        if verify:
            batch.decode_ex_into(framed, foff, nblk, vkv, sv, n, K, V, tail=4, verify=True)
        else:
            batch.decode_into(blocks, blk_off, nblk, out_kv, st_dec, n, K, V)

    ms = {}
    for verify in (True, False, True):
        run(verify)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(stream)
        for _ in range(reps):
            run(verify)
        ev[1].record(stream)
        torch.cuda.synchronize(dev)
        ms["verify" if verify else "plain"] = ev[0].elapsed_time(ev[1]) / reps
    ok = sv[3].item() == 0 and st_dec[3].item() == 0
    ok = ok and all(torch.equal(a, b) for a, b in ((vkv.keys[:K], out_kv.keys[:K]), (vkv.vals[:V], out_kv.vals[:V]),
                                                   (vkv.key_off, out_kv.key_off[:n + 1]),
                                                   (vkv.val_off, out_kv.val_off[:n + 1]), (vkv.ts, out_kv.ts[:n])))
    return {"kernels": "crc_stream + crc_verify + decode_lag",
            "framed_bytes": E + 4 * nblk, "verify_ms": round(ms["verify"], 4), "plain_decode_ms": round(ms["plain"], 4),
            "verify_gib_s": round(E / (ms["verify"] * 1e-3) / GiB, 2), "kv_equal_to_plain_decode": bool(ok)}


def framing_meta(blocks, blk_off, nblk, seg_t, st_enc, dev, stream, reps=5):
    """SST framing row: the BlockMeta section of every segment (SST) of the
    last re-encode (lsmblk_encode_segment_blocks + lsmblk_block_meta_batch: 4 small kernels +
    crc_stream_kernel over the sections + the CRC stores), HIP events on the launch stream.  Not part
    of `value`.  Spot check: every sampled section's u32 count equals its block count and its
    trailing CRC equals zlib.crc32 of the bytes after the count (table.rs:29-63)."""
    import zlib
    nseg = seg_t.numel() - 1
    seg_blk = torch.zeros(nseg + 1, dtype=torch.int32, device=dev)
    batch.segment_blocks_into(seg_t, nseg, st_enc, seg_blk)
    cap = 16 * nseg + 64 * nblk
    meta = batch._aligned_empty(cap, dev)
    meta_off = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    ob = blk_off[:nblk + 1]
    batch.block_meta_into(blocks, ob, nblk, seg_blk, nseg, meta, cap, meta_off, st)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for _ in range(reps):
        batch.block_meta_into(blocks, ob, nblk, seg_blk, nseg, meta, cap, meta_off, st)
    ev[1].record(stream)
    torch.cuda.synchronize(dev)
    ms = ev[0].elapsed_time(ev[1]) / reps
    mo = meta_off.cpu().numpy()
    sb = seg_blk.cpu().numpy().view(np.uint32)
    total = int(st[1].item())
    host = meta[:total].cpu().numpy().tobytes()
    ok = st[3].item() == 0 and int(mo[-1]) == total
    for g in np.linspace(0, nseg - 1, 16).astype(np.int64):
        sec = host[int(mo[g]):int(mo[g + 1])]
        ok = ok and int.from_bytes(sec[:4], "big") == int(sb[g + 1] - sb[g])
        ok = ok and int.from_bytes(sec[-4:], "big") == zlib.crc32(sec[4:-4])
    E = int(blk_off[nblk].item())
    return {"kernels": "meta_size/scan/write/seg + crc_stream_kernel + crc_put", "ms": round(ms, 4),
            "meta_bytes": total, "block_bytes_read": E, "sections": nseg,
            "gib_s_of_blocks": round(E / (ms * 1e-3) / GiB, 2), "checked_sections": 16 if ok else 0,
            "ok": bool(ok)}


def encode_slots(kv, seg_t, nseg, bs, blocks, blk_off, dev, stream, reps=5):
    """Re-encode with per-segment slots (LSMBLK_ENCODE_SEG_SLOTS: every SST's data section at a place
    known before the call, include/lsmblk.h) beside the packed headline encode: encode ms (HIP
    events over reps calls), and the slots packed == the input blocks.  Not part of `value`."""
    K, V = kv.byte_sizes()
    n = kv.n
    out_cap, blk_cap = K + V + 18 * n + 16, blk_off.numel() + 1
    out = batch._aligned_empty(out_cap, dev)
    off = torch.zeros(blk_cap, dtype=torch.int64, device=dev)
    so = torch.zeros(2 * nseg, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)

    def run():
        batch.encode_into(kv, seg_t, nseg, bs, out, out_cap, off, blk_cap, st, stream=stream, seg_out=so)
    run()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for _ in range(reps):
        run()
    ev[1].record(stream)
    torch.cuda.synchronize(dev)
    ms = ev[0].elapsed_time(ev[1]) / reps
    s = st.cpu().tolist()
    nblk = blk_off.numel() - 1
    ok = s[3] == 0 and s[0] == nblk
    if ok:
        pb, po = batch.slots_to_packed(out, off[:nblk + 1], so)
        ok = torch.equal(pb, blocks) and torch.equal(po, blk_off)
    return {"call": "lsmblk_encode_batch_ex(LSMBLK_ENCODE_SEG_SLOTS)", "ms": round(ms, 4), "segments": nseg,
            "packed_equal_input": bool(ok)}


def encode_framed(kv, seg_t, nseg, bs, blocks, blk_off, dev, stream, enc_ms, reps=5):
    """Re-encode as SST data sections (LSMBLK_ENCODE_FRAMED: every block followed by its BE
    crc32fast, SsTableBuilder::finish_block, reference src/table/builder.rs:112-123): encode ms (HIP
    events over reps calls) beside the unframed encode's; checked by the verifying framed decode
    (every CRC recomputed on the GPU and compared, tail 4), its KV stream == the step's decoded
    one, the framed offsets == the input's + 4 per block, and 256 sampled CRCs == zlib.  Not part
    of `value`."""
    import zlib
    K, V = kv.byte_sizes()
    n = kv.n
    out_cap, blk_cap = K + V + 22 * n + 16, blk_off.numel() + 1
    out = batch._aligned_empty(out_cap, dev)
    off = torch.zeros(blk_cap, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)

    def run():
        batch.encode_into(kv, seg_t, nseg, bs, out, out_cap, off, blk_cap, st, stream=stream, framed=True)
    run()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for _ in range(reps):
        run()
    ev[1].record(stream)
    torch.cuda.synchronize(dev)
    ms = ev[0].elapsed_time(ev[1]) / reps
    s = st.cpu().tolist()
    nblk = blk_off.numel() - 1
    ok = s[3] == 0 and s[0] == nblk and s[1] == int(blk_off[-1].item()) + 4 * nblk
    if ok:
        fo = off[:nblk + 1]
        ok = torch.equal(fo, blk_off + 4 * torch.arange(nblk + 1, dtype=torch.int64, device=dev))
    if ok:
        dkv = batch.decode_blocks(out[:s[1]], fo, stream=stream, tail=4, verify=True)
        ok = dkv.n == n and all(torch.equal(getattr(dkv, f)[:m], getattr(kv, f)[:m])
                                for f, m in (("key_off", n + 1), ("val_off", n + 1), ("ts", n), ("keys", K),
                                             ("vals", V)))
        del dkv
    if ok:
        fh, bo = fo.cpu().numpy(), blk_off.cpu().numpy()
        for i in np.linspace(0, nblk - 1, 256).astype(np.int64).tolist():
            blk = blocks[bo[i]:bo[i + 1]].cpu().numpy().tobytes()
            crc = out[fh[i + 1] - 4:fh[i + 1]].cpu().numpy().tobytes()
            ok = ok and crc == zlib.crc32(blk).to_bytes(4, "big")
    return {"call": "lsmblk_encode_batch_ex(LSMBLK_ENCODE_FRAMED)", "ms": round(ms, 4),
            "unframed_encode_ms": enc_ms, "framing_cost_ms": round(ms - enc_ms, 4),
            "gib_s": round((int(blk_off[-1].item()) + 4 * nblk) / (ms * 1e-3) / 2 ** 30, 2),
            "verified": bool(ok)}


def compaction_filter(kv, n, K, V, dev, stream, reps=5):
    """Compaction row (merge rules): lsmblk_compact_filter_batch over the
    decoded stream (unique keys; watermark 2^39 puts about half the 40-bit ts below it; bottom
    level; one prefix filter matching nothing).  Every entry is kept, so a launch reads and
    writes the whole stream: algorithmic bytes 2 D (+ 4 B keep flag per entry).  Not part of
    `value`."""
    import ctypes
    from lsm_amd._lib import check as _check, lib as _lib
    out = batch.KVStream(batch._aligned_empty(K + 16, dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                         batch._aligned_empty(V + 16, dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                         torch.empty(n, dtype=torch.int64, device=dev), 0)
    pfx = torch.tensor([0xFF, 0xFF, 0xFF], dtype=torch.uint8, device=dev)
    pfo = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    ci, co = kv._c(), out._c(n, K + 16, V + 16)
    ctx = batch._ctx(dev.index, stream)

    def run():
        _check(_lib().lsmblk_compact_filter_batch(ctx, ctypes.byref(ci), 1 << 39, 1, pfx.data_ptr(), pfo.data_ptr(), 1,
                                                  ctypes.byref(co), st.data_ptr(), stream.cuda_stream))
    run()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for _ in range(reps):
        run()
    ev[1].record(stream)
    torch.cuda.synchronize(dev)
    ms = ev[0].elapsed_time(ev[1]) / reps
    D = K + V + 16 * n
    s = st.cpu().tolist()
    ok = s[3] == 0 and s[0] == n and torch.equal(out.ts[:n], kv.ts[:n]) and torch.equal(out.vals[:V], kv.vals[:V])
    gbs = (2 * D + 4 * n) / (ms * 1e-3) / 1e9
    return {"kernels": "filt_flag + filt_scan + filt_write", "ms": round(ms, 4), "entries": n, "kept": int(s[0]),
            "achieved_gbs": round(gbs, 1), "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 4),
            "bytes_per_launch": 2 * D + 4 * n, "ok": bool(ok)}


def kernel_times(ctx, step, dev, reps=3, lead=3):
    """Per-kernel ms of one step (the library's dispatch start/stop events, hipExtLaunchKernelGGL).
    Each read follows `lead` back-to-back steps: after an idle gap (a synchronize) the first
    kernels ran ~8 % slower than in the timed region, as the clocks had dropped."""
    import ctypes
    check(lib().lsmblk_debug_set(ctx, 2, 1))
    acc = {k: [] for k in KERNELS}
    buf = (ctypes.c_float * 5)()
    for _ in range(reps):
        for _ in range(lead):
            step()
        torch.cuda.synchronize(dev)
        check(lib().lsmblk_ctx_kernel_times(ctx, buf))
        for i, k in enumerate(KERNELS):
            acc[k].append(buf[i])
    check(lib().lsmblk_debug_set(ctx, 2, 0))
    # a kernel the step did not launch reads -1 (the lagged decode has no count / scan launches)
    return {k: float(np.mean(v)) for k, v in acc.items() if min(v) >= 0}


def kernel_log_profile(ctx, step, dev, reps=3, lead=2):
    """{kernel: (launches, ms)} per step over `reps` back-to-back steps, every launch carrying its
    dispatch start / stop events (lsmblk_ctx_kernel_log), after `lead` untimed steps."""
    from lsm_amd._lib import kernel_log
    for _ in range(lead):
        step()
    torch.cuda.synchronize(dev)
    check(lib().lsmblk_debug_set(ctx, 2, 1))
    kernel_log(ctx)  # empties the log
    for _ in range(reps):
        step()
    torch.cuda.synchronize(dev)
    log = kernel_log(ctx)
    check(lib().lsmblk_debug_set(ctx, 2, 0))
    return {k: (n / reps, ms / reps) for k, (n, ms) in log.items()}


def measured_traffic(cfg, kernel, launches=1.0, default_size=True):
    """(HBM bytes per step of `kernel`, None) from profiles/traffic.json when it was measured at the
    kernel sources this run executes (tools/traffic.sh stamps it with lsm_amd/_build.py src_sha), else
    (None, the reason)."""
    from lsm_amd import _build
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if not default_size:
        return None, "batch size differs from the traffic passes (default sizes only)"
    if not os.path.exists(tpath):
        return None, "no profiles/traffic.json"
    tj = json.load(open(tpath))
    sha = _build.src_sha()
    if tj.get("src_sha256") != sha:
        return None, (f"profiles/traffic.json was measured at kernel sources {str(tj.get('src_sha256'))[:12]} "
                      f"(commit {tj.get('commit')}), this run's are {sha[:12]}")
    c = tj.get("configs", {}).get(cfg)
    if c is None:
        return None, f"no config {cfg} pass in profiles/traffic.json"
    # Kernel names are compared without spaces: the kernel log names a template instance as written
    # in the source (`mwrite_kernel<false,true>`), rocprofv3's demangler with a space after each
    # comma (`mwrite_kernel<false, true>`) -- VERDICT round 5: config C's traffic was null for it.
    norm = (lambda k: "".join(str(k).split()))
    bpl = {norm(k): v for k, v in c.get("bytes_per_launch", {}).items()}
    kern = {norm(k): v for k, v in c.get("kernels", {}).items()}
    if norm(kernel) in bpl:
        return int(bpl[norm(kernel)]), None
    if norm(kernel) in kern:
        return int(kern[norm(kernel)]["bytes_per_dispatch"] * launches), None
    return None, f"kernel {kernel} not in the config {cfg} passes"


def ablate(args, ctx, blocks, blk_off, nblk, out_kv, st_dec, n, K, V, stream):
    from lsm_amd._lib import lib as L
    res = {}
    masks = {0, 2, 4, 8, 14, 256, 1024, 2048, 3072, 256 | 3072, args.ablate}
    if args.ablate_only:
        masks = {0, args.ablate}
    elif args.ablate_lag:  # lagged decode: no count, no wait, no early base load, no tile finish, no publish
        masks = {0, 1024, 3072, 3072 | 4096, 3072 | 8192, 3072 | 8192 | 16384, 3072 | 4096 | 8192 | 16384,
                 256 | 3072 | 4096 | 8192 | 16384}
    for mask in sorted(masks):
        check(L().lsmblk_debug_set(ctx, 1, mask))
        for _ in range(2):
            batch.decode_into(blocks, blk_off, nblk, out_kv, st_dec, n, K + 16, V + 16)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            batch.decode_into(blocks, blk_off, nblk, out_kv, st_dec, n, K + 16, V + 16)
        e1.record(stream)
        torch.cuda.synchronize()
        res[mask] = round(e0.elapsed_time(e1) / args.steps, 3)
    check(L().lsmblk_debug_set(ctx, 1, 0))
    if args.ablate_lag or args.ablate_only:  # the lagged decode's per-tile realtime trace over one call
        import ctypes
        import numpy as _np
        check(L().lsmblk_debug_set(ctx, 5, 1))
        batch.decode_into(blocks, blk_off, nblk, out_kv, st_dec, n, K + 16, V + 16)
        NW = 16 + 8 * 32768
        w = (ctypes.c_uint64 * NW)()
        check(L().lsmblk_debug_counters(ctx, w, NW))
        check(L().lsmblk_debug_set(ctx, 5, 0))
        tr = _np.frombuffer(w, dtype=_np.uint64)[16:].reshape(-1, 8).astype(_np.int64)
        nt = min(len(tr), (nblk + 63) // 64)
        tr, m = tr[:nt], slice(1, max(2, nt - 256))
        q = lambda x: {p: round(float(_np.percentile(x, p)) / 100, 2) for p in (10, 50, 90, 99)}  # us (100 MHz)
        print(json.dumps({"trace_us": {
            "first_count_to_finish_start": q(tr[:, 0] - tr[:, 4]),
            "finish_duration": q(tr[:, 1] - tr[:, 0]),
            "finish_done_to_decoder_start": q(tr[m, 5] - tr[m, 1]),
            "decoder_wait": q(tr[m, 3] - tr[m, 2]),
            "decoder_start_to_wait": q(tr[m, 2] - tr[m, 5]),
            "kernel_span_us": round(float((tr[:, 3].max() - tr[:, 4].min()) / 100), 1)}}), flush=True)
    polls = {}
    for pm in (0, 1, 2):
        check(L().lsmblk_debug_set(ctx, 0, pm))
        for _ in range(2):
            batch.decode_into(blocks, blk_off, nblk, out_kv, st_dec, n, K + 16, V + 16)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            batch.decode_into(blocks, blk_off, nblk, out_kv, st_dec, n, K + 16, V + 16)
        e1.record(stream)
        torch.cuda.synchronize()
        polls[pm] = (round(e0.elapsed_time(e1) / args.steps, 3), st_dec.cpu().tolist()[3])
    print(json.dumps({"ablation_decode_ms_by_skip_mask": res, "decode_ms_err_by_poll_mode": polls}), flush=True)
    return 0


def cpu_baseline(blocks, blk_off, seg, bs, seconds):
    """The oracle's C restatement (single thread) on a bounded sample of the same workload:
    decode + re-encode of the first 16 Ki blocks, repeated for ~`seconds`."""
    from oracle import oracle as O
    nb = min(16384, blk_off.numel() - 1)
    off = blk_off[:nb + 1].cpu().numpy().view(np.uint64)
    host_blocks = blocks[:int(off[-1])].cpu().numpy()
    rc, kv = O.decode_blocks(host_blocks, off)
    assert rc == 0
    s = seg[seg < kv.n]
    s = np.concatenate([s, [kv.n]]).astype(np.uint32)
    reps, t0 = 0, time.perf_counter()
    while True:
        rc1, kv2 = O.decode_blocks(host_blocks, off)
        rc2, b2, o2 = O.encode_segments(kv2, s, bs)
        reps += 1
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    assert rc1 == 0 and rc2 == 0 and np.array_equal(b2, host_blocks)
    cpu = platform.processor() or platform.machine()
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    res = {"value": round(len(host_blocks) * reps / dt / GiB, 4), "unit": "GiB/s", "cores": 1, "kind": "port",
           "sample": f"{nb} blocks ({len(host_blocks) / 2**20:.1f} MiB encoded) decode+re-encode x{reps}, "
                     f"oracle/lsmblk_oracle.c -O3 single thread, {cpu}, host nproc={os.cpu_count()}"}
    res["all_cores"] = cpu_baseline_threads(host_blocks, off, s, bs, max(seconds / 2, 2.0))
    return res


def cpu_baseline_threads(host_blocks, off, s, bs, seconds):
    """the same sample on T host threads at once, one independent
    decode + re-encode replica per thread (the reference runs one builder per SST, so SSTs are
    the unit of host parallelism).  T = the job's CPU share (OMP_NUM_THREADS, else the
    affinity mask), at most 64.  ctypes releases the GIL inside the C oracle."""
    import threading
    from oracle import oracle as O
    T = int(os.environ.get("OMP_NUM_THREADS") or 0) or len(os.sched_getaffinity(0))
    T = max(1, min(T, 64))
    counts = [0] * T
    errs = []
    start = threading.Barrier(T + 1)
    stop = [False]

    def work(i):
        start.wait()
        while not stop[0]:
            rc1, kv2 = O.decode_blocks(host_blocks, off)
            rc2, b2, _ = O.encode_segments(kv2, s, bs)
            if rc1 or rc2 or len(b2) != len(host_blocks):
                errs.append((rc1, rc2))
                return
            counts[i] += 1

    th = [threading.Thread(target=work, args=(i,)) for i in range(T)]
    for t in th:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    time.sleep(seconds)
    stop[0] = True
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    return {"value": round(len(host_blocks) * sum(counts) / dt / GiB, 4), "unit": "GiB/s", "cores": T,
            "ok": not errs, "sample": f"{T} threads x the same {len(off) - 1}-block sample, {sum(counts)} passes"}


def pcie_inclusive(blocks, blk_off, nblk, kv, seg, bs, dev, chunks=16, reps=3):
    """Blocks start and end in pinned host memory (mmap'd SST files, memtable buffers): the batch
    is cut into `chunks` pieces at SST (segment) boundaries and pipelined over three HIP streams --
    H2D of chunk i+1 (blocks + their offsets) and D2H of chunk i-1 overlap the decode + re-encode
    of chunk i, device slots double-buffered.  The bound it is compared with: PCIe is full duplex,
    so with the copies overlapped the rate cannot exceed the slower of the measured pinned H2D and
    D2H bandwidths (each timed alone over the whole batch in this run).  Not `value`."""
    E = int(blk_off[nblk].item())
    off = blk_off.cpu().numpy().view(np.uint64).astype(np.int64)
    _, ent = batch.decode_blocks(blocks, blk_off, with_blk_ent=True)
    ent = ent.cpu().numpy().view(np.uint64).astype(np.int64)
    ko = kv.key_off[:kv.n + 1].cpu().numpy().view(np.uint32).astype(np.int64)
    vo = kv.val_off[:kv.n + 1].cpu().numpy().view(np.uint32).astype(np.int64)
    seg_blk = np.searchsorted(ent, seg[:-1].astype(np.int64))  # every segment starts a block
    cuts = sorted({0, nblk} | {int(seg_blk[np.searchsorted(seg_blk, (nblk * i) // chunks)]) for i in range(1, chunks)
                               if np.searchsorted(seg_blk, (nblk * i) // chunks) < len(seg_blk)})
    plan = []
    for b0, b1 in zip(cuts, cuts[1:]):
        e0, e1 = int(ent[b0]), int(ent[b1])
        sc = seg[(seg >= e0) & (seg < e1)].astype(np.int64) - e0
        sc = np.concatenate([sc, [e1 - e0]]).astype(np.uint32)
        ho = torch.from_numpy((off[b0:b1 + 1] - off[b0]).copy()).pin_memory()
        plan.append(dict(b0=b0, b1=b1, o0=int(off[b0]), o1=int(off[b1]), n=e1 - e0, K=int(ko[e1] - ko[e0]),
                         V=int(vo[e1] - vo[e0]), seg=torch.from_numpy(sc.view(np.int32)).to(dev), hoff=ho))
    mE = max(c["o1"] - c["o0"] for c in plan)
    mB = max(c["b1"] - c["b0"] for c in plan)
    mn, mK, mV = max(c["n"] for c in plan), max(c["K"] for c in plan), max(c["V"] for c in plan)
    slots = [dict(inb=batch._aligned_empty(mE + 16, dev), off=torch.zeros(mB + 1, dtype=torch.int64, device=dev),
                  kv=batch.KVStream(batch._aligned_empty(mK + 16, dev), torch.empty(mn + 1, dtype=torch.int32, device=dev),
                                    batch._aligned_empty(mV + 16, dev), torch.empty(mn + 1, dtype=torch.int32, device=dev),
                                    torch.empty(mn, dtype=torch.int64, device=dev), mn),
                  out=batch._aligned_empty(mE + 16, dev), oof=torch.zeros(mB + 2, dtype=torch.int64, device=dev),
                  sd=torch.zeros(4, dtype=torch.int64, device=dev), se=torch.zeros(4, dtype=torch.int64, device=dev))
             for _ in range(2)]
    hin = torch.empty(E, dtype=torch.uint8, pin_memory=True)
    hin.copy_(blocks[:E].cpu())
    hout = torch.empty(E, dtype=torch.uint8, pin_memory=True)
    s_h2d, s_cmp, s_d2h = torch.cuda.Stream(dev), torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    C = len(plan)

    def run():
        h2d = [torch.cuda.Event() for _ in range(C)]
        cmp_ = [torch.cuda.Event() for _ in range(C)]
        d2h = [torch.cuda.Event() for _ in range(C)]
        for i, c in enumerate(plan):
            sl = slots[i % 2]
            Ec, nb = c["o1"] - c["o0"], c["b1"] - c["b0"]
            with torch.cuda.stream(s_h2d):
                if i >= 2:
                    s_h2d.wait_event(cmp_[i - 2])     # the slot's input was consumed
                sl["inb"][:Ec].copy_(hin[c["o0"]:c["o1"]], non_blocking=True)
                sl["off"][:nb + 1].copy_(c["hoff"], non_blocking=True)
                h2d[i].record(s_h2d)
            with torch.cuda.stream(s_cmp):
                s_cmp.wait_event(h2d[i])
                if i >= 2:
                    s_cmp.wait_event(d2h[i - 2])     # the slot's output was copied out
                batch.decode_into(sl["inb"], sl["off"], nb, sl["kv"], sl["sd"], c["n"], c["K"] + 16, c["V"] + 16,
                                  stream=s_cmp)
                sl["kv"].n = c["n"]
                batch.encode_into(sl["kv"], c["seg"], c["seg"].numel() - 1, bs, sl["out"], mE + 16, sl["oof"], mB + 2,
                                  sl["se"], stream=s_cmp)
                cmp_[i].record(s_cmp)
            with torch.cuda.stream(s_d2h):
                s_d2h.wait_event(cmp_[i])
                hout[c["o0"]:c["o1"]].copy_(sl["out"][:Ec], non_blocking=True)
                d2h[i].record(s_d2h)
    run()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / reps
    ok = torch.equal(hout, hin) and all(sl["sd"][3].item() == 0 and sl["se"][3].item() == 0 for sl in slots)
    # the bound: pinned H2D and D2H of the whole batch, each alone
    dbuf = torch.empty(E, dtype=torch.uint8, device=dev)
    bw = {}
    for name, dst, src in (("h2d", dbuf, hin), ("d2h", hout, dbuf)):
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(reps):
            dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize(dev)
        bw[name] = E * reps / (time.perf_counter() - t1) / GiB
    bound = min(bw.values())
    rate = E / dt / GiB
    return {"gib_s": round(rate, 3), "chunks": C, "streams": "h2d / decode+re-encode / d2h, double-buffered",
            "h2d_gib_s": round(bw["h2d"], 2), "d2h_gib_s": round(bw["d2h"], 2),
            "bound": "min(pinned H2D, pinned D2H): PCIe full duplex with the copies overlapped",
            "bound_gib_s": round(bound, 2), "frac_of_bound": round(rate / bound, 4), "bit_exact": bool(ok)}


if __name__ == "__main__":
    sys.exit(main())
